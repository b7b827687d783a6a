"""tests/guarded.py on the CPU: every guard test of tests/test_caller_memory_gpu.py can fail.  A write one element in front
of the view or one element behind it trips ``check()`` and names the side; writes inside the view, all of it, do not."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from guarded import FILLS, MIN_GUARD, guarded, holds_fill, same_bytes  # noqa: E402

SHAPES = [((3, 5, 7), torch.float64, 0), ((3, 5, 7), torch.float64, 8), ((2, 9), torch.int32, 4), ((11,), torch.int8, 1),
          ((4, 130), torch.float32, 0), ((1000,), torch.uint8, 240), ((0,), torch.int32, 0)]


def _neighbours(view):
    """Flat tensors over the whole allocation in the view's dtype, and the view's first element's index in it."""
    raw = view.untyped_storage()
    whole = torch.empty(0, dtype=torch.uint8).set_(raw)
    start = view.data_ptr() - whole.data_ptr()
    return whole, start


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("shape,dtype,offset", SHAPES)
def test_guards_trip_on_either_side_and_only_there(shape, dtype, offset, fill):
    view, check = guarded(shape, dtype, "cpu", fill, offset_bytes=offset)
    assert tuple(view.shape) == shape and view.dtype == dtype and view.is_contiguous()
    assert (not view.numel() or view.data_ptr() % 512 == offset) and holds_fill(view, fill)
    itemsize, nbytes = view.element_size(), view.numel() * view.element_size()
    if not view.numel():
        return check()
    whole, start = _neighbours(view)
    row = itemsize * int(np.prod(shape[1:]))
    assert start >= max(MIN_GUARD, row) and whole.numel() - start - nbytes >= max(MIN_GUARD, row)
    assert holds_fill(whole, fill)
    check()
    other = np.uint8(fill ^ 0x21)
    # everything inside the view may be written
    whole[start:start + nbytes] = int(other)
    assert not nbytes or not holds_fill(view, fill)
    check()
    # one element in front
    whole[start - itemsize:start] = int(other)
    with pytest.raises(AssertionError, match="IN FRONT"):
        check("out")
    whole[start - itemsize:start] = fill
    check()
    # one element behind
    whole[start + nbytes:start + nbytes + itemsize] = int(other)
    with pytest.raises(AssertionError, match="BEHIND"):
        check("out")
    whole[start + nbytes:start + nbytes + itemsize] = fill
    check()
    # the far ends of both guards are guards too
    whole[0] = int(other)
    with pytest.raises(AssertionError, match="IN FRONT"):
        check()
    whole[0] = fill
    whole[-1] = int(other)
    with pytest.raises(AssertionError, match="BEHIND"):
        check()


def test_a_write_through_the_view_one_past_its_end_is_seen():
    """The way a kernel would do it: index arithmetic on the view's own pointer."""
    view, check = guarded((4, 6), torch.float64, "cpu", 0x55)
    flat = torch.empty(0, dtype=torch.float64).set_(view.untyped_storage(), view.storage_offset(), (view.numel() + 1,))
    flat[view.numel()] = 1.0
    with pytest.raises(AssertionError, match="BEHIND.* 0 to 7 bytes past"):
        check("acc")
    flat[view.numel()] = float(np.frombuffer(b"\x55" * 8, dtype=np.float64)[0])
    check()
    before = torch.empty(0, dtype=torch.float64).set_(view.untyped_storage(), view.storage_offset() - 1, (1,))
    before[0] = 1.0
    with pytest.raises(AssertionError, match="IN FRONT.* 8 to 1 bytes before"):
        check("acc")


def test_fills_and_offsets_are_checked():
    with pytest.raises(AssertionError):
        guarded((4,), torch.int32, "cpu", 0xAD)        # a byte of the strip pipeline's "not yet written" pattern
    with pytest.raises(AssertionError):
        guarded((4,), torch.float64, "cpu", 0x00, offset_bytes=4)   # below the natural alignment
    a = np.array([0.0, -0.0, np.nan])
    assert same_bytes(a, a.copy()) and not same_bytes(a, np.array([0.0, 0.0, np.nan]))
    assert not same_bytes(a, a.astype(np.float32))
