"""Guarded buffers for the entry points that write into caller-owned memory (tests/test_caller_memory_gpu.py).

``guarded(shape, dtype, device, fill)`` places a tensor inside a larger allocation that holds the byte ``fill``
everywhere -- inside the tensor too, so a call starts from known, non-zero contents -- and returns it with a ``check``
that asserts every byte in front of and behind it is still ``fill``.  The library's own "not yet written" patterns
(``sdp::kSentinel`` / ``kSentinel32``, csrc/sdp.h) are refused as fills: a consumer of the strip pipeline would take
them for a word that has not arrived and poll up to its bound."""
import numpy as np
import torch

# The only fills: all zeros, all ones (NaN as a float, -1 as an integer) and 0x55 (a large finite double, a positive
# int32).  Nothing that spells sdp::kSentinel = 0x7FF4DEAD7FF4DEAD or kSentinel32 = 0x7FF4DEAD belongs here.
FILLS = (0x00, 0xFF, 0x55)
MIN_GUARD = 4096
_ALIGN = 512   # where the view starts with offset_bytes = 0, whatever the allocator returned


def guarded(shape, dtype, device, fill, offset_bytes=0):
    """-> (view, check).  ``view``: a contiguous tensor of ``shape`` / ``dtype`` on ``device`` whose bytes are all
    ``fill``, at an address that is ``offset_bytes`` modulo 512 (a multiple of the element size).  In front of it and
    behind it lie guards of max(4096, bytes of one row) bytes each, a row being everything but the leading dimension
    (``view[0]``): more than any 256-byte rounding slack and more than one row of a strip.  ``check()`` asserts that
    both guards still hold ``fill`` and says which side was written and how far from the view."""
    fill = int(fill)
    assert fill in FILLS, "fill 0x%02X is not one of FILLS" % fill
    shape = tuple(int(s) for s in shape)
    itemsize = torch.empty((), dtype=dtype).element_size()
    assert offset_bytes >= 0 and offset_bytes % itemsize == 0, "offset_bytes must keep the natural alignment"
    nbytes = itemsize * int(np.prod(shape, dtype=np.int64))
    row = itemsize * int(np.prod(shape[1:], dtype=np.int64))
    guard = -(-max(MIN_GUARD, row) // _ALIGN) * _ALIGN
    raw = torch.full((guard + _ALIGN + offset_bytes + nbytes + guard,), fill, dtype=torch.uint8, device=device)
    start = guard + (-(raw.data_ptr() + guard)) % _ALIGN + offset_bytes
    view = raw[start:start + nbytes].view(dtype).view(shape)
    assert nbytes == 0 or (view.data_ptr() == raw.data_ptr() + start and view.data_ptr() % _ALIGN == offset_bytes % _ALIGN)

    def check(what="buffer"):
        front, behind = raw[:start], raw[start + nbytes:]
        assert front.numel() >= guard and behind.numel() >= guard
        hit = torch.nonzero(front != fill)
        if hit.numel():
            first, last = int(hit[0]), int(hit[-1])
            raise AssertionError("%s: %d guard bytes IN FRONT of the view were written, %d to %d bytes before its start"
                                 % (what, hit.numel(), start - first, start - last))
        hit = torch.nonzero(behind != fill)
        if hit.numel():
            first, last = int(hit[0]), int(hit[-1])
            raise AssertionError("%s: %d guard bytes BEHIND the view were written, %d to %d bytes past its end"
                                 % (what, hit.numel(), first, last))

    return view, check


def holds_fill(a, fill):
    """True if every byte of ``a`` (numpy array or tensor, any dtype) is ``fill``."""
    if torch.is_tensor(a):
        a = a.contiguous().cpu().numpy()
    return bool((np.ascontiguousarray(a).reshape(-1).view(np.uint8) == fill).all())


def same_bytes(a, b):
    """Bit-for-bit equality of two numpy arrays of one shape and dtype (NaN payloads and signed zeros included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
