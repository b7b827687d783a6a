"""rts_otw_create_refs / rts_wtw_create_refs (one reference per stream): every argument is checked before the first HIP
call, so the error codes and messages are the same on a machine without a GPU."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as ge
    ge.build()
    from real_time_audio_sync_amd import _native
    return _native


FAKE = ctypes.c_void_p(4096)  # never dereferenced: every call below fails its argument checks first


def _tables(first, lens):
    return np.array(first, dtype=np.int64), np.array(lens, dtype=np.int32)


def _otw(nat, refs=FAKE, F=12, n_ref=100, first=(0, 40, 40), lens=(40, 60, 10), c=50, tables=True):
    f, l = _tables(first, lens)
    h = ctypes.c_void_p()
    rc = nat.lib.rts_otw_create_refs(refs, nat.F32, F, n_ref, f.ctypes.data if tables else None,
                                     l.ctypes.data if tables else None, len(lens), c, 3, nat.VARIANT_OTW, nat.COST_DOT,
                                     ctypes.byref(h))
    assert not h.value  # nothing left behind on failure
    return rc, nat.lib.rts_last_error().decode()


def _wtw(nat, refs=FAKE, F=12, n_ref=100, first=(0, 40, 40), lens=(40, 60, 10), W=20, tables=True):
    f, l = _tables(first, lens)
    h = ctypes.c_void_p()
    rc = nat.lib.rts_wtw_create_refs(refs, F, n_ref, f.ctypes.data if tables else None,
                                     l.ctypes.data if tables else None, len(lens), W, 10, 0, ctypes.byref(h))
    assert not h.value
    return rc, nat.lib.rts_last_error().decode()


@pytest.mark.parametrize("kind", ["otw", "wtw"])
def test_create_refs_argument_errors(nat, kind):
    make = _otw if kind == "otw" else _wtw
    rc, msg = make(nat, refs=None)
    assert rc == -1 and "refs_dev is NULL" in msg
    rc, msg = make(nat, tables=False)
    assert rc == -1 and "NULL" in msg
    rc, msg = make(nat, F=13)
    assert rc == -2 and "12" in msg
    if kind == "otw":
        rc, msg = make(nat, c=2037)
        assert rc == -2 and "2037" in msg
    else:
        rc, msg = make(nat, W=16385)
        assert rc == -2 and "16384" in msg
    rc, msg = make(nat, lens=(40, 0, 10))
    assert rc == -1 and "stream 1" in msg and "len" in msg
    rc, msg = make(nat, first=(0, 40, -1))
    assert rc == -1 and "stream 2" in msg and "first" in msg
    rc, msg = make(nat, first=(0, 41, 40))                 # 41 + 60 > 100
    assert rc == -1 and "stream 1" in msg and "100" in msg
    rc, msg = make(nat, n_ref=49, first=(0, 0, 40), lens=(40, 40, 10))   # 40 + 10 > 49: the last stream
    assert rc == -1 and "stream 2" in msg


def test_create_refs_valid_arguments_pass_the_checks(nat):
    """Valid tables (overlapping and repeated ranges) pass every check: without a GPU the first HIP call is what fails,
    with one the handle is made (the reference is held, not read) and destroyed again."""
    f, l = _tables((0, 40, 40, 0), (40, 60, 10, 40))
    for kind in ("otw", "wtw"):
        h = ctypes.c_void_p()
        if kind == "otw":
            rc = nat.lib.rts_otw_create_refs(FAKE, nat.F32, 12, 100, f.ctypes.data, l.ctypes.data, 4, 50, 3,
                                             nat.VARIANT_OTW, nat.COST_DOT, ctypes.byref(h))
        else:
            rc = nat.lib.rts_wtw_create_refs(FAKE, 12, 100, f.ctypes.data, l.ctypes.data, 4, 20, 10, 0, ctypes.byref(h))
        assert rc in (0, -3, -4), nat.lib.rts_last_error()
        assert (rc == 0) == bool(h.value)
        if h.value:
            (nat.lib.rts_otw_destroy if kind == "otw" else nat.lib.rts_wtw_destroy)(h)


def test_create_refs_exports(nat):
    assert "rts_otw_create_refs" in nat.EXPORTS and "rts_wtw_create_refs" in nat.EXPORTS


BAD_TABLES = [dict(lens=(40, 0, 10)),                                  # len 0
              dict(first=(0, 40, -1)),                                 # first -1
              dict(first=(0, 41, 40)),                                 # 41 + 60 > 100
              dict(n_ref=49, first=(0, 0, 40), lens=(40, 40, 10))]     # the last stream past a 49-frame pool


@pytest.mark.parametrize("bad", BAD_TABLES)
def test_create_refs_one_rule_one_text(nat, bad):
    """Both trackers check the ranges with one routine: a bad table draws the same message from either."""
    rc_o, msg_o = _otw(nat, **bad)
    rc_w, msg_w = _wtw(nat, **bad)
    assert rc_o == rc_w == -1
    assert msg_o == msg_w and msg_o.startswith("stream ")


@pytest.mark.parametrize("kind", ["otw", "wtw"])
def test_create_refs_range_ending_at_the_pool_end_is_valid(nat, kind):
    """first == n_ref_frames - len (the last stream's range ends with the pool) passes the range check.  As in
    test_create_refs_valid_arguments_pass_the_checks a handle may come into being where a GPU is present."""
    f, l = _tables((0, 40, 90), (40, 60, 10))
    h = ctypes.c_void_p()
    if kind == "otw":
        rc = nat.lib.rts_otw_create_refs(FAKE, nat.F32, 12, 100, f.ctypes.data, l.ctypes.data, 3, 50, 3,
                                         nat.VARIANT_OTW, nat.COST_DOT, ctypes.byref(h))
    else:
        rc = nat.lib.rts_wtw_create_refs(FAKE, 12, 100, f.ctypes.data, l.ctypes.data, 3, 20, 10, 0, ctypes.byref(h))
    assert rc in (0, -3, -4), nat.lib.rts_last_error()
    assert (rc == 0) == bool(h.value)
    if h.value:
        (nat.lib.rts_otw_destroy if kind == "otw" else nat.lib.rts_wtw_destroy)(h)
