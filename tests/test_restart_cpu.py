"""rts_otw_restart / rts_wtw_restart / rts_live_restart without a GPU: the symbols exist with the header's signatures, and
the argument checks that come before the first HIP call answer RTS_ERR_INVALID with a message."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rts_otw_restart", "rts_wtw_restart", "rts_live_restart")


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as ge
    ge.build()
    from real_time_audio_sync_amd import _native
    return _native


def test_header_declares_the_three_entry_points():
    txt = open(os.path.join(ROOT, "include", "rtsync.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, handle in zip(NAMES, ("rts_otw", "rts_wtw", "rts_live")):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, name
        args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
        assert args == ["%s *h" % handle, "const uint8_t *mask_host", "const long long *first_host",
                        "const int32_t *len_host", "void *stream"], (name, args)


def test_symbols_are_exported_and_bound(nat):
    lib = ctypes.CDLL(nat.SO_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        fn = nat.EXPORTS[name]
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 5, name
    assert nat.lib.rts_version() == 101


def test_null_handle_and_null_mask_are_refused(nat):
    mask = (ctypes.c_uint8 * 4)(1, 0, 0, 1)
    not_a_handle = ctypes.create_string_buffer(4096)    # the mask is checked before the handle is looked at
    for name in NAMES:
        fn = nat.EXPORTS[name]
        nat.lib.rts_otw_set_waves(None, 4)               # leaves another message behind
        assert fn(None, mask, None, None, None) == -1, name
        msg = nat.lib.rts_last_error()
        assert msg and b"handle" in msg, (name, msg)
        assert fn(not_a_handle, None, None, None, None) == -1, name
        msg = nat.lib.rts_last_error()
        assert msg and b"mask" in msg, (name, msg)
