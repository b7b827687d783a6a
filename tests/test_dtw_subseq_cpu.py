"""rts_dtw_subseq_paths (subsequence DTW with paths, csrc/dtw.hip) without a GPU: the SERIAL RESTATEMENT of its contract
-- tests/dtw_subseq_model.py, which tests/test_dtw_subseq_gpu.py compares the kernels with bit for bit -- is itself pinned
to the restatement of rts_locate (tests/test_locate_cpu.py::locate_ref) and to the DTW oracle; the entry point exists at
every layer with the header's signature, and its argument checks answer before the first HIP call."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from dtw_subseq_model import dot_cost, path_cost, planted, subseq_from_cost
from test_locate_cpu import locate_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (M excerpt frames, N piece frames): one cell, one row, one column, N < M, both sides of the 64-row strip boundary,
# three strips against a piece that is no multiple of anything
SHAPES = [(1, 1), (1, 9), (7, 1), (5, 3), (63, 64), (64, 129), (65, 300), (130, 257)]


def _pair(M, N, seed):
    from real_time_audio_sync_amd import synth
    ref = synth.synth_ref(N, seed=seed)
    q = synth.synth_live(synth.synth_ref(M + 8, seed=seed + 1), seed=seed + 2)[:, :M]
    assert q.shape[1] == M
    return q, ref


@pytest.fixture(scope="module")
def cases():
    """{(M, N): (a, b, C, model result)}, computed once."""
    out = {}
    for M, N in SHAPES:
        a, b = _pair(M, N, 2000 + 7 * M + N)
        C = dot_cost(a, b)
        out[(M, N)] = (a, b, C, subseq_from_cost(C))
    return out


@pytest.mark.parametrize("M,N", SHAPES)
def test_model_equals_the_locate_restatement(cases, M, N):
    _, _, C, (path, total, start, end, row) = cases[(M, N)]
    cost, lend, lstart, D, _ = locate_ref(C)
    assert (total, end, start) == (cost, lend, lstart)
    assert row.dtype == np.float64 and np.array_equal(row.view(np.int64), D.view(np.int64))


@pytest.mark.parametrize("M,N", SHAPES)
def test_model_total_is_plain_dtw_of_the_reported_range(cases, M, N):
    import oracle.binding as ob
    a, b, _, (_, total, start, end, _) = cases[(M, N)]
    assert 0 <= start <= end < N
    assert total == ob.dtw(a, b[:, start:end + 1])[1][-1, -1]


@pytest.mark.parametrize("M,N", SHAPES)
def test_model_path_shape_and_cost(cases, M, N):
    _, _, C, (path, total, start, end, row) = cases[(M, N)]
    assert path.dtype == np.int32 and path.ndim == 2 and path.shape[1] == 2
    assert tuple(path[0]) == (0, start) and tuple(path[-1]) == (M - 1, end)
    assert (path[1:, 0] > 0).all()                                   # row 0 is left at once: the walk stops on it
    steps = {tuple(d) for d in np.diff(path, axis=0)}
    assert steps <= {(0, 1), (1, 0), (1, 1)}, steps
    assert path_cost(C, path) == total
    assert total == row[end] and end == int(np.argmin(row))
    assert 1 <= len(path) <= M + N


# The planted case: frames [A, A + L) of a 300-frame piece with noise 0.03, L = 64.  The piece holds every chord for 2 to
# 11 frames, so an end of the match may slide along a held chord at next to no cost.  What the model reports on the CPU for
# the three placements below (printed by the test): start - A = +3, 0, +2 and end - (A + L - 1) = -3, -4, -2.  The
# tolerance is 8 frames, twice the model's largest deviation and the one test_locate_cpu's planted case uses; it does not
# come from any kernel.
PLANT_N, PLANT_L, PLANT_TOL = 300, 64, 8


@pytest.mark.parametrize("A", [0, 117, PLANT_N - PLANT_L], ids=["front", "middle", "back"])
def test_planted_excerpt_is_found_where_it_was_planted(A):
    q, piece = planted(PLANT_N, A, PLANT_L, seed=800)
    path, total, start, end, _ = subseq_from_cost(dot_cost(q, piece))
    print("A = %d: start - A = %d, end - (A + L - 1) = %d, total %.6f" % (A, start - A, end - (A + PLANT_L - 1), total))
    assert abs(start - A) <= PLANT_TOL and abs(end - (A + PLANT_L - 1)) <= PLANT_TOL, (start, end)
    # the path stays near the plant's diagonal all the way
    assert (np.abs(path[:, 1] - (A + path[:, 0])) <= PLANT_TOL).all()


# ---- the ABI --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as ge
    ge.build()
    from real_time_audio_sync_amd import _native
    return _native


ARGS = ["const void *a_dev", "int a_dtype", "long long a_stride", "const int32_t *a_len_dev", "const void *b_dev",
        "int b_dtype", "long long b_stride", "const int32_t *b_len_dev", "int F", "int M_max", "int N_max", "int B",
        "int32_t *path_dev", "int32_t *path_len_dev", "double *total_dev", "int32_t *start_dev", "int32_t *end_dev",
        "double *row_dev", "void *ws_dev", "size_t ws_bytes", "void *stream"]
NAMES = [a.split()[-1].lstrip("*") for a in ARGS]


def test_header_declares_library_exports_binding_lists(nat):
    txt = open(os.path.join(ROOT, "include", "rtsync.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+rts_dtw_subseq_paths_workspace_bytes\s*\(\s*int M_max,\s*int N_max,\s*int B,\s*size_t \*bytes\s*\)\s*;", code)
    m = re.search(r"\bint\s+rts_dtw_subseq_paths\s*\(([^)]*)\)\s*;", code)
    assert m, "include/rtsync.h does not declare rts_dtw_subseq_paths"
    assert [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")] == ARGS
    assert "dtw.py:32-52" in txt and "tests.py:199-262" in txt
    lib = ctypes.CDLL(nat.SO_PATH)
    for sym in ("rts_dtw_subseq_paths_workspace_bytes", "rts_dtw_subseq_paths"):
        assert hasattr(lib, sym), "librtsync.so does not export %s" % sym
        assert sym in nat.EXPORTS and nat.EXPORTS[sym].restype is ctypes.c_int, sym
    assert len(nat.EXPORTS["rts_dtw_subseq_paths"].argtypes) == len(ARGS)
    assert len(nat.EXPORTS["rts_dtw_subseq_paths_workspace_bytes"].argtypes) == 4


def test_python_entry_points(nat):
    import torch
    from real_time_audio_sync_amd import dtw
    sig = inspect.signature(dtw.dtw_subseq_paths)
    assert list(sig.parameters) == ["a_dev", "b_dev", "a_len", "b_len", "want_row", "check"]
    assert [sig.parameters[k].default for k in ("a_len", "b_len", "want_row", "check")] == [None, None, False, False]
    sig = inspect.signature(dtw.align_excerpts)
    assert list(sig.parameters) == ["excerpts", "pieces", "device", "dtype"]
    assert sig.parameters["device"].default == "cuda:0" and sig.parameters["dtype"].default == torch.float64
    # the existing entry points keep their signatures
    assert list(inspect.signature(dtw.dtw_paths).parameters) == ["a_dev", "b_dev", "a_len", "b_len", "check"]
    assert list(inspect.signature(dtw.align_pairs).parameters) == ["seqs_a", "seqs_b", "device", "dtype"]


def test_workspace_is_the_path_only_calls(nat):
    for M, N, B in ((1, 1, 1), (769, 700, 9), (19380, 19380, 1)):
        a, b = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert nat.lib.rts_dtw_subseq_paths_workspace_bytes(M, N, B, ctypes.byref(a)) == 0
        assert nat.lib.rts_dtw_paths_workspace_bytes(M, N, B, ctypes.byref(b)) == 0
        assert a.value == b.value > 0
    size = ctypes.c_size_t(0)
    assert nat.lib.rts_dtw_subseq_paths_workspace_bytes(0, 90, 2, ctypes.byref(size)) == -1
    assert b"M_max" in nat.lib.rts_last_error()
    assert nat.lib.rts_dtw_subseq_paths_workspace_bytes(100, 90, 2, None) == -1 and b"bytes" in nat.lib.rts_last_error()


def test_argument_errors_come_before_any_hip_call(nat):
    INVALID, UNSUPPORTED = -1, -2
    nbytes = ctypes.c_size_t(0)
    nat.check(nat.lib.rts_dtw_subseq_paths_workspace_bytes(100, 90, 2, ctypes.byref(nbytes)))
    P = ctypes.c_void_p     # never dereferenced: every call below is refused on the host
    good = dict(a_dev=P(4096), a_dtype=nat.F32, a_stride=100, a_len_dev=None, b_dev=P(8192), b_dtype=nat.F32, b_stride=90,
                b_len_dev=None, F=12, M_max=100, N_max=90, B=2, path_dev=P(12288), path_len_dev=P(16384),
                total_dev=P(20480), start_dev=P(24576), end_dev=P(28672), row_dev=None, ws_dev=P(1 << 20),
                ws_bytes=nbytes.value, stream=None)
    assert NAMES == list(good)

    def call(**kw):
        nat.lib.rts_otw_set_waves(None, 4)    # leaves another message behind
        v = dict(good, **kw)
        rc = nat.lib.rts_dtw_subseq_paths(*[v[n] for n in NAMES])
        return rc, nat.lib.rts_last_error()

    for ptr in ("a_dev", "b_dev", "path_dev", "path_len_dev", "total_dev", "start_dev", "end_dev", "ws_dev"):
        rc, msg = call(**{ptr: None})
        assert rc == INVALID and ptr.encode() in msg, (ptr, rc, msg)
    rc, msg = call(a_stride=99)
    assert rc == INVALID and b"a_stride" in msg, msg
    rc, msg = call(b_stride=1)
    assert rc == INVALID and b"b_stride" in msg, msg
    rc, msg = call(F=13)
    assert rc == UNSUPPORTED and b"F" in msg and b"12" in msg, msg
    rc, msg = call(B=0)
    assert rc == INVALID and b"B" in msg, msg
    rc, msg = call(M_max=0)
    assert rc == INVALID and b"M_max" in msg, msg
    rc, msg = call(B=65536)
    assert rc == INVALID and b"65535" in msg, msg
    rc, msg = call(ws_bytes=nbytes.value - 1)
    assert rc == INVALID and b"workspace" in msg and b"rts_dtw_subseq_paths_workspace_bytes" in msg, msg
    rc, msg = call(ws_dev=P((1 << 20) + 8))
    assert rc == INVALID and b"16-byte aligned" in msg, msg


def test_product_does_not_import_the_oracle():
    for fn in ("dtw.py", "csrc/dtw.hip", "csrc/sdp.h", "csrc/sdp_plan.h"):
        src = open(os.path.join(ROOT, "real_time_audio_sync_amd", fn)).read()
        assert "import oracle" not in src and "from oracle" not in src and "liboracle" not in src, fn
