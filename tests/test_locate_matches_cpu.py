"""rts_locate_matches (ranked non-overlapping matches per piece, csrc/locate.hip) without a GPU: the entry points exist
with the header's signature, their argument checks answer before the first HIP call, the workspace has the stated size,
and the serial restatement tests/locate_matches_model.py -- which tests/test_locate_matches_gpu.py compares the kernels
with using ``==`` -- has the properties the contract promises, on rows ``locate_ref`` builds from the oracle's own cost.
``locate.nearest_to`` is plain Python and is checked here on hand-made lists."""
import ctypes
import os
import re

import numpy as np
import pytest

from locate_matches_model import matches_ref, matches_serial, repeat_case, slots
from test_locate_cpu import ARGS as LOCATE_ARGS, SHAPES, _pair, dot_cost, euclid_cost, locate_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# rts_locate's arguments from queries_dev through cost_kind, unchanged, then the new ones
ARGS = LOCATE_ARGS[:13] + ["int K", "double max_cost", "double *cost_dev", "int32_t *end_dev", "int32_t *start_dev",
                           "int32_t *n_dev", "void *ws_dev", "size_t ws_bytes", "void *stream"]
WS_ARGS = ["int B", "long long n_pool_frames", "size_t *bytes"]


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as ge
    ge.build()
    from real_time_audio_sync_amd import _native
    return _native


def _ws_bytes(B, n_pool):
    """The header's formula: 256 to align any ws_dev, rows double [B][n_pool] and starts int32 [B][n_pool], each rounded
    up to 256."""
    up = lambda n: -(-n // 256) * 256
    return 256 + up(8 * B * n_pool) + up(4 * B * n_pool)


def test_header_declares_exports_and_binding(nat):
    txt = open(os.path.join(ROOT, "include", "rtsync.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    so = ctypes.CDLL(nat.SO_PATH)
    for name, args in (("rts_locate_matches", ARGS), ("rts_locate_matches_workspace_bytes", WS_ARGS)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, "include/rtsync.h does not declare %s" % name
        assert [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")] == args
        assert hasattr(so, name)
        fn = nat.EXPORTS[name]
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(args)
    import real_time_audio_sync_amd as pkg
    from real_time_audio_sync_amd import locate
    assert pkg.locate_matches is locate.locate_matches and callable(locate.nearest_to)


def test_workspace_size_is_the_stated_value(nat):
    n = ctypes.c_size_t()
    for B, n_pool in ((1, 1), (1, 19380), (3, 777), (64, 64 * 2200), (65535, 1 << 20)):
        assert nat.lib.rts_locate_matches_workspace_bytes(B, n_pool, ctypes.byref(n)) == 0
        assert n.value == _ws_bytes(B, n_pool), (B, n_pool)
        assert 12 * B * n_pool <= n.value < 12 * B * n_pool + 3 * 256
    for B, n_pool in ((0, 10), (65536, 10), (1, 0)):
        assert nat.lib.rts_locate_matches_workspace_bytes(B, n_pool, ctypes.byref(n)) == -1
    assert nat.lib.rts_locate_matches_workspace_bytes(1, 10, None) == -1


def test_argument_errors_come_before_any_hip_call(nat):
    p = ctypes.c_void_p(4096)   # never dereferenced: every call below is refused on the host
    good = dict(queries_dev=p, q_dtype=nat.F32, M_max=64, q_len_dev=None, B=2, pool_dev=p, pool_dtype=nat.F32, F=12,
                n_pool_frames=100, piece_first_dev=p, piece_len_dev=p, P=3, cost_kind=nat.COST_DOT, K=4,
                max_cost=float("inf"), cost_dev=p, end_dev=p, start_dev=p, n_dev=p, ws_dev=p, ws_bytes=_ws_bytes(2, 100),
                stream=None)
    names = [a.split()[-1].lstrip("*") for a in ARGS]
    assert names == list(good)

    def call(**kw):
        nat.lib.rts_otw_set_waves(None, 4)    # leaves another message behind
        a = dict(good, **kw)
        rc = nat.lib.rts_locate_matches(*[a[n] for n in names])
        return rc, nat.lib.rts_last_error()

    for ptr in ("queries_dev", "pool_dev", "piece_first_dev", "piece_len_dev", "cost_dev", "end_dev", "start_dev", "n_dev",
                "ws_dev"):
        rc, msg = call(**{ptr: None})
        assert rc == -1 and ptr.encode() in msg, (ptr, rc, msg)
    rc, msg = call(K=0)
    assert rc == -1 and b"K " in msg, (rc, msg)
    rc, msg = call(K=33)
    assert rc == -2 and b"K " in msg, (rc, msg)
    rc, msg = call(max_cost=float("nan"))
    assert rc == -1 and b"max_cost" in msg, (rc, msg)
    rc, msg = call(ws_bytes=_ws_bytes(2, 100) - 1)
    assert rc == -1 and b"ws_bytes" in msg, (rc, msg)
    # rts_locate's own limits and errors
    rc, msg = call(M_max=0)
    assert rc == -1 and b"M_max" in msg, (rc, msg)
    rc, msg = call(M_max=257)
    assert rc == -2 and b"M_max" in msg, (rc, msg)
    rc, msg = call(F=13)
    assert rc == -2 and b"12" in msg and b"F " in msg, (rc, msg)
    for arg, bad in (("q_dtype", 2), ("pool_dtype", 7), ("cost_kind", 2), ("P", 0), ("P", 65536), ("B", 0), ("B", 65536),
                     ("n_pool_frames", 0)):
        rc, msg = call(**{arg: bad})
        assert rc == -1 and arg.encode() in msg, (arg, rc, msg)


def _disjoint(ranks):
    spans = sorted((s, e) for _, e, s in ranks)
    return all(s <= e for s, e in spans) and all(a[1] < b[0] for a, b in zip(spans, spans[1:]))


@pytest.mark.parametrize("M,N", SHAPES)
def test_model_properties_on_the_restatements_rows(M, N):
    q, ref = _pair(M, N, 1000 + 7 * M + N)
    for cost_fn in (dot_cost, euclid_cost):
        cost, end, start, D, S = locate_ref(cost_fn(q, ref))
        for K in (1, 3, 32):
            ranks = matches_ref(D, S, K)
            assert ranks == matches_serial(D, S, K)
            assert 1 <= len(ranks) <= K
            assert ranks[0] == (cost, end, start)                       # rank 0 is rts_locate's answer
            assert _disjoint(ranks)
            assert [c for c, _, _ in ranks] == sorted(c for c, _, _ in ranks)
            assert all(D[e] == c and S[e] == s for c, e, s in ranks)
        if M == 1:      # every range is one column: the K cheapest columns in stable order
            order = sorted(range(N), key=lambda j: (D[j], j))
            assert [e for _, e, _ in matches_ref(D, S, 3)] == order[:3]
            assert len(matches_ref(D, S, 32)) == min(N, 32)
        # a cut-off between two ranks ends the list there; one below rank 0 empties it
        ranks = matches_ref(D, S, 32)
        if len(ranks) > 1 and ranks[1][0] > ranks[0][0]:
            assert matches_ref(D, S, 32, max_cost=ranks[0][0]) == ranks[:1]
        assert matches_ref(D, S, 32, max_cost=np.nextafter(ranks[0][0], -np.inf)) == []
        assert matches_ref(D, S, 32, max_cost=ranks[0][0])[:1] == ranks[:1]      # cost == max_cost stays


def test_model_skips_non_finite_columns_and_fills_slots():
    D = np.array([np.nan, 3.0, np.inf, 1.0, 1.0, -np.inf, 2.0])
    S = np.array([0, 1, 2, 3, 4, 5, 5], dtype=np.int32)
    ranks = matches_ref(D, S, 8)
    assert ranks == matches_serial(D, S, 8) == [(1.0, 3, 3), (1.0, 4, 4), (2.0, 6, 5), (3.0, 1, 1)]
    c, e, s, n = slots(ranks, 8)
    assert n == 4 and np.isposinf(c[4:]).all() and (e[4:] == -1).all() and (s[4:] == -1).all()
    # a column whose own range reaches back into a taken one is suppressed although its end lies outside
    assert matches_ref([5.0, 1.0, 2.0], [0, 0, 1], 3) == [(1.0, 1, 0)]


def test_repeated_section_is_found_three_times():
    """The case of the issue with the oracle's cost: an excerpt of A in A | B | A | C | A."""
    piece, q, copies = repeat_case()
    cost, end, start, D, S = locate_ref(dot_cost(q, piece))
    ranks = matches_ref(D, S, 8)
    assert len(ranks) >= 4 and ranks[0] == (cost, end, start)
    three = sorted(ranks[:3], key=lambda r: r[2])
    for (c, e, s), at in zip(three, copies):
        assert abs(s - (at + 4)) <= 8 and abs(e - (at + 43)) <= 8, (s, e, at)
    assert ranks[0][0] == ranks[1][0] == ranks[2][0]
    assert [s for _, _, s in ranks[:3]] == sorted(s for _, _, s in ranks[:3])    # equal costs: ascending columns
    assert ranks[3][0] > 10 * ranks[2][0], ranks[:4]
    # what rts_locate alone reports is the first pass
    assert abs(start - 4) <= 8


def test_nearest_to_on_hand_made_lists():
    from real_time_audio_sync_amd.locate import Candidates, nearest_to
    pa, pb = object(), object()
    M = 40
    # three passes of a repeat on pa (the second and third a little dearer per step), one poor match on pb
    cand = [(pa, 10, 42, 7.30), (pa, 128, 160, 7.31), (pa, 231, 263, 7.40), (pb, 5, 60, 30.0)]
    step = [c / (M + e - s + 1) for _, s, e, c in cand]
    # slack 0: only the best per step is considered, wherever the stream was
    assert nearest_to({0: (pa, 230)}, 0.0, M=M)(0, cand) == 0
    # a slack that admits all three copies: the nearest start wins
    slack = step[2] - step[0]
    assert nearest_to({0: (pa, 230)}, slack, M=M)(0, cand) == 2
    assert nearest_to({0: (pa, 140)}, slack, M=M)(0, cand) == 1
    assert nearest_to({0: (pa, 0)}, slack, M=M)(0, cand) == 0
    # a slack that admits two of them: the third is out although it is the nearest
    assert nearest_to({0: (pa, 230)}, step[1] - step[0], M=M)(0, cand) == 1
    # where on another piece: its candidate is not within the slack -> the overall best; within -> that candidate
    assert nearest_to({0: (pb, 5)}, slack, M=M)(0, cand) == 0
    assert nearest_to({0: (pb, 5)}, step[3] - step[0], M=M)(0, cand) == 3
    # a stream `where` does not name, a piece nobody found, an empty list
    assert nearest_to({1: (pa, 230)}, slack, M=M)(0, cand) == 0
    assert nearest_to({0: (object(), 230)}, slack, M=M)(0, cand) == 0
    assert nearest_to({0: (pa, 230)}, slack, M=M)(0, []) is None
    # the excerpt's length comes with reacquire's lists; without either it is an error
    own = Candidates(cand)
    own.M = M
    assert nearest_to({0: (pa, 230)}, slack)(0, own) == 2
    with pytest.raises(ValueError):
        nearest_to({0: (pa, 230)}, slack)(0, cand)
