"""rts_locate_matches on the GPU (csrc/locate.hip; locate.locate_matches, BatchedOTW.locate / reacquire with ``matches``):
cost, end, start and n are compared with ``==`` against the serial restatement tests/locate_matches_model.py (only
compares of doubles the locate kernel wrote: no tolerance).

The restatement works on the last row (D, S) of rts_locate.  In the shape sweep that row is read from rts_locate itself
(``locate_batch(want_rows=True)``, which tests/test_locate_gpu.py pins to ``locate_ref`` bit for bit), so the sweep
checks the selection step at sizes where ``locate_ref`` in Python would take seconds; the repeat, tie and end-to-end
cases take their rows from ``locate_ref`` on the oracle's own cost.

Every call goes through ``_call``: outputs and workspace in guarded regions (tests/guarded.py), the call made twice with
two fill patterns in the workspace and the outputs, equal results and intact guards both times."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from guarded import guarded, same_bytes  # noqa: E402
from locate_matches_model import matches_ref, repeat_case, slots  # noqa: E402
from test_locate_cpu import dot_cost, euclid_cost, locate_ref  # noqa: E402

DEV = "cuda:0"
# one column; N < K; either side of a wave; no multiples of the workgroup of 256; more than one pass per lane -- laid
# out in the pool behind a gap of 7 frames each, the first one at frame 3
NS = [1, 5, 63, 64, 65, 257, 1000, 5000]
MS = [1, 64, 65, 130]
GAP = 7


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _frames(x, dtype):
    """(12, n) feature-major float64 (float32 values) -> device [n][12]."""
    return torch.from_numpy(np.ascontiguousarray(x.T)).to(dtype).to(DEV)


def _call(q, q_len, pool, first, lens, K, max_cost=float("inf"), euclid=False):
    """rts_locate_matches twice, fills 0xFF then 0x55 in outputs and workspace -> numpy (cost, end, start, n)."""
    from real_time_audio_sync_amd import _native as nat
    B, M_max, _ = q.shape
    P, n_pool = int(first.shape[0]), int(pool.shape[0])
    code = {torch.float32: nat.F32, torch.float64: nat.F64}
    nbytes = ctypes.c_size_t()
    nat.check(nat.lib.rts_locate_matches_workspace_bytes(B, n_pool, ctypes.byref(nbytes)))
    got = []
    for fill, off in ((0xFF, 0), (0x55, 8)):       # the second workspace is only 8-byte aligned
        cost, c0 = guarded((B, P, K), torch.float64, DEV, fill)
        end, c1 = guarded((B, P, K), torch.int32, DEV, fill)
        start, c2 = guarded((B, P, K), torch.int32, DEV, fill)
        n, c3 = guarded((B, P), torch.int32, DEV, fill)
        ws, c4 = guarded((nbytes.value,), torch.uint8, DEV, fill, offset_bytes=off)
        nat.check(nat.lib.rts_locate_matches(q.data_ptr(), code[q.dtype], M_max, q_len.data_ptr() if q_len is not None else None,
                                             B, pool.data_ptr(), code[pool.dtype], 12, n_pool, first.data_ptr(),
                                             lens.data_ptr(), P, nat.COST_EUCLID if euclid else nat.COST_DOT, K,
                                             float(max_cost), cost.data_ptr(), end.data_ptr(), start.data_ptr(),
                                             n.data_ptr(), ws.data_ptr(), nbytes.value,
                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        for chk, what in ((c0, "cost_dev"), (c1, "end_dev"), (c2, "start_dev"), (c3, "n_dev"), (c4, "ws_dev")):
            chk(what)
        got.append([t.cpu().numpy() for t in (cost, end, start, n)])
    for a, b, what in zip(got[0], got[1], ("cost", "end", "start", "n")):
        assert same_bytes(a, b), "%s depends on what the workspace or the outputs held before" % what
    return got[0]


def _assert_pair(got, b, p, ranks, K, n=None):
    cost, end, start, cnt = got
    ec, ee, es, en = slots(ranks, K)
    assert cnt[b, p] == (en if n is None else n), (b, p, cnt[b, p], en)
    assert same_bytes(cost[b, p], ec), (b, p, cost[b, p], ec)
    assert np.array_equal(end[b, p], ee) and np.array_equal(start[b, p], es), (b, p, end[b, p], ee, start[b, p], es)


@pytest.fixture(scope="module")
def sweep():
    from real_time_audio_sync_amd import synth
    first = np.cumsum([3] + [n + GAP for n in NS])[:-1].astype(np.int64)
    n_pool = int(first[-1]) + NS[-1] + GAP
    # a pool that repeats itself every 400 frames with a little noise: long pieces hold many near-equal matches
    base = synth.synth_ref(400, seed=81)
    pool = np.concatenate([base] * (n_pool // 400 + 1), axis=1)[:, :n_pool]
    pool = pool + 0.01 * np.random.RandomState(82).rand(12, n_pool)
    pool = (pool / np.sqrt((pool * pool).sum(axis=0, keepdims=True))).astype(np.float32).astype(np.float64)
    q = synth.synth_live(base, seed=83)[:, 20:20 + max(MS)]
    assert q.shape[1] == max(MS)
    return dict(pool=pool, q=q, first=first, rows={})


def _sweep_rows(sweep, dtype, euclid):
    """rts_locate's own answers and rows for the sweep's call, once per (dtype, cost kind)."""
    from real_time_audio_sync_amd.locate import locate_batch
    key = (dtype, euclid)
    if key not in sweep["rows"]:
        q = _frames(sweep["q"], torch.float64).unsqueeze(0).repeat(len(MS), 1, 1).contiguous()
        args = (q, torch.tensor(MS, dtype=torch.int32, device=DEV), _frames(sweep["pool"], dtype),
                torch.from_numpy(sweep["first"]).to(DEV), torch.tensor(NS, dtype=torch.int32, device=DEV))
        sweep["rows"][key] = (args, [t.cpu().numpy() for t in locate_batch(*args, euclid=euclid, want_rows=True)])
    return sweep["rows"][key]


@pytest.mark.parametrize("K", [1, 3, 8, 32])
@pytest.mark.parametrize("euclid", [False, True], ids=["dot", "euclid"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_every_piece_length_query_length_and_rank_count(sweep, dtype, euclid, K):
    args, (lc, le, ls, row, rowstart) = _sweep_rows(sweep, dtype, euclid)
    got = _call(*args, K, euclid=euclid)
    fewer = 0
    for b in range(len(MS)):
        for p, (f, n) in enumerate(zip(sweep["first"], NS)):
            ranks = matches_ref(row[b, f:f + n], rowstart[b, f:f + n], K)
            _assert_pair(got, b, p, ranks, K)
            # rank 0 is rts_locate's answer bit for bit
            assert (got[0][b, p, 0], got[1][b, p, 0], got[2][b, p, 0]) == (lc[b, p], le[b, p], ls[b, p]), (b, p)
            fewer += len(ranks) < K
            if MS[b] == 1:
                assert len(ranks) == min(n, K)
    if K == 8:
        assert got[3][0, 1] == 5 and fewer > 0          # N = 5 with K = 8: n < K
    if K == 32:
        assert (got[3] == 32).any(), "no pair fills all 32 ranks: the sweep is not what it is meant to be"


def _one_piece(piece, q, dtype=torch.float64):
    return (_frames(q, dtype).unsqueeze(0).contiguous(), None, _frames(piece, dtype),
            torch.zeros(1, dtype=torch.int64, device=DEV), torch.tensor([piece.shape[1]], dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("euclid", [False, True], ids=["dot", "euclid"])
def test_exact_copies_tie_and_come_in_ascending_column_order(euclid):
    """The same 30 frames three times in one piece, queried with exactly those frames: three ranks of one cost."""
    rs = np.random.RandomState(11)

    def rnd(n):
        x = rs.rand(12, n) ** 3
        return (x / np.sqrt((x * x).sum(axis=0, keepdims=True))).astype(np.float32).astype(np.float64)
    sec = rnd(30)
    piece = np.concatenate([rnd(50), sec, rnd(40), sec, rnd(20), sec, rnd(9)], axis=1)
    c, e, s, D, S = locate_ref((euclid_cost if euclid else dot_cost)(sec, piece))
    ranks = matches_ref(D, S, 5)
    assert [(r[1], r[2]) for r in ranks[:3]] == [(79, 50), (149, 120), (199, 170)]      # the input is the tie it is meant to be
    assert ranks[0][0] == ranks[1][0] == ranks[2][0] < ranks[3][0]
    got = _call(*_one_piece(piece, sec), 5, euclid=euclid)
    _assert_pair(got, 0, 0, ranks, 5)


def test_repeated_section_and_the_cut_off():
    piece, q, copies = repeat_case()
    c, e, s, D, S = locate_ref(dot_cost(q, piece))
    ranks = matches_ref(D, S, 8)
    assert len(ranks) >= 4 and ranks[2][0] < ranks[3][0]
    for dtype in (torch.float32, torch.float64):       # the values are float32 values: one expectation for both pools
        got = _call(*_one_piece(piece, q, dtype), 8)
        _assert_pair(got, 0, 0, ranks, 8)
        # max_cost between the third and the fourth rank, exactly the third's cost, just below rank 0
        between = 0.5 * (ranks[2][0] + ranks[3][0])
        _assert_pair(_call(*_one_piece(piece, q, dtype), 8, max_cost=between), 0, 0, ranks[:3], 8)
    _assert_pair(_call(*_one_piece(piece, q), 8, max_cost=ranks[2][0]), 0, 0, ranks[:3], 8)
    _assert_pair(_call(*_one_piece(piece, q), 8, max_cost=float(np.nextafter(ranks[0][0], -np.inf))), 0, 0, [], 8)
    _assert_pair(_call(*_one_piece(piece, q), 2, max_cost=between), 0, 0, ranks[:2], 2)


def _layout(pieces, K=3):
    """B = 3 streams (q_len 70, 17, 0) x the given P = 4 pieces of a 400-frame pool in one call -> (got, rows per
    stream and piece by locate_ref or None for the stream that heard nothing)."""
    from real_time_audio_sync_amd import synth
    n_pool, M_max, q_len = 400, 70, [70, 17, 0]
    poolh = synth.synth_ref(n_pool, seed=51)
    qh = [synth.synth_live(synth.synth_ref(90, seed=52 + b), seed=60 + b)[:, :M_max] for b in range(3)]
    q = torch.stack([_frames(x, torch.float32) for x in qh]).contiguous()
    got = _call(q, torch.tensor(q_len, dtype=torch.int32, device=DEV), _frames(poolh, torch.float32),
                torch.tensor([f for f, _ in pieces], dtype=torch.int64, device=DEV),
                torch.tensor([n for _, n in pieces], dtype=torch.int32, device=DEV), K)
    ref = [[locate_ref(dot_cost(qh[b][:, :q_len[b]], poolh[:, f:f + n])) if q_len[b] and 0 < n <= n_pool - f else None
            for f, n in pieces] for b in range(3)]
    return got, ref


def test_gaps_an_empty_piece_one_past_the_pool_and_a_silent_stream():
    K = 3
    got, ref = _layout([(10, 100), (150, 0), (350, 100), (200, 120)], K)
    for b in range(3):
        for p in range(4):
            if ref[b][p] is None:        # nothing to match: n = 0, empty slots
                _assert_pair(got, b, p, [], K)
            else:
                _assert_pair(got, b, p, matches_ref(ref[b][p][3], ref[b][p][4], K), K)
                assert (got[0][b, p, 0], got[1][b, p, 0], got[2][b, p, 0]) == ref[b][p][:3]
    assert got[3].tolist() == [[3, 0, 0, 3], [3, 0, 0, 3], [0, 0, 0, 0]]


def test_overlapping_pieces_are_flagged_and_keep_rts_locates_answer():
    """Pieces 1 and 2 share pool frames [150, 160); piece 3 repeats piece 0's range.  All four get n = -1 with
    rts_locate's own answer in slot 0 -- except for the stream that heard nothing, whose n is 0."""
    K = 3
    got, ref = _layout([(10, 100), (120, 40), (150, 90), (10, 100)], K)
    for b in range(3):
        for p in range(4):
            if ref[b][p] is None:
                _assert_pair(got, b, p, [], K)
            else:
                _assert_pair(got, b, p, [ref[b][p][:3]], K, n=-1)
    # and a call where only two of the four overlap: the others are ranked as usual
    got, ref = _layout([(10, 100), (120, 40), (159, 90), (300, 100)], K)
    for b in range(2):
        for p in (1, 2):
            _assert_pair(got, b, p, [ref[b][p][:3]], K, n=-1)
        for p in (0, 3):
            _assert_pair(got, b, p, matches_ref(ref[b][p][3], ref[b][p][4], K), K)
    # K = 1: slot 0 is all there is
    got1, _ = _layout([(10, 100), (120, 40), (159, 90), (300, 100)], 1)
    assert got1[3].tolist() == [[1, -1, -1, 1], [1, -1, -1, 1], [0, 0, 0, 0]]
    assert same_bytes(got1[0][:, :, 0], got[0][:, :, 0]) and np.array_equal(got1[1][:, :, 0], got[1][:, :, 0])


def test_graph_capture_and_a_replay():
    from real_time_audio_sync_amd import _native as nat
    piece, q, _ = repeat_case()
    qd, _, pool, first, lens = _one_piece(piece, q, torch.float32)
    K = 4
    c, e, s, D, S = locate_ref(dot_cost(q, piece))
    ranks = matches_ref(D, S, K)
    nbytes = ctypes.c_size_t()
    nat.check(nat.lib.rts_locate_matches_workspace_bytes(1, pool.shape[0], ctypes.byref(nbytes)))
    cost = torch.zeros((1, 1, K), dtype=torch.float64, device=DEV)
    end = torch.zeros((1, 1, K), dtype=torch.int32, device=DEV)
    start = torch.zeros((1, 1, K), dtype=torch.int32, device=DEV)
    n = torch.zeros((1, 1), dtype=torch.int32, device=DEV)
    ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=DEV)

    def call():
        nat.check(nat.lib.rts_locate_matches(qd.data_ptr(), nat.F32, q.shape[1], None, 1, pool.data_ptr(), nat.F32, 12,
                                             pool.shape[0], first.data_ptr(), lens.data_ptr(), 1, nat.COST_DOT, K,
                                             float("inf"), cost.data_ptr(), end.data_ptr(), start.data_ptr(), n.data_ptr(),
                                             ws.data_ptr(), nbytes.value,
                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = [t.cpu().numpy().copy() for t in (cost, end, start, n)]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):      # one stream, three launches in a row: no parallel branches
        call()
    for t in (cost, end, start, n, ws):
        t.fill_(0x55 if t.dtype == torch.uint8 else 7)
    g.replay()
    torch.cuda.synchronize()
    replayed = [t.cpu().numpy() for t in (cost, end, start, n)]
    assert all(same_bytes(a, b) for a, b in zip(eager, replayed))
    _assert_pair(replayed, 0, 0, ranks, K)


def test_python_wrapper_allocates_and_agrees():
    from real_time_audio_sync_amd.locate import locate_batch, locate_matches
    piece, q, _ = repeat_case()
    args = _one_piece(piece, q, torch.float32)
    got = [t.cpu().numpy() for t in locate_matches(*args, 4)]
    assert got[0].shape == (1, 1, 4) and got[3].shape == (1, 1)
    c, e, s, D, S = locate_ref(dot_cost(q, piece))
    _assert_pair(got, 0, 0, matches_ref(D, S, 4), 4)
    lc, le, ls = (t.cpu().numpy() for t in locate_batch(*args))
    assert (got[0][0, 0, 0], got[1][0, 0, 0], got[2][0, 0, 0]) == (lc[0, 0], le[0, 0], ls[0, 0])


def _repeat_expectation():
    piece, q, copies = repeat_case()
    c, e, s, D, S = locate_ref(dot_cost(q, piece))
    ranks = matches_ref(D, S, 3)
    M = q.shape[1]
    step = [c / (M + e - s + 1) for c, e, s in ranks]
    third = max(ranks, key=lambda r: r[2])
    assert abs(third[2] - (copies[2] + 4)) <= 8
    return piece, q, ranks, max(step) - min(step), third


def _packed_excerpt(q, dtype, B, b):
    buf = torch.zeros((B, q.shape[1], 12), dtype=dtype, device=DEV)
    buf[b] = _frames(q, dtype)
    lens = torch.zeros(B, dtype=torch.int32, device=DEV)
    lens[b] = q.shape[1]
    return buf, lens


def test_reacquire_on_the_pass_nearest_to_where_the_stream_was():
    """A stream lost in the third pass of A | B | A | C | A: reacquire() puts it into the first (today's behaviour),
    reacquire(matches=3, choose=nearest_to(...)) into the third, where it then follows."""
    from real_time_audio_sync_amd import _native as nat
    from real_time_audio_sync_amd.locate import nearest_to
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    piece, q, ranks, slack, third = _repeat_expectation()
    other = repeat_case()[0][:, 48:118].copy()       # B alone, as a second piece
    eng = BatchedOTW.with_references([other, piece], 50, 3, dtype=torch.float64, device=DEV)
    try:
        b = 1
        eng.push(*_packed_excerpt(q, torch.float64, 2, b))
        # locate(matches=3): every rank of every piece, cheapest first, ties in rank order
        found = eng.locate_recent(q.shape[1], streams=[b], matches=3)
        assert found[0] == [] and [x[0] is piece for x in found[b][:3]] == [True] * 3
        assert [(c, e, s) for _, s, e, c in found[b][:3]] == ranks
        assert [c for _, _, _, c in found[b]] == sorted(c for _, _, _, c in found[b])
        assert found[b][0] == eng.locate_recent(q.shape[1], streams=[b])[b][0]
        got = eng.reacquire([b], M=q.shape[1])
        assert got[b][0] is piece and (got[b][3], got[b][2], got[b][1]) == ranks[0]           # the first pass, as today
        seen = []

        def spy(bb, cand):
            seen.append((bb, list(cand), cand.M))
            return nearest_to({b: (piece, 230)}, slack)(bb, cand)
        got = eng.reacquire([b], M=q.shape[1], matches=3, choose=spy)
        assert (got[b][3], got[b][2], got[b][1]) == third and got[b][0] is piece
        assert len(seen) == 1 and seen[0][0] == b and seen[0][2] == q.shape[1] and len(seen[0][1]) >= 3
        assert list(eng.ref_lens) == [other.shape[1], piece.shape[1] - third[2]]
        # it follows there: exactly a tracker created on piece[:, start:] that was fed the excerpt ...
        import oracle
        o = oracle.OtwOracle(piece[:, third[2]:], 50, 3)
        o.run(q)
        assert np.array_equal(eng.path(b), o.path)
        st = eng.state(b)
        assert all(st[k] == o.state[k] for k in ("t", "j", "direction", "previous", "run_count", "status")), (st, o.state)
        # ... and it takes the frames that come next in that pass
        at = third[1] + 1
        nxt = torch.zeros((2, 269 - at, 12), dtype=torch.float64, device=DEV)
        nxt[b] = _frames(piece[:, at:], torch.float64)
        eng.push(nxt, torch.tensor([0, 269 - at], dtype=torch.int32, device=DEV))
        st2 = eng.state(b)
        assert st2["status"] in (nat.RUNNING, nat.STOP_REF_END) and st2["j"] >= st["j"] and st2["t"] >= st["t"], (st, st2)
        # choose -> None leaves the stream alone
        before = eng.state(b)
        assert eng.reacquire([b], M=q.shape[1], matches=3, choose=lambda bb, cand: None) == {b: None}
        assert eng.state(b) == before
    finally:
        eng.close()


def test_live_session_reacquire_with_matches():
    from real_time_audio_sync_amd.live import LiveSession
    from real_time_audio_sync_amd.locate import nearest_to
    piece, q, ranks, slack, third = _repeat_expectation()
    other = repeat_case()[0][:, 48:118].copy()
    sess = LiveSession([piece, other], batch=2, c=50, fft_len=512, hop_size=256, max_pending=4096)
    try:
        sess.otw.push(*_packed_excerpt(q, torch.float64, 2, 0))
        found = sess.locate_recent(q.shape[1], matches=3)
        assert found[1] == [] and [(c, e, s) for _, s, e, c in found[0][:3]] == ranks and found[0][0][0] is piece
        got = sess.reacquire([0, 1], M=q.shape[1])
        assert got[1] is None and got[0][0] is piece and (got[0][3], got[0][2], got[0][1]) == ranks[0]
        got = sess.reacquire([0, 1], M=q.shape[1], matches=3, choose=nearest_to({0: (piece, 230)}, slack))
        assert got[1] is None and got[0][0] is piece and (got[0][3], got[0][2], got[0][1]) == third
        sess.sync()
        assert list(sess.otw.ref_lens) == [piece.shape[1] - third[2], other.shape[1]]
    finally:
        sess.close()
