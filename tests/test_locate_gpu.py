"""rts_locate on the GPU (csrc/locate.hip; locate.locate_batch, BatchedOTW.locate): every output -- cost, end, start, the
last row of the accumulated-cost matrix and the start index each of its cells carries -- is compared with ``==`` against
the serial restatement of tests/test_locate_cpu.py (float64 sums and compares have one result: no tolerance), and the cost
against the pinned offline-DTW kernel on the reported range.

References are computed once per cost kind (module fixtures) and shared by the parametrised cases."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_locate_cpu import dot_cost, euclid_cost, excerpt_case, locate_ref  # noqa: E402

MS = [1, 63, 64, 65, 130, 256]         # one row; both sides of one strip; three strips with a ragged last; four full strips
NS = [1, 5, 40, 129, 300, 1000]        # one column; N < M; below / above one 64-column hand-off ring; many chunks
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _frames(x, dtype):
    """(12, n) feature-major float64 (float32 values) -> device [n][12]."""
    return torch.from_numpy(np.ascontiguousarray(x.T)).to(dtype).to(DEV)


@pytest.fixture(scope="module")
def strips():
    """One 256-frame query (its first M frames are the query of length M) and a pool of the six pieces back to back."""
    from real_time_audio_sync_amd import synth
    pool = synth.synth_ref(sum(NS), seed=41)
    q = synth.synth_live(synth.synth_ref(300, seed=42), seed=43)[:, :256]
    assert q.shape[1] == 256
    first = np.concatenate([[0], np.cumsum(NS)[:-1]]).astype(np.int64)
    return dict(pool=pool, q=q, first=first, cache={})


def _expected(strips, euclid):
    """{M: [(cost, end, start, D row, S row) per piece]} by the restatement, computed on first use."""
    if euclid not in strips["cache"]:
        C = (euclid_cost if euclid else dot_cost)(strips["q"], strips["pool"])
        strips["cache"][euclid] = {M: [locate_ref(C[:M, f:f + n]) for f, n in zip(strips["first"], NS)] for M in MS}
    return strips["cache"][euclid]


@pytest.mark.parametrize("euclid", [False, True], ids=["dot", "euclid"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("M", MS)
def test_strip_boundary_shapes(strips, M, dtype, euclid):
    from real_time_audio_sync_amd.locate import locate_batch
    exp = _expected(strips, euclid)[M]
    q = _frames(strips["q"][:, :M], dtype)
    pool = _frames(strips["pool"], dtype)
    first = torch.from_numpy(strips["first"]).to(DEV)
    lens = torch.tensor(NS, dtype=torch.int32, device=DEV)
    cost, end, start, row, rowstart = (t.cpu().numpy() for t in locate_batch(q, None, pool, first, lens, euclid=euclid, want_rows=True))
    for p, (c, e, s, D, S) in enumerate(exp):
        f, n = int(strips["first"][p]), NS[p]
        assert np.array_equal(row[0, f:f + n], D), (p, np.flatnonzero(row[0, f:f + n] != D)[:5])
        assert np.array_equal(rowstart[0, f:f + n], S), (p, np.flatnonzero(rowstart[0, f:f + n] != S)[:5])
        assert (cost[0, p], end[0, p], start[0, p]) == (c, e, s), (p, cost[0, p], end[0, p], start[0, p], c, e, s)


def test_all_lengths_in_one_call_with_idle_strips(strips):
    """The same results when every stream is launched with four strips (M_max = 256) and owns fewer: B = 6 streams of
    q_len = MS in one call, float64 queries against a float32 pool."""
    from real_time_audio_sync_amd.locate import locate_batch
    q = _frames(strips["q"], torch.float64).unsqueeze(0).repeat(len(MS), 1, 1).contiguous()
    pool = _frames(strips["pool"], torch.float32)
    first = torch.from_numpy(strips["first"]).to(DEV)
    lens = torch.tensor(NS, dtype=torch.int32, device=DEV)
    q_len = torch.tensor(MS, dtype=torch.int32, device=DEV)
    cost, end, start, row, rowstart = (t.cpu().numpy() for t in locate_batch(q, q_len, pool, first, lens, want_rows=True))
    for b, M in enumerate(MS):
        exp = _expected(strips, False)[M]
        assert np.array_equal(row[b], np.concatenate([e[3] for e in exp])), b
        assert np.array_equal(rowstart[b], np.concatenate([e[4] for e in exp])), b
        assert [(cost[b, p], end[b, p], start[b, p]) for p in range(len(NS))] == [e[:3] for e in exp], b


def test_cost_is_the_pinned_dtw_kernels_on_the_reported_range(strips):
    """rts_dtw (pinned to the reference's dtw.py) of the query against piece[start .. end]: acc[-1][-1] == cost."""
    from real_time_audio_sync_amd.dtw import dtw_batch
    from real_time_audio_sync_amd.locate import locate_batch
    pool = _frames(strips["pool"], torch.float32)
    first = torch.from_numpy(strips["first"]).to(DEV)
    lens = torch.tensor(NS, dtype=torch.int32, device=DEV)
    for M, p in ((63, 3), (130, 4), (256, 5)):
        q = _frames(strips["q"][:, :M], torch.float32)
        cost, end, start = (t.cpu().numpy() for t in locate_batch(q, None, pool, first, lens))
        f, s, e = int(strips["first"][p]), int(start[0, p]), int(end[0, p])
        assert 0 <= s <= e < NS[p]
        acc = dtw_batch(q, pool[f + s:f + e + 1].contiguous(), want_back=False, check=True)[1]
        assert float(acc[0, -1, -1].item()) == cost[0, p], (M, p)


MARK, IMARK = -12345.5, -77


def test_batched_call_invalid_ranges_untouched_cells_and_guard_rows():
    from real_time_audio_sync_amd import _native as nat, synth
    B, P, M_max, n_pool = 3, 5, 70, 400
    poolh = synth.synth_ref(n_pool, seed=51)
    qh = [synth.synth_live(synth.synth_ref(90, seed=52 + b), seed=60 + b)[:, :M_max] for b in range(B)]
    q_len = [M_max, 17, 0]
    pieces = [(10, 100), (200, 50), (10, 100), (60, 120), (350, 100)]    # repeated: 0 and 2; 3 overlaps them; 4 leaves the pool
    q = torch.stack([_frames(x, torch.float32) for x in qh]).contiguous()
    pool = _frames(poolh, torch.float32)
    first = torch.tensor([f for f, _ in pieces], dtype=torch.int64, device=DEV)
    lens = torch.tensor([n for _, n in pieces], dtype=torch.int32, device=DEV)
    qlen = torch.tensor(q_len, dtype=torch.int32, device=DEV)
    # every output between two guard rows
    cost = torch.full((B + 2, P), MARK, dtype=torch.float64, device=DEV)
    end = torch.full((B + 2, P), IMARK, dtype=torch.int32, device=DEV)
    start = torch.full((B + 2, P), IMARK, dtype=torch.int32, device=DEV)
    row = torch.full((B + 2, n_pool), MARK, dtype=torch.float64, device=DEV)
    rowstart = torch.full((B + 2, n_pool), IMARK, dtype=torch.int32, device=DEV)
    nat.check(nat.lib.rts_locate(q.data_ptr(), nat.F32, M_max, qlen.data_ptr(), B, pool.data_ptr(), nat.F32, 12, n_pool,
                                 first.data_ptr(), lens.data_ptr(), P, nat.COST_DOT, cost[1].data_ptr(), end[1].data_ptr(),
                                 start[1].data_ptr(), row[1].data_ptr(), rowstart[1].data_ptr(),
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    cost, end, start, row, rowstart = (t.cpu().numpy() for t in (cost, end, start, row, rowstart))
    for t, mark in ((cost, MARK), (end, IMARK), (start, IMARK), (row, MARK), (rowstart, IMARK)):
        assert (t[0] == mark).all() and (t[-1] == mark).all(), "a guard row was written"
    cost, end, start, row, rowstart = cost[1:-1], end[1:-1], start[1:-1], row[1:-1], rowstart[1:-1]
    covered = np.zeros(n_pool, dtype=bool)
    for f, n in pieces[:4]:
        covered[f:f + n] = True
    for b in range(B):
        assert np.isposinf(cost[b, 4]) and end[b, 4] == -1 and start[b, 4] == -1     # the range outside the pool
        assert (row[b, ~covered] == MARK).all() and (rowstart[b, ~covered] == IMARK).all()
        if q_len[b] == 0:
            assert np.isposinf(cost[b]).all() and (end[b] == -1).all() and (start[b] == -1).all()
            assert (row[b] == MARK).all() and (rowstart[b] == IMARK).all()
            continue
        C = dot_cost(qh[b][:, :q_len[b]], poolh)
        exp = [locate_ref(C[:, f:f + n]) for f, n in pieces[:4]]
        assert [(cost[b, p], end[b, p], start[b, p]) for p in range(4)] == [e[:3] for e in exp], b
        assert exp[0][:3] == exp[2][:3]
        for p, lo, hi in ((1, 200, 250), (0, 10, 60), (3, 110, 180)):      # cells one piece (or two identical ones) owns
            f = pieces[p][0]
            assert np.array_equal(row[b, lo:hi], exp[p][3][lo - f:hi - f]), (b, p)
            assert np.array_equal(rowstart[b, lo:hi], exp[p][4][lo - f:hi - f]), (b, p)
        a0, a3 = exp[0][3][50:100], exp[3][3][0:50]                          # frames [60, 110): piece 0's or piece 3's value
        assert ((row[b, 60:110] == a0) | (row[b, 60:110] == a3)).all(), b


def test_q_len_above_m_max_is_clamped(strips):
    from real_time_audio_sync_amd.locate import locate_batch
    q = _frames(strips["q"][:, :63], torch.float32)
    pool = _frames(strips["pool"], torch.float32)
    first = torch.from_numpy(strips["first"]).to(DEV)
    lens = torch.tensor(NS, dtype=torch.int32, device=DEV)
    a = locate_batch(q, torch.tensor([1000], dtype=torch.int32, device=DEV), pool, first, lens)
    exp = _expected(strips, False)[63]
    assert [(float(a[0][0, p]), int(a[1][0, p]), int(a[2][0, p])) for p in range(len(NS))] == [e[:3] for e in exp]


def _tie_case():
    rs = np.random.RandomState(11)

    def rnd(n):
        x = rs.rand(12, n) ** 3
        return (x / np.sqrt((x * x).sum(axis=0, keepdims=True))).astype(np.float32).astype(np.float64)
    sec = rnd(30)
    return np.concatenate([rnd(50), sec, rnd(40), sec, rnd(20)], axis=1), sec


@pytest.mark.parametrize("euclid", [False, True], ids=["dot", "euclid"])
def test_exact_tie_reports_the_first_end(euclid):
    """A piece that holds the same 30 frames at [50, 80) and [120, 150), queried with exactly those frames: both ends
    cost the same double, the first one is reported."""
    from real_time_audio_sync_amd.locate import locate_batch
    piece, sec = _tie_case()
    c, e, s, D, S = locate_ref((euclid_cost if euclid else dot_cost)(sec, piece))
    assert (e, s) == (79, 50) and D[149] == D[79] and S[149] == 120         # the input is the tie it is meant to be
    first = torch.zeros(1, dtype=torch.int64, device=DEV)
    lens = torch.tensor([piece.shape[1]], dtype=torch.int32, device=DEV)
    cost, end, start, row, rowstart = locate_batch(_frames(sec, torch.float64), None, _frames(piece, torch.float64), first,
                                                   lens, euclid=euclid, want_rows=True)
    assert (float(cost[0, 0]), int(end[0, 0]), int(start[0, 0])) == (c, 79, 50)
    assert np.array_equal(row[0].cpu().numpy(), D) and np.array_equal(rowstart[0].cpu().numpy(), S)


def test_graph_capture_and_two_replays(strips):
    from real_time_audio_sync_amd import _native as nat
    M, P = 65, len(NS)
    q = _frames(strips["q"][:, :M], torch.float32)
    pool = _frames(strips["pool"], torch.float32)
    first = torch.from_numpy(strips["first"]).to(DEV)
    lens = torch.tensor(NS, dtype=torch.int32, device=DEV)
    cost = torch.zeros((1, P), dtype=torch.float64, device=DEV)
    end = torch.zeros((1, P), dtype=torch.int32, device=DEV)
    start = torch.zeros((1, P), dtype=torch.int32, device=DEV)
    row = torch.zeros((1, pool.shape[0]), dtype=torch.float64, device=DEV)

    def call():
        nat.check(nat.lib.rts_locate(q.data_ptr(), nat.F32, M, None, 1, pool.data_ptr(), nat.F32, 12, pool.shape[0],
                                     first.data_ptr(), lens.data_ptr(), P, nat.COST_DOT, cost.data_ptr(), end.data_ptr(),
                                     start.data_ptr(), row.data_ptr(), None,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    exp = _expected(strips, False)[M]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for _ in range(2):
        for t in (cost, end, start, row):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert [(float(cost[0, p]), int(end[0, p]), int(start[0, p])) for p in range(P)] == [e[:3] for e in exp]
        assert np.array_equal(row[0].cpu().numpy(), np.concatenate([e[3] for e in exp]))


def test_end_to_end_locate_then_restart_there():
    """A microphone that joins inside piece 1: locate() ranks piece 1 first and finds the bar, restart() puts the stream
    there, and the tracker follows from that frame."""
    from real_time_audio_sync_amd import _native as nat
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    from real_time_audio_sync_amd.wtw import BatchedWTW
    pieces, q, A = excerpt_case()
    twin = pieces[1].copy()               # the same piece uploaded a second time: an exact tie, upload order decides
    sess = BatchedOTW.with_references(pieces, 50, 3, variant="livenote", dtype=torch.float32, device=DEV, extra_refs=[twin])
    found = sess.locate([q, np.zeros((12, 0)), q[:, :20]])
    assert found[1] == []                                           # nothing heard yet: no answer
    assert len(found[0]) == 4 and len(found[2]) == 4
    assert found[0][0][0] is pieces[1] and found[0][1][0] is twin and found[0][0][1:] == found[0][1][1:]
    exp = [locate_ref(dot_cost(q, p))[:3] for p in pieces]
    for ref_obj, start, end, cost in found[0]:
        k = 1 if ref_obj is twin else [i for i, p in enumerate(pieces) if p is ref_obj][0]
        assert (cost, end, start) == exp[k]
    assert [c for _, _, _, c in found[0]] == sorted(c for _, _, _, c in found[0])
    ref_obj, start, end, cost = found[0][0]
    assert abs(start - A) <= 8
    # the Euclidean cost on request, and the tracker's own by default
    fe = sess.locate([q, np.zeros((12, 0)), np.zeros((12, 0))], euclid=True)[0][0]
    assert fe[0] is pieces[1] and (fe[3], fe[2], fe[1]) == locate_ref(euclid_cost(q, pieces[1]))[:3]
    for b, entries in enumerate(found):                             # every returned entry is a valid restart
        for r, s, _, _ in entries:
            sess.restart([b], refs=[r], offsets=[s])
    sess.restart([0], refs=[pieces[1]], offsets=[start])
    nxt = torch.zeros((3, 50, 12), dtype=torch.float32, device=DEV)
    nxt[0] = _frames(pieces[1][:, A + 64:A + 114], torch.float32)
    sess.push(nxt, torch.tensor([50, 0, 0], dtype=torch.int32, device=DEV))
    st = sess.state(0)
    assert st["status"] == nat.RUNNING and st["consumed"] == 50 and st["j"] > 0, st
    sess.close()
    # a handle without per-stream references has no repertoire to search
    single = BatchedOTW(pieces[0], 50, 3, batch=1, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError):
        single.locate([q])
    single.close()
    # BatchedWTW gets the same method
    chroma = [torch.from_numpy(np.ascontiguousarray(p.T)).to(DEV) for p in pieces]
    w = BatchedWTW.with_references(chroma[:2], 40, 20, extra_refs=chroma[2:])
    fw = w.locate(_frames(q, torch.float64).unsqueeze(0).repeat(2, 1, 1).contiguous(), q_len=[64, 0])
    assert fw[1] == [] and fw[0][0][0] is chroma[1] and (fw[0][0][3], fw[0][0][2], fw[0][0][1]) == exp[1]
    w.close()


def test_live_session_locate_names_the_objects_given_at_create():
    from real_time_audio_sync_amd.live import LiveSession
    pieces, q, A = excerpt_case()
    sess = LiveSession([pieces[0], pieces[2]], batch=2, c=30, extra_refs=[pieces[1]])
    found = sess.locate([np.zeros((12, 0)), q])
    exp = locate_ref(dot_cost(q, pieces[1]))[:3]
    assert found[0] == [] and found[1][0][0] is pieces[1] and (found[1][0][3], found[1][0][2], found[1][0][1]) == exp
    assert {id(r) for r, _, _, _ in found[1]} == {id(p) for p in pieces}
    sess.restart([1], refs=[found[1][0][0]], offsets=[found[1][0][1]])
    sess.sync()
    assert list(sess.otw.ref_lens) == [pieces[0].shape[1], pieces[1].shape[1] - found[1][0][1]]
    sess.close()
    single = LiveSession(pieces[0], batch=1, c=30)
    with pytest.raises(ValueError):
        single.locate([q])
    single.close()
