"""Re-acquiring lost streams on the GPU: rts_otw_recent / rts_wtw_recent, rts_otw_path_cost, rts_live_watch /
rts_live_confidence and the Python composition (``recent``, ``path_cost``, ``locate_recent``, ``reacquire``).  Every
float64 and int32 result is compared with ``==`` against the serial restatements of tests/test_reacquire_cpu.py
(``recent_ref``, ``path_cost_ref``: the oracle's own cell costs, sequential sums), built from the frames the test pushed,
the path the tracker recorded and the reference it follows.

Geometry of the kernel tests: B = 4 streams on references of N = 8, 20, 70, 130 frames (history stride 260) that have
consumed 20, 0, 64 and 250 frames: a stream pushed past its own capacity 2 N = 16 (it has long stopped at the end of its
reference; the count still runs on, and len must stop at 16), one that heard nothing, one with exactly 64 frames, one
with more than any M_max but 256; their paths hold 7, 0, 87 and 367 points (variant otw), so every K has a stream with
fewer points and one with more."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_locate_cpu import dot_cost, locate_ref  # noqa: E402
from test_reacquire_cpu import lost_case, path_cost_ref, recent_ref  # noqa: E402

DEV = "cuda:0"
NS = (8, 20, 70, 130)
COUNTS = (20, 0, 64, 250)
C, MRC = 10, 3
MARK, IMARK = -12345.5, -77


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _frames(x, dtype):
    """(12, n) feature-major -> device [n][12]."""
    return torch.from_numpy(np.ascontiguousarray(x.T)).to(dtype).to(DEV)


@pytest.fixture(scope="module")
def geom():
    """The four references and what every stream hears: a slow rendition of its own piece (float32 values)."""
    from real_time_audio_sync_amd import synth
    refs = [synth.synth_ref(n, seed=900 + b) for b, n in enumerate(NS)]
    heard = [synth.synth_live(np.concatenate([refs[b]] * 4, axis=1), seed=950 + b, lo=0.45, hi=0.55)[:, :COUNTS[b]]
             for b in range(4)]
    assert [h.shape[1] for h in heard] == list(COUNTS)
    return refs, heard


def _packed(heard, dtype, lo=0.0, hi=1.0):
    """Frames [lo * count, hi * count) of every stream as one push: (device [B][n_max][12], int32 [B])."""
    parts = [h[:, int(lo * h.shape[1]):int(hi * h.shape[1])] for h in heard]
    n_max = max(max(p.shape[1] for p in parts), 1)
    buf = torch.zeros((len(parts), n_max, 12), dtype=dtype)
    for b, p in enumerate(parts):
        buf[b, :p.shape[1]] = torch.from_numpy(np.ascontiguousarray(p.T)).to(dtype)
    return buf.to(DEV), torch.tensor([p.shape[1] for p in parts], dtype=torch.int32, device=DEV)


def _recent_raw(eng, M, mask=None):
    """rts_*_recent between two guard rows -> (out [B][M][12], len [B]) as numpy."""
    from real_time_audio_sync_amd import _native as nat
    out = torch.full((eng.B + 2, M, 12), MARK, dtype=torch.float64, device=DEV)
    ln = torch.full((eng.B + 2,), IMARK, dtype=torch.int32, device=DEV)
    m = torch.tensor(mask, dtype=torch.uint8, device=DEV) if mask is not None else None
    nat.check(eng._fn("recent")(eng._h, M, out[1].data_ptr(), ln[1:].data_ptr(), m.data_ptr() if m is not None else None,
                                _stream()))
    out, ln = out.cpu().numpy(), ln.cpu().numpy()
    assert (out[0] == MARK).all() and (out[-1] == MARK).all() and ln[0] == IMARK and ln[-1] == IMARK, "a guard row was written"
    return out[1:-1], ln[1:-1]


def _check_recent(eng, heard, caps, Ms=(1, 64, 65, 256), mask=None):
    for M in Ms:
        out, ln = _recent_raw(eng, M, mask)
        for b in range(eng.B):
            eo, el = recent_ref(heard[b].T, M, caps[b], masked=mask is not None and not mask[b])
            assert ln[b] == el, (M, b, ln[b], el)
            assert np.array_equal(out[b], eo), (M, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["otw", "wtw"])
def test_recent_is_the_tail_of_the_history(geom, kind, dtype):
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    from real_time_audio_sync_amd.wtw import BatchedWTW
    refs, heard = geom
    if kind == "otw":
        eng = BatchedOTW.with_references(refs, C, MRC, dtype=torch.float32, device=DEV)
    else:
        eng = BatchedWTW.with_references([_frames(r, torch.float64) for r in refs], 8, 4)
    caps = [2 * n for n in NS]
    try:
        # a fresh handle (the OTW history is not even allocated yet): len 0 everywhere, all-zero rows
        _check_recent(eng, [h[:, :0] for h in heard], caps, Ms=(1, 65))
        if kind == "otw":       # two pushes: the tail spans both
            eng.push(*_packed(heard, dtype, 0.0, 0.5))
            _check_recent(eng, [h[:, :int(0.5 * h.shape[1])] for h in heard], caps, Ms=(64,))
            eng.push(*_packed(heard, dtype, 0.5, 1.0))
        else:                   # one push: a WTW stream that has stopped takes no further column (wtw.py:76-77)
            eng.push(*_packed(heard, dtype))
        _check_recent(eng, heard, caps)
        out, ln = _recent_raw(eng, 256)
        assert list(ln) == [16, 0, 64, 250]                         # the case is what it is meant to be
        _check_recent(eng, heard, caps, Ms=(64, 65), mask=[1, 1, 0, 1])
        _check_recent(eng, heard, caps, Ms=(65,), mask=[0, 0, 0, 0])
        # the Python method: same tensors, `streams` as the mask
        fr, ln = eng.recent(65, streams=[0, 3])
        for b in range(4):
            eo, el = recent_ref(heard[b].T, 65, caps[b], masked=b not in (0, 3))
            assert int(ln[b]) == el and np.array_equal(fr[b].cpu().numpy(), eo), b
        # a restarted stream has heard nothing; the others are unchanged
        eng.restart([3])
        _check_recent(eng, [heard[0], heard[1], heard[2], heard[3][:, :0]], caps, Ms=(64, 256))
    finally:
        eng.close()


def test_recent_and_path_cost_refuse_the_frames_of_a_run(geom):
    from real_time_audio_sync_amd import _native as nat
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    refs, heard = geom
    eng = BatchedOTW(refs[2], C, MRC, batch=2, dtype=torch.float32, device=DEV)
    try:
        lv, ln = eng.pack([heard[2], heard[2][:, :30]])
        eng.run(lv, ln)
        with pytest.raises(nat.RtsyncError, match="error -2.*rts_otw_run"):
            eng.recent(64)
        with pytest.raises(nat.RtsyncError, match="error -2.*rts_otw_run"):
            eng.path_cost(16)
        eng.push(lv[:, :4].contiguous())                            # "mixed": still the caller's frames in part
        with pytest.raises(nat.RtsyncError, match="error -2"):
            eng.recent(64)
        eng.reset()
        eng.push(lv[:, :4].contiguous())
        fr, n = eng.recent(8)
        assert list(n.cpu().numpy()) == [4, 4]
        assert np.array_equal(fr[0, :4].cpu().numpy(), heard[2].T[:4]) and not fr[:, 4:].any()
    finally:
        eng.close()


def _check_path_cost(eng, heard, ref_ranges, euclid, Ks=(1, 63, 64, 65, 256)):
    """path_cost(K, want_costs) of every stream against the restatement; -> {K: means}."""
    paths = [eng.path(b) for b in range(eng.B)]
    means = {}
    for K in Ks:
        mean, n, costs = (t.cpu().numpy() for t in eng.path_cost(K, want_costs=True))
        m2, n2 = (t.cpu().numpy() for t in eng.path_cost(K))
        assert np.array_equal(m2, mean, equal_nan=True) and np.array_equal(n2, n)
        for b in range(eng.B):
            em, en, ec = path_cost_ref(paths[b], heard[b].T, ref_ranges[b], K, euclid)
            assert n[b] == en, (K, b, n[b], en)
            assert np.array_equal(costs[b], ec, equal_nan=True), (K, b, np.flatnonzero(costs[b] != ec)[:5])
            assert (np.isnan(mean[b]) and np.isnan(em)) or mean[b] == em, (K, b, mean[b], em)
        means[K] = mean
    return paths, means


@pytest.mark.parametrize("euclid,dtype,variant", [(False, torch.float32, "otw"), (False, torch.float64, "otw"),
                                                  (True, torch.float32, "otw"), (True, torch.float64, "otw"),
                                                  (False, torch.float32, "livenote_v2")],
                         ids=["dot-f32", "dot-f64", "euclid-f32", "euclid-f64", "dot-f32-livenote_v2"])
def test_path_cost_equals_the_restatement(geom, euclid, dtype, variant):
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    refs, heard = geom
    eng = BatchedOTW.with_references(refs, C, MRC, variant=variant, euclid=euclid, dtype=dtype, device=DEV)
    try:
        eng.push(*_packed(heard, torch.float32, 0.0, 0.4))
        eng.push(*_packed(heard, torch.float32, 0.4, 1.0))
        stored = [r.T.astype(np.float32 if dtype == torch.float32 else np.float64) for r in refs]
        paths, means = _check_path_cost(eng, heard, stored, euclid)
        if variant == "otw":
            assert [len(p) for p in paths] == [7, 0, 87, 367]       # fewer points than K and more, in one batch
        assert len(paths[1]) == 0 and np.isnan(means[64][1])        # an empty path: n = 0 (checked above), mean NaN
        assert np.isfinite(means[256][[0, 2, 3]]).all()
        # stream 2 restarted onto an offset range of its piece and pushed again: reference frames first + 5 + j
        eng.restart([2], offsets=[5])
        again = torch.zeros((4, 40, 12), dtype=torch.float32, device=DEV)
        again[2] = _frames(heard[2][:, 5:45], torch.float32)
        eng.push(again, torch.tensor([0, 0, 40, 0], dtype=torch.int32, device=DEV))
        heard2 = [heard[0], heard[1], heard[2][:, 5:45], heard[3]]
        paths2, means2 = _check_path_cost(eng, heard2, [stored[0], stored[1], stored[2][5:], stored[3]], euclid, Ks=(64, 65))
        assert 0 < len(paths2[2]) and all(np.array_equal(paths2[b], paths[b]) for b in (0, 1, 3))
        assert np.array_equal(means2[64][[0, 3]], means[64][[0, 3]])
    finally:
        eng.close()


@pytest.mark.parametrize("euclid", [False, True], ids=["dot", "euclid"])
def test_path_cost_on_a_single_reference_handle(geom, euclid):
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    refs, heard = geom
    eng = BatchedOTW(refs[2], C, MRC, batch=3, euclid=euclid, dtype=torch.float64, device=DEV)
    try:
        lives = [heard[2], heard[2][:, :3], heard[3][:, :64]]
        eng.push(*_packed(lives, torch.float64))
        _check_path_cost(eng, lives, [refs[2].T] * 3, euclid, Ks=(1, 64, 65))
    finally:
        eng.close()


def test_a_nan_column_makes_that_streams_mean_nan_and_no_other(geom):
    """Stream 1 is a silent microphone: every column it hears normalises to NaN, so every cell cost of that stream is NaN.
    Whatever points its tracker records, each costs NaN -- it pairs a NaN frame with the reference, or lies outside the
    history, which the contract answers with NaN as well -- and the kernel equals the restatement on the recorded path;
    streams 0 and 2 equal theirs and stay finite."""
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    refs, heard = geom
    silent = np.full((12, 12), np.nan)
    lives = [heard[2][:, :12], silent, heard[3][:, :12]]
    eng = BatchedOTW.with_references([refs[2], refs[2], refs[3]], C, MRC, dtype=torch.float64, device=DEV)
    try:
        eng.push(*_packed(lives, torch.float64))
        _, means = _check_path_cost(eng, lives, [refs[2].T, refs[2].T, refs[3].T], False, Ks=(256,))
        n = eng.path_cost(256)[1].cpu().numpy()
        assert n[1] > 0 and np.isnan(means[256][1]), (n, means[256])
        assert np.isfinite(means[256][[0, 2]]).all()
    finally:
        eng.close()


def test_graph_capture_of_recent_locate_and_path_cost(geom):
    """recent + rts_locate + path_cost captured into one graph and replayed twice with pushes in between: the results
    follow the handle's new state."""
    from real_time_audio_sync_amd import _native as nat
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    refs, heard = geom
    eng = BatchedOTW.with_references(refs, C, MRC, dtype=torch.float32, device=DEV)
    M, K, P = 65, 64, 4
    first = torch.tensor([f for _, f, _ in eng._pool.values()], dtype=torch.int64, device=DEV)
    lens = torch.tensor([n for _, _, n in eng._pool.values()], dtype=torch.int32, device=DEV)
    fr = torch.zeros((4, M, 12), dtype=torch.float64, device=DEV)
    ln = torch.zeros(4, dtype=torch.int32, device=DEV)
    cost = torch.zeros((4, P), dtype=torch.float64, device=DEV)
    end = torch.zeros((4, P), dtype=torch.int32, device=DEV)
    start = torch.zeros((4, P), dtype=torch.int32, device=DEV)
    mean = torch.zeros(4, dtype=torch.float64, device=DEV)
    n = torch.zeros(4, dtype=torch.int32, device=DEV)

    def call():
        s = _stream()
        nat.check(nat.lib.rts_otw_recent(eng._h, M, fr.data_ptr(), ln.data_ptr(), None, s))
        nat.check(nat.lib.rts_locate(fr.data_ptr(), nat.F64, M, ln.data_ptr(), 4, eng.ref.data_ptr(), nat.F32, 12,
                                     eng.ref.shape[0], first.data_ptr(), lens.data_ptr(), P, nat.COST_DOT, cost.data_ptr(),
                                     end.data_ptr(), start.data_ptr(), None, None, s))
        nat.check(nat.lib.rts_otw_path_cost(eng._h, K, mean.data_ptr(), n.data_ptr(), None, s))
    try:
        eng.push(*_packed(heard, torch.float32, 0.0, 0.3))          # (the history exists from the first push on)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        stored = [r.T.astype(np.float32) for r in refs]
        for lo, hi in ((0.3, 0.6), (0.6, 1.0)):
            eng.push(*_packed(heard, torch.float32, lo, hi))
            for t in (fr, ln, cost, end, start, mean, n):
                t.zero_()
            g.replay()
            torch.cuda.synchronize()
            now = [h[:, :int(hi * h.shape[1])] for h in heard]
            for b in range(4):
                eo, el = recent_ref(now[b].T, M, 2 * NS[b])
                assert int(ln[b]) == el and np.array_equal(fr[b].cpu().numpy(), eo), (hi, b)
                em, en, _ = path_cost_ref(eng.path(b), now[b].T, stored[b], K)
                assert int(n[b]) == en and ((np.isnan(em) and bool(torch.isnan(mean[b]))) or float(mean[b]) == em), (hi, b)
                for p in range(P):
                    if el == 0:
                        assert np.isposinf(float(cost[b, p])) and int(end[b, p]) == -1
                    else:
                        exp = locate_ref(dot_cost(eo[:el].T, refs[p]))[:3]
                        assert (float(cost[b, p]), int(end[b, p]), int(start[b, p])) == exp, (hi, b, p)
    finally:
        eng.close()


def _oracle_on(ref, live):
    import oracle
    o = oracle.OtwOracle(ref, 50, 3)
    o.run(live)
    return o


def test_reacquire_end_to_end():
    """The case tests/test_reacquire_cpu.py establishes on the oracle alone: stream 1 follows piece 0 but hears 64 frames
    of piece 1; its mean path cost is the higher one, reacquire() finds piece 1 near frame 117, and afterwards the stream
    is exactly a tracker created on p1[:, start:] that was fed the same 64 frames.  Streams 0 and 2 are not touched."""
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    pieces, heard, A = lost_case()
    p0, p1, p2 = pieces
    from real_time_audio_sync_amd import synth
    lives = [heard["good"], heard["lost"], synth.synth_live(p2, seed=6)]
    eng = BatchedOTW.with_references([p0, p0, p2], 50, 3, dtype=torch.float64, device=DEV, extra_refs=[p1])
    try:
        eng.push(*_packed(lives, torch.float64))
        paths, means = _check_path_cost(eng, lives, [p0.T, p0.T, p2.T], False, Ks=(32,))
        assert means[32][1] > means[32][0], means[32]
        before = dict(paths=paths, states=eng.states(), recent=[t.cpu().numpy() for t in eng.recent(64)])
        got = eng.reacquire([1], M=64)
        assert set(got) == {1} and got[1][0] is p1 and abs(got[1][1] - A) <= 8, got
        piece, start, end, cost = got[1]
        assert (cost, end, start) == locate_ref(dot_cost(heard["lost"], p1))[:3]
        o = _oracle_on(p1[:, start:], heard["lost"])
        assert np.array_equal(eng.path(1), o.path)
        st = eng.state(1)
        assert all(st[k] == o.state[k] for k in ("t", "j", "direction", "previous", "run_count", "status", "first_insert")), (st, o.state)
        assert list(eng.ref_lens) == [p0.shape[1], p1.shape[1] - start, p2.shape[1]]
        states = eng.states()
        after_recent = [t.cpu().numpy() for t in eng.recent(64)]
        for b in (0, 2):
            assert np.array_equal(eng.path(b), paths[b]) and np.array_equal(states[b][:15], before["states"][b][:15]), b
            assert np.array_equal(after_recent[0][b], before["recent"][0][b]) and after_recent[1][b] == before["recent"][1][b]
        assert after_recent[1][1] == 64 and np.array_equal(after_recent[0][1], heard["lost"].T)
        _, means2 = _check_path_cost(eng, lives, [p0.T, p1[:, start:].T, p2.T], False, Ks=(32,))
        assert means2[32][1] < means[32][1] and means2[32][0] == means[32][0]
        # a stream that has heard nothing gets no answer and no restart; locate_recent names the unlisted ones []
        eng.restart([2])
        assert eng.reacquire([2], M=64) == {2: None} and eng.state(2)["first_insert"] == 1
        found = eng.locate_recent(64, streams=[1])
        assert found[0] == [] and found[2] == [] and found[1][0][0] is p1
    finally:
        eng.close()


def _feed(sessions, rs, n):
    block = (0.1 * rs.randn(2, n)).astype(np.float32)
    for s in sessions:
        s.feed_block(block)


@pytest.mark.parametrize("features,euclid", [("chroma", False), ("chroma_diff", True)], ids=["chroma-dot", "diff-euclid"])
def test_live_session_watch_and_confidence(features, euclid):
    from real_time_audio_sync_amd import synth
    from real_time_audio_sync_amd.live import LiveSession
    ref = synth.synth_ref(200, seed=77)      # long enough that no stream reaches its end in these feeds
    if features == "chroma_diff":
        ref = np.clip(np.diff(ref, axis=1), 0, np.inf)
    mk = lambda: LiveSession(ref, batch=2, c=C, max_run_count=MRC, fft_len=512, hop_size=256, features=features,
                             euclid=euclid, max_pending=4096)
    sess, plain = mk(), mk()
    rs = np.random.RandomState(12)
    hist = [np.zeros((0, 12)), np.zeros((0, 12))]

    def feed(n):
        _feed((sess, plain), rs, n)
        sess.sync()
        cols, nc = sess.last_columns()
        for b in range(2):
            hist[b] = np.concatenate([hist[b], cols[b, :int(nc[b])].cpu().numpy()])

    def restated(K=16):
        return [path_cost_ref(sess.path(b), hist[b], ref.T, K, euclid) for b in range(2)]
    try:
        from real_time_audio_sync_amd import _native as nat
        with pytest.raises(nat.RtsyncError, match="error -1"):
            sess.confidence()                                       # before any watch
        with pytest.raises(nat.RtsyncError, match="error -1.*K"):
            sess.watch(257)
        sess.watch(16)
        for n in (1280, 1024, 777):
            feed(n)
        plain.sync()
        conf, info = sess.confidence(), sess.poll()
        assert conf["feeds_done"] == 3 == info["feeds_done"]
        pinfo = plain.poll()
        assert all(np.array_equal(info[k], pinfo[k]) for k in info), (info, pinfo)       # poll() unchanged by the watch
        mean, n = (t.cpu().numpy() for t in sess.otw.path_cost(16))
        assert np.array_equal(conf["n"], n) and np.array_equal(conf["mean"], mean, equal_nan=True)
        exp = restated()
        assert [e[1] for e in exp] == list(conf["n"]) and min(conf["n"]) > 0
        assert all(conf["mean"][b] == exp[b][0] for b in range(2)), (conf, exp)
        # a restarted stream reads n = 0, mean NaN, also after a feed that completes no column; the other keeps its words
        sess.restart([0])
        plain.restart([0])
        hist[0] = np.zeros((0, 12))
        sess.sync()
        c1 = sess.confidence()
        assert c1["n"][0] == 0 and np.isnan(c1["mean"][0]) and c1["n"][1] == conf["n"][1] and c1["mean"][1] == conf["mean"][1]
        feed(100)
        c2 = sess.confidence()
        assert int(sess.last_columns()[1].sum()) == 0 and c2["feeds_done"] == 4
        assert c2["n"][0] == 0 and np.isnan(c2["mean"][0]) and c2["n"][1] == conf["n"][1] and c2["mean"][1] == conf["mean"][1]
        feed(1500)
        c3, exp = sess.confidence(), restated()
        assert [e[1] for e in exp] == list(c3["n"]) and all(c3["mean"][b] == exp[b][0] for b in range(2)), (c3, exp)
        # watch off: the feed goes on, the words stay
        sess.watch(0)
        n_path = len(sess.path(1))
        feed(1500)
        c4 = sess.confidence()
        assert len(sess.path(1)) > n_path and c4["feeds_done"] == 6
        assert np.array_equal(c4["n"], c3["n"]) and np.array_equal(c4["mean"], c3["mean"])
        assert np.array_equal(sess.path(1), plain.path(1)) and np.array_equal(sess.path(0), plain.path(0))
        # reset republishes n = 0, mean NaN for every stream
        sess.reset()
        c5 = sess.confidence()
        assert list(c5["n"]) == [0, 0] and np.isnan(c5["mean"]).all()
    finally:
        sess.close()
        plain.close()


def test_live_session_reacquire_and_wtw_refusal():
    from real_time_audio_sync_amd import _native as nat
    from real_time_audio_sync_amd.live import LiveSession
    pieces, heard, A = lost_case()
    p0, p1, p2 = pieces
    sess = LiveSession([p0, p2], batch=2, c=50, fft_len=512, hop_size=256, extra_refs=[p1], max_pending=4096)
    try:
        # the excerpt goes into the bound tracker as its columns (what the ingestion would have handed it)
        sess.otw.push(*_packed([heard["lost"], heard["lost"][:, :0]], torch.float64))
        got = sess.reacquire([0, 1], M=64)
        assert got[1] is None and got[0][0] is p1 and abs(got[0][1] - A) <= 8
        o = _oracle_on(p1[:, got[0][1]:], heard["lost"])
        assert np.array_equal(sess.path(0), o.path) and list(sess.pending()) == [0, 0]
        found = sess.locate_recent(64)
        assert found[1] == [] and found[0][0][0] is p1
    finally:
        sess.close()
    w = LiveSession(p0, batch=2, fft_len=512, hop_size=256, wtw_params={'dtw_win_size': 256 * 10, 'dtw_hop_size': 256 * 5},
                    max_pending=4096)
    try:
        with pytest.raises(nat.RtsyncError, match="error -2"):
            w.watch(16)
    finally:
        w.close()
