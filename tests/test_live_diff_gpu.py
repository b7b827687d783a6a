"""Live ingestion with chroma-difference features (rts_live_create_features / RTS_FEATURE_CHROMA_DIFF, live_diff_kernel
in csrc/live.hip; LiveSession(features="chroma_diff")): the columns handed to the tracker are read after every feed
through LiveSession.last_columns() and compared bit for bit with np.clip(np.diff(.), 0, inf) of ChromaPlan.frames on
the same plan over all samples of the stream -- a float64 subtraction and a compare have one result, so no tolerance --
their per-feed counts with the carry model of tests/test_live_diff_cpu.py, the tracker state with an offline push of the
same columns and with the CPU oracle, and the chopin recording with the golden the reference's own code made
(tests/golden/make_livenote_diff_golden.py; test_live_diff_cpu.py shows that its path does not move within the chroma
gate, which is what allows exact equality here).

As committed these tests have not been run on an MI355X (only collected, and their schedules checked without a GPU); the
OBSERVED line of the columns test prints the largest error against the oracle before it asserts (run with -s)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_chroma_gpu import CHROMA_ATOL  # noqa: E402
from test_chroma_paths_gpu import synth  # noqa: E402
from test_live_diff_cpu import C, GOLDEN, MRC, carry_model, clip_diff, live_samples  # noqa: E402
from test_live_model_cpu import FS, GEOMETRIES, OTW_C, OTW_MRC, drop, max_pending  # noqa: E402

B = 4
COLUMN_GEOMETRIES = [(4096, 2048), (4096, 441), (512, 128)]
assert all(g in GEOMETRIES for g in COLUMN_GEOMETRIES) and any(2 * hop != L for L, hop in COLUMN_GEOMETRIES)
N_FEEDS = 70


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def schedule(L, hop, seed, n_feeds=N_FEEDS):
    """Per-feed sample counts [n_feeds][B].  Placed: a feed in which nobody completes a hop, the feed in which stream 1
    reaches exactly fft_len samples (one chroma column, its first: nothing for the tracker), another feed without a
    column; stream 2 receives one sample at a time for 20 feeds, stream 3 nothing for 10.  The rest is seeded."""
    rs = np.random.RandomState(seed)
    cap = max_pending(L, hop)
    pend = [0] * B
    feeds = []

    def add(c):
        feeds.append(list(c))
        for b in range(B):
            pend[b] = drop(pend[b] + c[b], L, hop)[0]

    add([3, L - 1, 1, 0])
    add([min(hop, L - 5), 1, 1, 0])
    add([1, 5, 1, 0])
    while len(feeds) < n_feeds:
        c = []
        for b in range(B):
            room = cap - pend[b]
            r = rs.rand()
            n = 0 if r < 0.1 else rs.randint(1, 16) if r < 0.25 else rs.randint(1, 2 * hop + 2) if r < 0.85 else rs.randint(1, room + 1)
            c.append(min(int(n), room))
        if len(feeds) < 20:
            c[2] = 1
        if len(feeds) < 10:
            c[3] = 0
        add(c)
    return feeds


def chroma_counts(feeds, L, hop):
    """[B][feed] chroma columns completed per feed (integer form of the reference's loop)."""
    out, pend = [[] for _ in range(B)], [0] * B
    for c in feeds:
        for b in range(B):
            pend[b], n = drop(pend[b] + c[b], L, hop)
            out[b].append(n)
    return out


def audio(feeds, hop, seed):
    """(pcm int16, float32 = pcm / 32768 exactly) per stream, as long as the schedule needs."""
    totals = [sum(c[b] for c in feeds) for b in range(B)]
    pcm = [np.round(synth(totals[b] + 1, max(hop, 16), seed + 1000 * b).astype(np.float64) * 32768.0).astype(np.int16)
           for b in range(B)]
    return pcm, [p.astype(np.float32) / np.float32(32768.0) for p in pcm]


def read_columns(sess):
    """After a sync: ([b] -> [n_cols[b]][12] numpy copies of the last feed's columns, n_cols as a list)."""
    sess.sync()
    cols, n = sess.last_columns()
    assert cols.dtype == torch.float64 and n.dtype == torch.int32 and cols.shape[0] == sess.B and cols.shape[2] == 12
    n = [int(v) for v in n.cpu().numpy()]
    assert max(n) <= cols.shape[1] or max(n) == 0
    return [cols[b, :n[b]].cpu().numpy().reshape(-1, 12) for b in range(sess.B)], n


def run_feeds(sess, feeds, src, pos=None, first=0, last=None):
    """Feeds feeds[first:last]; returns per stream the list of per-feed column arrays, and per stream the n_cols."""
    pos = pos if pos is not None else [0] * sess.B
    got, counts = [[] for _ in range(sess.B)], [[] for _ in range(sess.B)]
    for c in feeds[first:last]:
        sess.feed([src[b][pos[b]:pos[b] + c[b]] if c[b] else None for b in range(sess.B)])
        for b in range(sess.B):
            pos[b] += c[b]
        cols, n = read_columns(sess)
        for b in range(sess.B):
            got[b].append(cols[b])
            counts[b].append(n[b])
    return got, counts


def offline_chroma(plan, x, L, hop):
    """ChromaPlan.frames on the same plan over all samples -> device [K][12] float64."""
    if len(x) < L:
        return torch.zeros((0, 12), dtype=torch.float64, device=plan.device)
    ch, _ = plan.frames(torch.from_numpy(np.ascontiguousarray(x)).to(plan.device), pad_left=0)
    torch.cuda.synchronize()
    assert ch.shape == ((len(x) - L) // hop + 1, 12)
    return ch


def oracle_chroma(x, L, hop):
    from oracle import chroma_oracle as co
    n = (len(x) - L) // hop + 1 if len(x) >= L else 0
    return co.live_loop_columns([x[m * hop:m * hop + L] for m in range(n)], L, FS)


def diff_reference(x, L, hop):
    """Stream 0's own recording framed at 1.25 hop, differenced: the same music at another tempo, as wav_to_chroma_diff
    would give it (12, M)."""
    from oracle import chroma_oracle as co
    h2 = hop * 5 // 4
    n = (len(x) - L) // h2 + 1
    return np.ascontiguousarray(clip_diff(co.live_loop_columns([x[m * h2:m * h2 + L] for m in range(n)], L, FS)).T)


def open_session(ref, L, hop, **kw):
    from real_time_audio_sync_amd.live import LiveSession
    kw.setdefault("features", "chroma_diff")
    kw.setdefault("batch", B)
    return LiveSession(ref, c=OTW_C, max_run_count=OTW_MRC, variant="livenote_v2", euclid=True, fft_len=L,
                       hop_size=hop, fs=FS, max_pending=max_pending(L, hop), **kw)


@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("L,hop", COLUMN_GEOMETRIES)
def test_columns_bit_for_bit_and_tracker_state(L, hop, dtype):
    """Columns: per stream the concatenation of what every feed handed over equals clip-diff of the offline columns
    exactly, n_cols equals the carry model, and the same concatenation is within 2 * CHROMA_ATOL of the oracle's
    clip-diff (each operand within CHROMA_ATOL, clip is 1-Lipschitz).  Tracker: path, poll(), state and both bands equal
    a BatchedOTW pushed the offline difference columns, and path and (t, j, status) the oracle fed the same columns."""
    import oracle
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    feeds = schedule(L, hop, seed=11 * L + hop)
    per_feed = chroma_counts(feeds, L, hop)
    assert any(all(per_feed[b][i] == 0 for b in range(B)) for i in range(len(feeds)))
    assert per_feed[1][:3] == [0, 1, 0] and feeds[5][2] == 1 and all(sum(p) >= 6 for p in per_feed)
    pcm, flt = audio(feeds, hop, seed=L + hop)
    ref = diff_reference(flt[0], L, hop)
    sess = open_session(ref, L, hop)
    eng = BatchedOTW(ref, OTW_C, OTW_MRC, batch=B, variant="livenote_v2", euclid=True, dtype=torch.float64)
    try:
        got, counts = run_feeds(sess, feeds, pcm if dtype == "int16" else flt)
        info = sess.poll()
        assert info["feeds_done"] == info["feeds_submitted"] == len(feeds)
        worst, offline = 0.0, []
        for b in range(B):
            assert counts[b] == carry_model(per_feed[b])[0], b
            x = flt[b][:sum(c[b] for c in feeds)]
            off = offline_chroma(sess.plan, x, L, hop)
            want = clip_diff(off.cpu().numpy())
            have = np.concatenate(got[b])
            assert have.shape == want.shape == (sum(per_feed[b]) - 1, 12), b
            assert np.array_equal(have, want), b
            dev_diff = sess.plan.diff(off)                       # chroma_diff_kernel on the offline columns: the same again
            assert np.array_equal(dev_diff.cpu().numpy(), want), b
            err = float(np.abs(have - clip_diff(oracle_chroma(x, L, hop))).max())
            worst = max(worst, err)
            offline.append(dev_diff)
        print("OBSERVED live diff columns L=%d hop=%d %s: max |delta| vs oracle clip-diff %.3g (gate %.3g)"
              % (L, hop, dtype, worst, 2 * CHROMA_ATOL))
        assert worst <= 2 * CHROMA_ATOL
        # the tracker
        k = [int(o.shape[0]) for o in offline]
        cols = torch.zeros((B, max(k), 12), dtype=torch.float64, device=eng.device)
        for b in range(B):
            cols[b, :k[b]] = offline[b]
        eng.push(cols, torch.tensor(k, dtype=torch.int32, device=eng.device))
        for b in range(B):
            assert np.array_equal(sess.path(b), eng.path(b)), b
            sa, sb = sess.otw.state(b), eng.state(b)
            sa.pop("band_recomputes"), sb.pop("band_recomputes")   # bookkeeping differs with launch granularity
            assert sa == sb, b
            for x, y in zip(sess.otw.bands(b), eng.bands(b)):
                assert np.array_equal(x, y, equal_nan=True), b
            o = oracle.OtwOracle(ref, OTW_C, OTW_MRC, variant=oracle.LIVENOTE_V2, cost=oracle.COST_EUCLID)
            o.run(np.ascontiguousarray(offline[b].cpu().numpy().T))
            assert np.array_equal(sess.path(b), o.path), b
            assert (sa["t"], sa["j"], sa["status"]) == (o.state["t"], o.state["j"], o.state["status"]), b
            assert tuple(info["positions"][b]) == (sa["t"], sa["j"]) and info["status"][b] == sa["status"], b
        assert len(sess.path(0)) > OTW_C
    finally:
        eng.close()
        sess.close()


def test_reference_made_golden(chopin_audio):
    """tests.py:145-163 from microphones: three streams with different buffer sizes, stream 2 delivering PCM16.  The float
    streams must give the golden path of the recording, the PCM16 stream the golden path of the recording as PCM16 (the
    rounding to PCM16 moves path points: test_live_diff_cpu.py::test_pcm16_rounding_moves_the_path)."""
    from real_time_audio_sync_amd import chroma
    from real_time_audio_sync_amd.live import LiveSession
    g = np.load(GOLDEN)
    plan = chroma._plan()
    ref_dev = torch.from_numpy(chopin_audio["ref"]).to(plan.device)
    ref_diff = plan.diff(plan.frames(ref_dev, pad_left=chroma.fft_len // 2)[0]).t().contiguous().cpu().numpy()
    assert ref_diff.shape == (12, int(g["n_ref_cols"]))
    live, _ = live_samples(chopin_audio, "")
    _, pcm = live_samples(chopin_audio, "_pcm16")
    src, sizes = [live, live, pcm], (1500, 4096, 9000)
    sess = LiveSession(ref_diff, batch=3, c=C, max_run_count=MRC, variant="livenote_v2", euclid=True, features="chroma_diff")
    try:
        pos = [0, 0, 0]
        while any(pos[b] < len(live) for b in range(3)):
            bufs = []
            for b in range(3):
                n = min(sizes[b], len(live) - pos[b])
                bufs.append(src[b][pos[b]:pos[b] + n] if n > 0 else None)
                pos[b] += max(n, 0)
            sess.feed(bufs)
        sess.sync()
        info = sess.poll()
        assert info["feeds_done"] == info["feeds_submitted"]
        for b, suffix in enumerate(("", "", "_pcm16")):
            assert np.array_equal(sess.path(b), g["path" + suffix]), b
            assert tuple(info["positions"][b]) == (int(g["live_ptr" + suffix]), int(g["ref_ptr" + suffix])), b
            assert sess.otw.state(b)["consumed"] == int(g["consumed" + suffix]), b
        assert sess.stopped() == [b for b, s in enumerate(("", "", "_pcm16")) if int(g["stopped" + s])]
    finally:
        sess.close()


@pytest.mark.parametrize("per_stream_refs", [False, True])
def test_restart_and_reset_drop_the_carry(per_stream_refs):
    """Stream 1 is restarted between two feeds that each complete columns for it: the feed behind the restart hands over
    one column fewer than it completes, from there on the stream equals a fresh session on the samples fed since, the
    others are untouched; after reset() every stream is fresh.  With per-stream references the restarted stream moves on
    to an extra piece."""
    L, hop = 512, 128
    feeds = schedule(L, hop, seed=5, n_feeds=50)
    at = 25
    feeds[at - 1][1] = feeds[at + 1][1] = 3 * hop + 7            # columns for stream 1 right before the restart ...
    feeds[at][1] = L + hop + 5                                    # ... and two chroma columns in the first feed behind it
    per_feed = chroma_counts(feeds, L, hop)
    _, flt = audio(feeds, hop, seed=77)
    ref = diff_reference(flt[0], L, hop)
    other = diff_reference(flt[1], L, hop)
    refs = [ref] * B if per_stream_refs else ref
    kw = dict(extra_refs=[other]) if per_stream_refs else {}
    sess, plain = open_session(refs, L, hop, **kw), open_session(refs, L, hop, **kw)
    fresh = open_session(other if per_stream_refs else ref, L, hop, batch=1)
    try:
        pos = [0] * B
        got_a, cnt_a = run_feeds(sess, feeds, flt, pos, 0, at)
        assert per_feed[1][at - 1] > 0 and per_feed[1][at] > 0 and sess.pending()[1] > 0
        since = pos[1]
        sess.restart([1], refs=[other] if per_stream_refs else None)
        assert sess.pending()[1] == 0
        got_b, cnt_b = run_feeds(sess, feeds, flt, pos, at, None)
        want, cnt_p = run_feeds(plain, feeds, flt)
        # the restarted stream: its samples since the restart, framed from there
        sub = [[c[1]] for c in feeds[at:]]
        pend, new_counts = 0, []
        for c in sub:
            pend, n = drop(pend + c[0], L, hop)
            new_counts.append(n)
        assert cnt_b[1] == carry_model(new_counts)[0] and cnt_b[1][0] == new_counts[0] - 1 >= 1
        got_f, cnt_f = run_feeds(fresh, sub, [flt[1][since:]])
        assert cnt_f[0] == cnt_b[1]
        assert all(np.array_equal(x, y) for x, y in zip(got_f[0], got_b[1]))
        assert np.array_equal(np.concatenate(got_b[1]),
                              clip_diff(offline_chroma(sess.plan, flt[1][since:pos[1]], L, hop).cpu().numpy()))
        assert np.array_equal(sess.path(1), fresh.path(0)) and len(fresh.path(0)) > 3
        for b in (0, 2, 3):
            assert cnt_a[b] + cnt_b[b] == cnt_p[b] == carry_model(per_feed[b])[0], b
            assert all(np.array_equal(x, y) for x, y in zip(got_a[b] + got_b[b], want[b])), b
            assert np.array_equal(sess.path(b), plain.path(b)), b
        # reset: every stream behaves as fresh
        sess.reset()
        got_r, cnt_r = run_feeds(sess, feeds, flt, None, 0, 12)
        for b in range(B):
            assert cnt_r[b] == cnt_p[b][:12], b
            assert all(np.array_equal(x, y) for x, y in zip(got_r[b], want[b][:12])), b
    finally:
        for s in (sess, plain, fresh):
            s.close()


def test_refusals():
    from real_time_audio_sync_amd import _native as nat, synth as rsynth
    from real_time_audio_sync_amd.live import LiveSession
    from real_time_audio_sync_amd.wtw import BatchedWTW
    ref = rsynth.synth_ref(60, seed=3)
    params = {'dtw_win_size': 4096 * 10, 'dtw_hop_size': 2048 * 10}
    with pytest.raises(ValueError):
        LiveSession(ref, batch=2, wtw_params=params, features="chroma_diff")
    with pytest.raises(ValueError):
        LiveSession(ref, batch=2, features="chroma_difference")
    # the C ABI: a WTW handle, an unknown kind
    sess = LiveSession(ref, batch=2, c=10, features="chroma_diff", euclid=True, variant="livenote_v2", max_pending=3 * 4096)
    wtw = BatchedWTW(torch.from_numpy(np.ascontiguousarray(ref.T, dtype=np.float64)).to(sess.dev), 10, 5, 2)
    try:
        h = ctypes.c_void_p()
        rc = nat.lib.rts_live_create_features(sess.plan._h, None, wtw._h, 2, 3 * 4096, nat.FEATURE_CHROMA_DIFF, ctypes.byref(h))
        assert rc == -2 and not h.value and b"WTW" in nat.lib.rts_last_error()          # RTS_ERR_UNSUPPORTED
        rc = nat.lib.rts_live_create_features(sess.plan._h, sess.otw._h, None, 2, 3 * 4096, 7, ctypes.byref(h))
        assert rc == -1 and not h.value and b"feature_kind" in nat.lib.rts_last_error()  # RTS_ERR_INVALID
        # a refused feed advances neither the pending counts nor the carry mirror
        rs = np.random.RandomState(1)
        x = (rs.rand(2, 40000) - 0.5).astype(np.float32)
        twin = LiveSession(ref, batch=2, c=10, features="chroma_diff", euclid=True, variant="livenote_v2", max_pending=3 * 4096)
        for s in (sess, twin):
            s.feed_block(x[:, :100])                                  # nothing complete, no carry yet
        with pytest.raises(nat.RtsyncError):
            sess.feed_block(x[:, 100:100 + 3 * 4096])                 # 100 + 12288 > max_pending; would complete columns
        assert list(sess.pending()) == [100, 100]
        for s in (sess, twin):
            s.feed_block(x[:, 100:100 + 4096 + 2048])                 # 6244 pending: two chroma columns, the first of the run
        a, na = read_columns(sess)
        b, nb = read_columns(twin)
        assert na == nb == [1, 1] and all(np.array_equal(p, q) for p, q in zip(a, b))
        assert [s.otw.state(i)["consumed"] for s in (sess, twin) for i in range(2)] == [1] * 4
        assert list(sess.pending()) == list(twin.pending()) == [6244 - 2 * 2048] * 2
        twin.close()
    finally:
        wtw.close()
        sess.close()


def test_default_mode_is_untouched():
    """features="chroma" and a plain LiveSession on the same feeds: bit-equal last_columns() after every feed, equal
    paths; and last_columns() in chroma mode is ChromaPlan.frames."""
    from real_time_audio_sync_amd.live import LiveSession
    L, hop = 512, 128
    feeds = schedule(L, hop, seed=9, n_feeds=40)
    per_feed = chroma_counts(feeds, L, hop)
    pcm, flt = audio(feeds, hop, seed=31)
    from oracle import chroma_oracle as co
    h2 = hop * 5 // 4
    ref = np.ascontiguousarray(co.live_loop_columns([flt[0][m * h2:m * h2 + L] for m in range((len(flt[0]) - L) // h2 + 1)], L, FS).T)
    kw = dict(batch=B, c=OTW_C, max_run_count=OTW_MRC, fft_len=L, hop_size=hop, fs=FS, max_pending=max_pending(L, hop))
    named, plain = LiveSession(ref, features="chroma", **kw), LiveSession(ref, **kw)
    try:
        got_n, cnt_n = run_feeds(named, feeds, pcm)
        got_p, cnt_p = run_feeds(plain, feeds, pcm)
        for b in range(B):
            assert cnt_n[b] == cnt_p[b] == per_feed[b], b
            assert all(np.array_equal(x, y) for x, y in zip(got_n[b], got_p[b])), b
            off = offline_chroma(named.plan, flt[b][:sum(c[b] for c in feeds)], L, hop).cpu().numpy()
            assert np.array_equal(np.concatenate(got_n[b]), off), b
            assert np.array_equal(named.path(b), plain.path(b)), b
        assert len(named.path(0)) > OTW_C
    finally:
        named.close()
        plain.close()


@pytest.mark.parametrize("dtype", ["float32", "int16"])
def test_silence_into_the_headline_configuration(dtype):
    """Digital silence (tests/silence_inputs.py::silent_audio) into LiveNoteV2 on chroma_diff with the Euclidean cost,
    against a reference whose audio also begins with silence: the difference of two silent columns is all zeros, zero
    against zero costs exactly 0 and the band minima tie.  Columns, path, position and status equal the oracle chain
    (chroma oracle -> clip-diff -> OtwOracle)."""
    import oracle
    import silence_inputs as si
    from test_live_paths_gpu import run_silent_session
    L, hop = si.LIVE_L, si.LIVE_HOP
    ref = diff_reference(si.silent_audio()[1][0], L, hop)          # stream 0, silent from the first sample, at 1.25 hop
    n_zero = int(np.argmax(ref.any(axis=0)))
    assert n_zero > OTW_C and not ref[:, :n_zero].any()
    sess = open_session(ref, L, hop)
    try:
        device, oracle_cols, info = run_silent_session(sess, dtype, diff=True)
        for b in range(B):
            sa = sess.otw.state(b)
            for cols in (device[b], oracle_cols[b]):
                o = oracle.OtwOracle(ref, OTW_C, OTW_MRC, variant=oracle.LIVENOTE_V2, cost=oracle.COST_EUCLID)
                o.run(np.ascontiguousarray(cols.T))
                assert np.array_equal(sess.path(b), o.path), b
                assert (sa["t"], sa["j"], sa["status"]) == (o.state["t"], o.state["j"], o.state["status"]), b
            assert tuple(info["positions"][b]) == (sa["t"], sa["j"]) and info["status"][b] == sa["status"], b
        census = si.band_tie_census(ref, np.ascontiguousarray(oracle_cols[0].T), OTW_C, OTW_MRC, "livenote_v2", True)
        assert census["tied_fill"] >= 1 and census["tied_steady"] >= 1 and census["largest"] == OTW_C + 1, census
    finally:
        sess.close()
