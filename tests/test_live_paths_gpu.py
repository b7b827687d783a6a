"""The device-side live ingestion (csrc/live.hip: live_append_kernel, live_compact_kernel, the staging ring, the host
mirror of the pending counts) checked column by column, at six framing geometries, against the reference's own loop.

Sessions run with the WTW tracker, whose live chroma history [B][2M][12] (rts_wtw_device_views) is the very columns the
ingestion produced.  Per stream the history is compared three ways: bit for bit with ChromaPlan.frames on the same
plan over all samples of the stream (a frame's value depends neither on its position nor on batching:
test_chroma_paths_gpu.py::test_frame_values_do_not_depend_on_position, ::test_frames_batch_ragged_streams -- so any
difference is a sample that the append or the compaction put in the wrong place); within CHROMA_ATOL of the oracle
columns of oracle.chroma_oracle.LiveLoopModel; and exactly zero past the model's column count, with chroma_ptr equal to
it.  After every feed the host mirror (pending()) equals the model's len(buf); at the end poll() equals the tracker's
own state.  The OTW tracker keeps no readable history and is checked at state level against a BatchedOTW push of the
offline columns (bit-equal) and against oracle.OtwOracle.

Schedules, audio and tracker sizes come from tests/test_live_model_cpu.py, which asserts on the reference alone that
every schedule holds the boundary feeds (pending fft_len - 1, fft_len, fft_len + hop - 1, max_pending with cols_cap
columns, a refused feed, one-sample feeds, zero-count runs, a feed without a column, 14 feeds back to back), that
adjacent oracle columns differ by >= 1000 * CHROMA_ATOL and that the trackers stay RUNNING.

What three mutations of live.hip would break, by reading:
  * the compaction moving rem - 1 elements: after every drop the last pending sample, buf[rem - 1], keeps what lay there
    before.  rem < fft_len after every drop, so that sample lies inside the stream's next frame, and the next column
    differs from ChromaPlan.frames: the bit-equality in check_history fails for every stream at every geometry (and the
    oracle gate with it, one wrong sample in a frame is far above 1e-11).
  * the append slice bound hi one short: every slice leaves its last sample unwritten, a stale value inside a frame,
    so the same bit-equality fails; the one-sample feeds (per = 1) then append nothing at all and stream 2 has no
    correct column.  hi one long: slices overlap harmlessly, but the last slice writes dst[n], which the next append
    overwrites -- except in the feed that fills stream 1 to exactly max_pending, where dst[n] is sample 0 of stream
    2's buffer: stream 2's next column fails the bit-equality.  That feed exists in every schedule for this reason.
  * the int16 source offset taken in floats (the offset added to a float pointer before the cast): stream b reads its
    PCM from twice its offset, other samples for every stream behind the first non-empty one.  All int16 cases fail
    the bit-equality and the oracle gate for those streams; the float32 cases pass.  Counts are mostly odd, so an
    offset taken in bytes or rounded to a pair would show as well.

19 test cases.  Largest |delta| of a history column against the oracle (gate CHROMA_ATOL = 1e-11): the tests print it
per case on an OBSERVED line before they assert (run with -s).
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_chroma_gpu import CHROMA_ATOL  # noqa: E402
from test_chroma_paths_gpu import bit_equal  # noqa: E402
from test_live_model_cpu import (B, FS, GEOMETRIES, OTW_C, OTW_GEOMETRIES, OTW_MRC, RESTART_GEOMETRY,  # noqa: E402
                                 RESTART_STREAMS, WTW_HOPF, WTW_W, build_case, otw_ref, wtw_refs)
from test_restart_gpu import _device_to_host  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def np_dtype(name):
    return np.int16 if name == "int16" else np.float32


def open_wtw(case, refs, extra=()):
    from real_time_audio_sync_amd.live import LiveSession
    return LiveSession(refs, batch=B, fft_len=case.L, hop_size=case.hop, fs=FS, max_pending=case.cap,
                       wtw_params={'dtw_win_size': WTW_W * case.hop, 'dtw_hop_size': WTW_HOPF * case.hop},
                       extra_refs=extra)


def give(sess, how, bufs, dt):
    if how == "block":
        sess.feed_block(np.stack(bufs))
    elif how == "submit":                      # straight into the pinned slot; nothing is read, polled or synchronised
        cv, sv = sess.staging(dt)
        off = 0
        for b, x in enumerate(bufs):
            cv[b] = len(x)
            sv[off:off + len(x)] = x
            off += len(x)
        sess.submit(dt)
    else:
        sess.feed(bufs)


def run_schedule(sess, case, dtype, on_restart=None):
    """Feeds the whole schedule; pending() is compared with the model after every feed, except inside the run of
    back-to-back submits, where it is compared after the last one.  Returns the number of feeds enqueued."""
    from real_time_audio_sync_amd import _native as nat
    dt = np_dtype(dtype)
    src = case.pcm if dt == np.int16 else case.live
    pos = [0] * B
    done = 0
    for i, f in enumerate(case.feeds):
        if i == case.restart_at:
            on_restart(i)
        bufs = [src[b][pos[b]:pos[b] + f["counts"][b]] for b in range(B)]
        assert [len(x) for x in bufs] == f["counts"]
        if f["refused"]:
            with pytest.raises(nat.RtsyncError):
                give(sess, f["how"], bufs, dt)
            assert list(sess.pending()) == case.pending[i] == case.pending[i - 1], i
            continue
        give(sess, f["how"], bufs, dt)
        done += 1
        for b in range(B):
            pos[b] += f["counts"][b]
        in_burst = f["how"] == "submit" and i + 1 < len(case.feeds) and case.feeds[i + 1]["how"] == "submit"
        if not in_burst:
            assert list(sess.pending()) == case.pending[i], i
    assert pos == case.fed
    return done


def history(sess):
    from real_time_audio_sync_amd import _native as nat
    lc, rows = ctypes.c_void_p(), ctypes.c_int()
    nat.check(nat.lib.rts_wtw_device_views(sess.wtw._h, ctypes.byref(lc), ctypes.byref(rows), None))
    return _device_to_host(lc.value, (B, rows.value, 12))


def offline_columns(plan, case, b):
    """ChromaPlan.frames on the same plan over the samples of stream b's current run -> [K][12] float64 (numpy)."""
    k = case.n_cols[b]
    if k == 0:
        return np.zeros((0, 12))
    L, hop = case.L, case.hop
    if hop <= L:
        x = case.live[b][case.since[b]:case.fed[b]]
        assert case.models[b].starts == [m * hop for m in range(k)] and (len(x) - L) // hop + 1 == k
    else:   # the clamp: columns start where the model says; laid out hop apart, which a frame's value does not depend on
        x = np.zeros((k - 1) * hop + L, dtype=np.float32)
        for m, s in enumerate(case.models[b].slices):
            x[m * hop:m * hop + L] = s
    ch, _ = plan.frames(torch.from_numpy(np.ascontiguousarray(x)).to(plan.device), pad_left=0)
    torch.cuda.synchronize()
    assert ch.shape == (k, 12) and ch.dtype == torch.float64
    return ch.cpu().numpy()


def check_history(sess, case, n_feeds, label):
    """After the last feed: poll() against the tracker's own state, the history three ways.  Returns the largest error
    against the oracle."""
    from real_time_audio_sync_amd import _native as nat
    sess.sync()
    info = sess.poll()
    assert info["feeds_done"] == info["feeds_submitted"] == n_feeds
    states = sess.wtw.states()
    hist = history(sess)
    worst = 0.0
    for b in range(B):
        st = sess.wtw.state(b)
        k = case.n_cols[b]
        assert st["status"] == nat.RUNNING == info["status"][b], (label, b)
        assert tuple(info["positions"][b]) == (st["live_ptr"], st["ref_ptr"]) == (states[b][1], states[b][2]), (label, b)
        assert st["chroma_ptr"] == k, (label, b)
        assert k <= hist.shape[1]
        got = hist[b, :k]
        assert bit_equal(got, offline_columns(sess.plan, case, b)), (label, b)
        if k:
            err = float(np.abs(got - case.oracle_cols[b]).max())
            worst = max(worst, err)
            assert err <= CHROMA_ATOL, (label, b, err)
        assert not hist[b, k:].any(), (label, b)
    assert sess.stopped() == []
    assert sum(sess.wtw.state(b)["windows"] for b in range(B)) > B
    print("OBSERVED live ingestion %-28s cols=%-5d chroma=%.3g" % (label, sum(case.n_cols), worst))
    return worst


@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("L,hop", GEOMETRIES)
def test_history_columns_follow_the_model(L, hop, dtype):
    case = build_case(L, hop)
    sess = open_wtw(case, wtw_refs(case))
    try:
        n = run_schedule(sess, case, dtype)
        check_history(sess, case, n, "L=%d hop=%d %s" % (L, hop, dtype))
        # the session is still usable: a reset and the first frame again
        sess.reset()
        assert not sess.pending().any()
        sess.feed([case.live[b][:L] for b in range(B)], wait=True)
        assert list(sess.pending()) == [max(L - hop, 0)] * B
        assert [sess.wtw.state(b)["chroma_ptr"] for b in range(B)] == [1] * B
    finally:
        sess.close()


@pytest.mark.parametrize("dtype", ["float32", "int16"])
def test_restart_in_mid_run_with_per_stream_references(dtype):
    """Per-stream references of different lengths; two streams are restarted in mid-run (one onto a spare piece) while
    holding pending samples: pending reads 0, their history reads zero, then holds the new run's columns from row 0 --
    fewer than the old run had, so stale rows would show -- and no sample fed before the restart is in any of them."""
    L, hop = RESTART_GEOMETRY
    case = build_case(L, hop, True)
    refs = wtw_refs(case, per_stream=True)
    sess = open_wtw(case, refs[:B], extra=refs[B:])

    def restart(i):
        before = list(sess.pending())
        assert before == case.pending[i - 1] == case.pending_at_restart
        sess.restart(list(RESTART_STREAMS), refs=[refs[RESTART_STREAMS[0]], refs[B]])
        after = list(sess.pending())
        assert after == [0 if b in RESTART_STREAMS else before[b] for b in range(B)]
        sess.sync()
        hist = history(sess)
        info = sess.poll()
        for b in range(B):
            if b in RESTART_STREAMS:
                assert not hist[b].any() and tuple(info["positions"][b]) == (0, 0), b
                assert sess.wtw.state(b)["chroma_ptr"] == 0

    try:
        n = run_schedule(sess, case, dtype, on_restart=restart)
        check_history(sess, case, n, "L=%d hop=%d %s restart" % (L, hop, dtype))
    finally:
        sess.close()


def test_mixed_int16_and_float_buffers_in_one_feed():
    """LiveSession.feed with int16 next to float32 buffers, the dtype of every stream alternating from feed to feed (so
    frames hold samples of both kinds): the history equals, bit for bit, that of a session fed the scaled float32
    values, and the offline columns."""
    L, hop = 512, 128
    case = build_case(L, hop)
    refs = wtw_refs(case)
    mixed, plain = open_wtw(case, refs), open_wtw(case, refs)
    try:
        pos = [0] * B
        n = n_mixed = 0
        for i, f in enumerate(case.feeds):
            if f["refused"]:
                continue
            a, c = [], []
            for b in range(B):
                k = f["counts"][b]
                sl = slice(pos[b], pos[b] + k)
                a.append(None if k == 0 else case.pcm[b][sl] if (b + i) % 2 == 0 else case.live[b][sl])
                c.append(None if k == 0 else case.live[b][sl])
                pos[b] += k
            kinds = set(x.dtype for x in a if x is not None)
            n_mixed += len(kinds) == 2
            mixed.feed(a)
            plain.feed(c)
            n += 1
            assert list(mixed.pending()) == list(plain.pending()) == case.pending[i]
        assert n_mixed >= 20
        check_history(plain, case, n, "L=%d hop=%d all float32" % (L, hop))
        check_history(mixed, case, n, "L=%d hop=%d mixed feeds" % (L, hop))
        assert bit_equal(history(mixed), history(plain))
    finally:
        mixed.close()
        plain.close()


@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("L,hop", OTW_GEOMETRIES)
def test_otw_state_follows_the_offline_push_and_the_oracle(L, hop, dtype):
    """The same schedules into an OTW session: path, state and both bands equal a BatchedOTW that is pushed the offline
    ChromaPlan.frames columns in one go (bit-equal columns in, so everything out is equal), and path and (t, j, status)
    equal oracle.OtwOracle on the model's oracle columns (test_live_model_cpu.py asserts that this reference makes the
    oracle take row, column and both steps)."""
    import oracle
    from real_time_audio_sync_amd.live import LiveSession
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    case = build_case(L, hop)
    ref = otw_ref(case)
    sess = LiveSession(ref, batch=B, c=OTW_C, max_run_count=OTW_MRC, fft_len=L, hop_size=hop, fs=FS,
                       max_pending=case.cap)
    eng = BatchedOTW(ref, OTW_C, OTW_MRC, batch=B, dtype=torch.float64)
    try:
        n = run_schedule(sess, case, dtype)
        sess.sync()
        info = sess.poll()
        assert info["feeds_done"] == info["feeds_submitted"] == n
        cols = np.zeros((B, max(case.n_cols), 12))
        for b in range(B):
            cols[b, :case.n_cols[b]] = offline_columns(sess.plan, case, b)
        eng.push(torch.from_numpy(cols).to(eng.device),
                 torch.tensor(case.n_cols, dtype=torch.int32, device=eng.device))
        statuses = set()
        for b in range(B):
            assert np.array_equal(sess.path(b), eng.path(b)), b
            sa, sb = sess.otw.state(b), eng.state(b)
            sa.pop("band_recomputes"), sb.pop("band_recomputes")   # bookkeeping differs with launch granularity
            assert sa == sb, b
            for x, y in zip(sess.otw.bands(b), eng.bands(b)):
                assert np.array_equal(x, y, equal_nan=True), b
            o = oracle.OtwOracle(ref, OTW_C, OTW_MRC)
            o.run(case.oracle_cols[b].T)
            assert np.array_equal(sess.path(b), o.path), b
            assert (sa["t"], sa["j"], sa["status"]) == (o.state["t"], o.state["j"], o.state["status"]), b
            assert tuple(info["positions"][b]) == (sa["t"], sa["j"]) and info["status"][b] == sa["status"], b
            statuses.add(sa["status"])
        assert oracle.RUNNING in statuses
        assert sess.stopped() == [b for b in range(B) if sess.otw.state(b)["status"] == oracle.STOP_REF_END]
    finally:
        eng.close()
        sess.close()


# ---- digital silence ------------------------------------------------------------------------------------------------------

def run_silent_session(sess, dtype, diff=False):
    """Feeds tests/silence_inputs.py::silent_audio to a 4-stream session in feeds of 421 samples and returns, per stream,
    the columns the feeds handed to the tracker (read through last_columns after every feed), after checking them: bit for
    bit ChromaPlan.frames on the same plan over all samples (their clip-diff with ``diff``), within the chroma gate of the
    oracle's columns, and a column whose whole frame is silent exactly zero in both -- zero, not NaN."""
    import silence_inputs as si
    from test_live_diff_cpu import clip_diff
    from test_live_diff_gpu import offline_chroma, oracle_chroma, read_columns
    pcm, flt, sil = si.silent_audio()
    src = pcm if dtype == "int16" else flt
    L, hop = si.LIVE_L, si.LIVE_HOP
    got = [[] for _ in range(4)]
    n = len(flt[0])
    for a in range(0, n, 421):
        sess.feed([x[a:a + 421] for x in src])
        cols, _ = read_columns(sess)
        for b in range(4):
            got[b].append(cols[b])
    info = sess.poll()
    assert info["feeds_done"] == info["feeds_submitted"] == (n + 420) // 421
    device, oracle_cols = [], []
    for b in range(4):
        have = np.concatenate(got[b])
        off = offline_chroma(sess.plan, flt[b], L, hop).cpu().numpy()
        orc = oracle_chroma(flt[b], L, hop)
        assert off.shape == orc.shape == (si.LIVE_COLS + 1, 12)
        silent = si.silent_columns(sil[b], len(off))
        assert len(silent) == (0 if sil[b] is None else si.LIVE_SILENT_COLS), b
        assert not off[silent].any() and not orc[silent].any(), b      # exactly zero, and therefore not NaN
        rest = [m for m in range(len(off)) if m not in silent]
        assert off[rest].any(axis=1).all() and not np.isnan(off).any() and not np.isnan(orc).any(), b
        assert np.abs(off - orc).max() <= CHROMA_ATOL, b
        if diff:
            off, orc = clip_diff(off), clip_diff(orc)
        assert bit_equal(have, off), b
        device.append(have)
        oracle_cols.append(orc)
    return device, oracle_cols, info


@pytest.mark.parametrize("dtype", ["float32", "int16"])
def test_silence_into_an_otw_session(dtype):
    """int16 zeros and float32 zeros from the first sample, for 30 frames in the middle, and beginning and ending half a
    hop into a hop: the silent chroma columns are all zeros, cost exactly 1.0 against every reference frame, and the OTW
    session equals the oracle chain (chroma oracle -> OtwOracle) in path, position and status."""
    import oracle
    import silence_inputs as si
    from oracle import chroma_oracle as co
    from real_time_audio_sync_amd.live import LiveSession
    L, hop = si.LIVE_L, si.LIVE_HOP
    x, h2 = si.silent_audio()[1][3], hop * 5 // 4                # the stream without silence at another tempo
    ref = np.ascontiguousarray(co.live_loop_columns([x[m * h2:m * h2 + L] for m in range((len(x) - L) // h2 + 1)], L, FS).T)
    sess = LiveSession(ref, batch=4, c=OTW_C, max_run_count=OTW_MRC, fft_len=L, hop_size=hop, fs=FS,
                       max_pending=L + 5 * hop + 77)
    try:
        device, oracle_cols, info = run_silent_session(sess, dtype)
        for b in range(4):
            sa = sess.otw.state(b)
            for cols in (device[b], oracle_cols[b]):
                o = oracle.OtwOracle(ref, OTW_C, OTW_MRC)
                o.run(np.ascontiguousarray(cols.T))
                assert np.array_equal(sess.path(b), o.path), b
                assert (sa["t"], sa["j"], sa["status"]) == (o.state["t"], o.state["j"], o.state["status"]), b
            assert tuple(info["positions"][b]) == (sa["t"], sa["j"]) and info["status"][b] == sa["status"], b
    finally:
        sess.close()


@pytest.mark.parametrize("dtype", ["float32", "int16"])
def test_silence_into_a_wtw_session(dtype):
    """The same audio into a WTW session: a silent column is all zeros in the history, its costs are NaN (wtw.py:169), and
    windows that lie partly and wholly inside the silence run.  History, path, pointers and status equal the oracle chain
    (chroma oracle -> WtwOracle)."""
    import oracle
    import silence_inputs as si
    from real_time_audio_sync_amd import synth as rsynth
    from real_time_audio_sync_amd.live import LiveSession
    L, hop = si.LIVE_L, si.LIVE_HOP
    k = si.LIVE_COLS + 1
    ref = rsynth.synth_ref((k // WTW_HOPF + 1) * (WTW_W - 1) + WTW_W + 8 + k // 4, seed=L + hop)   # wtw_ref_frames
    sess = LiveSession(ref, batch=4, fft_len=L, hop_size=hop, fs=FS, max_pending=L + 5 * hop + 77,
                       wtw_params={'dtw_win_size': WTW_W * hop, 'dtw_hop_size': WTW_HOPF * hop})
    try:
        device, oracle_cols, info = run_silent_session(sess, dtype)
        lc, rows = ctypes.c_void_p(), ctypes.c_int()
        from real_time_audio_sync_amd import _native as nat
        nat.check(nat.lib.rts_wtw_device_views(sess.wtw._h, ctypes.byref(lc), ctypes.byref(rows), None))
        hist = _device_to_host(lc.value, (4, rows.value, 12))
        shares = []
        for b in range(4):
            st = sess.wtw.state(b)
            assert st["chroma_ptr"] == k and bit_equal(hist[b, :k], device[b]) and not hist[b, k:].any(), b
            for cols in (device[b], oracle_cols[b]):
                rec = si.wtw_window_record(ref, np.ascontiguousarray(cols.T), WTW_W, WTW_HOPF)
                assert np.array_equal(sess.wtw.path(b), rec["path"]), b
                assert (st["live_ptr"], st["ref_ptr"], st["status"], st["windows"]) == (
                    rec["live_ptr"], rec["ref_ptr"], rec["status"], len(rec["windows"])), b
            assert tuple(info["positions"][b]) == (st["live_ptr"], st["ref_ptr"]) and info["status"][b] == st["status"], b
            shares.append([w[2] for w in rec["windows"]])
        for b in range(3):
            assert any(0 < s < 1 for s in shares[b]) and any(s == 1 for s in shares[b]), (b, shares[b])
        assert not any(shares[3])
    finally:
        sess.close()
