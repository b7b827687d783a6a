"""The level gate of the live chain (rts_live_gate: live_level_kernel and live_gate_kernel in csrc/live_gate.h, the
launches in live_enqueue, LiveSession.gate / levels / frame_columns) against tests/live_gate_model.py, at four framing
geometries, hold 0 and 3, float32 and PCM16, with both trackers, both feature kinds and behind the resampler.

The inputs come from tests/test_live_gate_cpu.py, which asserts on the model alone what they contain (an always-loud
stream, digital zeros, a quiet lead-in, gaps of exactly hold, hold + 1 and more columns, pass / drop / pass inside one
feed, a feed that hands nothing on, a gap over three feeds, a restart inside a gap, one NaN sample) and that no level lies
within 1 +- 1e-9 of the threshold, so the GPU's rounding (at most about fft_len * 2^-53 relative) cannot flip a decision.

A WTW session's chroma history is exactly the columns the ingestion handed on: it is compared bit for bit with
ChromaPlan.frames of the kept columns' frames (a frame's value depends neither on its position nor on batching:
test_chroma_paths_gpu.py), within CHROMA_ATOL with the oracle's columns, and is zero behind them.  levels() is compared
with the model at every point where the test synchronises; the largest relative error of a level is printed on an
OBSERVED line (gate fft_len * 2^-52).

Which test fails for which mutation of the device code, by reading:
  * the compaction destination off by one (dest row d + 1, or counts one short): every kept column lands one row late
    in the gated buffer, so the tracker takes a stale row first -- test_wtw_history_follows_the_model fails its
    bit-equality for every stream that ever hands on a column (and test_otw_session its paths).
  * q not carried from feed to feed (every feed starts closed, or starts at 0): with hold = 3 a rest that begins in one
    feed and goes on in the next passes too many or too few columns; `passed` and the history length differ from the
    model in test_wtw_history_follows_the_model[*-3-*] (the gap over three feeds, the restart gap), and with q starting
    at 0 the never-opening stream opens.
  * the previous-passed word not carried: in diff mode the first column of a feed is then never (or always) handed on;
    test_diff_columns_per_feed compares counts and columns after every feed and fails at the first feed that begins
    inside the music (never), or at the first feed behind a dropped column (always).  Not cleared on restart: no
    decision changes -- a restarted stream has no carry, live_diff_kernel makes no difference column for its first
    chroma column, and live_gate_kernel skips that column by the same count (m < skip), whatever the word says; the
    word is cleared so that the state is the defined one, and no test can tell.  What a restart must clear and tests do
    tell: q (test_wtw_history_follows_the_model restarts stream 4 inside a gap, and the zero stream), seen and passed
    (levels() and frame_columns() right after the restart, and every ordinal of the new run).
  * the level taken at m * hop of the staging slot instead of the pending buffer: a column's level is then that of
    other samples (the slot holds only the new ones, at another offset); decisions differ wherever a gap's edge is not
    aligned with the feeds, and `level` itself misses the fft_len * 2^-52 gate in every test that reads levels().
  * ordinals counting passed columns instead of seen columns: frame_columns() then reads 0, 1, 2, .. for every stream;
    the comparison with the model's ordinals fails for every stream with a lead-in or a gap
    (test_wtw_history_follows_the_model).
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from live_gate_model import GateStreamModel  # noqa: E402
from test_chroma_gpu import CHROMA_ATOL  # noqa: E402
from test_chroma_paths_gpu import bit_equal  # noqa: E402
from test_live_diff_cpu import clip_diff  # noqa: E402
from test_live_gate_cpu import (CASES, HOLDS, MIN_DB, MIN_LEVEL, RESTART_STREAMS, S_LEAD, S_LOUD, S_RESTART,  # noqa: E402
                                S_ZERO, build_gate_case, kept_oracle_columns)
from test_live_model_cpu import B, FS, OTW_C, OTW_GEOMETRIES, OTW_MRC, WTW_HOPF, WTW_W, otw_ref, wtw_refs  # noqa: E402
from test_live_paths_gpu import give, history, np_dtype, open_wtw  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_offline = {}


def offline_of_frames(plan, frames, L, hop, key=None):
    """ChromaPlan.frames of the given frames (lists of samples) -> [K][12] float64 numpy: the frames are laid out
    ceil(L / hop) hops apart, which a frame's value does not depend on."""
    if key is not None and key in _offline:
        return _offline[key]
    k = len(frames)
    out = np.zeros((0, 12))
    if k:
        r = -(-L // hop)
        x = np.zeros((k - 1) * r * hop + L, dtype=np.float32)
        for m, s in enumerate(frames):
            x[m * r * hop:m * r * hop + L] = s
        ch, _ = plan.frames(torch.from_numpy(x).to(plan.device), pad_left=0)
        torch.cuda.synchronize()
        out = ch.cpu().numpy()[::r]
        assert out.shape == (k, 12)
    if key is not None:
        _offline[key] = out
    return out


def run_columns(plan, case, b, run, key):
    return offline_of_frames(plan, case.run_slices[b][run], case.L, case.hop, key + (b, run))


class Worst(object):
    level = 0.0


def check_levels(sess, case, i, n_feeds, worst, restarted=()):
    """levels() after a sync against the model's snapshot after schedule entry i."""
    got = sess.levels()
    assert got["feeds_done"] == sess.poll()["feeds_submitted"] == n_feeds
    for b in range(B):
        seen, passed, is_open, level = case.snap[i][b]
        if b in restarted:
            seen, passed, is_open, level = 0, 0, False, float("nan")
        assert (got["seen"][b], got["passed"][b], bool(got["open"][b])) == (seen, passed, is_open), (i, b)
        if math.isnan(level):
            assert math.isnan(got["level"][b]), (i, b)
        elif level == 0.0:
            assert got["level"][b] == 0.0 and got["level_db"][b] == 10 * np.log10(1e-20), (i, b)
        else:
            rel = abs(got["level"][b] - level) / level
            worst.level = max(worst.level, rel)
            assert rel <= case.L * 2.0 ** -52, (i, b, rel)
            assert got["level_db"][b] == 10 * np.log10(min(max(got["level"][b], 1e-20), 1.0)), (i, b)


def run_gated(sess, case, dtype, worst, on_restart=None, after_feed=None, other=None):
    """Feeds the whole schedule; pending() is compared with the (ungated) loop after every feed outside the back-to-back
    submits.  Around the first feed that completes columns and hands none on, the tracker's states are read: they do not
    change.  ``other``: a second session fed the same.  Returns the number of feeds enqueued."""
    from real_time_audio_sync_amd import _native as nat
    dt = np_dtype(dtype)
    src = case.pcm if dt == np.int16 else case.live
    pos, done = [0] * B, 0
    dropped = [k for k, row in enumerate(case.feed_log) if sum(n for n, _ in row) > 0 and sum(h for _, h in row) == 0][0]
    eng = sess.otw or sess.wtw
    for i, f in enumerate(case.feeds):
        if i == case.restart_at:
            for s in (sess, other):
                if s is not None:
                    s.restart(list(RESTART_STREAMS))
            if on_restart:
                on_restart(i, done)
        bufs = [src[b][pos[b]:pos[b] + f["counts"][b]] for b in range(B)]
        if f["refused"]:
            with pytest.raises(nat.RtsyncError):
                give(sess, f["how"], bufs, dt)
            if other is not None:
                with pytest.raises(nat.RtsyncError):
                    give(other, f["how"], bufs, dt)
            continue
        if done == dropped:
            sess.sync()
            before = eng.states().copy()
        give(sess, f["how"], bufs, dt)
        if other is not None:
            give(other, f["how"], bufs, dt)
        done += 1
        if done == dropped + 1:
            sess.sync()
            assert np.array_equal(eng.states(), before)          # consumed counts, positions, status: untouched
            check_levels(sess, case, i, done, worst)
        for b in range(B):
            pos[b] += f["counts"][b]
        in_burst = f["how"] == "submit" and i + 1 < len(case.feeds) and case.feeds[i + 1]["how"] == "submit"
        if not in_burst:
            assert list(sess.pending()) == case.pending[i], i
        if after_feed:
            after_feed(i, done)
    assert pos == case.fed
    return done


@pytest.mark.parametrize("L,hop,hold,dtype", CASES)
def test_wtw_history_follows_the_model(L, hop, hold, dtype):
    """A gated and an ungated WTW session on the same input.  Gated: history, chroma_ptr, pending, levels, ordinals as the
    model says; restart inside a gap; the all-dropped feed.  The always-loud stream is bit-identical in both sessions."""
    from real_time_audio_sync_amd import _native as nat
    case = build_gate_case(L, hop, hold, dtype)
    refs = wtw_refs(case)
    sess, plain = open_wtw(case, refs), open_wtw(case, refs)
    worst = Worst()
    try:
        with pytest.raises(nat.RtsyncError):
            sess.levels()                                        # before the first gate(min_db)
        sess.gate(MIN_DB, hold)
        start = sess.levels()
        assert np.isnan(start["level"]).all() and not start["open"].any() and not start["seen"].any()

        def on_restart(i, done):
            sess.sync()
            check_levels(sess, case, i - 1, done, worst, restarted=RESTART_STREAMS)
            hist = history(sess)
            for b in RESTART_STREAMS:
                assert len(sess.frame_columns(b)) == 0 and not hist[b].any(), b
            for b in set(range(B)) - set(RESTART_STREAMS):       # the others are untouched
                assert list(sess.frame_columns(b)) == case.ordinals_at_restart[b], b

        n = run_gated(sess, case, dtype, worst, on_restart=on_restart, other=plain)
        sess.sync()
        plain.sync()
        check_levels(sess, case, len(case.feeds) - 1, n, worst)
        hist, hist_plain = history(sess), history(plain)
        err = 0.0
        for b in range(B):
            st, kept = sess.wtw.state(b), case.kept[b]
            assert st["status"] == nat.RUNNING and st["chroma_ptr"] == len(kept) == case.models[b].passed, b
            off = run_columns(sess.plan, case, b, len(case.run_slices[b]) - 1, (L, hop, hold, dtype))
            got = hist[b, :len(kept)]
            assert bit_equal(got, off[kept].reshape(-1, 12)), b
            assert not np.isnan(got).any() and not hist[b, len(kept):].any(), b
            if kept:
                err = max(err, float(np.abs(got - kept_oracle_columns(case, b)).max()))
            assert list(sess.frame_columns(b)) == kept, b
        assert err <= CHROMA_ATOL
        # the stream that is always loud: as if there were no gate
        b = S_LOUD
        assert case.kept[b] == list(range(case.n_cols[b])) and bit_equal(hist[b], hist_plain[b])
        assert sess.wtw.state(b) == plain.wtw.state(b) and np.array_equal(sess.wtw.path(b), plain.wtw.path(b))
        assert plain.wtw.state(S_ZERO)["chroma_ptr"] == case.n_cols[S_ZERO] and sess.wtw.state(S_ZERO)["chroma_ptr"] == 0
        if dtype == "float32":
            assert np.isnan(hist_plain[S_LEAD]).any()            # without the gate the NaN frames reach the tracker
        print("OBSERVED live gate L=%d hop=%d hold=%d %s: kept %s of %s columns, level rel err %.3g (gate %.3g), chroma %.3g"
              % (L, hop, hold, dtype, [len(k) for k in case.kept], case.n_cols, worst.level, L * 2.0 ** -52, err))
    finally:
        sess.close()
        plain.close()


@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("L,hop", OTW_GEOMETRIES)
def test_otw_session(L, hop, hold):
    """States, paths and bands equal a BatchedOTW pushed the kept offline columns, and the oracle on the kept oracle
    columns."""
    import oracle
    from real_time_audio_sync_amd.live import LiveSession
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    case = build_gate_case(L, hop, hold, "float32")
    ref = otw_ref(case)
    sess = LiveSession(ref, batch=B, c=OTW_C, max_run_count=OTW_MRC, fft_len=L, hop_size=hop, fs=FS, max_pending=case.cap)
    eng = BatchedOTW(ref, OTW_C, OTW_MRC, batch=B, dtype=torch.float64)
    worst = Worst()
    try:
        sess.gate(MIN_DB, hold)
        n = run_gated(sess, case, "float32", worst)
        sess.sync()
        check_levels(sess, case, len(case.feeds) - 1, n, worst)
        info = sess.poll()
        assert info["feeds_done"] == info["feeds_submitted"] == n
        k = [len(x) for x in case.kept]
        cols = np.zeros((B, max(k), 12))
        for b in range(B):
            off = run_columns(sess.plan, case, b, len(case.run_slices[b]) - 1, (L, hop, hold, "float32"))
            cols[b, :k[b]] = off[case.kept[b]].reshape(-1, 12)
        assert not np.isnan(cols).any()
        eng.push(torch.from_numpy(cols).to(eng.device), torch.tensor(k, dtype=torch.int32, device=eng.device))
        for b in range(B):
            assert np.array_equal(sess.path(b), eng.path(b)), b
            sa, sb = sess.otw.state(b), eng.state(b)
            sa.pop("band_recomputes"), sb.pop("band_recomputes")   # bookkeeping differs with launch granularity
            assert sa == sb, b
            for x, y in zip(sess.otw.bands(b), eng.bands(b)):
                assert np.array_equal(x, y, equal_nan=True), b
            o = oracle.OtwOracle(ref, OTW_C, OTW_MRC)
            o.run(np.ascontiguousarray(kept_oracle_columns(case, b).T))
            assert np.array_equal(sess.path(b), o.path), b
            assert (sa["t"], sa["j"], sa["status"]) == (o.state["t"], o.state["j"], o.state["status"]), b
            assert tuple(info["positions"][b]) == (sa["t"], sa["j"]), b
            assert list(sess.frame_columns(b)) == case.kept[b][:2 * ref.shape[1]], b
        assert len(sess.path(S_LOUD)) > 2 * OTW_C and len(sess.path(S_ZERO)) == 0
    finally:
        eng.close()
        sess.close()


@pytest.mark.parametrize("hold", HOLDS)
def test_diff_columns_per_feed(hold):
    """Difference features: what every feed hands on (last_columns after a sync) is the model's difference columns made of
    ChromaPlan.frames columns, bit for bit, and the end state is that of a push of those columns."""
    import oracle  # noqa: F401
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    from test_live_diff_gpu import diff_reference, open_session, read_columns
    L, hop = 512, 128
    case = build_gate_case(L, hop, hold, "float32", diff=True)
    assert case.cap == L + 5 * hop + 77
    ref = diff_reference(case.live[S_LOUD][:case.fed[S_LOUD]], L, hop)
    sess = open_session(ref, L, hop, batch=B)
    eng = BatchedOTW(ref, OTW_C, OTW_MRC, batch=B, variant="livenote_v2", euclid=True, dtype=torch.float64)
    worst = Worst()
    handed = [[] for _ in range(B)]       # difference columns of the current run, as the model hands them on
    try:
        sess.gate(MIN_DB, hold)
        key = (L, hop, hold, "float32")

        def on_restart(i, done):
            for b in RESTART_STREAMS:
                handed[b] = []

        def after_feed(i, done):
            got, n = read_columns(sess)
            check_levels(sess, case, i, done, worst)
            for b in range(B):
                run, ords = case.feed_handed[done - 1][b]
                assert n[b] == len(ords), (i, b)
                off = run_columns(sess.plan, case, b, run, key)
                want = np.array([clip_diff(off[m - 1:m + 1])[0] for m in ords]).reshape(-1, 12)
                assert bit_equal(got[b], want), (i, b)
                handed[b].append(want)

        n = run_gated(sess, case, "float32", worst, on_restart=on_restart, after_feed=after_feed)
        assert n == len(case.feed_handed)
        # the first column of a run is never handed on, a column behind a dropped one neither
        for b in range(B):
            assert case.kept[b] == [m for m in range(case.n_cols[b]) if m and case.models[b].passes[m]
                                    and case.models[b].passes[m - 1]], b
        assert 0 < len(case.kept[S_RESTART]) < sum(case.models[S_RESTART].passes)
        cols_b = [np.concatenate(h) if h else np.zeros((0, 12)) for h in handed]
        k = [len(x) for x in cols_b]
        assert k == [len(x) for x in case.kept]
        cols = np.zeros((B, max(k), 12))
        for b in range(B):
            cols[b, :k[b]] = cols_b[b]
        assert not np.isnan(cols).any()
        eng.push(torch.from_numpy(cols).to(eng.device), torch.tensor(k, dtype=torch.int32, device=eng.device))
        for b in range(B):
            assert np.array_equal(sess.path(b), eng.path(b)), b
            sa, sb = sess.otw.state(b), eng.state(b)
            sa.pop("band_recomputes"), sb.pop("band_recomputes")
            assert sa == sb, b
            assert list(sess.frame_columns(b)) == case.kept[b][:2 * ref.shape[1]], b
        print("OBSERVED live gate diff hold=%d: handed %s of %s chroma columns, level rel err %.3g" %
              (hold, k, case.n_cols, worst.level))
    finally:
        eng.close()
        sess.close()


def test_gate_only_before_the_first_feed():
    """After a feed rts_live_gate is refused and the session carries on unchanged; after reset() it is accepted, and
    gate(None) then gives the ungated result."""
    from real_time_audio_sync_amd import _native as nat
    L, hop, hold = 512, 128, 3
    case = build_gate_case(L, hop, hold, "float32")
    refs = wtw_refs(case)
    sess, plain = open_wtw(case, refs), open_wtw(case, refs)
    try:
        for bad in (float("nan"), float("inf")):
            with pytest.raises(nat.RtsyncError):
                sess.gate(bad)
        with pytest.raises(nat.RtsyncError):
            sess.gate(MIN_DB, hold=-1)
        with pytest.raises(nat.RtsyncError):
            sess.gate(MIN_DB, hold=65536)
        assert nat.lib.rts_live_gate(sess._h, -1e-6, 0) == -1
        sess.gate(MIN_DB, hold)
        x = [case.live[b][:2 * L] for b in range(B)]
        sess.feed(x, wait=True)
        with pytest.raises(nat.RtsyncError) as e:
            sess.gate(None)
        assert "first feed" in str(e.value)
        with pytest.raises(nat.RtsyncError):
            sess.gate(-20.0, 0)
        y = [case.live[b][2 * L:2 * L + 6 * hop] for b in range(B)]
        sess.feed(y, wait=True)                                  # still gated with the first setting
        models = [GateStreamModel(L, hop, MIN_LEVEL, hold) for _ in range(B)]
        for b in range(B):
            models[b].feed(x[b])
            models[b].feed(y[b])
        got = sess.levels()
        assert list(got["passed"]) == [m.passed for m in models] and list(got["seen"]) == [m.seen for m in models]
        assert [sess.wtw.state(b)["chroma_ptr"] for b in range(B)] == [m.passed for m in models]
        assert got["passed"][S_LOUD] == got["seen"][S_LOUD] > 0 and got["passed"][S_ZERO] == 0
        # reset keeps the setting and closes every stream
        sess.reset()
        got = sess.levels()
        assert not got["seen"].any() and not got["open"].any() and np.isnan(got["level"]).all()
        sess.feed(x, wait=True)
        assert list(sess.levels()["passed"]) == [len(m.per_feed[0][1]) for m in models]
        sess.reset()
        sess.gate(None)
        for s in (sess, plain):
            s.feed(x)
            s.feed(y, wait=True)
        assert bit_equal(history(sess), history(plain))
        assert [sess.wtw.state(b) for b in range(B)] == [plain.wtw.state(b) for b in range(B)]
        assert sess.wtw.state(S_ZERO)["chroma_ptr"] == models[S_ZERO].seen > 0
        cols, n = sess.last_columns()
        cols_p, n_p = plain.last_columns()
        assert torch.equal(n, n_p) and torch.equal(cols, cols_p)
    finally:
        sess.close()
        plain.close()


def test_resampled_session():
    """fs_in = 48000: decisions and kept columns equal the model run on the one-shot resampling of each stream's input
    (the prefix property: a stream fed n samples has handed on the first avail(n) of them)."""
    from real_time_audio_sync_amd import _native as nat
    from real_time_audio_sync_amd import chroma
    from real_time_audio_sync_amd.live import LiveSession
    L, hop, hold = 512, 128, 3
    case = build_gate_case(L, hop, hold, "int16")                # float32 of PCM16, no NaN
    refs = wtw_refs(case)
    sess = LiveSession(refs, batch=B, fft_len=L, hop_size=hop, fs=FS, max_pending=case.cap, fs_in=48000,
                       wtw_params={'dtw_win_size': WTW_W * hop, 'dtw_hop_size': WTW_HOPF * hop})
    try:
        sess.gate(MIN_DB, hold)
        one_shot = [np.asarray(chroma.resample(case.live[b][:case.fed[b]], 48000, FS)) for b in range(B)]
        models = [GateStreamModel(L, hop, MIN_LEVEL, hold) for _ in range(B)]
        pos, n = [0] * B, 0
        for f in case.feeds:
            if f["refused"]:
                continue
            sess.feed([case.live[b][pos[b]:pos[b] + f["counts"][b]] for b in range(B)])
            n += 1
            for b in range(B):
                a0, a1 = sess.resampler.avail(pos[b]), sess.resampler.avail(pos[b] + f["counts"][b])
                models[b].feed(one_shot[b][a0:a1])
                pos[b] += f["counts"][b]
            assert list(sess.pending()) == [len(m.loop.buf) for m in models]
        sess.sync()
        got = sess.levels()
        assert got["feeds_done"] == n
        hist = history(sess)
        worst = 0.0
        for b in range(B):
            m = models[b]
            for lv in m.levels:
                assert not (MIN_LEVEL * (1 - 1e-9) <= lv <= MIN_LEVEL * (1 + 1e-9)), (b, lv)
            assert (got["seen"][b], got["passed"][b], bool(got["open"][b])) == (m.seen, m.passed, m.open), b
            if m.seen and m.level > 0:
                worst = max(worst, abs(got["level"][b] - m.level) / m.level)
            off = offline_of_frames(sess.plan, m.loop.slices, L, hop)
            assert sess.wtw.state(b)["chroma_ptr"] == m.passed and sess.wtw.state(b)["status"] == nat.RUNNING, b
            assert bit_equal(hist[b, :m.passed], off[m.ordinals].reshape(-1, 12)) and not hist[b, m.passed:].any(), b
            assert list(sess.frame_columns(b)) == m.ordinals, b
        assert worst <= L * 2.0 ** -52
        kept = [m.passed for m in models]
        assert kept[S_ZERO] == 0 and kept[S_LOUD] == models[S_LOUD].seen > 5 and 0 < kept[S_LEAD] < models[S_LEAD].seen
        print("OBSERVED live gate resampled 48000 -> %d: kept %s of %s, level rel err %.3g" %
              (FS, kept, [m.seen for m in models], worst))
    finally:
        sess.close()


def test_frame_columns_after_reacquire():
    """reacquire() restarts a stream, which empties its ordinals, and pushes the excerpt into the tracker itself: those
    frames read -1 in frame_columns, the columns of the feeds that follow count from 0, and restart() drops both."""
    from real_time_audio_sync_amd.live import LiveSession
    from test_chroma_paths_gpu import synth
    from test_reacquire_gpu import _packed, lost_case
    pieces, heard, A = lost_case()
    p0, p1, p2 = pieces
    L, hop = 512, 256
    sess = LiveSession([p0, p2], batch=2, c=50, fft_len=L, hop_size=hop, extra_refs=[p1], max_pending=4096)
    try:
        sess.gate(MIN_DB, 0)
        sess.otw.push(*_packed([heard["lost"], heard["lost"][:, :0]], torch.float64))
        got = sess.reacquire([0, 1], M=64)
        assert got[1] is None and got[0][0] is p1
        n = sess.otw.state(0)["consumed"]
        assert n == 64 and list(sess.frame_columns(0)) == [-1] * n and len(sess.frame_columns(1)) == 0
        x = synth(L + 4 * hop, hop, 3)
        sess.feed([x, x[:L + hop] * np.float32(2.0 ** -12)], wait=True)
        assert list(sess.frame_columns(0)) == [-1] * n + [0, 1, 2, 3, 4] and sess.otw.state(0)["consumed"] == n + 5
        assert len(sess.frame_columns(1)) == 0 and list(sess.levels()["seen"]) == [5, 2]
        sess.restart([0])
        assert len(sess.frame_columns(0)) == 0
    finally:
        sess.close()
