"""Tempo on the device (csrc/tempo.hip) against the plain-Python model of the definition (tests/tempo_model.py, itself held
to closed forms in tests/test_tempo_cpu.py): the curve kernel on a ragged batch that crosses every chunk and wave
boundary, the tail kernel on OTW and WTW handles, and the words a live session publishes with every feed, for both
trackers, across a restart, with and without annotations.  Floats are compared bit for bit."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import tempo_model as tm  # noqa: E402
from conftest import GOLDEN  # noqa: E402
from guarded import guarded, holds_fill, same_bytes  # noqa: E402
from real_time_audio_sync_amd import evaluate, synth  # noqa: E402

REF_CSV = os.path.join(GOLDEN, "chopin_rubinstein_20b.csv")
LIVE_CSV = os.path.join(GOLDEN, "chopin_rachmaninoff_20b.csv")
FS = evaluate.FRAME_SECONDS
DEV = "cuda:0"

LENGTHS = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097]
KS = [2, 3, 64, 256, 1000, 1024]
X_LIMIT = 1 << 22
Y_LIMIT = 1 << 21           # 1024^2 * 2^22 * 2^21 = 2^63 is refused: K = 1024 runs with y_limit_for(K)
P_MAX = 4100


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def walk(rs, n, x0=0, y0=0):
    """A monotone random walk of n points with steps in {(1, 0), (0, 1), (1, 1)}."""
    steps = np.array([(1, 0), (0, 1), (1, 1)])[rs.randint(0, 3, size=max(n - 1, 0))]
    pts = np.zeros((n, 2), dtype=np.int64)
    if n:
        pts[0] = (x0, y0)
        pts[1:] = np.cumsum(steps, axis=0).reshape(-1, 2) + (x0, y0)
    return pts


@pytest.fixture(scope="module")
def ragged():
    """B = 17 paths of LENGTHS points: random walks, but one all-same-x path, one near x_limit = 2^22 (64-bit products), and
    one with a negative and an over-limit point in the middle."""
    rs = np.random.RandomState(5)
    paths = [walk(rs, n) for n in LENGTHS]
    same_x = LENGTHS.index(257)
    paths[same_x][:, 0] = 7
    paths[same_x][:, 1] = np.arange(257)
    big = LENGTHS.index(2049)
    paths[big] = walk(rs, 2049, X_LIMIT - 2049 - 5, Y_LIMIT - 2049 - 5)
    assert paths[big][:, 0].max() < X_LIMIT and paths[big][:, 1].max() < Y_LIMIT and paths[big][-1, 0] > X_LIMIT - 1500
    bad = LENGTHS.index(4097)
    paths[bad][1500] = (-1, paths[bad][1500, 1])
    paths[bad][2600] = (paths[bad][2600, 0], Y_LIMIT)               # y == y_limit: outside
    host = np.zeros((len(LENGTHS), P_MAX, 2), dtype=np.int32)
    for b, p in enumerate(paths):
        host[b, :len(p)] = p
        host[b, len(p):] = (-7, 1 << 30)                            # behind len: never read into a window
    return paths, host


def y_limit_for(K):
    return Y_LIMIT if K < 1024 else Y_LIMIT - 1


@pytest.fixture(scope="module")
def model(ragged):
    """The model's curves of every path at every K (ahead = 0 and ahead = 2.5), computed once."""
    paths, _ = ragged
    out = {}
    for K in KS:
        for ahead in (0.0, 2.5):
            if ahead and K not in (3, 256):
                continue
            out[K, ahead] = [tm.curve(p.tolist(), K, ahead, X_LIMIT, y_limit_for(K)) for p in paths]
    return out


@pytest.mark.parametrize("K", KS)
def test_curve_equals_the_model(ragged, model, K):
    from real_time_audio_sync_amd import _native as nat
    paths, host = ragged
    B = len(paths)
    want = model[K, 0.0]
    flat = np.concatenate([np.array(w[0]) for w in want if len(w[0])])
    assert np.isfinite(flat).sum() > 1000 and np.isnan(flat).sum() > 250            # both kinds of result are checked
    bad = LENGTHS.index(4097)
    nan_at = set(np.nonzero(np.isnan(np.array(want[bad][0])))[0].tolist())
    covered = {0} | set(range(1500, min(1500 + K, 4097))) | set(range(2600, min(2600 + K, 4097)))
    assert covered <= nan_at and (K < 64 or covered == nan_at)     # exactly the windows that contain a bad point (short
    #                                                                windows are NaN on a vertical run of the walk as well)
    assert np.isnan(np.array(want[LENGTHS.index(257)][0])).all()                    # the live index never moves
    path_d = torch.from_numpy(host).to(DEV)
    len_d = torch.tensor(LENGTHS, dtype=torch.int32, device=DEV)
    for fill, with_pos in ((0xFF, True), (0x55, True), (0x55, False)):
        slope, check_slope = guarded((B, P_MAX), torch.float64, DEV, fill)
        pos, check_pos = guarded((B, P_MAX), torch.float64, DEV, fill)
        nat.check(nat.lib.rts_path_tempo(path_d.data_ptr(), P_MAX, len_d.data_ptr(), B, K, 0.0, X_LIMIT, y_limit_for(K),
                                         slope.data_ptr(), pos.data_ptr() if with_pos else None, None))
        torch.cuda.synchronize()
        check_slope("slope_dev")
        check_pos("pos_dev")
        slope, pos = slope.cpu().numpy(), pos.cpu().numpy()
        for b, n in enumerate(LENGTHS):
            assert same_bytes(slope[b, :n], np.array(want[b][0], dtype=np.float64)), (fill, b, n)
            assert holds_fill(slope[b, n:], fill), (fill, b)                        # entries behind len: untouched
            if with_pos:
                assert same_bytes(pos[b, :n], np.array(want[b][1], dtype=np.float64)), (fill, b, n)
                assert holds_fill(pos[b, n:], fill), (fill, b)
        if not with_pos:
            assert holds_fill(pos, fill)


@pytest.mark.parametrize("K", [3, 256])
def test_curve_ahead_and_the_wrappers(ragged, model, K):
    from real_time_audio_sync_amd import tempo
    paths, host = ragged
    want = model[K, 2.5]
    slope, pos = tempo.path_tempo(torch.from_numpy(host).to(DEV), LENGTHS, K, ahead=2.5, x_limit=X_LIMIT, y_limit=Y_LIMIT)
    slope, pos = slope.cpu().numpy(), pos.cpu().numpy()
    for b, n in enumerate(LENGTHS):
        assert same_bytes(slope[b, :n], np.array(want[b][0], dtype=np.float64)), b
        assert same_bytes(pos[b, :n], np.array(want[b][1], dtype=np.float64)), b
    assert any(not same_bytes(np.array(want[b][1]), np.array(model[K, 0.0][b][1])) for b in range(len(paths)))
    # the list form takes its limits from the largest coordinate: the over-limit point of the last path is then inside
    good = paths[:-1]
    got = tempo.tempo_curves(good, K, ahead=2.5, device=DEV)
    top = max(int(p.max()) for p in good if len(p)) + 1
    for b, p in enumerate(good):
        s, q = tm.curve(p.tolist(), K, 2.5, top, top)
        assert same_bytes(got[b][0], np.array(s, dtype=np.float64)) and same_bytes(got[b][1], np.array(q, dtype=np.float64)), b


def test_curve_lengths_outside_the_buffer(ragged, model):
    """len <= 0 (the -1 fault marker of rts_dtw_paths included) writes nothing; len > P_max is clamped."""
    from real_time_audio_sync_amd import _native as nat
    paths, host = ragged
    b = LENGTHS.index(1025)
    path_d = torch.from_numpy(np.ascontiguousarray(host[[b, b, b]][:, :600])).to(DEV)
    len_d = torch.tensor([-1, 10 ** 6, 0], dtype=torch.int32, device=DEV)
    slope, check_slope = guarded((3, 600), torch.float64, DEV, 0x55)
    pos, check_pos = guarded((3, 600), torch.float64, DEV, 0x55)
    nat.check(nat.lib.rts_path_tempo(path_d.data_ptr(), 600, len_d.data_ptr(), 3, 64, 0.0, X_LIMIT, Y_LIMIT, slope.data_ptr(),
                                     pos.data_ptr(), None))
    torch.cuda.synchronize()
    check_slope("slope_dev")
    check_pos("pos_dev")
    slope, pos = slope.cpu().numpy(), pos.cpu().numpy()
    assert holds_fill(slope[0], 0x55) and holds_fill(slope[2], 0x55) and holds_fill(pos[0], 0x55) and holds_fill(pos[2], 0x55)
    want = model[64, 0.0][b]
    assert same_bytes(slope[1], np.array(want[0][:600])) and same_bytes(pos[1], np.array(want[1][:600]))


# ---- trackers ---------------------------------------------------------------------------------------------------------

def frames(x, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x).T)).to(dtype).to(DEV)


def packed(lives, dtype=torch.float64):
    n_max = max(max(l.shape[1] for l in lives), 1)
    buf = torch.zeros((len(lives), n_max, 12), dtype=dtype, device=DEV)
    for b, l in enumerate(lives):
        buf[b, :l.shape[1]] = frames(l, dtype)
    return buf, torch.tensor([l.shape[1] for l in lives], dtype=torch.int32, device=DEV)


def check_tracker(eng, ref_lens, expect_empty, Ks=(2, 16, 256), ahead=1.5):
    """tempo(K) == the model on paths() == the last entry of path_tempo on the same path."""
    from real_time_audio_sync_amd import tempo
    paths = [eng.path(b) for b in range(eng.B)]
    assert [b for b, p in enumerate(paths) if len(p) == 0] == expect_empty
    finite = 0
    for K in Ks:
        slope, pos, n = eng.tempo(K, ahead)
        want = [tm.tail(p.tolist(), K, ahead, 2 * ref_lens[b], ref_lens[b]) for b, p in enumerate(paths)]
        assert n.tolist() == [w[2] for w in want] == [min(K, len(p)) for p in paths], K
        assert same_bytes(slope, np.array([w[0] for w in want])), (K, slope, want)
        assert same_bytes(pos, np.array([w[1] for w in want])), (K, pos, want)
        finite += int(np.isfinite(slope).sum())
        for b, p in enumerate(paths):
            if len(p):
                dev = torch.from_numpy(np.ascontiguousarray(p[None])).to(DEV)
                s, q = tempo.path_tempo(dev, [len(p)], K, ahead, x_limit=2 * ref_lens[b], y_limit=ref_lens[b])
                assert same_bytes(s[0, -1:].cpu().numpy(), slope[b:b + 1]) and same_bytes(q[0, -1:].cpu().numpy(), pos[b:b + 1]), (K, b)
    assert finite >= len(Ks) * 2
    return paths


@pytest.mark.parametrize("variant", ["otw", "livenote", "livenote_v2"])
def test_otw_tempo_equals_the_model(variant):
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    N, B = 120, 5
    ref, lives = synth.synth_batch(N, B, seed=3)
    lives = [lives[0], lives[1][:, :40], lives[2][:, :0], lives[3][:, :7], lives[4]]      # stream 2 gets no frame
    eng = BatchedOTW(ref, 10, 3, batch=B, variant=variant, dtype=torch.float64, device=DEV)
    try:
        eng.push(*packed(lives))
        paths = check_tracker(eng, [N] * B, [2])
        assert max(len(p) for p in paths) > 100 > 16 > min(len(p) for p in paths if len(p))   # windows full and not
        eng.restart([4])                                                                 # restarted at the end: n = 0, NaN
        check_tracker(eng, [N] * B, [2, 4], Ks=(16,))
    finally:
        eng.close()


def test_otw_tempo_with_per_stream_references():
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    Ns = [120, 60, 90]
    refs = [synth.synth_ref(n, seed=20 + i) for i, n in enumerate(Ns)]
    lives = [synth.synth_live(r, seed=30 + i) for i, r in enumerate(refs)]
    eng = BatchedOTW.with_references(refs, 10, 3, dtype=torch.float64, device=DEV)
    try:
        eng.push(*packed(lives))
        check_tracker(eng, Ns, [])
    finally:
        eng.close()


@pytest.mark.parametrize("per_stream", [False, True])
def test_wtw_tempo_equals_the_model(per_stream):
    from real_time_audio_sync_amd.wtw import BatchedWTW
    B = 5
    Ms = [120, 80, 120, 100, 120] if per_stream else [120] * B
    refs = [synth.synth_ref(m, seed=40 + (i if per_stream else 0)) for i, m in enumerate(Ms)]
    lives = [synth.synth_live(r, seed=50 + i) for i, r in enumerate(refs)]
    lives = [lives[0], lives[1][:, :40], lives[2][:, :0], lives[3][:, :9], lives[4]]
    if per_stream:
        eng = BatchedWTW.with_references([frames(r) for r in refs], 8, 4)
    else:
        eng = BatchedWTW(frames(refs[0]), 8, 4, batch=B)
    try:
        eng.push(*packed(lives))
        paths = check_tracker(eng, Ms, [2])
        p = paths[0]
        assert (np.diff(p, axis=0) == 0).all(axis=1).any()          # the duplicated hand-over points are in the window
        eng.restart([4])
        check_tracker(eng, Ms, [2, 4], Ks=(16,))
    finally:
        eng.close()


# ---- live -------------------------------------------------------------------------------------------------------------

L, HOP, RATE = 512, 128, 22050
N_REF = 120


def live_audio(B, seconds=1.2):
    """Synthetic microphones: a few drifting tones over noise, different for every stream."""
    rs = np.random.RandomState(9)
    t = np.arange(int(seconds * RATE)) / float(RATE)
    out = []
    for b in range(B):
        x = 0.05 * rs.randn(len(t))
        for k in range(4):
            x += 0.2 * np.sin(2 * np.pi * (220.0 * 2 ** ((3 * k + b + 2 * t) / 12.0)) * t)
        out.append(x.astype(np.float32))
    return out


def open_session(kind):
    from real_time_audio_sync_amd.live import LiveSession
    ref = synth.synth_ref(N_REF, seed=60)
    wtw = {'dtw_win_size': 8 * HOP, 'dtw_hop_size': 4 * HOP} if kind == "wtw" else None
    return LiveSession(ref, batch=3, c=10, max_run_count=3, fft_len=L, hop_size=HOP, fs=RATE, max_pending=1 << 14,
                       wtw_params=wtw, device=DEV)


def model_words(sess, K, ahead, table, frame_seconds):
    rows = []
    for b in range(sess.B):
        p = sess.path(b).tolist()
        s, q, n = tm.tail(p, K, ahead, 2 * N_REF, N_REF)
        bpm = tm.bpm(s, p[-1][1], table[0], table[1], frame_seconds) if p and table is not None else tm.NAN
        rows.append((s, q, bpm, n))
    return rows


def check_words(sess, feeds, K, ahead, table, frame_seconds, where):
    got = sess.tempo()
    assert got["feeds_done"] == feeds == sess.poll()["feeds_done"], where
    want = model_words(sess, K, ahead, table, frame_seconds)
    for q, key in enumerate(("slope", "pos", "bpm")):
        assert same_bytes(got[key], np.array([w[q] for w in want], dtype=np.float64)), (where, key, got[key], want)
    assert got["n"].tolist() == [w[3] for w in want], where
    return got


SIZES = [(1500, 900, 2100), (513, 0, 1300), (128, 1407, 1), (2000, 700, 1999)]


def cut(audio, pos, sizes):
    bufs = []
    for b, n in enumerate(sizes):
        bufs.append(audio[b][pos[b]:pos[b] + n])
        pos[b] += n
    return bufs


@pytest.mark.parametrize("kind", ["otw", "wtw"])
def test_live_tempo_words(kind):
    from real_time_audio_sync_amd import _native as nat
    from real_time_audio_sync_amd.annotate import AnnotationTables
    audio = live_audio(3)
    K, ahead = 16, 4.0
    sess, plain = open_session(kind), open_session(kind)
    tab = AnnotationTables([REF_CSV, LIVE_CSV], device=DEV)
    table = evaluate.read_ground_truth(REF_CSV)
    try:
        with pytest.raises(nat.RtsyncError, match="before any rts_live_follow_tempo"):
            sess.tempo()
        sess.follow_tempo(K, ahead)
        got = sess.tempo()
        assert np.isnan(got["slope"]).all() and np.isnan(got["pos"]).all() and np.isnan(got["bpm"]).all()
        assert got["n"].tolist() == [0, 0, 0] and got["feeds_done"] == 0
        pos, ppos, feeds = [0] * 3, [0] * 3, 0
        for i in range(6):                                          # annotations off: slope and position, bpm NaN
            sess.feed(cut(audio, pos, SIZES[i % 4]))
            plain.feed(cut(audio, ppos, SIZES[i % 4]))
            feeds += 1
            sess.sync()
            got = check_words(sess, feeds, K, ahead, None, FS, i)
        assert np.isnan(got["bpm"]).all() and max(got["n"]) == K and np.isfinite(got["slope"]).any()
        sess.annotate(tab)                                          # a single reference: table 0, frame0 = 0
        plain.annotate(tab)
        for i in range(6, 12):
            sess.feed(cut(audio, pos, SIZES[i % 4]))
            plain.feed(cut(audio, ppos, SIZES[i % 4]))
            feeds += 1
            sess.sync()
            got = check_words(sess, feeds, K, ahead, table, FS, i)
        assert np.isfinite(got["bpm"]).any()
        # AnnotationTables.bpm agrees with the published words
        last = [int(sess.path(b)[-1][1]) for b in range(3)]
        again = tab.bpm([[f] for f in last], [[s] for s in got["slope"]], [0, 0, 0])
        assert same_bytes(np.array([a[0] for a in again]), got["bpm"])
        assert sess.beats()["ref_frame"].tolist() == last           # the frame rts_live_beats reports
        # the session that never followed the tempo did the same work
        plain.sync()
        for b in range(3):
            assert np.array_equal(sess.path(b), plain.path(b)), b
        eng, peng = (sess.otw or sess.wtw), (plain.otw or plain.wtw)
        assert np.array_equal(eng.states(), peng.states())
        mine, theirs = sess.beats(), plain.beats()
        for key in ("beat", "label", "ref_frame"):
            assert same_bytes(mine[key], theirs[key]), key
        # restart of one stream: NaN / 0 for it alone
        before = sess.tempo()
        sess.restart([1])
        sess.sync()
        after = sess.tempo()
        assert after["n"].tolist() == [before["n"][0], 0, before["n"][2]]
        for key in ("slope", "pos", "bpm"):
            assert np.isnan(after[key][1]) and same_bytes(after[key][[0, 2]], before[key][[0, 2]]), key
        sess.feed(cut(audio, pos, SIZES[3]))
        feeds += 1
        sess.sync()
        check_words(sess, feeds, K, ahead, table, FS, "after the restart")
        # off: the words stay
        sess.follow_tempo(0)
        kept = sess.tempo()
        sess.feed(cut(audio, pos, SIZES[0]))
        feeds += 1
        sess.sync()
        later = sess.tempo()
        assert later["feeds_done"] == feeds
        for key in ("slope", "pos", "bpm", "n"):
            assert same_bytes(later[key], kept[key]), key
        sess.reset()
        sess.sync()
        cleared = sess.tempo()
        assert np.isnan(cleared["slope"]).all() and cleared["n"].tolist() == [0, 0, 0]
    finally:
        sess.close()
        plain.close()
        tab.close()


def test_bpm_equals_the_model():
    from real_time_audio_sync_amd import _native as nat
    from real_time_audio_sync_amd.annotate import AnnotationTables
    zero = ([0.0, 1.0, 1.0, 2.5], [4, 5, 6, 7])                     # i == 0 and times[0] == 0; a row without width
    host = [evaluate.read_ground_truth(REF_CSV), evaluate.read_ground_truth(LIVE_CSV), zero]
    tab = AnnotationTables([REF_CSV, LIVE_CSV, zero], device=DEV)
    try:
        B, n_max = 4, 300
        n = [300, 257, 40, 5]
        pieces = [0, 1, 2, 9]                                        # stream 3: no such piece
        frame0 = [0, 40, 0, 0]
        rs = np.random.RandomState(4)
        fr = rs.randint(-2, 520, size=(B, n_max)).astype(np.int32)
        fr[2, :40] = np.arange(40)
        slopes = rs.uniform(0.3, 2.5, size=(B, n_max))
        slopes[rs.rand(B, n_max) < 0.1] = np.nan
        want = np.zeros((B, n_max))
        for b in range(B):
            t = host[pieces[b]] if pieces[b] < len(host) else ([], [])
            for k in range(n[b]):
                want[b, k] = tm.bpm(float(slopes[b, k]), int(fr[b, k]), list(t[0]), list(t[1]), FS, frame0[b])
        assert np.isfinite(want[0, :n[0]]).sum() > 100 and np.isnan(want[0, :n[0]]).sum() > 20
        assert np.isfinite(want[2, :n[2]]).any() and np.isnan(want[2, 0]) and np.isnan(want[3, :n[3]]).all()
        d = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).to(DEV)  # noqa: E731
        out, check = guarded((B, n_max), torch.float64, DEV, 0x55)
        fr_d, slopes_d, n_d, pieces_d, frame0_d = d(fr), torch.from_numpy(slopes).to(DEV), d(n), d(pieces), d(frame0)
        nat.check(nat.lib.rts_annot_bpm(tab._h, fr_d.data_ptr(), slopes_d.data_ptr(), n_max, n_d.data_ptr(), pieces_d.data_ptr(),
                                        frame0_d.data_ptr(), B, out.data_ptr(), None))
        torch.cuda.synchronize()
        check("bpm_dev")
        out = out.cpu().numpy()
        for b in range(B):
            assert same_bytes(out[b, :n[b]], want[b, :n[b]]), b
            assert holds_fill(out[b, n[b]:], 0x55), b
        got = tab.bpm([fr[b, :n[b]] for b in range(B)], [slopes[b, :n[b]] for b in range(B)], pieces, frame0)
        for b in range(B):
            assert same_bytes(got[b], want[b, :n[b]]), b
    finally:
        tab.close()
