"""Following a score on the device: rts_score_chroma equals the serial model of tests/score_model.py with ``==`` (float64
output bit for bit, float32 output equal to the rounded float64), at the smallest shapes at which the kernel can go wrong,
inside guarded buffers; then the way from a score to a followed performance, end to end and small."""
import functools
import math

import numpy as np
import pytest
import torch

import score_model as sm
from guarded import FILLS, guarded, same_bytes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
I63 = 2 ** 63 - 1
PLANS = {"tiny": dict(L=64, H=32, K=3, half_life_s=0.002), "real": dict(L=4096, H=2048, K=64, half_life_s=math.log(2.0) / 6.0)}


@functools.lru_cache(maxsize=None)
def host_tables(name):
    from real_time_audio_sync_amd import score
    g = PLANS[name]
    return score.tables(g["L"], g["H"], 22050, half_life_s=g["half_life_s"], K=g["K"])


@functools.lru_cache(maxsize=None)
def case(name, pad):
    """The note pool and the piece tables of one plan and one pad_left: numpy arrays, and what each piece is there for."""
    g = PLANS[name]
    L, H, K = g["L"], g["H"], g["K"]
    rng = np.random.RandomState(11)
    notes, pieces = [], []          # notes: (onset, end, pitch, energy); pieces: (note_first, note_len, n_frames)

    def piece(ns, n_frames):
        pieces.append((len(notes), len(ns), n_frames))
        notes.extend(ns)

    def w0(m):
        return m * H - pad

    # 0: one frame, two notes
    piece([(0, L, 60, 1.0), (L // 4, L // 2, 64, 0.25)], 1)
    # 1: 63 frames, a chord of 70 notes on one onset: the order among equal onsets
    piece([(5 * H, 5 * H + int(rng.randint(1, 20 * H)), int(rng.randint(30, 100)), float(rng.uniform(0.01, 1.0))) for _ in range(70)], 63)
    # 2: 64 frames, one note that spans the whole piece among 200 short ones: the lower end of the walk
    short = sorted(int(v) for v in rng.randint(0, 64 * H, 200))
    piece([(0, I63, 36, 0.5)] + [(o, o + int(rng.randint(1, H)), int(rng.randint(40, 90)), float(rng.uniform(0.1, 1.0))) for o in short], 64)
    # 3: 65 frames: a note ending exactly on window 10's first sample and one starting exactly on its end (neither takes
    # part in frame 10), a zero-length note, and one note of each invalid kind between valid ones
    edge = [(max(w0(10) - 3 * H, 0), w0(10), 50, 1.0), (w0(12), w0(12), 52, 1.0), (w0(10) + L, w0(10) + L + 2 * H, 55, 1.0),
            (w0(20), w0(20) + H, 57, 0.7), (w0(21), w0(23), -1, 1.0), (w0(22), w0(24), 128, 1.0), (-5, w0(30), 60, 1.0),
            (w0(25), w0(25) - 1, 60, 1.0), (w0(26), w0(28), 61, -0.5), (w0(27), w0(29), 62, float("nan")),
            (w0(28), w0(30), 63, float("inf")), (w0(40), w0(44) + 7, 64, 0.3), (2 ** 62, I63, 65, 1.0)]
    piece(edge, 65)
    # 4: 130 frames (three waves, two workgroups' worth of tiles): random notes, and one longer than K + 3 frames
    starts = sorted(int(v) for v in rng.randint(0, 128 * H, 60))
    piece([(5 * H + 3, 5 * H + 3 + (K + 10) * H, 43, 0.9)]
          + [(o, o + int(rng.randint(1, 6 * H)), int(rng.randint(0, 128)), float(rng.uniform(0.0, 1.0))) for o in starts], 130)
    # 5: no notes -> zero columns; 6: n_frames = 0 with notes; 7: the notes of piece 1 again, 10 frames
    piece([], 5)
    piece([(0, 3 * H, 70, 1.0)], 0)
    pieces.append((pieces[1][0], pieces[1][1], 10))
    # 8: its frame range leaves the pool; 9: its note range leaves the notes
    piece([(0, 4 * H, 71, 1.0)], 40)
    pieces.append((len(notes) - 1, 5, 4))
    onset, end, pitch, energy = (np.array([n[i] for n in notes], dtype=dt) for i, dt in enumerate((np.int64, np.int64, np.int32, np.float64)))
    # frame offsets that are no multiple of 64, one frame of gap between neighbours
    frame_first, at = [], 3
    for p, (_, _, fr) in enumerate(pieces):
        frame_first.append(at)
        at += fr + 1 if p not in (8,) else 1
    n_pool = at + 2
    frame_first[8] = n_pool - 39                       # one frame too many
    frame_first[9] = 0                                 # would overlap piece 0's gap: nothing may be written
    return dict(L=L, H=H, K=K, pad=pad, onset=onset, end=end, pitch=pitch, energy=energy,
                note_first=np.array([p[0] for p in pieces], dtype=np.int64), note_len=np.array([p[1] for p in pieces], dtype=np.int32),
                frame_first=np.array(frame_first, dtype=np.int64), n_frames=np.array([p[2] for p in pieces], dtype=np.int32), n_pool=n_pool)


@functools.lru_cache(maxsize=None)
def model(name, pad, normalize):
    c = case(name, pad)
    T, CW, DK = host_tables(name)
    out, skipped, status = sm.chroma(T, CW, DK, c["L"], c["H"], pad, c["onset"].tolist(), c["end"].tolist(), c["pitch"].tolist(),
                                     c["energy"].tolist(), c["note_first"], c["note_len"], c["frame_first"], c["n_frames"], c["n_pool"],
                                     normalize, np.zeros((c["n_pool"], 12)))
    written = np.zeros(c["n_pool"], dtype=bool)
    for p in range(len(status)):
        if status[p] == 0 and c["n_frames"][p] >= 1:
            written[c["frame_first"][p]:c["frame_first"][p] + c["n_frames"][p]] = True
    for a in (out, skipped, status, written):
        a.setflags(write=False)
    return out, skipped, status, written


@functools.lru_cache(maxsize=None)
def plan(name, pad):
    from real_time_audio_sync_amd import score
    g = PLANS[name]
    return score.ScorePlan(g["L"], g["H"], 22050, K=g["K"], device=DEV, pad_left=pad, host_tables=host_tables(name))


def run_case(name, pad, normalize, dtype, fill):
    c, pl = case(name, pad), plan(name, pad)
    dev = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    P = len(c["note_first"])
    out, check_out = guarded((c["n_pool"], 12), dtype, DEV, fill)
    skipped, check_sk = guarded((P,), torch.int32, DEV, fill)
    status, check_st = guarded((P,), torch.int32, DEV, fill)
    ws, check_ws = guarded((pl.workspace_bytes(len(c["onset"])),), torch.uint8, DEV, fill)
    pl.run(dev(c["onset"]), dev(c["end"]), dev(c["pitch"]), dev(c["energy"]), dev(c["note_first"]), dev(c["note_len"]),
           dev(c["frame_first"]), dev(c["n_frames"]), out, normalize, skipped, status, ws)
    torch.cuda.synchronize()
    for chk, what in ((check_out, "out"), (check_sk, "skipped"), (check_st, "status"), (check_ws, "workspace")):
        chk(what)
    return out.cpu().numpy(), skipped.cpu().numpy(), status.cpu().numpy()


CASES = [(n, half, norm, dt) for n in ("tiny", "real") for half in (0, 1) for norm in (0, 1) for dt in (torch.float64, torch.float32)]


@pytest.mark.parametrize("k", range(len(CASES)), ids=["%s-pad%s-norm%d-%s" % (n, "L/2" if h else "0", nm, str(d)[6:]) for n, h, nm, d in CASES])
def test_device_equals_model(k):
    name, half, normalize, dtype = CASES[k]
    pad = PLANS[name]["L"] // 2 if half else 0
    fill = FILLS[k % len(FILLS)]
    want, want_skipped, want_status, written = model(name, pad, normalize)
    got, skipped, status = run_case(name, pad, normalize, dtype, fill)
    assert skipped.tolist() == want_skipped.tolist() and status.tolist() == want_status.tolist()
    assert want_skipped[3] == 7 and want_status.tolist() == [0] * 8 + [sm.FRAMES, sm.NOTES]
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    expect = np.frombuffer(bytes([fill]) * (want.size * np.dtype(np_dtype).itemsize), dtype=np_dtype).reshape(want.shape).copy()
    expect[written] = want[written].astype(np_dtype)
    rows = np.flatnonzero([not same_bytes(got[r], expect[r]) for r in range(len(expect))])
    assert rows.size == 0, "frames %s differ (written: %s)" % (rows[:10].tolist(), written[rows[:10]].tolist())
    # the piece without notes: zero columns; the edge notes take no part in frame 10 of piece 3 (only the spanning kinds do)
    c = case(name, pad)
    assert not want[c["frame_first"][5]:c["frame_first"][5] + 5].any()
    assert np.isfinite(want[written]).all() and want[written].any()


def test_result_does_not_depend_on_what_the_buffers_held():
    a = run_case("tiny", 32, 1, torch.float64, 0x00)
    b = run_case("tiny", 32, 1, torch.float64, 0xFF)
    written = model("tiny", 32, 1)[3]
    assert same_bytes(a[0][written], b[0][written]) and same_bytes(a[1], b[1]) and same_bytes(a[2], b[2])


def test_refusals():
    from real_time_audio_sync_amd import _native as nat
    from real_time_audio_sync_amd import score
    T, CW, DK = host_tables("tiny")
    with pytest.raises(nat.RtsyncError, match="fft_len"):
        score.ScorePlan(96, 32, 22050, K=3, device=DEV, host_tables=(T, np.zeros(97), DK))
    bad = CW.copy()
    bad[5] = bad[4] - 1.0
    with pytest.raises(nat.RtsyncError, match="CW_host: entry 5"):
        score.ScorePlan(64, 32, 22050, K=3, device=DEV, host_tables=(T, bad, DK))
    pl, c = plan("tiny", 0), case("tiny", 0)
    dev = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    out = torch.zeros((c["n_pool"], 12), dtype=torch.float64, device=DEV)
    args = [dev(c[k]) for k in ("onset", "end", "pitch", "energy", "note_first", "note_len", "frame_first", "n_frames")]
    with pytest.raises(nat.RtsyncError, match="workspace"):
        pl.run(*args, out, workspace=torch.zeros((8,), dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
    assert not out.any()


# ---- end to end, small ---------------------------------------------------------------------------------------------------------
SEED = 3      # the CPU oracle tracker alone meets the one-beat bound for this seed at c = 50 (every path point within a beat)
C = 50


@pytest.fixture(scope="module")
def followed():
    from real_time_audio_sync_amd import chroma, score
    notes = sm.synth_score(SEED)
    perf = sm.perform(notes, SEED)
    audio_perf, audio_score = sm.render_audio(perf, SEED), sm.render_audio(notes, SEED + 1)
    cp = chroma.ChromaPlan(sm.FFT_LEN, sm.HOP, sm.FS, device=DEV)

    def device_chroma(x):
        return cp.frames(torch.from_numpy(x).to(DEV), pad_left=sm.FFT_LEN // 2)[0].t().contiguous().cpu().numpy()

    def as_score(n):
        return score.Score.from_notes(n[0], n[1], n[2], [127] * len(n[0]), beat_times=np.arange(sm.N_BEATS + 1) * sm.BEAT_S)

    sp = score.ScorePlan(sm.FFT_LEN, sm.HOP, sm.FS, half_life_s=math.log(2.0) / 6.0, device=DEV)
    scores = [as_score(sm.synth_score(SEED + 1)), as_score(notes), as_score(sm.synth_score(SEED + 2))]
    refs, beat_tables = score.references(scores, sp)
    pool = sp.chroma(scores)
    return dict(live=device_chroma(audio_perf), audio_ref=device_chroma(audio_score), refs=refs, beat_tables=beat_tables, pool=pool,
                scores=scores)


def true_beats(live_frames):
    sk, pk = sm.tempo_map(SEED)
    return np.interp(np.asarray(live_frames) * (sm.HOP / sm.FS), pk, sk) / sm.BEAT_S


def test_offline_path_against_the_score(followed):
    from real_time_audio_sync_amd import dtw
    (p_score, _), (p_audio, _) = dtw.align_pairs([followed["live"], followed["live"]], [followed["refs"][1], followed["audio_ref"]], device=DEV)
    d_score, d_audio = sm.path_distance(p_score, SEED), sm.path_distance(p_audio, SEED)
    print("mean distance from the true time map: score %.3f frames, audio %.3f frames" % (d_score, d_audio))
    assert d_score <= d_audio + 1.0


def test_tracker_follows_the_score_to_its_end(followed):
    from real_time_audio_sync_amd import annotate, otw_batch
    live, ref = followed["live"], followed["refs"][1]
    eng = otw_batch.BatchedOTW(ref, C, 3, batch=1, dtype=torch.float64, device=DEV)
    eng.run(*eng.pack([live]))
    path = eng.path(0)
    eng.close()
    assert path[-1][0] == live.shape[1] - 1            # every live frame was taken
    tables = annotate.AnnotationTables([followed["beat_tables"][1]], frame_seconds=sm.HOP / sm.FS, device=DEV)
    (beat, _), = tables.beats([path[:, 1]], [0])
    tables.close()
    off = np.abs(beat - true_beats(path[:, 0]))
    print("within one beat: %.1f %% of %d points, worst %.2f beats" % (100.0 * np.mean(off <= 1.0), len(off), np.nanmax(off)))
    assert np.mean(off <= 1.0) >= 0.9                  # a NaN (no beat) counts as off
    assert off[-1] <= 1.0                              # and it is at the performance's end when the performance ends


def test_excerpt_is_located_in_the_right_score(followed):
    from real_time_audio_sync_amd import locate
    pool, first, lens, views = followed["pool"]
    assert [tuple(v.shape) for v in views] == [r.shape for r in followed["refs"]]
    excerpt = torch.from_numpy(np.ascontiguousarray(followed["live"][:, 100:164].T)).to(DEV)
    cost, end, start = locate.locate_batch(excerpt, None, pool, first, lens)
    cost = cost.cpu().numpy()[0]
    print("locate costs per score:", cost.tolist())
    assert int(np.argmin(cost)) == 1
