"""The score model in plain numpy: the serial restatement of include/rtsync.h's rts_score_create section, a tiny standard
MIDI file *writer* for the fixtures, and the synthetic score / performance / audio the quality tests are made of.

``chroma`` scans ALL notes of a piece for every frame, in index order, with no pruning: whatever the kernel leaves out must
not show against it.  Every float64 operation is one numpy operation, so nothing is fused."""
import struct

import numpy as np

TINY = 2.2250738585072014e-308
OK, FRAMES, NOTES = 0, 1, 2   # RTS_SCORE_*


def note_ok(onset, end, pitch, energy):
    return 0 <= pitch <= 127 and onset >= 0 and end >= onset and bool(np.isfinite(energy)) and energy >= 0.0


def piece_frames(T, CW, DK, L, H, pad_left, onset, end, pitch, energy, n_frames, normalize):
    """[n_frames][12] float64 of one piece's notes (sequences of Python ints / floats)."""
    K = len(DK) - 1
    n_frames = max(int(n_frames), 0)
    m = np.arange(n_frames, dtype=np.int64)
    w0 = m * H - pad_left
    acc = np.zeros((n_frames, 12), dtype=np.float64)
    lo, hi = (int(w0.min()), int(w0.max()) + L) if n_frames else (0, 0)
    for on, en, p, e in zip(onset, end, pitch, energy):
        on, en, p = int(on), int(en), int(p)
        if not note_ok(on, en, p, e) or n_frames == 0:
            continue
        a = np.clip(min(max(on, lo), hi) - w0, 0, L)
        b = np.clip(min(max(en, lo), hi) - w0, 0, L)
        q = min((on + pad_left) // H, n_frames)          # exact: Python integers
        k = np.clip(m - q, 0, K)
        wgt = (np.float64(e) * DK[k]) * (CW[b] - CW[a])
        term = wgt[:, None] * T[p][None, :]
        part = b > a
        acc[part] = acc[part] + term[part]
    s = np.zeros(n_frames, dtype=np.float64)
    for c in range(12):
        s = s + acc[:, c] * acc[:, c]
    length = np.sqrt(s)
    if not normalize:
        length = np.ones_like(length)
    length = np.where(length < TINY, 1.0, length)
    return acc / length[:, None]


def chroma(T, CW, DK, L, H, pad_left, onset, end, pitch, energy, note_first, note_len, frame_first, n_frames, n_pool,
           normalize, before):
    """The whole call.  ``before``: what the output pool [n_pool][12] float64 held; -> (pool, skipped [P], status [P])."""
    out = np.array(before, dtype=np.float64, copy=True)
    P, n_notes = len(note_first), len(onset)
    skipped, status = np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int32)
    for p in range(P):
        nf, nl, ff, fr = int(note_first[p]), int(note_len[p]), int(frame_first[p]), int(n_frames[p])
        if nf < 0 or nl < 0 or nf + nl > n_notes:
            status[p] |= NOTES
        if fr >= 1 and (ff < 0 or ff + fr > n_pool):
            status[p] |= FRAMES
        if status[p] & NOTES:
            continue
        sl = slice(nf, nf + nl)
        skipped[p] = sum(1 for i in range(nf, nf + nl) if not note_ok(int(onset[i]), int(end[i]), int(pitch[i]), energy[i]))
        if status[p] or fr < 1:
            continue
        out[ff:ff + fr] = piece_frames(T, CW, DK, L, H, pad_left, onset[sl], end[sl], pitch[sl], energy[sl], fr, normalize)
    return out, skipped, status


# ---- a tiny standard MIDI file writer -----------------------------------------------------------------------------------
def vlq(n):
    out = [n & 0x7F]
    n >>= 7
    while n:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    return bytes(reversed(out))


def tempo(us_per_quarter):
    return b"\xFF\x51\x03" + struct.pack(">I", us_per_quarter)[1:]


def timesig(num, den):
    return b"\xFF\x58\x04" + bytes([num, {1: 0, 2: 1, 4: 2, 8: 3, 16: 4}[den], 24, 8])


def on(ch, pitch, vel):
    return bytes([0x90 | ch, pitch, vel])


def off(ch, pitch, vel=64):
    return bytes([0x80 | ch, pitch, vel])


def cc(ch, num, val):
    return bytes([0xB0 | ch, num, val])


def track(events):
    """``events``: [(delta ticks, raw event bytes)] -- a raw event without its status byte uses running status."""
    body = b"".join(vlq(d) + e for d, e in events) + b"\x00\xFF\x2F\x00"
    return b"MTrk" + struct.pack(">I", len(body)) + body


def midi_file(fmt, division, tracks):
    return b"MThd" + struct.pack(">IHHH", 6, fmt, len(tracks), division) + b"".join(tracks)


# ---- the synthetic score, its performance and their audio ----------------------------------------------------------------
FS, FFT_LEN, HOP = 22050, 4096, 2048
BEAT_S, N_BEATS = 0.5, 48


def synth_score(seed):
    """3 voices, 48 beats of 0.5 s, MIDI pitches 48-83: (onset_s, end_s, pitch) arrays, notes of one or two beats."""
    rng = np.random.RandomState(seed)
    on_s, end_s, pit = [], [], []
    for voice, (lo, hi) in enumerate(((48, 60), (60, 72), (72, 84))):
        beat = 0
        while beat < N_BEATS:
            n = min(int(rng.choice([1, 1, 2])), N_BEATS - beat)
            on_s.append(beat * BEAT_S)
            end_s.append((beat + n) * BEAT_S)
            pit.append(int(rng.randint(lo, hi)))
            beat += n
    order = np.argsort(np.array(on_s), kind="stable")
    return np.array(on_s)[order], np.array(end_s)[order], np.array(pit, dtype=np.int32)[order]


def tempo_map(seed):
    """Score time -> performance time: tempo factors drawn from 0.8-1.25 per 8 beats.  -> (score knots, performance knots)
    in seconds, piecewise linear."""
    rng = np.random.RandomState(seed + 1000)
    factors = rng.uniform(0.8, 1.25, N_BEATS // 8)
    sk = np.arange(0, N_BEATS + 1, 8) * BEAT_S
    pk = np.concatenate([[0.0], np.cumsum(np.diff(sk) / factors)])
    return sk, pk


def perform(score, seed):
    on_s, end_s, pit = score
    sk, pk = tempo_map(seed)
    return np.interp(on_s, sk, pk), np.interp(end_s, sk, pk), pit


def render_audio(notes, seed, fs=FS):
    """5 harmonics at 1/h, amplitude envelope exp(-3 t), a little noise: float64 samples."""
    on_s, end_s, pit = notes
    rng = np.random.RandomState(seed + 2000)
    n = int(round(float(np.max(end_s)) * fs))
    x = np.zeros(n, dtype=np.float64)
    for a, b, p in zip(on_s, end_s, pit):
        i0, i1 = int(round(a * fs)), min(int(round(b * fs)), n)
        t = np.arange(i1 - i0, dtype=np.float64) / fs
        f0 = 440.0 * 2.0 ** ((int(p) - 69) / 12.0)
        tone = sum(np.sin(2 * np.pi * f0 * h * t) / h for h in range(1, 6) if f0 * h < fs / 2)
        x[i0:i1] += 0.2 * np.exp(-3.0 * t) * tone
    return x + 1e-4 * rng.standard_normal(n)


def model_chroma(tabs, notes, n_samples, fs=FS, L=FFT_LEN, H=HOP, normalize=True):
    """Feature-major (12, N) model chroma of (onset_s, end_s, pitch) at unit energy, framed like wav_to_chroma frames
    ``n_samples`` samples."""
    T, CW, DK = tabs
    on_s, end_s, pit = notes
    on = np.floor(np.asarray(on_s) * fs + 0.5).astype(np.int64)
    en = np.floor(np.asarray(end_s) * fs + 0.5).astype(np.int64)
    n_frames = (n_samples + L // 2 - L) // H + 1
    return piece_frames(T, CW, DK, L, H, L // 2, on.tolist(), en.tolist(), list(pit), [1.0] * len(on), n_frames, normalize).T


def dtw_path(a, b):
    """Plain DTW of feature-major (12, M) / (12, N) with cost 1 - <a, b>: the path as an (P, 2) array."""
    cost = 1.0 - a.T @ b
    M, N = cost.shape
    acc = np.full((M + 1, N + 1), np.inf)
    acc[0, 0] = 0.0
    for i in range(1, M + 1):
        row, prev, c = acc[i], acc[i - 1], cost[i - 1]
        for j in range(1, N + 1):
            row[j] = c[j - 1] + min(prev[j - 1], prev[j], row[j - 1])
    i, j, path = M, N, []
    while i > 0 and j > 0:
        path.append((i - 1, j - 1))
        step = int(np.argmin((acc[i - 1, j - 1], acc[i - 1, j], acc[i, j - 1])))
        i, j = (i - 1, j - 1) if step == 0 else (i - 1, j) if step == 1 else (i, j - 1)
    return np.array(path[::-1], dtype=np.int64)


def path_distance(path, seed, fs=FS, H=HOP):
    """Mean distance, in frames of column 1, of a path (performance frame, score frame) from the true time map."""
    sk, pk = tempo_map(seed)
    true = np.interp(path[:, 0] * (H / fs), pk, sk) * (fs / H)
    return float(np.mean(np.abs(path[:, 1] - true)))
