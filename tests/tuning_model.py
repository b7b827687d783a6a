"""The tuning estimator of include/rtsync.h (rts_tuning_accumulate, rts_tuning_pick) restated serially in numpy, frame by
frame and peak by peak, every float64 operation a numpy operation of its own (numpy fuses nothing), and the synthetic
source both tuning suites use.  tests/test_tuning_cpu.py checks the model; tests/test_tuning_gpu.py holds the device to it
bit for bit."""
import numpy as np

FS, FFT_LEN, HOP = 22050, 4096, 2048
THR_POW = 0.1 * 0.1          # TuningPlan's default: magnitude ratio 0.1
MASK = (1 << 64) - 1


def peaks(P, k_lo, k_hi, thr_pow):
    """The peak bins of one frame's power spectrum, ascending."""
    lim = np.float64(thr_pow) * P.max()
    k = np.arange(k_lo, k_hi + 1)
    return k[(P[k] > P[k - 1]) & (P[k] >= P[k + 1]) & (P[k] >= lim)]


def peak_frequency(P, k, bin_hz):
    a, b, c = np.sqrt(P[k - 1]), np.sqrt(P[k]), np.sqrt(P[k + 1])
    avg = np.float64(0.5) * (c - a)
    sh = (np.float64(2.0) * b - c) - a
    d = avg / sh if sh > 0 else np.float64(0.0)
    return (np.float64(k) + d) * np.float64(bin_hz)


def histogram(stft, k_lo, k_hi, E, R, bin_hz, thr_pow=THR_POW, seg=None, S=1, hist=None):
    """stft: [M][n_bins] complex128.  Returns hist [S][R] of Python-exact uint64 counts (adds to ``hist`` when given)."""
    stft = np.asarray(stft)
    E = np.asarray(E, dtype=np.float64)
    hist = np.zeros((S, R), dtype=np.uint64) if hist is None else hist
    for m in range(stft.shape[0]):
        s = 0 if seg is None else int(seg[m])
        if s < 0 or s >= S:
            continue
        re, im = np.ascontiguousarray(stft[m].real), np.ascontiguousarray(stft[m].imag)
        P = re * re + im * im
        for k in peaks(P, k_lo, k_hi, thr_pow):
            f = peak_frequency(P, int(k), bin_hz)
            n = int(np.searchsorted(E, f, "right")) - 1
            if n < 0 or n >= len(E) - 1:
                continue
            hist[s, n % R] += np.uint64(1)
    return hist


def score(h, W):
    R = len(h)
    return [sum((W + 1 - abs(d)) * int(h[(i + d) % R]) for d in range(-W, W + 1)) & MASK for i in range(R)]


def pick(h, W=5):
    """(cents, n) of one histogram row."""
    R = len(h)
    assert W >= 0 and 2 * W + 1 <= R
    N = sum(int(v) for v in h) & MASK
    if N == 0:
        return 0.0, 0
    sc = score(h, W)
    i = sc.index(max(sc))                                          # the first maximum
    cents = (np.float64(i) + np.float64(0.5)) * np.float64(100.0) / np.float64(R) - np.float64(50.0)
    return float(cents), N


def pick_cases():
    """(name, histogram row as a list of ints, W) for both suites: the driver of csrc/tuning_plan.h and the pick kernel
    must both give ``pick`` of each."""
    big = 1 << 40
    cases = []

    def add(name, R, W, counts):
        h = [0] * R
        for i, v in counts.items():
            h[i % R] = v
        cases.append((name, h, W))

    add("spike", 100, 5, {37: 9})
    add("spike-at-0", 100, 5, {0: 1})
    add("spike-at-R-1", 100, 5, {99: 4})
    add("wrap", 100, 5, {98: 5, 99: 9, 0: 9, 1: 5, 40: 8, 41: 8})
    add("wrap-W2", 100, 2, {98: 5, 99: 9, 0: 9, 1: 5, 40: 8, 41: 8})
    add("two-equal-maxima", 100, 5, {20: 7, 70: 7})
    add("two-equal-maxima-across-the-wrap", 100, 3, {95: 6, 5: 6})
    add("all-zero", 100, 5, {})
    add("R1", 1, 0, {0: 12})
    add("R1-empty", 1, 0, {})
    add("R7-W0", 7, 0, {2: 3, 5: 3, 6: 1})
    add("R7-Wmax", 7, 3, {0: 2, 3: 5, 4: 5, 6: 1})
    add("R1024-W0", 1024, 0, {1023: 2, 511: 2, 700: 1})
    add("R1024-W5", 1024, 5, {1020: 3, 1023: 4, 2: 3, 512: 9})
    add("R1024-Wmax", 1024, 511, {0: 1, 300: 2, 301: 2, 900: 3})
    add("R101-Wmax", 101, 50, {0: 1, 50: 1, 100: 1})
    add("near-2^40", 100, 5, {10: big + 1, 11: big, 60: big + 1, 61: big + 1, 62: 3})
    add("near-2^40-Wmax", 99, 49, {k: big - k for k in range(0, 99, 3)})
    rs = np.random.RandomState(11)
    cases.append(("random", [int(v) for v in rs.randint(0, 50, 100)], 5))
    cases.append(("random-R1024", [int(v) for v in rs.randint(0, 3, 1024)], 10))
    return cases


def circular_error(got, want):
    """Distance of two offsets in cents on the circle of one semitone."""
    d = (got - want) % 100.0
    return min(d, 100.0 - d)


def stft(x, fft_len=FFT_LEN, hop=HOP):
    """The reference's framing (zero-pad fft_len / 2 in front, symmetric Hann, rfft) -> [M][n_bins] complex128."""
    x = np.concatenate((np.zeros(fft_len // 2), np.asarray(x, dtype=np.float64)))
    n = (len(x) - fft_len) // hop + 1
    win = np.hanning(fft_len)
    return np.stack([np.fft.rfft(x[m * hop:m * hop + fft_len] * win) for m in range(n)])


def source(cents, seconds=6.0, seed=3, fs=FS):
    """Three voices of decaying tones with 5 harmonics, MIDI 48-83, notes of 0.5 s, a little noise; float32.  Every pitch
    is ``cents`` away from equal temperament at A4 = 440 Hz.  The same seed gives the same notes at every offset."""
    rs = np.random.RandomState(seed)
    n_note = int(round(0.5 * fs))
    n_notes = int(np.ceil(seconds / 0.5))
    t = np.arange(n_note) / float(fs)
    env = np.exp(-3.0 * t)
    out = np.zeros(n_notes * n_note)
    for voice in range(3):
        for j in range(n_notes):
            midi = rs.randint(48, 84)
            phase = rs.rand(5) * 2.0 * np.pi
            f0 = 440.0 * 2.0 ** ((midi - 69) / 12.0 + cents / 1200.0)
            note = sum(np.sin(2.0 * np.pi * f0 * (h + 1) * t + phase[h]) / (h + 1) for h in range(5))
            out[j * n_note:(j + 1) * n_note] += env * note
    out = 0.1 * out + 1e-4 * rs.randn(len(out))
    return out[:int(round(seconds * fs))].astype(np.float32)
