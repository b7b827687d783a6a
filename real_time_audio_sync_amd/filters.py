"""Constant tables of the chroma front end, built once on the host and uploaded to the device.

``chroma_filterbank`` restates the published algorithm of ``librosa.filters.chroma`` (the
reference calls it at chroma.py:69 and wtw.py:39; librosa itself is not a dependency of this
package and is absent from the build image): a Gaussian bump per pitch class around each FFT bin's
fractional chroma position, columns L2-normalised, a Gaussian octave weighting centred on
``ctroct`` octaves above A0/16, rows rolled so that row 0 is C."""
import math
import wave

import numpy as np


def chroma_filterbank(sr=22050, n_fft=4096, n_chroma=12, a440=440.0, ctroct=5.0, octwidth=2.0, base_c=True):
    bins = np.arange(1, n_fft) * (float(sr) / n_fft)
    pos = n_chroma * np.log2(bins / (float(a440) / 16))
    pos = np.concatenate(([pos[0] - 1.5 * n_chroma], pos))          # DC bin: 1.5 octaves below bin 1
    width = np.concatenate((np.maximum(np.diff(pos), 1.0), [1.0]))
    dist = pos[None, :] - np.arange(n_chroma, dtype=np.float64)[:, None]
    half = np.round(n_chroma / 2.0)
    dist = np.remainder(dist + half + 10 * n_chroma, n_chroma) - half
    w = np.exp(-0.5 * (2.0 * dist / width[None, :]) ** 2)
    w = w / np.sqrt((w * w).sum(axis=0, keepdims=True))
    if octwidth is not None:
        w = w * np.exp(-0.5 * ((pos / n_chroma - ctroct) / octwidth) ** 2)[None, :]
    if base_c:
        w = np.roll(w, -3, axis=0)
    return np.ascontiguousarray(w[:, : n_fft // 2 + 1], dtype=np.float64)


def tuning_a440(cents):
    """The A4 of a source that lies ``cents`` from 440 Hz: what ``chroma_filterbank(a440=...)`` takes."""
    return 440.0 * 2.0 ** (float(cents) / 1200.0)


def tuning_edges(fs, n_fft, f_min=150.0, f_max=4000.0, R=100):
    """(k_lo, k_hi, E) for the tuning estimator (rts_tuning_create): the FFT bins whose peaks count, those with centres in
    [f_min, f_max], and the ascending float64 edge table E[n] = 440 * 2^((s_lo - 0.5 + n/R)/12), n = 0 .. (s_hi - s_lo) * R,
    that cuts every semitone from s_lo to s_hi (relative to A4 = 440) into R parts starting half a semitone below the
    pitch.  A frequency between E[n] and E[n+1] lies in histogram bin n mod R, which holds the offsets
    [-50 + 100 i/R, -50 + 100 (i+1)/R) cents from the nearest equal-tempered pitch.  The table covers every frequency an
    interpolated peak of a bin in [k_lo, k_hi] can have, (k_lo - 0.5) to (k_hi + 0.5) bins, with a semitone to spare."""
    fs, n_fft, R = float(fs), int(n_fft), int(R)
    k_lo = max(1, int(math.ceil(f_min * n_fft / fs)))
    k_hi = min(n_fft // 2 - 1, int(math.floor(f_max * n_fft / fs)))
    s_lo = int(math.floor(12.0 * math.log2((k_lo - 0.5) * fs / n_fft / 440.0) + 0.5)) - 1
    s_hi = int(math.ceil(12.0 * math.log2((k_hi + 0.5) * fs / n_fft / 440.0) + 0.5)) + 1
    n = np.arange((s_hi - s_lo) * R + 1, dtype=np.float64)
    E = 440.0 * np.exp2((s_lo - 0.5 + n / R) / 12.0)
    return k_lo, k_hi, np.ascontiguousarray(E, dtype=np.float64)


def hann_window(n):
    """The symmetric window the reference multiplies every frame by (np.hanning, chroma.py:39,:62)."""
    return np.hanning(n).astype(np.float64)


def hann_window_periodic(n):
    """The periodic Hann window, 0.5 - 0.5 cos(2 pi m / n): its two halves sum to one at a hop of n / 2, which the
    symmetric form above does not, so overlap-add of unmoved frames gives the input back (render.WarpPlan's default)."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(int(n), dtype=np.float64) / int(n))


def resample_ratio(fs_in, fs_out=22050):
    """(L, M) with L / M = fs_out / fs_in, reduced by the gcd: 44 100 -> 22 050 is (1, 2), 48 000 -> 22 050 (147, 320)."""
    fs_in, fs_out = int(fs_in), int(fs_out)
    if fs_in < 1 or fs_out < 1:
        raise ValueError("sample rates must be positive integers")
    g = math.gcd(fs_in, fs_out)
    return fs_out // g, fs_in // g


def resample_taps(fs_in, fs_out=22050, zeros=16, atten_db=80.0, rolloff=0.945):
    """The resampler's filter table h[-half .. half] as 2 * half + 1 float64 taps (index 0 is h[-half]): a Kaiser-windowed
    sinc at the rate fs_in * L with ``zeros`` zero crossings on either side, cut off at ``rolloff`` of the lower Nyquist
    frequency, gain L.  half = zeros * max(L, M), fc = rolloff / max(L, M),
    h[n] = L * fc * sinc(fc * n) * kaiser(2 * half + 1, 0.1102 * (atten_db - 8.7))[n + half].
    This table stands where librosa.load's resampling filter stands in the reference (chroma.py:27, wtw.py:23); like the
    chroma filterbank it is handed to the library as host doubles (rts_resample_create)."""
    L, M = resample_ratio(fs_in, fs_out)
    half = int(zeros) * max(L, M)
    fc = float(rolloff) / max(L, M)
    n = np.arange(-half, half + 1, dtype=np.float64)
    h = L * fc * np.sinc(fc * n) * np.kaiser(2 * half + 1, 0.1102 * (float(atten_db) - 8.7))
    return np.ascontiguousarray(h, dtype=np.float64)


def load_wav_native(path):
    """``load_wav`` without the refusal: (float32 samples scaled by 1/32768 with the channels averaged, the file's own
    rate).  What ``librosa.load(path, sr=None)`` returns; bringing it to 22 050 Hz is the device resampler's job
    (chroma.resample, the ``resample=True`` keyword of the file entry points)."""
    with wave.open(path, "rb") as w:
        if w.getsampwidth() != 2:
            raise ValueError("only 16-bit PCM WAV files are supported")
        fs = w.getframerate()
        nch = w.getnchannels()
        raw = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    x = raw.reshape(-1, nch).astype(np.float32) / np.float32(32768.0)
    y = x.mean(axis=1, dtype=np.float32) if nch > 1 else x[:, 0]
    return np.ascontiguousarray(y, dtype=np.float32), fs


def load_wav(path):
    """What ``librosa.load(path)`` returns for the recordings this project uses -- PCM16 WAV, any
    channel count, already at the file's native rate: float32 samples scaled by 1/32768, channels
    averaged.  No resampling: the reference asserts fs == 22050 right after loading
    (chroma.py:28, wtw.py:24), and so do the callers here."""
    with wave.open(path, "rb") as w:
        if w.getsampwidth() != 2:
            raise ValueError("only 16-bit PCM WAV files are supported")
        fs = w.getframerate()
        nch = w.getnchannels()
        raw = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    if fs != 22050:
        # librosa.load(path) would resample to 22 050 Hz here (chroma.py:27, wtw.py:23); its resampler is a
        # third-party dependency the reference does not pin, so it is not reproduced: refuse instead of drifting
        raise ValueError("%s is sampled at %d Hz; this build takes 22 050 Hz input only (the reference relies on "
                         "librosa.load's resampler for other rates -- resample the file first)" % (path, fs))
    x = raw.reshape(-1, nch).astype(np.float32) / np.float32(32768.0)
    y = x.mean(axis=1, dtype=np.float32) if nch > 1 else x[:, 0]
    return np.ascontiguousarray(y, dtype=np.float32), fs
