"""The resampler's definition (DESIGN.md "Resampler", include/rtsync.h) restated in numpy, for the tests only.

    c    = k * M + half
    y[k] = float32( sum over n = ceil((c - 2 half) / L) .. floor(c / L), ascending, of h[c - n L - half] * float64(x[n]) )

one float64 multiply and one float64 add per term, x[n] = 0 outside the signal (such a term adds a zero and is skipped),
h given as the array of 2 half + 1 taps with h[-half] first.  ``resample_model`` is that sentence as a plain loop per
output.  ``resample_model_fast`` runs the same loop for many outputs side by side, one numpy operation per term, so every
output sees the same operations in the same order; tests/test_resample_cpu.py holds the two against each other bit for
bit, and the larger GPU cases use the fast one."""
import math

import numpy as np


def ratio(fs_in, fs_out=22050):
    g = math.gcd(int(fs_in), int(fs_out))
    return int(fs_out) // g, int(fs_in) // g


def as_float32(x):
    """Samples as the device takes them: float32, PCM16 scaled by 1/32768 (exact)."""
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(np.float32) * np.float32(1.0 / 32768.0)
    return x.astype(np.float32)


def out_len(n_in, L, M):
    return -((-n_in * L) // M) if n_in > 0 else 0


def avail(in_total, L, M, half):
    """Outputs whose last input sample, floor((k M + half) / L), is among the first in_total."""
    k = 0
    while (k * M + half) // L <= in_total - 1:
        k += 1
    return k


def avail_closed(in_total, L, M, half):
    return max(0, -((-(in_total * L - half)) // M))


def resample_model(x, L, M, h, ks=None):
    """Outputs ``ks`` (default: all out_len(len(x)) of the one-shot run) of the resampling of ``x``."""
    x = as_float32(x)
    half = (len(h) - 1) // 2
    if ks is None:
        ks = range(out_len(len(x), L, M))
    y = np.zeros(len(ks), dtype=np.float32)
    for i, k in enumerate(ks):
        c = int(k) * M + half
        s = np.float64(0.0)
        for n in range(-((-(c - 2 * half)) // L), c // L + 1):
            if 0 <= n < len(x):
                s = s + h[c - n * L] * np.float64(x[n])
        y[i] = np.float32(s)
    return y


def resample_model_fast(x, L, M, h, ks=None):
    x64 = as_float32(x).astype(np.float64)
    half = (len(h) - 1) // 2
    ks = np.arange(out_len(len(x64), L, M), dtype=np.int64) if ks is None else np.asarray(ks, dtype=np.int64)
    if len(ks) == 0 or len(x64) == 0:
        return np.zeros(len(ks), dtype=np.float32)
    c = ks * M + half
    q = c // L
    J = (2 * half - (c - q * L)) // L + 1          # terms of every output
    n_lo = q - J + 1                               # = ceil((c - 2 half) / L)
    s = np.zeros(len(ks), dtype=np.float64)
    for i in range(int(J.max())):
        n = n_lo + i
        ok = (i < J) & (n >= 0) & (n < len(x64))
        nn = np.clip(n, 0, len(x64) - 1)
        term = h[np.clip(c - nn * L, 0, 2 * half)] * x64[nn]
        s = np.where(ok, s + term, s)
    return s.astype(np.float32)
