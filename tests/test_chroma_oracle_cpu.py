"""The chroma oracle's FFT against a direct DFT in extended precision.

Every value gate of the chroma GPU tests (tests/test_chroma_gpu.py, tests/test_chroma_paths_gpu.py) compares the HIP
FFT with np.fft.rfft at 1e-11 of the frame's largest bin.  That only means something if np.fft.rfft itself is right
to well below 1e-11, so it is pinned here independently: a direct O(L) sum per bin in np.longdouble, with a
longdouble pi and the angle index k*n reduced mod L in integers before it becomes an angle (so the argument of
cos/sin never exceeds 2 pi and loses no bits).

Gate: |rfft - DFT| <= 1e-14 * max|X| per frame.  Measured worst over the five lengths on x86-64 (80-bit longdouble):
1.9e-16 on these frames (2.3e-16 on others), so the gate is about 40 times the measurement and 1000 times tighter than the GPU gate.

``longdouble_dft`` and ``dft_bins`` are exported: the GPU tests compare the HIP STFT with the same direct DFT."""
import numpy as np
import pytest

from oracle import chroma_oracle as co

DFT_RTOL = 1e-14
LENGTHS = (64, 128, 512, 4096, 8192)
_PI = np.longdouble("3.14159265358979323846264338327950288")


def dft_bins(L, seed=0, n_random=39):
    """The fixed bins the direct DFT is evaluated at: both ends, the middle, and seeded random ones (about 45)."""
    fixed = [0, 1, 2, L // 4, L // 2 - 1, L // 2]
    rs = np.random.RandomState(1000 + seed + L)
    rest = [int(k) for k in rs.permutation(L // 2 + 1) if int(k) not in fixed][:n_random]
    return np.array(sorted(set(fixed + rest)), dtype=np.int64)


def longdouble_dft(frame, bins):
    """X[k] = sum_n frame[n] exp(-2 pi i k n / L) for k in bins, summed directly in np.longdouble.
    ``frame`` is the already windowed real frame (float64 values, taken exactly)."""
    x = np.asarray(frame, dtype=np.float64).astype(np.longdouble)
    L = x.shape[0]
    n = np.arange(L, dtype=np.int64)
    out = np.empty(len(bins), dtype=np.clongdouble)
    for i, k in enumerate(bins):
        r = (int(k) * n) % L                                   # exact, in integers
        ang = (np.longdouble(-2) * _PI / np.longdouble(L)) * r.astype(np.longdouble)
        out[i] = np.sum(x * np.cos(ang)) + 1j * np.sum(x * np.sin(ang))
    return out


def windowed_random_frame(L, seed=0):
    rs = np.random.RandomState(77 + seed + L)
    return (rs.rand(L) - 0.5).astype(np.float32).astype(np.float64) * np.hanning(L)


@pytest.mark.parametrize("L", LENGTHS)
def test_rfft_against_longdouble_dft(L):
    frame = windowed_random_frame(L)
    X = np.fft.rfft(frame)
    bins = dft_bins(L)
    assert len(bins) == min(45, L // 2 + 1) and bins[0] == 0 and bins[-1] == L // 2   # L = 64 has 33 bins in all
    D = longdouble_dft(frame, bins)
    err = float(np.abs(X[bins].astype(np.clongdouble) - D).max() / np.abs(X).max())
    print("L=%d: worst |rfft - longdouble DFT| / max|X| = %.3g over %d bins" % (L, err, len(bins)))
    assert err <= DFT_RTOL


def test_oracle_create_stft_is_that_rfft():
    """co.create_stft is the framing around the same np.fft.rfft (zero-pad L/2, np.hanning): its columns must be
    bit-identical to np.fft.rfft of the restated slices, so the pin above carries over to the oracle."""
    rs = np.random.RandomState(5)
    for L, H in ((64, 16), (512, 128), (4096, 2048)):
        x = (rs.rand(3 * L + 17) - 0.5).astype(np.float32)
        st = co.create_stft(x, L, H)
        xp = np.concatenate((np.zeros(L // 2), x))
        assert st.shape[1] == (len(xp) - L) // H + 1
        for m in (0, 1, st.shape[1] - 1):
            want = np.fft.rfft(xp[m * H:m * H + L] * np.hanning(L))
            assert np.array_equal(st[:, m], want)
        D = longdouble_dft(xp[H:H + L] * np.hanning(L), dft_bins(L))
        assert np.abs(st[dft_bins(L), 1] - D).max() <= DFT_RTOL * np.abs(st[:, 1]).max()
