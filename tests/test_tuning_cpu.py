"""Tuning without a GPU: the numpy model of the estimator (tests/tuning_model.py) on the synthetic source and on the chopin
fixture; the host tables of filters.py; what a tuned filterbank buys, through the numpy chroma oracle; the four symbols of the
C ABI and the refusals that need no device; the pick, the edge search, the refusal rules and the LDS layout of
csrc/tuning_plan.h through a stand-alone driver built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a
child process.  Every comparison of floats is `==` or bit for bit."""
import ctypes
import math
import os
import struct

import numpy as np
import pytest

import tuning_model as tm
from real_time_audio_sync_amd import filters
from test_sanitize_cpu import ENV, FLAGS, OUT, SAN, _clean_report, _run

BIN_HZ = tm.FS / tm.FFT_LEN
(OK, BAD_FFT, BAD_BINS, BAD_R, BIG_R, FEW_EDGES, NO_EDGES, BAD_EDGES, BAD_THR, BAD_BIN_HZ, BAD_W) = range(11)   # TuningRefusal


def hexbits(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]


@pytest.fixture(scope="module")
def defaults():
    return filters.tuning_edges(tm.FS, tm.FFT_LEN)


def estimate(x, defaults, W=5):
    k_lo, k_hi, E = defaults
    h = tm.histogram(tm.stft(x), k_lo, k_hi, E, 100, BIN_HZ)
    return tm.pick(h[0], W)


# ---- (a) the model ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cents", [-50.0, -49.5, -37.0, -3.0, 0.0, 0.5, 25.0, 49.0, 49.5])
def test_model_recovers_the_offset_of_the_synthetic_source(defaults, cents):
    got, n = estimate(tm.source(cents), defaults)
    print("cents %+.1f: estimate %+.1f from %d peaks" % (cents, got, n))
    assert n > 500
    assert tm.circular_error(got, cents) <= 1.0                     # one histogram bin at R = 100


def test_model_on_the_chopin_fixture(defaults, chopin_audio):
    assert estimate(chopin_audio["ref"], defaults) == (3.5, 2549)
    assert estimate(chopin_audio["live"], defaults) == (-1.5, 3118)


def test_model_rules_on_crafted_frames(defaults):
    k_lo, k_hi, E = defaults
    n_bins = tm.FFT_LEN // 2 + 1
    z = np.zeros((1, n_bins), dtype=np.complex128)
    assert tm.histogram(z, k_lo, k_hi, E, 100, BIN_HZ).sum() == 0   # an all-zero frame has no peak
    P = np.zeros(n_bins)
    P[100:103] = 4.0                                                # a plateau: only its first bin rises above the bin before
    assert list(tm.peaks(P, k_lo, k_hi, 0.01)) == [100]
    P[99] = 4.0                                                     # P[k] == P[k-1] is no peak: the plateau now starts at 99
    assert list(tm.peaks(P, k_lo, k_hi, 0.01)) == [99]
    P[103] = 5.0                                                    # the rule looks one bin either way, no further
    assert list(tm.peaks(P, k_lo, k_hi, 0.01)) == [99, 103]
    P[:] = 0.0
    P[k_lo] = P[k_hi] = 1.0                                         # the ends of the range count, one bin outside does not
    P[k_lo - 2] = P[k_hi + 2] = 1.0
    assert list(tm.peaks(P, k_lo, k_hi, 0.01)) == [k_lo, k_hi]
    P[500] = 0.0099                                                 # below thr_pow * Pmax
    assert 500 not in tm.peaks(P, k_lo, k_hi, 0.01) and 500 in tm.peaks(P, k_lo, k_hi, 0.0099)
    # a symmetric peak sits on its bin: d == 0 and f == k * bin_hz exactly
    P[:] = 0.0
    P[299:302] = [1.0, 9.0, 1.0]
    assert tm.peak_frequency(P, 300, BIN_HZ) == 300 * BIN_HZ
    # segments: rows by seg, out-of-range values count nowhere, counts add up over calls
    st = tm.stft(tm.source(8.0, seconds=1.0))
    M = st.shape[0]
    seg = np.arange(M) % 3
    by_seg = tm.histogram(st, k_lo, k_hi, E, 100, BIN_HZ, seg=seg, S=3)
    assert (by_seg.sum(axis=0) == tm.histogram(st, k_lo, k_hi, E, 100, BIN_HZ)[0]).all() and (by_seg.sum(axis=1) > 0).all()
    seg2 = seg.copy()
    seg2[seg2 == 1] = -1
    seg2[seg2 == 2] = 3
    dropped = tm.histogram(st, k_lo, k_hi, E, 100, BIN_HZ, seg=seg2, S=3)
    assert (dropped[0] == by_seg[0]).all() and dropped[1:].sum() == 0
    twice = tm.histogram(st[:4], k_lo, k_hi, E, 100, BIN_HZ)
    twice = tm.histogram(st[4:], k_lo, k_hi, E, 100, BIN_HZ, hist=twice)
    assert (twice == by_seg.sum(axis=0)).all()


def test_model_pick_cases():
    got = {name: tm.pick(h, W) for name, h, W in tm.pick_cases()}
    assert got["spike"] == (-12.5, 9) and got["spike-at-0"] == (-49.5, 1) and got["spike-at-R-1"] == (49.5, 4)
    assert got["wrap"] == (-49.5, 44)                               # bins 99 and 0 tie across the wrap and beat 40 / 41, which a
    assert got["wrap-W2"] == (-49.5, 44)                            # sum that does not wrap would pick; index 0 is the first
    assert got["two-equal-maxima"] == (-29.5, 14)                   # the first of two equal maxima
    assert got["all-zero"] == (0.0, 0) and got["R1-empty"] == (0.0, 0)
    assert got["R1"] == (0.0, 12)
    assert got["near-2^40"][1] == 4 * (1 << 40) + 6


# ---- (b) the host tables ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs,n_fft,R", [(22050, 4096, 100), (22050, 64, 100), (22050, 1024, 7), (44100, 8192, 1024), (8000, 256, 1)])
def test_tuning_edges(fs, n_fft, R):
    kw = dict(f_min=150.0, f_max=4000.0) if n_fft > 64 else dict(f_min=0.0, f_max=1e9)
    k_lo, k_hi, E = filters.tuning_edges(fs, n_fft, R=R, **kw)
    bin_hz = fs / n_fft
    assert E.dtype == np.float64 and (np.diff(E) > 0).all() and np.isfinite(E).all() and E[0] > 0
    assert 1 <= k_lo <= k_hi <= n_fft // 2 - 1
    assert E[0] <= (k_lo - 0.5) * bin_hz and E[-1] > (k_hi + 0.5) * bin_hz
    assert (len(E) - 1) % R == 0
    if n_fft == 64:
        assert (k_lo, k_hi) == (1, 31)
    if R % 2 == 0:
        s_lo = int(round(12 * math.log2(E[0] / 440.0) + 0.5))
        for s in range(s_lo, s_lo + (len(E) - 1) // R):
            n = int(np.searchsorted(E, 440 * 2 ** (s / 12), "right")) - 1
            assert n % R == R // 2, s


def test_tuning_edges_defaults():
    k_lo, k_hi, E = filters.tuning_edges(22050, 4096)
    assert (k_lo, k_hi, len(E)) == (28, 743, 6001)


def test_tuning_a440():
    assert filters.tuning_a440(0.0) == 440.0
    assert filters.tuning_a440(1200.0) == 880.0 and filters.tuning_a440(-1200.0) == 220.0
    assert abs(filters.tuning_a440(-40.0) - 429.9503) < 1e-3
    a = filters.chroma_filterbank(22050, 4096, a440=filters.tuning_a440(0.0))
    assert a.tobytes() == filters.chroma_filterbank(22050, 4096).tobytes()
    assert filters.chroma_filterbank(22050, 4096, a440=filters.tuning_a440(25.0)).tobytes() != a.tobytes()


def test_what_a_tuned_filterbank_buys_through_the_oracle(defaults):
    """The bounds of the GPU suite's test of the same name, cleared first by the numpy chain: chroma of the in-tune source
    against chroma of the same notes 40 cents flat, mean cosine per frame."""
    from oracle import chroma_oracle as co
    x0, x1 = tm.source(0.0), tm.source(-40.0)
    est, _ = estimate(x1, defaults)
    est0, _ = estimate(x0, defaults)

    def chroma(x, cents):
        fb = co.chroma_filterbank(a440=filters.tuning_a440(cents)) if cents is not None else co.chroma_filterbank()
        return co.l2_normalize_columns(np.dot(fb, np.abs(co.create_stft(x)) ** 2))

    def mean_cos(a, b):
        return float((a * b).sum(axis=0).mean())

    plain = mean_cos(chroma(x0, None), chroma(x1, None))
    tuned = mean_cos(chroma(x0, est0), chroma(x1, est))
    print("mean cosine: untuned %.4f, tuned %.4f (estimates %+.1f, %+.1f)" % (plain, tuned, est0, est))
    assert plain <= 0.96 - 0.01 and tuned >= 0.99 + 0.005           # with slack, so the device test keeps 0.96 / 0.99


# ---- (c) the ABI --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as ge
    ge.build()
    from real_time_audio_sync_amd import _native
    return _native


def test_abi_symbols(nat):
    lib = ctypes.CDLL(nat.SO_PATH)
    dbl = ctypes.c_double
    for name, n_args, doubles in (("rts_tuning_create", 9, [6, 7]), ("rts_tuning_destroy", 1, []),
                                  ("rts_tuning_accumulate", 7, []), ("rts_tuning_pick", 7, [])):
        assert hasattr(lib, name), name
        assert name in nat.EXPORTS and len(nat.EXPORTS[name].argtypes) == n_args, name
        assert [i for i, t in enumerate(nat.EXPORTS[name].argtypes) if t is dbl] == doubles, name
    assert nat.EXPORTS["rts_tuning_accumulate"].argtypes[2] is ctypes.c_longlong
    assert nat.TUNING_MAX_R == 1024


def test_abi_refusals_without_a_device(nat, defaults):
    k_lo, k_hi, E = defaults
    err = lambda: nat.lib.rts_last_error().decode()                # noqa: E731
    INVALID, UNSUPPORTED = -1, -2

    def create(fft_len=4096, k_lo=k_lo, k_hi=k_hi, R=100, edges=E, n_edges=None, bin_hz=BIN_HZ, thr_pow=0.01, out=True):
        h = ctypes.c_void_p(7)
        e = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64)
        rc = nat.lib.rts_tuning_create(fft_len, k_lo, k_hi, R, (len(e) if e is not None else 2) if n_edges is None else n_edges,
                                       e.ctypes.data if e is not None else None, bin_hz, thr_pow,
                                       ctypes.byref(h) if out else None)
        assert not out or h.value is None                           # a refused create leaves NULL behind
        return rc

    assert create(out=False) == INVALID and "out" in err()
    for L in (32, 16384, 4095, 0, -4096, 3000):
        assert create(fft_len=L, k_lo=1, k_hi=1) == UNSUPPORTED and "fft_len" in err(), L
    for lo, hi in ((0, 10), (-1, 10), (11, 10), (1, 2048), (2048, 2048)):
        assert create(k_lo=lo, k_hi=hi) == INVALID and "k_lo" in err(), (lo, hi)
    for R in (0, -3):
        assert create(R=R) == INVALID and "R must be" in err()
    assert create(R=1025) == UNSUPPORTED and "1024" in err()
    for n in (1, 0, -5):
        assert create(n_edges=n) == INVALID and "n_edges" in err()
    assert create(edges=None) == INVALID and "edges_host" in err()
    for at, v in ((0, 0.0), (0, -1.0), (17, float("nan")), (6000, float("inf")), (40, E[39]), (40, E[38]), (1, -float("inf"))):
        bad = E.copy()
        bad[at] = v
        assert create(edges=bad) == INVALID and "edges_host[%d]" % at in err(), (at, v)
    for t in (-1e-9, 1.0000001, float("nan"), float("inf")):
        assert create(thr_pow=t) == INVALID and "thr_pow" in err(), t
    for b in (0.0, -1.0, float("nan"), float("inf")):
        assert create(bin_hz=b) == INVALID and "bin_hz" in err(), b
    # the other entry points: the handle comes first
    x = ctypes.c_void_p(16)
    assert nat.lib.rts_tuning_accumulate(None, x, 1, None, 1, x, None) == INVALID and "handle" in err()
    assert nat.lib.rts_tuning_pick(None, x, 1, 5, x, x, None) == INVALID and "handle" in err()
    assert nat.lib.rts_tuning_destroy(None) == 0


# ---- (d) csrc/tuning_plan.h under the sanitizers ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "tuning_plan_driver")
    rc, out, err = _run(["g++", "-std=c++17", "-ffp-contract=off"] + FLAGS +
                        [os.path.join(SAN, "tuning_plan_driver.cpp"), "-o", exe], timeout=300)
    assert rc == 0, err[-3000:]
    return exe


def run_driver(driver, tmp_path, picks=(), creates=(), pickchecks=(), searches=(), layouts=()):
    lines = ["%d %d %d %d %d" % (len(picks), len(creates), len(pickchecks), len(searches), len(layouts))]
    for h, W in picks:
        lines.append("%d %d" % (len(h), W))
        lines.append(" ".join(str(int(v)) for v in h))
    for (fft_len, k_lo, k_hi, R, n_edges, bin_hz, thr_pow, kind, at) in creates:
        lines.append("%d %d %d %d %d %s %s %d %d" % (fft_len, k_lo, k_hi, R, n_edges, hexbits(bin_hz), hexbits(thr_pow), kind, at))
    for R, W in pickchecks:
        lines.append("%d %d" % (R, W))
    for E, R, fs in searches:
        lines.append("%d %d %d" % (len(E), R, len(fs)))
        lines.append(" ".join(hexbits(float(v)) for v in E))
        lines.append(" ".join(hexbits(float(v)) for v in fs))
    for l in layouts:
        lines.append("%d %d %d" % l)
    case = tmp_path / "case.txt"
    case.write_text("\n".join(lines) + "\n")
    rc, out, err = _run([driver, str(case)], env=ENV, timeout=120)
    _clean_report(err)
    assert rc == 0, (rc, out[-1000:], err[-2000:])
    got = [l.split() for l in out.splitlines()]
    assert got[-1] == ["sweep", "checked"]                          # the driver's own sweep over grids and layouts
    return got[:-1]


def test_plan_pick_equals_the_model(driver, tmp_path):
    cases = tm.pick_cases()
    got = run_driver(driver, tmp_path, picks=[(h, W) for _, h, W in cases])
    assert len(got) == len(cases) >= 18
    for (name, h, W), line in zip(cases, got):
        cents, n = tm.pick(h, W)
        assert line == ["pick", hexbits(cents), str(n)], (name, line, cents, n)


def test_plan_refusals(driver, tmp_path):
    nan, inf = float("nan"), float("inf")
    good = (4096, 28, 743, 100, 6001, BIN_HZ, 0.01, 0, 0)

    def case(**kw):
        d = dict(zip(("fft_len", "k_lo", "k_hi", "R", "n_edges", "bin_hz", "thr_pow", "kind", "at"), good))
        d.update(kw)
        return tuple(d[k] for k in ("fft_len", "k_lo", "k_hi", "R", "n_edges", "bin_hz", "thr_pow", "kind", "at"))

    creates = [(good, OK, -1)]
    creates += [(case(fft_len=L, k_lo=1, k_hi=1), BAD_FFT, -1) for L in (32, 63, 65, 4095, 16384, 0, -64)]
    creates += [(case(fft_len=L, k_lo=1, k_hi=L // 2 - 1), OK, -1) for L in (64, 128, 8192)]
    creates += [(case(k_lo=lo, k_hi=hi), BAD_BINS, -1) for lo, hi in ((0, 5), (6, 5), (1, 2048), (-3, -2))]
    creates += [(case(k_lo=1, k_hi=2047), OK, -1), (case(k_lo=2047, k_hi=2047), OK, -1)]
    creates += [(case(R=0), BAD_R, -1), (case(R=-1), BAD_R, -1), (case(R=1025), BIG_R, -1), (case(R=1024), OK, -1), (case(R=1), OK, -1)]
    creates += [(case(n_edges=1), FEW_EDGES, -1), (case(n_edges=0), FEW_EDGES, -1), (case(n_edges=2), OK, -1)]
    creates += [(case(kind=1), NO_EDGES, -1)]
    creates += [(case(kind=k, at=at), BAD_EDGES, at) for k in (2, 3, 4, 5, 6) for at in (1, 3000, 6000)]
    creates += [(case(kind=k, at=0), BAD_EDGES, 0) for k in (3, 4, 5, 6)]
    creates += [(case(thr_pow=t), BAD_THR, -1) for t in (-0.5, 1.5, nan, inf, -inf)]
    creates += [(case(thr_pow=t), OK, -1) for t in (0.0, 1.0, -0.0)]
    creates += [(case(bin_hz=b), BAD_BIN_HZ, -1) for b in (0.0, -1.0, nan, inf)]
    creates += [(case(fft_len=100, R=0, n_edges=0, thr_pow=nan), BAD_FFT, -1)]      # the first rule broken is reported
    pickchecks = [((100, 5), OK), ((100, 49), OK), ((100, 50), BAD_W), ((101, 50), OK), ((1, 0), OK), ((1, 1), BAD_W), ((7, 3), OK),
                  ((7, 4), BAD_W), ((100, -1), BAD_W), ((1024, 511), OK), ((1024, 512), BAD_W), ((100, 2 ** 31 - 1), BAD_W)]
    got = run_driver(driver, tmp_path, creates=[c for c, _, _ in creates], pickchecks=[p for p, _ in pickchecks])
    for (c, why, bad), line in zip(creates, got):
        assert line == ["create", str(why), str(int(why in (BAD_FFT, BIG_R))), str(bad)], (c, line)
    for (p, why), line in zip(pickchecks, got[len(creates):]):
        assert line == ["pickcheck", str(why)], (p, line)


def test_plan_edge_search_and_layout(driver, tmp_path, defaults):
    k_lo, k_hi, E = defaults
    rs = np.random.RandomState(5)
    fs = np.concatenate([E[[0, 1, 2999, 5999, 6000]], np.nextafter(E[[0, 1, 2999, 6000]], 0.0), np.nextafter(E[[0, 5999, 6000]], np.inf),
                         [0.0, -1.0, 1e-300, 1e300, np.inf, -np.inf, np.nan], rs.uniform(100.0, 4500.0, 200)])
    small = np.array([1.0, 2.0, 4.0])
    one = np.array([3.0])
    fsmall = np.array([0.5, 1.0, 1.5, 2.0, 3.9, 4.0, 5.0, np.nan])
    got = run_driver(driver, tmp_path, searches=[(E, 100, fs), (small, 7, fsmall), (one, 1, fsmall), (E, 1024, fs[:20])],
                     layouts=[(4096, 6001, 100), (8192, 6001, 100), (64, 6001, 100), (4096, 6001, 1024), (8192, 2, 1)])

    def want(E, R, fs):
        out = []
        for f in fs:
            n = -1 if np.isnan(f) else int(np.searchsorted(E, f, "right")) - 1
            out.append("%d:%d" % (n, -1 if (n < 0 or n >= len(E) - 1) else n % R))
        return out

    assert got[0] == ["search"] + want(E, 100, fs)
    assert got[1] == ["search"] + want(small, 7, fsmall) == ["search", "-1:-1", "0:0", "0:0", "1:1", "1:1", "2:-1", "2:-1", "-1:-1"]
    assert got[2] == ["search"] + want(one, 1, fsmall)
    assert got[3] == ["search"] + want(E, 1024, fs[:20])
    # the default layout stages the edge table and fits 64 KiB: P 2050 doubles, 6001 edges, 8 wave maxima, 100 counters
    assert got[4] == ["layout", "2050", "1", "16400", str(16400 + 48008), str(16400 + 48008 + 64), str(16400 + 48008 + 64 + 400)]
    assert int(got[4][6]) <= 65536
    assert got[5][:3] == ["layout", "4098", "0"] and got[5][3] == got[5][4]        # 8192-point frames leave the table to L2
    assert got[6][:3] == ["layout", "34", "1"]
    assert got[7][:3] == ["layout", "2050", "0"]
    assert got[8] == ["layout", "4098", "1", "32784", "32800", "32864", "32868"]
