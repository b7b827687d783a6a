"""Tempo without a GPU: the plain-Python model of the definition (tests/tempo_model.py) on closed forms; the six symbols
of the C ABI and their refusals that need no device; the limits, the overflow rule and the ring arithmetic of
csrc/tempo_plan.h through a stand-alone driver built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a
child process.  Every comparison of floats is `==` or bit for bit."""
import ctypes
import math
import os
import struct

import pytest

import tempo_model as tm
from test_sanitize_cpu import ENV, FLAGS, OUT, SAN, _clean_report, _run

BIG = 1 << 40


def bits(v):
    return struct.pack("<d", v)


# ---- (a) the model on closed forms ----------------------------------------------------------------------------------------

def test_model_nan_is_canonical():
    assert bits(tm.NAN) == struct.pack("<Q", 0x7ff8000000000000)


@pytest.mark.parametrize("K", [2, 3, 16, 1024])
def test_model_line_through_the_origin(K):
    pts = [(x, 2 * x) for x in range(60)]
    slopes, pos = tm.curve(pts, K, 0.0, BIG, BIG)
    assert math.isnan(slopes[0]) and math.isnan(pos[0])            # one point has no slope
    assert all(s == 2.0 for s in slopes[1:])                       # exactly, at every i >= 1
    assert all(p == float(2 * x) for (x, _), p in zip(pts[1:], pos[1:]))
    ahead = tm.curve(pts, K, 7.5, BIG, BIG)[1]
    assert all(p == 2.0 * x + 15.0 for (x, _), p in zip(pts[1:], ahead[1:]))


def test_model_vertical_run_and_horizontal_run():
    vertical = [(5, y) for y in range(10)]
    slopes, pos = tm.curve(vertical, 4, 0.0, BIG, BIG)
    assert all(bits(s) == bits(tm.NAN) for s in slopes) and all(bits(p) == bits(tm.NAN) for p in pos)
    horizontal = [(x, 5) for x in range(10)]
    slopes, pos = tm.curve(horizontal, 4, 3.0, BIG, BIG)
    assert all(s == 0.0 for s in slopes[1:]) and all(p == 5.0 for p in pos[1:])
    # a vertical run inside a moving path: NaN exactly while the whole window stands on one live frame
    pts = [(x, x) for x in range(5)] + [(4, 4 + k) for k in range(1, 6)] + [(5 + k, 10 + k) for k in range(5)]
    slopes = tm.curve(pts, 3, 0.0, BIG, BIG)[0]
    stuck = [i for i in range(len(pts)) if i >= 2 and len(set(x for x, _ in pts[i - 2:i + 1])) == 1]
    assert stuck and [i for i, s in enumerate(slopes) if i >= 2 and math.isnan(s)] == stuck


def test_model_recovers_a_piecewise_warp():
    # y = x up to 100, then two reference frames per live frame, then one per two
    pts = [(x, x) for x in range(100)]
    pts += [(100 + k, 100 + 2 * k) for k in range(100)]
    pts += [(200 + k, 300 + k // 2) for k in range(100)]
    K = 16
    slopes, pos = tm.curve(pts, K, 0.0, BIG, BIG)
    for lo, hi, want in ((0, 100, 1.0), (100, 200, 2.0)):
        for i in range(lo + K - 1, hi):                            # the window lies within the piece
            assert slopes[i] == want and pos[i] == float(pts[i][1]), i
    tail = slopes[200 + K - 1:]
    assert all(abs(s - 0.5) < 0.02 for s in tail) and not all(s == 0.5 for s in tail)   # a staircase: near, not on, 0.5
    assert 1.0 < slopes[100 + K // 2] < 2.0                        # a window across the change of tempo lies between
    # translation invariance, and the trailing-window identity: entry i is the tail of the path cut at i
    moved = [(x + 12345, y + 777) for x, y in pts]
    s2, p2 = tm.curve(moved, K, 0.0, BIG, BIG)
    assert [bits(a) for a in s2] == [bits(a) for a in slopes]
    assert all(p2[i] == pos[i] + 777.0 for i in range(K - 1, 100))          # where the position is an integer
    for i in (0, 1, 50, 150, 299):
        s, p, n = tm.tail(pts[:i + 1], K, 0.0, BIG, BIG)
        assert bits(s) == bits(slopes[i]) and bits(p) == bits(pos[i]) and n == min(K, i + 1)
    assert tm.tail([], K, 0.0, BIG, BIG)[2] == 0


def test_model_bad_points_and_limits():
    pts = [(x, x) for x in range(20)]
    pts[9] = (-1, 9)
    pts[15] = (15, 40)                                             # over y_limit = 30
    slopes = tm.curve(pts, 4, 0.0, 30, 30)[0]
    want_nan = {0} | set(range(9, 13)) | set(range(15, 19))
    assert {i for i, s in enumerate(slopes) if math.isnan(s)} == want_nan
    with pytest.raises(AssertionError):                            # sums that leave int64 are outside the promise
        tm.curve([(0, 0), (2 ** 31 - 1, 2 ** 33)], 2, 0.0, 1 << 62, 1 << 62)
    assert tm.overflows(1024, 1 << 21, 1 << 22) and not tm.overflows(1024, 1 << 21, (1 << 22) - 1)


def test_model_curve_is_the_window_at_every_point():
    import random
    rnd = random.Random(8)
    pts, x, y = [], 4000000, 17
    for k in range(400):
        dx, dy = rnd.choice([(1, 0), (0, 1), (1, 1)])
        x, y = x + dx, y + dy
        pts.append((x, y))
    pts[120] = (-3, pts[120][1])
    pts[300] = (pts[300][0], 1 << 21)
    for K in (2, 5, 64, 1024):
        slopes, pos = tm.curve(pts, K, 1.25, 1 << 22, 1 << 21)
        direct = [tm.window(pts, i, K, 1.25, 1 << 22, 1 << 21) for i in range(len(pts))]
        assert [bits(s) for s in slopes] == [bits(d[0]) for d in direct], K
        assert [bits(p) for p in pos] == [bits(d[1]) for d in direct], K
        assert any(math.isnan(s) for s in slopes[2:]) and any(not math.isnan(s) for s in slopes)


def test_model_bpm():
    times, beats = [1.0, 2.0, 2.0, 4.0], [0, 1, 2, 3]
    h = 0.5
    assert tm.bpm(1.0, 1, times, beats, h) == 60.0                 # i == 0: the segment from time zero, 1 s wide
    assert tm.bpm(0.5, 3, times, beats, h) == 30.0                 # row 1: 1 s wide
    assert tm.bpm(1.5, 5, times, beats, h) == 45.0                 # row 3, start = times[2]: 2 s wide
    assert tm.bpm(1.0, 3, times, beats, h, frame0=2) == tm.bpm(1.0, 5, times, beats, h)
    for frame in (9, -1):                                          # past the table; negative
        assert bits(tm.bpm(1.0, frame, times, beats, h)) == bits(tm.NAN)
    assert bits(tm.bpm(tm.NAN, 1, times, beats, h)) == bits(tm.NAN)
    assert bits(tm.bpm(1.0, 0, [0.0, 1.0], [0, 1], h)) == bits(tm.NAN)          # i == 0 and times[0] == 0
    assert bits(tm.bpm(1.0, 1, [], [], h)) == bits(tm.NAN)                      # no such piece


# ---- (b) the ABI ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as ge
    ge.build()
    from real_time_audio_sync_amd import _native
    return _native


def test_abi_symbols(nat):
    lib = ctypes.CDLL(nat.SO_PATH)
    dbl = ctypes.c_double
    for name, n_args, doubles in (("rts_path_tempo", 11, [5]), ("rts_otw_tempo", 7, [2]), ("rts_wtw_tempo", 7, [2]),
                                  ("rts_annot_bpm", 10, []), ("rts_live_follow_tempo", 3, [2]), ("rts_live_tempo", 6, [])):
        assert hasattr(lib, name), name
        assert name in nat.EXPORTS and len(nat.EXPORTS[name].argtypes) == n_args, name
        assert [i for i, t in enumerate(nat.EXPORTS[name].argtypes) if t is dbl] == doubles, name
    assert nat.EXPORTS["rts_path_tempo"].argtypes[6] is ctypes.c_longlong and nat.EXPORTS["rts_path_tempo"].argtypes[7] is ctypes.c_longlong
    assert (nat.TEMPO_MIN_K, nat.TEMPO_MAX_K) == (tm.MIN_K, tm.MAX_K)
    assert nat.lib.rts_version() == 101 and nat.ANNOT_COUNTS == 10


def test_abi_refusals_without_a_device(nat):
    x = ctypes.c_void_p(16)                                        # never dereferenced: every check comes before the launch
    err = lambda: nat.lib.rts_last_error().decode()                # noqa: E731
    INVALID, UNSUPPORTED = -1, -2

    def curve(path=x, P_max=8, lens=x, B=1, K=4, ahead=0.0, xl=100, yl=100, slope=x, pos=x):
        return nat.lib.rts_path_tempo(path, P_max, lens, B, K, ahead, xl, yl, slope, pos, None)
    assert curve(lens=None) == INVALID and "len_dev" in err()
    assert curve(slope=None) == INVALID and "slope_dev" in err()
    assert curve(path=None) == INVALID and "path_dev" in err()
    assert curve(P_max=-1) == INVALID and "P_max" in err()
    assert curve(B=0) == INVALID and "B" in err()
    for K in (1, 1025, 0, -5):
        assert curve(K=K) == INVALID and "K must be in [2, 1024]" in err(), K
    for ahead in (float("nan"), float("inf"), -float("inf")):
        assert curve(ahead=ahead) == INVALID and "ahead" in err()
    assert curve(xl=0) == INVALID and "x_limit" in err()
    assert curve(yl=-3) == INVALID and "y_limit" in err()
    # the overflow rule, at both sides of 2^63, from the limits alone
    assert curve(K=1024, xl=1 << 21, yl=1 << 22) == UNSUPPORTED and "2^63" in err()
    assert curve(K=2, xl=1 << 31, yl=1 << 30) == UNSUPPORTED
    assert curve(K=2, xl=(1 << 62) + 5, yl=1) == UNSUPPORTED
    assert curve(K=1024, xl=1 << 21, yl=(1 << 22) - 1, P_max=0, path=None) == 0      # passes every check; nothing to launch
    assert curve(K=2, xl=1 << 31, yl=(1 << 30) - 1, P_max=0, path=None) == 0
    # handles come first
    assert nat.lib.rts_otw_tempo(None, 4, 0.0, x, x, x, None) == INVALID and "handle" in err()
    assert nat.lib.rts_wtw_tempo(None, 4, 0.0, x, x, x, None) == INVALID and "handle" in err()
    assert nat.lib.rts_annot_bpm(None, x, x, 1, None, x, None, 1, x, None) == INVALID and "handle" in err()
    assert nat.lib.rts_live_follow_tempo(None, 4, 0.0) == INVALID and "handle" in err()
    assert nat.lib.rts_live_follow_tempo(None, 0, 0.0) == INVALID
    assert nat.lib.rts_live_tempo(None, None, None, None, None, None) == INVALID and "handle" in err()


# ---- (c) csrc/tempo_plan.h under the sanitizers ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "tempo_plan_driver")
    rc, out, err = _run(["g++", "-std=c++17"] + FLAGS + [os.path.join(SAN, "tempo_plan_driver.cpp"), "-o", exe], timeout=300)
    assert rc == 0, err[-3000:]
    return exe


def run_driver(driver, tmp_path, limits=(), rings=(), grids=()):
    case = tmp_path / "case.txt"
    case.write_text("%d %d %d\n" % (len(limits), len(rings), len(grids)) + "".join("%d %d %d\n" % l for l in limits)
                    + "".join("%d %d %d\n" % r for r in rings) + "".join("%d %d\n" % g for g in grids))
    rc, out, err = _run([driver, str(case)], env=ENV, timeout=120)
    _clean_report(err)
    assert rc == 0, (rc, out[-1000:], err[-2000:])
    lines = [l.split() for l in out.splitlines()]
    assert lines[-1] == ["sweep", "checked"]                        # the driver's own sweep over every K
    return [tuple(int(v) for v in l[1:]) for l in lines[:-1]]


def test_plan_limits_and_overflow_rule(driver, tmp_path):
    top = 2 ** 63
    limits = []
    for K in (-1, 0, 1, 2, 3, 64, 1000, 1024, 1025):
        kk = max(K * K, 1)
        for x in (1, 2, 1 << 22, 1 << 31, 2 ** 63 - 1):
            edge = -(-top // (kk * x))                             # the smallest y that reaches 2^63
            for y in (1, edge - 1, edge, edge + 1, 2 ** 63 - 1):
                if 1 <= y < 2 ** 63:
                    limits.append((K, x, y))
    got = run_driver(driver, tmp_path, limits=limits)
    assert len(got) == len(limits) > 150
    seen = set()
    for (K, x, y), line in zip(limits, got):
        k_ok = tm.MIN_K <= K <= tm.MAX_K
        assert line == (K, x, y, int(k_ok), int(k_ok and tm.overflows(K, x, y))), (K, x, y)
        seen.add(line[3:])
    assert seen == {(0, 0), (1, 0), (1, 1)}


def test_plan_ring_and_geometry(driver, tmp_path):
    rings = [(K, P_max, n) for K in (2, 3, 63, 64, 255, 256, 257, 1000, 1023, 1024)
             for P_max, n in ((0, 5), (1, 1), (255, 255), (256, 256), (257, 257), (4097, 4097), (3000, 10 ** 6), (3000, -1),
                              (2 * K + 600, 2 * K + 600))]
    grids = [(1, 1), (5, 256), (5, 257), (64, 2100), (65535, 1), (17, 0)]
    got = run_driver(driver, tmp_path, rings=rings, grids=grids)
    for (K, P_max, n), line in zip(rings, got):
        eff = max(0, min(n, P_max))
        assert line == (K, P_max, n, 256 + K, (256 + K) * 36, -(-eff // 256), max(0, eff - K)), (K, P_max, n)
        assert line[4] + 4 * 36 <= 64 * 1024
    assert got[len(rings):] == [(B, n, -(-n // 256), B) for B, n in grids]
