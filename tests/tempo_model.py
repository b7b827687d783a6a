"""The tempo definition of include/rtsync.h (rts_path_tempo) restated in plain Python, for tests/test_tempo_cpu.py (closed
forms) and tests/test_tempo_gpu.py (which holds the kernels against it).  The sums are Python integers, so they are exact
whatever their size; the model asserts that num and den fit in int64, the condition under which the library promises the
same integers.  Python floats are float64, float(int) rounds to nearest even, and every expression is written in the
operation order of the definition, so a bit-for-bit comparison of its results is meaningful.  The beats-per-minute rule
sits on top of tests/annot_model.py's lookup.  Nothing here imports the package."""
import bisect
import math

import annot_model as am

NAN = float("nan")      # the canonical quiet NaN 0x7ff8000000000000
MIN_K, MAX_K = 2, 1024


def overflows(K, x_limit, y_limit):
    """The host-only refusal: K^2 * x_limit * y_limit >= 2^63."""
    return K * K * x_limit * y_limit >= 2 ** 63


def window(points, i, K, ahead, x_limit, y_limit):
    """-> (slope, pos, n) of the window of length K at point i of `points` (a list of (x, y) integers)."""
    assert MIN_K <= K <= MAX_K and math.isfinite(ahead)
    p0 = max(0, i - K + 1)
    win = [(int(x), int(y)) for x, y in points[p0:i + 1]]
    n = len(win)
    if any(not (0 <= x < x_limit and 0 <= y < y_limit) for x, y in win):
        return NAN, NAN, n
    sx = sum(x for x, _ in win)
    sy = sum(y for _, y in win)
    sxx = sum(x * x for x, _ in win)
    sxy = sum(x * y for x, y in win)
    den = n * sxx - sx * sx
    num = n * sxy - sx * sy
    assert abs(num) < 2 ** 63 and abs(den) < 2 ** 63, "the window's sums leave int64: outside the library's promise"
    if not den > 0:
        return NAN, NAN, n
    slope = float(num) / float(den)
    xi, yi = win[-1]
    sxr = sx - n * xi
    syr = sy - n * yi
    pos = (float(yi) + (float(syr) - slope * float(sxr)) / float(n)) + slope * ahead
    if pos != pos:
        pos = NAN
    return slope, pos, n


def curve(points, K, ahead, x_limit, y_limit):
    """-> (slopes, positions), one entry per point: `window` at every point, the window sums taken as differences of
    running sums (Python integers: exact, so these are the integers of `window`)."""
    assert MIN_K <= K <= MAX_K and math.isfinite(ahead)
    points = [(int(x), int(y)) for x, y in points]
    run = [(0, 0, 0, 0, 0)]                       # sums of x, y, x^2, xy and the count of bad points before point k
    for x, y in points:
        sx, sy, sxx, sxy, bad = run[-1]
        run.append((sx + x, sy + y, sxx + x * x, sxy + x * y, bad + (not (0 <= x < x_limit and 0 <= y < y_limit))))
    slopes, positions = [], []
    for i, (xi, yi) in enumerate(points):
        p0 = max(0, i - K + 1)
        n = i - p0 + 1
        sx, sy, sxx, sxy, bad = (a - b for a, b in zip(run[i + 1], run[p0]))
        slope = pos = NAN
        if not bad:
            den = n * sxx - sx * sx
            num = n * sxy - sx * sy
            assert abs(num) < 2 ** 63 and abs(den) < 2 ** 63, "the window's sums leave int64: outside the library's promise"
            if den > 0:
                slope = float(num) / float(den)
                pos = (float(yi) + (float(sy - n * yi) - slope * float(sx - n * xi)) / float(n)) + slope * ahead
                if pos != pos:
                    pos = NAN
        slopes.append(slope)
        positions.append(pos)
    return slopes, positions


def tail(points, K, ahead, x_limit, y_limit):
    """What a tracker publishes for a path whose stored points are `points`: (slope, pos, n), n = min(K, stored)."""
    points = [(int(x), int(y)) for x, y in points]
    if not points:
        return NAN, NAN, 0
    return window(points, len(points) - 1, K, ahead, x_limit, y_limit)


def bpm(slope, frame, times, beats, frame_seconds, frame0=0):
    """(slope * 60.0) / (times[i] - start) with i and start what annot_model.lookup uses for the same frame; NaN where
    there is no row, the row has no width, i == 0 and times[0] == 0, or the slope is NaN.  `times` empty: no such piece."""
    if frame < 0 or slope != slope or not len(times):
        return NAN
    beat, seg = am.lookup(frame, times, beats, frame_seconds, frame0)
    if beat is None:
        return NAN
    time = float(frame + frame0) * frame_seconds
    i = bisect.bisect_left(times, time)          # the row that lookup used
    assert i < len(times) and seg == (0 if i == 0 else i - 1)
    if i == 0 and times[0] == 0:
        return NAN
    start = 0.0 if i == 0 else times[i - 1]
    if times[i] == start:
        return NAN
    out = (slope * 60.0) / (times[i] - start)
    return out if out == out else NAN
