"""The time map of a path (include/rtsync.h, rts_path_map) in plain Python: the definition, and the reference
of tests/test_pathmap_cpu.py and tests/test_pathmap_gpu.py.  Python floats are float64 and every expression below is
written in the operation order of the definition, so `==` on its results is a bit-for-bit comparison (`same` compares NaN
with NaN).  Nothing here imports the package."""
import bisect
import struct

OK, EMPTY, BACKWARD, NEGATIVE = 0, 1, 2, 4
NAN = float("nan")


def columns(path, from_side=0, off=(0, 0), length=None):
    """(u, v): the `from_side` column and the other one, offsets added (off[c] belongs to column c), the first `length`
    points (None: all; below 0: none)."""
    n = len(path) if length is None else max(0, min(int(length), len(path)))
    u = [int(path[t][from_side]) + int(off[from_side]) for t in range(n)]
    v = [int(path[t][1 - from_side]) + int(off[1 - from_side]) for t in range(n)]
    return u, v


def status(path, from_side=0, off=(0, 0), length=None):
    u, v = columns(path, from_side, off, length)
    if len(u) < 1:
        return EMPTY
    st = OK
    if any(a < 0 for a in u) or any(a < 0 for a in v):
        st |= NEGATIVE
    if any(u[t] < u[t - 1] or v[t] < v[t - 1] for t in range(1, len(u))):
        st |= BACKWARD
    return st


def knots(path, from_side=0, off=(0, 0), length=None):
    """(k, m) of a usable path: the distinct values of u, and the middle of v's run at each."""
    u, v = columns(path, from_side, off, length)
    k, m = [], []
    t = 0
    while t < len(u):
        e = t
        while e + 1 < len(u) and u[e + 1] == u[t]:
            e += 1
        k.append(u[t])
        m.append(float(v[t] + v[e]) * 0.5)
        t = e + 1
    return k, m


def image(k, m, x):
    """y(x) on the knots (k, m)."""
    x = float(x)
    if x != x or x < k[0] or x > k[-1]:
        return NAN
    i = bisect.bisect_right(k, x) - 1          # the last knot with k_i <= x
    if x == k[i]:
        return m[i]
    return m[i] + ((x - float(k[i])) * (m[i + 1] - m[i])) / float(k[i + 1] - k[i])


def map_positions(path, xs, from_side=0, off=(0, 0), length=None):
    """-> ([y(x) for x in xs], status); all NaN for a refused path."""
    st = status(path, from_side, off, length)
    if st:
        return [NAN for _ in xs], st
    k, m = knots(path, from_side, off, length)
    return [image(k, m, x) for x in xs], OK


def transfer(path, times, frame_seconds, from_side=0, off=(0, 0), length=None):
    """The times of a table carried along the path -> (new times with NaN for "no image", status)."""
    frame_seconds = float(frame_seconds)
    ys, st = map_positions(path, [float(t) / frame_seconds for t in times], from_side, off, length)
    return [NAN if y != y else y * frame_seconds for y in ys], st


def carried_table(path, table, frame_seconds, from_side=0, off=(0, 0)):
    """What AnnotationTables.transfer keeps of `table` = (times, beats[, labels]): ((times, beats, labels | None), dropped
    row indices)."""
    new, st = transfer(path, table[0], frame_seconds, from_side, off)
    assert st == OK, st
    keep = [r for r, y in enumerate(new) if y == y]
    labels = None if len(table) < 3 or table[2] is None else [table[2][r] for r in keep]
    return ([new[r] for r in keep], [table[1][r] for r in keep], labels), [r for r, y in enumerate(new) if y != y]


def bits(values):
    return struct.pack("<%dd" % len(values), *[float(v) for v in values])


def same(a, b):
    """Bit-for-bit equality of two sequences of floats."""
    return len(a) == len(b) and bits(a) == bits(b)
