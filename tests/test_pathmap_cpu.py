"""The time map of a path without a GPU: the plain-Python definition (tests/pathmap_model.py) and its consequences; what it
does with the committed chopin pair (dtw_golden's dtw_chopin/path, made by the reference's own dtw.py, and the two hand-made
tables); the carried table inside the existing metric; csrc/pathmap_plan.h through a stand-alone driver built with
AddressSanitizer and UndefinedBehaviorSanitizer; the argument refusals of the C ABI that need no device.  Every comparison
of floats is `==` (bit for bit through `pm.same` where NaN occurs), except the 1.0 s bound of the accuracy test."""
import ctypes
import math
import os
import random

import pytest

import annot_model as am
import pathmap_model as pm
from conftest import GOLDEN
from real_time_audio_sync_amd import evaluate
from test_sanitize_cpu import ENV, FLAGS, OUT, SAN, _clean_report, _run

RUB_CSV = os.path.join(GOLDEN, "chopin_rubinstein_20b.csv")        # column 1 of dtw_chopin/path, 380 frames
RACH_CSV = os.path.join(GOLDEN, "chopin_rachmaninoff_20b.csv")     # column 0, 401 frames
FS = evaluate.FRAME_SECONDS


def random_path(rng, n_knots, max_run=4, max_gap=3, start=(0, 0)):
    """A usable path with vertical and horizontal runs and steps larger than 1 on both columns."""
    u, v = start
    pts = [(u, v)]
    for _ in range(n_knots):
        for _ in range(rng.randrange(max_run)):                     # a vertical run: u stays
            v += rng.randrange(max_gap + 1)
            pts.append((u, v))
        u += 1 + rng.randrange(max_gap)                             # a new knot, maybe behind a gap, maybe flat in v
        v += rng.randrange(max_gap + 1)
        pts.append((u, v))
    return pts


# ---- (1) the model's properties -----------------------------------------------------------------------------------------

def test_identity_path_gives_the_position_back():
    path = [(t, t) for t in range(300)]
    xs = list(range(300)) + [0.5, 1.25, 7.0 / 3.0, 298.999999, 100.0 + 2.0 ** -40, math.pi * 50]
    for side in (0, 1):
        ys, st = pm.map_positions(path, xs, side)
        assert st == pm.OK and pm.same(ys, xs)


def test_knots_map_to_the_middle_of_their_runs():
    path = [(0, 0), (0, 1), (0, 4), (1, 4), (3, 5), (3, 6), (7, 6), (8, 9)]
    assert pm.knots(path, 0) == ([0, 1, 3, 7, 8], [2.0, 4.0, 5.5, 6.0, 9.0])
    assert pm.knots(path, 1) == ([0, 1, 4, 5, 6, 9], [0.0, 0.0, 0.5, 3.0, 5.0, 8.0])
    rng = random.Random(5)
    for side in (0, 1):
        for trial in range(20):
            p = random_path(rng, 60)
            k, m = pm.knots(p, side)
            assert k == sorted(set(k)) and all(a <= b for a, b in zip(m, m[1:]))
            ys, st = pm.map_positions(p, k, side)
            assert st == pm.OK and pm.same(ys, m)
    # between two knots: the operations in their order
    k, m = pm.knots(path, 0)
    assert pm.image(k, m, 4.5) == 5.5 + ((4.5 - 3.0) * (6.0 - 5.5)) / 4.0 and pm.image(k, m, 2.0) == 4.0 + (1.0 * 1.5) / 2.0


def test_the_map_does_not_decrease():
    rng = random.Random(11)
    for side in (0, 1):
        p = random_path(rng, 400, max_run=5, max_gap=7, start=(3, 9))
        k, _ = pm.knots(p, side)
        near = [float(a) for a in k[:300]] + [math.nextafter(float(a), s) for a in k[1:251] for s in (-math.inf, math.inf)]
        xs = sorted(near + [rng.uniform(k[0], k[-1]) for _ in range(10000 - len(near))])
        assert len(xs) == 10000 and len(k) >= 300
        ys, st = pm.map_positions(p, xs, side)
        assert st == pm.OK and all(y == y for y in ys[:-1]) and all(a <= b for a, b in zip(ys, ys[1:]) if b == b)


def test_nan_exactly_outside_the_knots():
    path = [(2, 5), (2, 6), (4, 6), (9, 8)]
    k, m = pm.knots(path, 0)
    assert (k[0], k[-1]) == (2, 9)
    inside = [2.0, math.nextafter(2.0, 3.0), 5.5, math.nextafter(9.0, 0.0), 9.0]
    outside = [math.nextafter(2.0, 0.0), math.nextafter(9.0, 10.0), 0.0, -0.0, -1.0, 2.0 ** 31, 1e300, math.inf, -math.inf, math.nan]
    ys, st = pm.map_positions(path, inside + outside, 0)
    assert st == pm.OK and all(y == y for y in ys[:len(inside)]) and all(y != y for y in ys[len(inside):])
    assert ys[0] == 5.5 and ys[4] == 8.0
    # -0.0 is a position like 0.0
    assert pm.same(pm.map_positions([(0, 3), (1, 4)], [-0.0, 0.0], 0)[0], [3.0, 3.0])


def test_offsets_shift_both_sides():
    rng = random.Random(2)
    p = random_path(rng, 50)
    moved = [(a + 1000, b + 70) for a, b in p]
    for side in (0, 1):
        xs = [rng.uniform(0, 1200) for _ in range(400)]
        ys, st = pm.map_positions(p, xs, side, off=(1000, 70))          # the path with offsets is the shifted path
        assert st == pm.OK and pm.same(ys, pm.map_positions(moved, xs, side)[0]) and sum(y == y for y in ys) > 20
        k, m = pm.knots(p, side)                                        # and at the knots the shift is exact
        ys, _ = pm.map_positions(p, [float(a + (1000, 70)[side]) for a in k], side, off=(1000, 70))
        assert pm.same(ys, [b + float((70, 1000)[side]) for b in m])
    # an offset can make a path usable, or refuse it
    assert pm.status([(-3, 0), (-2, 1)], 0) == pm.NEGATIVE and pm.status([(-3, 0), (-2, 1)], 0, off=(3, 0)) == pm.OK
    assert pm.status([(0, 0), (1, 1)], 0, off=(0, -1)) == pm.NEGATIVE


def test_a_one_point_path_maps_only_its_own_u():
    ys, st = pm.map_positions([(7, 3)], [7.0, 6.999, 7.001, 3.0, math.nan], 0)
    assert st == pm.OK and pm.same(ys, [3.0] + [pm.NAN] * 4)
    ys, st = pm.map_positions([(7, 3), (7, 4), (7, 8)], [7.0, 8.0], 0)          # one knot, a run
    assert st == pm.OK and pm.same(ys, [5.5, pm.NAN])
    assert pm.same(pm.map_positions([(7, 3)], [3.0, 7.0], 1)[0], [7.0, pm.NAN])


def test_refusal_bits_alone_and_combined():
    good = [(0, 0), (1, 1), (2, 1)]
    assert pm.status(good) == pm.OK
    assert pm.status([]) == pm.EMPTY and pm.status(good, length=0) == pm.EMPTY and pm.status(good, length=-1) == pm.EMPTY
    assert pm.status([(0, 0), (1, 1), (0, 2)]) == pm.BACKWARD and pm.status([(0, 1), (1, 0)]) == pm.BACKWARD
    assert pm.status([(0, 1), (1, 0)], length=1) == pm.OK                        # only the first `length` points count
    assert pm.status([(-1, 0), (0, 1)]) == pm.NEGATIVE and pm.status([(0, -1), (0, 1)], 1) == pm.NEGATIVE
    assert pm.status([(0, 0), (-1, 1)]) == pm.BACKWARD | pm.NEGATIVE
    assert pm.status(good, off=(-2, 0)) == pm.NEGATIVE and pm.status([(0, 5), (1, 4)], off=(0, -5)) == pm.BACKWARD | pm.NEGATIVE
    for bad in ([], [(0, 1), (1, 0)], [(-1, 0)]):
        ys, st = pm.map_positions(bad, [0.0, 1.0, math.nan], 0)
        assert st != pm.OK and pm.same(ys, [pm.NAN] * 3)
    assert pm.same(pm.transfer([], [1.0, 2.0], 0.5)[0], [pm.NAN] * 2)
    new, st = pm.transfer([(0, 0), (4, 8)], [0.0, 1.0, 2.0, 2.5], 0.5)          # frames 0, 2, 4 and 5: the last has no image
    assert st == pm.OK and pm.same(new, [0.0, 2.0, 4.0, pm.NAN])


# ---- (2) the committed chopin pair ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chopin(dtw_golden):
    path = [(int(a), int(b)) for a, b in dtw_golden["dtw_chopin/path"]]
    tables = {0: evaluate.read_annotations(RACH_CSV), 1: evaluate.read_annotations(RUB_CSV)}
    return path, tables


@pytest.mark.parametrize("side", (0, 1))
def test_accuracy_on_the_chopin_pair(chopin, side):
    """Each hand-made table carried onto the other recording lies within 1.0 s of that recording's own hand-made table, the
    smallest of the reference's THRESHOLDS and the level at which eval_golden.json reports 0 % for this path."""
    path, tables = chopin
    src, want = tables[side], tables[1 - side]
    assert pm.status(path, side) == pm.OK and list(src[1]) == list(want[1]) and len(src[0]) == 20
    (times, beats, labels), dropped = pm.carried_table(path, src, FS, side)
    assert dropped == [19]                                       # the last row lies behind the last aligned frame
    assert beats == list(src[1][:19]) and labels == list(src[2][:19])
    err = [abs(t - w) for t, w in zip(times, want[0])]
    print("side %d: mean %.3f s, worst %.3f s" % (side, sum(err) / len(err), max(err)))
    assert max(err) <= 1.0
    assert all(a <= b for a, b in zip(times, times[1:])) and all(math.isfinite(t) for t in times)


def test_carried_table_in_the_existing_metric(chopin):
    """Rubinstein's table carried onto Rachmaninoff and held against Rubinstein's own along the path: no point off by more
    than one beat, what eval_golden.json says of the hand-made pair."""
    path, tables = chopin
    (times, beats, _), _ = pm.carried_table(path, tables[1], FS, 1)
    err, counts = am.metric(path, (times, beats), (tables[1][0], tables[1][1]), FS)
    assert counts[0] > 300 and counts[9] == 0
    assert am.stats(err, counts)["pct_off_beats"][1] == 0


# ---- (4) csrc/pathmap_plan.h under the sanitizers -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "pathmap_plan_driver")
    rc, out, err = _run(["g++", "-std=c++17"] + FLAGS + [os.path.join(SAN, "pathmap_plan_driver.cpp"), "-o", exe], timeout=300)
    assert rc == 0, err[-3000:]
    return exe


(R_OK, R_PMAX, R_NO_PATH, R_NO_LEN, R_FROM, R_ENTRIES, R_NO_IN, R_BATCH, R_NO_OUT, R_NO_STATUS) = range(10)   # PathmapRefusal


def test_plan_header_under_sanitizers(driver, tmp_path):
    good = dict(path=1, P_max=8, len=1, frm=0, inp=1, needed=0, n_max=4, B=3, out=1, status=1)
    order = ("path", "P_max", "len", "frm", "inp", "needed", "n_max", "B", "out", "status")
    checks = [({}, R_OK), (dict(P_max=-1), R_PMAX), (dict(P_max=2 ** 30, n_max=2 ** 30), R_OK), (dict(P_max=2 ** 30 + 1), R_PMAX),
              (dict(n_max=2 ** 30 + 1), R_ENTRIES), (dict(path=0), R_NO_PATH), (dict(path=0, P_max=0), R_OK), (dict(len=0), R_NO_LEN),
              (dict(frm=2), R_FROM), (dict(frm=-1), R_FROM), (dict(frm=1), R_OK), (dict(n_max=-1), R_ENTRIES), (dict(inp=0), R_NO_IN),
              (dict(inp=0, n_max=0), R_OK), (dict(inp=0, n_max=0, needed=1), R_NO_IN), (dict(B=0), R_BATCH), (dict(B=-4), R_BATCH),
              (dict(B=65535), R_OK), (dict(B=65536), R_BATCH), (dict(out=0), R_NO_OUT), (dict(out=0, n_max=0, inp=0), R_OK),
              (dict(status=0), R_NO_STATUS), (dict(P_max=-1, path=0, len=0, frm=5, B=0), R_PMAX), (dict(len=0, frm=5, B=0), R_NO_LEN)]
    cases = [("C",) + tuple(dict(good, **c)[k] for k in order) for c, _ in checks]
    offs = [(0, 40000, 420), (1, 1, 1), (26843, 40000, 2100), (26844, 40000, 2100), (65534, 40000, 40000), (65534, 2 ** 31 - 1, 2 ** 31 - 1),
            (7, 0, 0)]
    cases += [("O",) + o for o in offs]
    geoms = [(-1, 10), (0, 10), (1, 10), (255, 300), (256, 300), (257, 300), (1025, 2000), (5000, 300), (40000, 40000), (2 ** 31 - 1, 2 ** 31 - 1)]
    cases += [("G",) + g for g in geoms]
    ents = [(0, 5, 9), (1, 5, 9), (1, -1, 9), (1, 10, 9), (1, 0, 0), (0, -3, 0), (1, 2 ** 31 - 1, 2 ** 31 - 1)]
    cases += [("E",) + e for e in ents]
    cases += [("B", b) for b in (1, 64, 65535)]
    case = tmp_path / "case.txt"
    case.write_text("".join(" ".join(str(v) for v in c) + "\n" for c in cases))
    rc, out, err = _run([driver, str(case)], env=ENV, timeout=120)
    _clean_report(err)
    assert rc == 0, (rc, out[-1000:], err[-2000:])
    lines = out.splitlines()
    assert lines[-1] == "sweep checked" and len(lines) == len(cases) + 1
    words = {R_PMAX: "P_max", R_NO_PATH: "path_dev", R_NO_LEN: "len_dev", R_FROM: "from", R_BATCH: "B", R_NO_STATUS: "status_dev"}
    for (_, want), line in zip(checks, lines):
        head, msg_map, msg_transfer = line.split(" | ")
        assert int(head.split()[-1]) == want, line
        if want in words:
            assert words[want] in msg_map and msg_map == msg_transfer, line
        elif want != R_OK:
            a, b = {R_ENTRIES: ("n_max", "rows_max"), R_NO_IN: ("x_dev", "piece_dev"), R_NO_OUT: ("y_dev", "times_dev")}[want]
            assert a in msg_map and b in msg_transfer, line
    rest = [[int(v) for v in l.split()[1:]] for l in lines[len(checks):-1]]
    for c, got in zip(cases[len(checks):], rest):
        a = list(c[1:])
        if c[0] == "O":
            assert got == a + [a[0] * a[1] * 2, a[0] * a[2]], c
        elif c[0] == "G":
            pts = max(0, min(a[0], a[1]))
            assert got == a + [pts, -(-pts // 256)], c
        elif c[0] == "E":
            assert got == a + [a[2] if not a[0] else max(0, min(a[1], a[2]))], c
        else:
            assert got == a + a, c
    assert 26844 * 40000 * 2 > 2 ** 31 > 26843 * 40000 * 2 and 65534 * 40000 * 2 > 2 ** 32


# ---- (5) refusals that need no device ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as ge
    ge.build()
    from real_time_audio_sync_amd import _native
    return _native


def test_abi_refusals_without_a_device(nat):
    for name, n_args in (("rts_path_map", 12), ("rts_annot_transfer", 13)):
        assert name in nat.EXPORTS and len(nat.EXPORTS[name].argtypes) == n_args, name
    assert (nat.PATHMAP_OK, nat.PATHMAP_EMPTY, nat.PATHMAP_BACKWARD, nat.PATHMAP_NEGATIVE) == (pm.OK, pm.EMPTY, pm.BACKWARD, pm.NEGATIVE)
    p = ctypes.c_void_p(16)                                          # never dereferenced: every case is refused first
    good = [p, 8, p, None, 0, p, 4, None, 2, p, p, None]
    for pos, bad, word in ((0, None, b"path_dev"), (1, -1, b"P_max"), (2, None, b"len_dev"), (4, 2, b"from"), (4, -1, b"from"),
                           (5, None, b"x_dev"), (6, -1, b"n_max"), (8, 0, b"B"), (8, 65536, b"B"), (9, None, b"y_dev"),
                           (10, None, b"status_dev")):
        args = list(good)
        args[pos] = bad
        assert nat.lib.rts_path_map(*args) == -1 and word in nat.lib.rts_last_error(), word
    good = [p, p, 8, p, None, 1, p, 2, 20, p, p, p, None]
    for pos, bad, word in ((0, None, b"handle"), (1, None, b"path_dev"), (2, -1, b"P_max"), (3, None, b"len_dev"), (5, 2, b"from"),
                           (6, None, b"piece_dev"), (7, 0, b"B"), (7, 65536, b"B"), (8, -1, b"rows_max"), (9, None, b"times_dev"),
                           (10, None, b"n_rows_dev"), (11, None, b"status_dev")):
        args = list(good)                                            # the handle is read only after all of these
        args[pos] = bad
        assert nat.lib.rts_annot_transfer(*args) == -1 and word in nat.lib.rts_last_error(), word
