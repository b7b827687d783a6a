"""Beats and labels without a GPU: the plain-Python model of the definition (tests/annot_model.py) against the project's
host form of the reference (evaluate.get_beat, AlignmentError.stats) and against the numbers the reference's own
test_simple class printed (tests/golden/eval_golden.json); the table checks of csrc/annot_plan.h through a stand-alone
driver built with AddressSanitizer and UndefinedBehaviorSanitizer; the argument refusals of the C ABI that need no
device.  Every comparison of floats is `==`."""
import ctypes
import json
import os

import numpy as np
import pytest

import annot_model as am
from conftest import GOLDEN
from real_time_audio_sync_amd import evaluate
from test_sanitize_cpu import ENV, FLAGS, OUT, SAN, _clean_report, _run

REF_CSV = os.path.join(GOLDEN, "chopin_rubinstein_20b.csv")
LIVE_CSV = os.path.join(GOLDEN, "chopin_rachmaninoff_20b.csv")
FS = evaluate.FRAME_SECONDS

OK, NO_PIECES, SHORT, RANGE, TIME, ORDER, BEAT = range(7)     # AnnotRefusal


def golden_paths(wtw_known_answer, dtw_golden):
    gold = json.load(open(os.path.join(GOLDEN, "eval_golden.json")))
    paths = {"wtw_known_answer": wtw_known_answer, "dtw_chopin": dtw_golden["dtw_chopin/path"],
             "shifted": np.array(gold["_paths"]["shifted"]), "drift": np.array(gold["_paths"]["drift"])}
    return gold, {k: [(int(l), int(r)) for l, r in v] for k, v in paths.items()}


def percent_lines(stats):
    return [stats["pct_off_beats"][t] for t in (1, 3, 5, 10)] + [stats["pct_off_seconds"][t] for t in (1, 3, 5, 10)]


# ---- (a) the lookup ---------------------------------------------------------------------------------------------------

def same_beat(frame, times, beats, frame_seconds):
    want = evaluate.get_beat(frame, times, beats, frame_seconds)
    got, seg = am.lookup(frame, times, beats, frame_seconds)
    assert (got is None) == (want is None) and (got is None or got == want), (frame, got, want)
    return got, seg


@pytest.mark.parametrize("csv", [REF_CSV, LIVE_CSV])
def test_model_lookup_equals_get_beat_on_the_chopin_tables(csv):
    times, beats = evaluate.read_ground_truth(csv)
    got = [same_beat(f, times, beats, FS) for f in range(501)]
    last = int(times[-1] / FS)
    assert last < 500 and got[last][0] is not None and got[last + 1] == (None, -1)      # the end of the table is inside
    assert got[0][1] == 0 and max(s for _, s in got) == len(times) - 2                  # every label index occurs
    assert sorted(set(s for _, s in got if s >= 0)) == list(range(len(times) - 1))


def test_model_lookup_on_synthetic_tables():
    h = 0.5                                                            # frame * h is exact: frames land on rows' times
    one = ([3.0], [7])
    zero = ([0.0, 1.0, 2.5], [4, 5, 6])
    rep = ([1.0, 2.0, 2.0, 2.0, 3.5], [0, 1, 2, 3, 4])                 # repeated times, beats[0] == 0
    for times, beats in (one, zero, rep):
        for f in range(12):
            same_beat(f, times, beats, h)
    assert am.lookup(6, *one, frame_seconds=h) == (7.0, 0) and am.lookup(7, *one, frame_seconds=h) == (None, -1)
    assert am.lookup(0, *one, frame_seconds=h) == (6.0, 0)
    assert am.lookup(0, *zero, frame_seconds=h) == (4.0, 0)            # i == 0 and times[0] == 0: the beat itself
    assert am.lookup(2, *zero, frame_seconds=h) == (5.0, 0) and am.lookup(3, *zero, frame_seconds=h)[1] == 1
    # a frame exactly on a repeated time belongs to the first row that has it; the rows behind it are never the first
    assert am.lookup(4, *rep, frame_seconds=h) == (1.0, 0)
    assert am.lookup(5, *rep, frame_seconds=h) == (4.0 - (3.5 - 2.5) / (3.5 - 2.0), 3)
    assert am.lookup(0, *rep, frame_seconds=h) == (-1.0, 0) and am.lookup(2, *rep, frame_seconds=h) == (0.0, 0)
    assert am.lookup(-1, *rep, frame_seconds=h) == (None, -1)
    assert am.lookup(1, *rep, frame_seconds=h, frame0=3) == am.lookup(4, *rep, frame_seconds=h)


def test_sticky_words():
    times, beats = [1.0, 2.0, 3.0], [0, 1, 2]
    s = am.Sticky()
    assert s.words() == (None, -1, -1)
    s.feed(None, times, beats, 0.5)
    assert s.words() == (None, -1, -1)
    s.feed(2, times, beats, 0.5, label_ok=[0, 1, 1])               # beat exactly 0.0: not taken; label 0 is empty
    assert s.words() == (None, -1, 2)
    s.feed(3, times, beats, 0.5, label_ok=[0, 1, 1])
    assert s.words() == (0.5, -1, 3)
    s.feed(5, times, beats, 0.5, label_ok=[0, 1, 1])
    assert s.words() == (1.5, 1, 5)
    s.feed(9, times, beats, 0.5, label_ok=[0, 1, 1])               # past the table: beat and label stay
    assert s.words() == (1.5, 1, 9)
    s.feed(1, times, beats, 0.5, frame0=2)                         # no flags: the label always changes
    assert s.words() == (0.5, 0, 3)


# ---- (b) the metric ---------------------------------------------------------------------------------------------------

def test_model_metric_equals_the_reference_numbers(wtw_known_answer, dtw_golden):
    gold, paths = golden_paths(wtw_known_answer, dtw_golden)
    live, ref = evaluate.read_ground_truth(LIVE_CSV), evaluate.read_ground_truth(REF_CSV)
    for name, path in paths.items():
        err, counts = am.metric(path, live, ref, FS)
        st = am.stats(err, counts)
        want = evaluate.AlignmentError(REF_CSV, LIVE_CSV, path).stats()
        assert counts[9] == 0 and st["count"] == want["count"], name
        assert percent_lines(st) == gold[name]["percent_lines"] and st["pct_off_seconds"][3] == gold[name]["returned"], name
        assert st["squared_beat_error"] == want["squared_beat_error"], name
        assert st == want, name


def test_model_metric_skips_and_index_errors():
    live = ([1.0, 2.0, 3.0], [0, 1, 2])
    ref = ([1.0, 2.0, 3.0, 4.0], [2, 3, 4, 5])
    # (2, 0): l_beat == 0.0, skipped; (3, 0): counts; (4, 4): r_beat 3.0 -> int() == len(live table): index error;
    # (7, 0): l_beat none
    err, counts = am.metric([(2, 0), (3, 0), (4, 4), (7, 0)], live, ref, 0.5)
    assert counts == [1, 0, 0, 0, 0, 0, 0, 0, 0, 1] and err == 0.5 * 0.5
    assert am.stats(0.0, [0] * 10) is None
    assert am.pymod1(2.25) == 0.25 and am.pymod1(-0.25) == 0.75 and am.pymod1(3.0) == 0.0
    assert am.time_of(-0.5, live[0]) == 1.0 + 0.5 * 1.0 and am.time_of(-1.0, live[0]) is None and am.time_of(3.0, live[0]) is None
    assert am.time_of(2.5, live[0]) == 3.0                          # the last row: nothing is interpolated


def test_read_annotations(tmp_path):
    times, beats, labels = evaluate.read_annotations(REF_CSV)
    assert (times, beats) == evaluate.read_ground_truth(REF_CSV) and labels == ["0"] * len(times)
    two = tmp_path / "two.csv"
    two.write_text("0.5,1\n1.5,2\n")
    assert evaluate.read_annotations(str(two)) == ([0.5, 1.5], [1, 2], None)
    three = tmp_path / "three.csv"
    three.write_text("0.5,1,A\n1.5,2,\n2.5,3\n")
    assert evaluate.read_annotations(str(three)) == ([0.5, 1.5, 2.5], [1, 2, 3], ["A", "", ""])


# ---- (c) the plan's checks ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "annot_driver")
    rc, out, err = _run(["g++", "-std=c++17"] + FLAGS + [os.path.join(SAN, "annot_driver.cpp"), "-o", exe], timeout=300)
    assert rc == 0, err[-3000:]
    return exe


def run_driver(driver, tmp_path, ranges, rows, n_rows=None, geoms=(), P=None):
    n_rows = len(rows) if n_rows is None else n_rows
    case = tmp_path / "case.txt"
    case.write_text("%d %d %d\n" % (len(ranges) if P is None else P, n_rows, len(geoms))
                    + "".join("%d %d\n" % r for r in ranges) + "".join("%s %d\n" % r for r in rows[:n_rows])
                    + "".join("%d %d\n" % g for g in geoms))
    rc, out, err = _run([driver, str(case)], env=ENV, timeout=120)
    _clean_report(err)
    assert rc == 0, (out[-1000:], err[-2000:])
    lines = out.splitlines()
    head, msg = lines[0].split(" msg=")
    d = dict((k, int(v)) for k, v in (item.split("=") for item in head.split()))
    return (d["rule"], d["piece"], d["row"]), msg, [tuple(int(x) for x in l.split()[1:]) for l in lines[1:]]


def test_plan_checks(driver, tmp_path):
    good = [("0.5", 1), ("1.5", 2), ("1.5", 2), ("0", 0), ("-1", 3), ("2", 3)]      # pieces (0, 3), (3, 1), (4, 2)
    ranges = [(0, 3), (3, 1), (4, 2)]
    assert run_driver(driver, tmp_path, ranges, good)[0] == (OK, 2, 1)
    assert run_driver(driver, tmp_path, [(4, 2), (0, 3), (1, 2)], good)[0][0] == OK           # any order, overlapping

    def bad(i, row):
        rows = list(good)
        rows[i] = row
        return rows
    got, msg, _ = run_driver(driver, tmp_path, ranges, bad(2, ("1.25", 2)))
    assert got == (ORDER, 0, 2) and "piece 0" in msg and "row 2" in msg
    got, msg, _ = run_driver(driver, tmp_path, ranges, bad(5, ("nan", 3)))
    assert got == (TIME, 2, 1) and "piece 2" in msg and "row 1" in msg
    assert run_driver(driver, tmp_path, ranges, bad(3, ("inf", 0)))[0] == (TIME, 1, 0)
    assert run_driver(driver, tmp_path, ranges, bad(4, ("-inf", 3)))[0] == (TIME, 2, 0)
    got, msg, _ = run_driver(driver, tmp_path, ranges, bad(1, ("1.5", -1)))
    assert got == (BEAT, 0, 1) and "piece 0" in msg and "row 1" in msg
    # the first piece's rule comes first, and inside a row the time's
    assert run_driver(driver, tmp_path, ranges, bad(1, ("nan", -1)))[0] == (TIME, 0, 1)
    for short in (0, -3):
        got, msg, _ = run_driver(driver, tmp_path, [(0, 3), (3, short), (4, 2)], good)
        assert got == (SHORT, 1, -1) and "piece 1" in msg
    # ranges past the pool: one row too many, a first behind the pool, a negative first, lengths near 2^31 -- no row of
    # such a piece is read (the arrays are exactly n_rows long)
    for rng in ((4, 3), (6, 1), (-1, 2), (5, 2 ** 31 - 1), (2 ** 62, 1)):
        got, msg, _ = run_driver(driver, tmp_path, [(0, 3), rng], good)
        assert got == (RANGE, 1, -1) and "piece 1" in msg and "6 rows" in msg, rng
    assert run_driver(driver, tmp_path, [(0, 1)], good, n_rows=0)[0] == (RANGE, 0, -1)
    for P in (0, -1):
        assert run_driver(driver, tmp_path, [], good, P=P)[0] == (NO_PIECES, -1, -1)


def test_plan_geometry(driver, tmp_path):
    geoms = [(1, 1), (5, 256), (5, 257), (64, 2100), (65535, 1), (65, 1), (128, 0)]
    got = run_driver(driver, tmp_path, [(0, 1)], [("1", 1)], geoms=geoms)[2]
    assert got == [(B, n, -(-n // 256), B, -(-B // 64)) for B, n in geoms]


# ---- (d) refusals that need no device ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as ge
    ge.build()
    from real_time_audio_sync_amd import _native
    return _native


def create(nat, ranges, times, beats, frame_seconds=FS, n_rows=None, out=True):
    first = np.array([r[0] for r in ranges], dtype=np.int64)
    lens = np.array([r[1] for r in ranges], dtype=np.int32)
    t, b = np.array(times, dtype=np.float64), np.array(beats, dtype=np.int32)
    h = ctypes.c_void_p()
    rc = nat.lib.rts_annot_create(len(ranges), len(t) if n_rows is None else n_rows, first.ctypes.data, lens.ctypes.data,
                                  t.ctypes.data, b.ctypes.data, None, frame_seconds, ctypes.byref(h) if out else None)
    return rc, nat.lib.rts_last_error().decode(), h


def test_abi_refusals_without_a_device(nat):
    for name, n_args in (("rts_annot_create", 9), ("rts_annot_destroy", 1), ("rts_annot_beats", 10),
                         ("rts_annot_path_error", 10), ("rts_live_annotate", 6), ("rts_live_beats", 5)):
        assert name in nat.EXPORTS and len(nat.EXPORTS[name].argtypes) == n_args, name
    assert nat.EXPORTS["rts_annot_create"].argtypes[7] is ctypes.c_double and nat.ANNOT_COUNTS == 10
    rc, msg, h = create(nat, [(0, 2)], [1.0, 2.0], [1, 2], out=False)
    assert rc == -1 and "out" in msg
    rc, msg, h = create(nat, [(0, 2), (2, 3)], [1.0, 2.0, 0.5, 3.0, 2.5], [1, 2, 0, 1, 2])
    assert rc == -1 and "piece 1" in msg and "row 2" in msg and not h.value
    rc, msg, h = create(nat, [(0, 2)], [1.0, float("nan")], [1, 2])
    assert rc == -1 and "piece 0" in msg and "row 1" in msg and not h.value
    rc, msg, h = create(nat, [(0, 2)], [1.0, 2.0], [1, -2])
    assert rc == -1 and "row 1" in msg and "negative" in msg
    rc, msg, h = create(nat, [(0, 0)], [1.0], [1])
    assert rc == -1 and "piece 0" in msg
    rc, msg, h = create(nat, [(1, 2)], [1.0, 2.0], [1, 2])
    assert rc == -1 and "piece 0" in msg and "pool" in msg
    rc, msg, h = create(nat, [], [1.0], [1])
    assert rc == -1 and "P" in msg
    for fs in (0.0, -1.0, float("nan"), float("inf")):
        rc, msg, h = create(nat, [(0, 1)], [1.0], [1], frame_seconds=fs)
        assert rc == -1 and "frame_seconds" in msg, fs
    assert create(nat, [(0, 1)], [1.0], [1], n_rows=0)[0] == -1
    x = ctypes.c_void_p(16)                                          # never dereferenced: the handle is checked first
    assert nat.lib.rts_annot_beats(None, x, 1, None, x, None, 1, x, None, None) == -1
    assert b"handle" in nat.lib.rts_last_error()
    assert nat.lib.rts_annot_path_error(None, x, 1, x, x, x, 1, x, x, None) == -1
    assert b"handle" in nat.lib.rts_last_error()
    assert nat.lib.rts_annot_destroy(None) == 0
    assert nat.lib.rts_live_annotate(None, None, None, None, None, None) == -1
    assert nat.lib.rts_live_beats(None, None, None, None, None) == -1 and b"handle" in nat.lib.rts_last_error()
