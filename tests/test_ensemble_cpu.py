"""Ensemble following without a GPU: (a) the plain-Python model of the three definitions (tests/ensemble_model.py) against
closed forms, the golden tables and evaluate.get_beat; (b) the host form ensemble.frames_of_beat against the model; (c) the
refusals the entry points make before any device call; (d) csrc/ensemble_plan.h and annot_invertible of csrc/annot_plan.h
through a stand-alone driver built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process.  Every
comparison of floats is `==` or bit for bit."""
import ctypes
import math
import os
import struct

import pytest

import annot_model as am
import ensemble_model as em
from conftest import GOLDEN
from test_sanitize_cpu import ENV, FLAGS, OUT, SAN, _clean_report, _run

FS = 2048 / 22050.
CSVS = [os.path.join(GOLDEN, "chopin_rubinstein_20b.csv"), os.path.join(GOLDEN, "chopin_rachmaninoff_20b.csv")]
INF = math.inf


def bits(x):
    return struct.pack("<d", x)


def read_table(path):
    times, beats = [], []
    for line in open(path):
        row = line.strip().split(",")
        if len(row) >= 2:
            times.append(float(row[0]))
            beats.append(int(row[1]))
    return times, beats


# ---- (a) invert ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("csv_path", CSVS)
def test_invert_round_trip_on_the_golden_tables(csv_path):
    from real_time_audio_sync_amd import evaluate
    times, beats = read_table(csv_path)
    assert em.invertible(beats)
    last = int(times[-1] / FS) + 3
    with_beat = 0
    for frame in range(last):
        beat = am.lookup(frame, times, beats, FS)[0]
        want = evaluate.get_beat(frame, times, beats)
        assert (beat is None) == (want is None) and (beat is None or bits(beat) == bits(float(want)))
        if beat is None:
            continue
        with_beat += 1
        assert em.invert(beat, times, beats, FS) == frame, frame      # every frame that has a beat comes back exactly
    assert with_beat > 200 and with_beat < last                       # frames behind the last row were looked at too


SYNTH_TIMES = [0.0, 1.0, 1.0, 2.5, 4.0, 7.0]      # times[0] == 0, a zero-width row (row 2)
SYNTH_BEATS = [0, 1, 2, 3, 7, 8]                  # a gap: beats 4..6 have no row


def test_invert_edge_cases():
    t, b = SYNTH_TIMES, SYNTH_BEATS
    fs = 0.25
    for i in range(len(t)):                                          # the row beats themselves: the row's own time
        assert em.invert(float(b[i]), t, b, fs) == math.floor(t[i] / fs + 0.5)
    assert em.invert(0.0, t, b, fs) == 0 and em.invert(-0.0, t, b, fs) == 0      # times[0] == 0: beat 0 is frame 0
    assert em.invert(-0.5, t, b, fs) == 0                            # before row 0 within one beat: time 0 (end == start == 0)
    assert em.invert(-1.0, t, b, fs) == 0 and em.invert(-1.0000001, t, b, fs) == -1
    assert em.invert(0.5, t, b, fs) == 2                             # 1.0 - 0.5 * 1.0 = 0.5 s
    assert em.invert(1.5, t, b, fs) == 4                             # the zero-width row: its one time, 1.0 s
    assert em.invert(2.5, t, b, fs) == 7                             # 2.5 - 0.5 * 1.5 = 1.75 s
    assert em.invert(5.0, t, b, fs) == -1 and em.invert(5.999, t, b, fs) == -1   # the gap
    assert em.invert(6.0, t, b, fs) == 10 and em.invert(6.5, t, b, fs) == 13     # 7 - 1: the stretch row 4 interpolates
    assert em.invert(8.0, t, b, fs) == 28
    assert em.invert(8.0000001, t, b, fs) == -1 and em.invert(INF, t, b, fs) == -1   # beyond the last beat
    assert em.invert(-INF, t, b, fs) == -1
    assert em.invert(em.NAN, t, b, fs) == -1 and em.invert(float("nan"), t, b, fs) == -1
    for bad in ([0, 1, 1, 3, 7, 8], [0, 2, 1, 3, 7, 8]):             # not strictly increasing: never a frame
        assert not em.invertible(bad)
        assert all(em.invert(x, t, bad, fs) == -1 for x in (0.0, 0.5, 1.0, 3.0, 8.0))
    assert em.invert(3.0, [1e300, 2e300], [1, 3], 1e-300) == -1      # the quotient overflows
    assert em.invert(1.0, [3e9, 4e9], [1, 2], 1.0) == -1             # above INT32_MAX
    assert em.invert(1.0, [2147483647.0, 4e9], [1, 2], 1.0) == 2147483647
    # a table whose first row is later than zero: the stretch before it is interpolated from time zero
    assert em.invert(0.5, [2.0, 3.0], [1, 2], 0.5) == 2 and em.invert(0.0, [2.0, 3.0], [1, 2], 0.5) == 0


def test_frames_of_beat_equals_the_model():
    from real_time_audio_sync_amd import ensemble
    tables = [(SYNTH_TIMES, SYNTH_BEATS, 0.25), (SYNTH_TIMES, [0, 1, 1, 3, 7, 8], 0.25), ([1e300, 2e300], [1, 3], 1e-300),
              ([2147483647.0, 4e9], [1, 2], 1.0)] + [read_table(p) + (FS,) for p in CSVS]
    checked = 0
    for times, beats, fs in tables:
        xs = [em.NAN, INF, -INF, -1.0, -1.0000001, -0.0, 0.0, 5.0, 6.0] + [float(v) for v in beats]
        xs += [beats[0] - 1 + k * (beats[-1] - beats[0] + 2) / 997.0 for k in range(998)]
        for x in xs:
            assert ensemble.frames_of_beat((times, beats), x, fs) == em.invert(x, times, beats, fs), (x, fs)
            checked += 1
    assert checked > 6000


# ---- (a) fuse_step ------------------------------------------------------------------------------------------------------

def step(betas, strikes=None, out=None, max_dev=INF, patience=1):
    s = [0] * len(betas) if strikes is None else strikes
    o = [0] * len(betas) if out is None else out
    return em.fuse_step(betas, s, o, max_dev, patience) + (s, o)


def test_fuse_single_member_and_counts():
    c, sp, n_in, n_valid, devs, s, o = step([3.25])
    assert (c, sp, n_in, n_valid, devs, s, o) == (3.25, 0.0, 1, 1, [0.0], [0], [0])
    c, sp, n_in, n_valid, devs, _, _ = step([5.0, 1.0, 3.0])                       # odd: the middle one
    assert (c, sp, n_in, n_valid, devs) == (3.0, 4.0, 3, 3, [2.0, -2.0, 0.0])
    c, sp, n_in, n_valid, devs, _, _ = step([5.0, 1.0, 3.0, 4.0])                  # even: the mean of the middle two
    assert (c, sp, n_in, n_valid, devs) == (3.5, 4.0, 4, 4, [1.5, -2.5, -0.5, 0.5])
    c, sp, n_in, n_valid, devs, _, _ = step([5.0, em.NAN, 1.0])                    # a member without a beat does not vote
    assert (c, sp, n_in, n_valid) == (3.0, 4.0, 2, 2) and bits(devs[1]) == bits(em.NAN) and devs[0] == 2.0


def test_fuse_signed_zeros_tie_and_the_index_decides():
    c, sp, _, _, devs, _, _ = step([0.0, -0.0, 1.0])                 # sorted: 0.0 (member 0), -0.0 (member 1), 1.0
    assert bits(c) == bits(-0.0) and sp == 1.0
    c, _, _, _, _, _, _ = step([-0.0, 0.0, 1.0])
    assert bits(c) == bits(0.0)
    c, sp, _, _, _, _, _ = step([0.0, -0.0])                         # (0.0 + -0.0) * 0.5 = +0.0;  spread -0.0 - 0.0 = -0.0
    assert bits(c) == bits(0.0) and bits(sp) == bits(-0.0 - 0.0)


def test_fuse_all_nan_changes_nothing():
    s, o = [2, 0, 3], [0, 0, 1]
    c, sp, n_in, n_valid, devs, s, o = step([em.NAN] * 3, s, o, 1.0, 3)
    assert bits(c) == bits(em.NAN) and bits(sp) == bits(em.NAN) and (n_in, n_valid) == (0, 0)
    assert all(bits(d) == bits(em.NAN) for d in devs) and s == [2, 0, 3] and o == [0, 0, 1]


def test_fuse_two_arbitrary_members_of_five_cannot_move_the_consensus_outside_the_others():
    import random
    rnd = random.Random(11)
    for _ in range(500):
        good = [rnd.uniform(90.0, 110.0) for _ in range(3)]
        wild = [rnd.choice([rnd.uniform(-1e6, 1e6), INF, -INF, 0.0]) for _ in range(2)]
        members = good + wild
        rnd.shuffle(members)
        c = step(members)[0]
        assert min(good) <= c <= max(good)


def test_fuse_out_after_patience_steps_and_back_after_one():
    s, o = [0, 0, 0], [0, 0, 0]
    for k in range(1, 6):
        c, _, n_in, _, devs, s, o = step([10.0, 10.5, 20.0], s, o, 2.0, 4)
        if k < 4:                                                    # still heard: the median of all three
            assert (c, n_in, s, o) == (10.5, 3, [0, 0, k], [0, 0, 0])
        elif k == 4:                                                 # the step that strikes it out still heard it
            assert (c, n_in, s, o) == (10.5, 3, [0, 0, 4], [0, 0, 1])
        else:                                                        # outvoted: the other two alone; strikes saturate
            assert (c, n_in, s, o) == (10.25, 2, [0, 0, 4], [0, 0, 1]) and devs[2] == 9.75
    for _ in range(7):                                               # strikes stay at patience however long it lasts
        s, o = step([10.0, 10.5, 20.0], s, o, 2.0, 4)[5:]
    assert s == [0, 0, 4] and o == [0, 0, 1]
    c, _, n_in, n_valid, devs, s, o = step([10.0, 10.5, 12.0], s, o, 2.0, 4)       # one step within max_dev: in again
    assert (c, n_in, n_valid, s, o) == (10.25, 2, 3, [0, 0, 0], [0, 0, 0]) and devs[2] == 1.75
    assert step([10.0, 10.5, 12.0], s, o, 2.0, 4)[:3] == (10.5, 2.0, 3)
    # fabs(dev) == max_dev is within it; patience 1 strikes out at once
    assert step([0.0, 0.0, 2.0], None, None, 2.0, 1)[6] == [0, 0, 0]
    assert step([0.0, 0.0, 2.5], None, None, 2.0, 1)[6] == [0, 0, 1]


def test_fuse_all_out_fallback_hears_everyone_valid():
    s, o = [3, 3, 0], [1, 1, 0]
    c, _, n_in, n_valid, _, s, o = step([4.0, 6.0, em.NAN], s, o, 0.5, 3)           # the only member that is in has no beat
    assert (c, n_in, n_valid) == (5.0, 2, 2)
    assert s == [3, 3, 0] and o == [1, 1, 0]                                       # both 1.0 away: still struck, saturated
    c, _, n_in, _, _, s, o = step([4.0, 4.25, em.NAN], s, o, 0.5, 3)
    assert (c, n_in, s, o) == (4.125, 2, [0, 0, 0], [0, 0, 0])


def test_curve_is_the_step_along_the_paths():
    times, beats = [1.0, 2.0, 3.0, 4.0], [1, 2, 3, 4]
    fs = 0.5
    paths = [[(0, 0), (1, 1), (2, 2), (3, 3)], [(1, 0), (1, 2), (3, 4)], [], [(0, -1), (2, 6)]]
    cons, spread, n_in, outs = em.curve(paths, [0, 0, 0, 0], [(times, beats)], [0] * 4, [0] * 4, 5, fs, INF, 1)
    look = lambda y: am.lookup(y, times, beats, fs)[0]               # noqa: E731
    # t = 0: member 0 at y 0 alone (member 1 starts at x = 1, member 3's y is negative)
    assert cons[0][0] == look(0) and n_in[0][0] == 1
    # t = 1: member 0 at y 1, member 1 at its last point with x <= 1: y 2
    assert cons[0][1] == (look(1) + look(2)) * 0.5 and n_in[0][1] == 2
    # t = 2: y 2, y 2 and member 3 at y 6
    assert cons[0][2] == look(2) and n_in[0][2] == 3 and spread[0][2] == look(6) - look(2)
    # t = 4: behind every path's end the last points hold
    assert cons[0][4] == sorted([look(3), look(4), look(6)])[1]
    assert outs == [[0] * 5] * 4


# ---- (c) refusals before any device call -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as ge
    ge.build()
    from real_time_audio_sync_amd import _native
    return _native


def test_abi_refusals_without_a_device(nat):
    x = ctypes.c_void_p(16)                                          # never dereferenced: every check comes before the launch
    err = lambda: nat.lib.rts_last_error().decode()                  # noqa: E731
    INVALID = -1
    h = ctypes.c_void_p()
    grp = (ctypes.c_int32 * 4)(0, 0, 1, -1)
    create = nat.lib.rts_ensemble_create
    assert create(4, grp, 2, 1.0, 1, None) == INVALID and "out" in err()
    assert create(4, None, 2, 1.0, 1, ctypes.byref(h)) == INVALID and "group_host" in err()
    assert create(0, grp, 2, 1.0, 1, ctypes.byref(h)) == INVALID and "B" in err()
    assert create(4, grp, 5, 1.0, 1, ctypes.byref(h)) == INVALID and "n_groups" in err()
    assert create(4, grp, 0, 1.0, 1, ctypes.byref(h)) == INVALID and "n_groups" in err()
    for bad in (0.0, -1.0, float("nan")):
        assert create(4, grp, 2, bad, 1, ctypes.byref(h)) == INVALID and "max_dev" in err()
    for bad in (0, -3, 65536):
        assert create(4, grp, 2, 1.0, bad, ctypes.byref(h)) == INVALID and "patience" in err()
    assert create(4, (ctypes.c_int32 * 4)(0, 2, 1, -1), 2, 1.0, 1, ctypes.byref(h)) == INVALID and "stream 1" in err()
    assert create(4, (ctypes.c_int32 * 4)(0, -2, 1, -1), 2, 1.0, 1, ctypes.byref(h)) == INVALID and "stream 1" in err()
    assert create(4, (ctypes.c_int32 * 4)(1, 1, 1, -1), 2, 1.0, 1, ctypes.byref(h)) == INVALID and "group 0" in err()
    assert not h.value
    assert nat.lib.rts_ensemble_destroy(None) == 0
    assert nat.lib.rts_ensemble_reset(None, None, None) == INVALID and "NULL" in err()
    assert nat.lib.rts_annot_frames(None, x, 4, None, x, 1, x, None) == INVALID and "handle" in err()
    for name in ("rts_otw_consensus", "rts_wtw_consensus"):
        assert getattr(nat.lib, name)(None, x, x, x, None, x, x, x, x, None) == INVALID and "handle" in err()
    assert nat.lib.rts_path_consensus(None, x, x, 4, x, x, None, 4, x, None, None, None, None) == INVALID and "e is NULL" in err()
    assert nat.lib.rts_live_follow_consensus(None, x) == INVALID and "NULL" in err()
    assert nat.lib.rts_live_consensus(None, None, None, None, None, None, None, None, None) == INVALID and "NULL" in err()


# ---- (d) csrc/ensemble_plan.h under the sanitizers -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "ensemble_plan_driver")
    rc, out, err = _run(["g++", "-std=c++17"] + FLAGS + [os.path.join(SAN, "ensemble_plan_driver.cpp"), "-o", exe], timeout=300)
    assert rc == 0, err[-3000:]
    return exe


def run_driver(driver, tmp_path, tables=(), pieces=()):
    text = "%d %d\n" % (len(tables), len(pieces))
    for B, G, max_dev, patience, group in tables:
        text += "%d %d %s %d\n%s\n" % (B, G, max_dev, patience, " ".join(str(g) for g in group))
    for beats in pieces:
        text += "%d\n%s\n" % (len(beats), " ".join(str(b) for b in beats))
    case = tmp_path / "case.txt"
    case.write_text(text)
    rc, out, err = _run([driver, str(case)], env=ENV, timeout=120)
    _clean_report(err)
    assert rc == 0, (rc, out[-1000:], err[-2000:])
    lines = out.splitlines()
    assert len(lines) == len(tables) + len(pieces)
    return lines


OK, BATCH, GROUPS, MAXDEV, PATIENCE, ENTRY, EMPTY, LARGE = range(8)      # EnsembleRefusal


def test_plan_every_refusal(driver, tmp_path):
    good = [0, 1, 0, -1]
    tables = [(0, 1, "1.0", 1, []), (-2, 1, "1.0", 1, []),                                   # B
              (4, 0, "1.0", 1, good), (4, 5, "1.0", 1, good), (4, -1, "1.0", 1, good),        # n_groups
              (4, 2, "0", 1, good), (4, 2, "-1.5", 1, good), (4, 2, "nan", 1, good), (4, 2, "-inf", 1, good),   # max_dev
              (4, 2, "1.0", 0, good), (4, 2, "1.0", -1, good), (4, 2, "1.0", 65536, good),    # patience
              (4, 2, "1.0", 1, [0, 1, 2, -1]), (4, 2, "1.0", 1, [0, 1, 0, -2]),               # an entry out of range
              (4, 3, "1.0", 1, [0, 2, 0, -1]), (4, 2, "1.0", 1, [1, 1, 1, 1]),                # an empty group
              (4, 2, "inf", 65535, good), (4, 2, "1e-300", 1, good)]                          # the edges that pass
    got = [l.split() for l in run_driver(driver, tmp_path, tables=tables)]
    why = [int(l[1]) for l in got]
    assert why == [BATCH] * 2 + [GROUPS] * 3 + [MAXDEV] * 4 + [PATIENCE] * 3 + [ENTRY] * 2 + [EMPTY] * 2 + [OK] * 2
    assert got[12][2:5] == ["2", "2", "0"] and got[13][2:5] == ["3", "-2", "0"]               # stream and entry are named
    assert got[14][2:5] == ["-1", "1", "0"] and got[15][2:5] == ["-1", "0", "0"]              # the first empty group
    for l, word in zip(got[:16], ["B"] * 2 + ["n_groups"] * 3 + ["max_dev"] * 4 + ["patience"] * 3 + ["stream"] * 2 + ["member"] * 2):
        assert word in " ".join(l[l.index("|"):]), l


def test_plan_csr_of_an_interleaved_table(driver, tmp_path):
    group = [2, 0, -1, 1, 0, 2, 2, -1, 0, 1, -1]
    line = run_driver(driver, tmp_path, tables=[(11, 3, "2.0", 4, group)])[0].split()
    assert line[:10] == ["table", "0", "grouped", "8", "loose", "3", "waves", "4", "grid", "1"]
    first = [int(v) for v in line[line.index("first") + 1:line.index("members")]]
    members = [int(v) for v in line[line.index("members") + 1:]]
    assert first == [0, 3, 5, 8]
    assert members == [1, 4, 8, 3, 9, 0, 5, 6, 2, 7, 10]             # ascending inside every group, then the streams in none


def test_plan_groups_of_64_and_65(driver, tmp_path):
    g64 = [0] * 64 + [1]
    g65 = [0] * 65 + [1]
    mixed = [b % 2 for b in range(128)] + [-1] * 130                  # two groups of 64, interleaved; 130 streams in none
    lines = run_driver(driver, tmp_path, tables=[(65, 2, "1.0", 1, g64), (66, 2, "1.0", 1, g65), (258, 2, "1.0", 1, mixed)])
    a, b, c = (l.split() for l in lines)
    assert a[:10] == ["table", "0", "grouped", "65", "loose", "0", "waves", "2", "grid", "1"]
    assert [int(v) for v in a[a.index("members") + 1:]] == list(range(65))
    assert b[:5] == ["table", str(LARGE), "-1", "0", "65"] and "65 members" in " ".join(b)
    assert c[:10] == ["table", "0", "grouped", "128", "loose", "130", "waves", "5", "grid", "2"]   # 2 + ceil(130 / 64) waves
    members = [int(v) for v in c[c.index("members") + 1:]]
    assert members == list(range(0, 128, 2)) + list(range(1, 128, 2)) + list(range(128, 258))


def test_plan_invertible_flag(driver, tmp_path):
    pieces = [[0], [5], [0, 1, 2, 3], [0, 1, 1, 3], [0, 2, 1], [3, 2], [0, 1, 5, 6, 2147483647], SYNTH_BEATS] \
        + [read_table(p)[1] for p in CSVS]
    lines = run_driver(driver, tmp_path, pieces=pieces)
    assert [l.split() for l in lines] == [["piece", str(int(em.invertible(p)))] for p in pieces]
    assert [l.split()[1] for l in lines] == ["1", "1", "1", "0", "0", "0", "1", "1", "1", "1"]
