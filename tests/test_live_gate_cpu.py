"""The level gate of the live chain without a GPU: the three new symbols of the ABI, tests/live_gate_model.py against a
closed-form restatement of the decision, and the inputs tests/test_live_gate_gpu.py runs, checked on the model alone.

The inputs are the schedules and the synth audio of tests/test_live_model_cpu.py (build_schedule, synth), multiplied per
stream, before the PCM rounding, by an envelope of gains 1, 2^-10 and exactly 0.  The envelope is laid out by columns: a
first pass runs the ungated loop model over the schedule (framing does not depend on the gate), which gives every
column's feed and first sample; a run of quiet columns [a, a + k) then is gain 2^-10 on the samples from column a's first
to column a + k - 1's last.  Where hop < fft_len the neighbours of such a run hold some quiet samples and stay loud: the
threshold (-70 dB) lies 2^-20 * (loud power) * ~2 above the quiet columns and well below one loud hop -- the tests below
assert what came out, not what was meant.  Stream roles: 0 always loud, 3 digital zeros, 1 a short lead-in and gaps of
exactly hold + 1 (inside the feed that completes cols_cap columns) and hold columns, 2 a closed first column, 5 a long
lead-in and a long gap with one NaN sample deep inside it, 4 a gap with a restart in it (3 is restarted with it)."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest

from live_gate_model import GateStreamModel, decide, frame_level
from test_chroma_paths_gpu import synth  # noqa: E402
from test_live_model_cpu import (B, FS, OTW_GEOMETRIES, build_schedule, max_pending, otw_ref, otw_step_kinds,  # noqa: E402
                                 run_wtw_oracle, wtw_refs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GATE_GEOMETRIES = [(512, 128), (64, 1), (256, 1000), (4096, 441)]
HOLDS = (0, 3)
MIN_DB = -70.0
MIN_LEVEL = 10.0 ** (MIN_DB / 10.0)
QUIET = 2.0 ** -10
S_LOUD, S_EDGE, S_FIRST, S_ZERO, S_RESTART, S_LEAD = 0, 1, 2, 3, 4, 5
RESTART_STREAMS = (S_RESTART, S_ZERO)
RESTART_AT = 49                  # index into the schedule: the restart comes before this feed
CASES = [(L, hop, hold, "float32") for L, hop in GATE_GEOMETRIES for hold in HOLDS] + \
        [(512, 128, hold, "int16") for hold in HOLDS]


# ---- ABI ------------------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = {"rts_live_gate": 3, "rts_live_levels": 6, "rts_live_gate_columns": 6}


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as ge
    ge.build()
    from real_time_audio_sync_amd import _native
    return _native


def test_symbols_are_exported_and_declared(nat):
    txt = open(os.path.join(ROOT, "include", "rtsync.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = ctypes.CDLL(nat.SO_PATH)
    for name, n_args in NEW_SYMBOLS.items():
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, "include/rtsync.h does not declare %s" % name
        assert len(m.group(1).split(",")) == n_args, (name, m.group(1))
        assert name in nat.EXPORTS and len(nat.EXPORTS[name].argtypes) == n_args, name
    assert nat.EXPORTS["rts_live_gate"].argtypes[1] is ctypes.c_double


def test_null_handle_is_refused_with_a_message(nat):
    n = ctypes.c_int()
    for rc in (nat.lib.rts_live_gate(None, 1e-6, 0),
               nat.lib.rts_live_levels(None, None, None, None, None, ctypes.byref(n)),
               nat.lib.rts_live_gate_columns(None, 0, None, 0, ctypes.byref(n), None)):
        assert rc == -1 and nat.lib.rts_last_error()
    with pytest.raises(nat.RtsyncError):
        nat.check(nat.lib.rts_live_gate(None, 0.0, 0))


# ---- the model against a closed form ------------------------------------------------------------------------------------------

def passes_closed_form(loud, hold):
    """A column passes iff one of the `hold` + 1 columns ending with it is loud (a fresh stream has heard none)."""
    return [any(loud[max(0, i - hold):i + 1]) for i in range(len(loud))]


def gap(n):
    return [1e-9] * n


@pytest.mark.parametrize("hold", HOLDS)
def test_decide_equals_the_closed_form(hold):
    loud, nan = [1e-2], [float("nan")]
    seqs = {
        "gaps": loud * 3 + gap(hold) + loud * 2 + gap(hold + 1) + loud + gap(3 * hold + 2) + loud * 2,
        "lead-in": gap(7) + loud * 4 + gap(2),
        "all quiet": gap(12),
        "nan": loud * 2 + nan + loud + nan * (hold + 2) + loud,
        "at the threshold": [MIN_LEVEL, math.nextafter(MIN_LEVEL, 0.0), MIN_LEVEL] + gap(hold + 1),
    }
    for name, levels in seqs.items():
        flags = [lv >= MIN_LEVEL for lv in levels]
        want = passes_closed_form(flags, hold)
        got, q = decide(levels, MIN_LEVEL, hold, hold + 1)
        assert got == want, name
        # cut anywhere into two feeds: q carries the decision across
        for cut in range(len(levels) + 1):
            a, qa = decide(levels[:cut], MIN_LEVEL, hold, hold + 1)
            b, qb = decide(levels[cut:], MIN_LEVEL, hold, qa)
            assert a + b == want and qb == q, (name, cut)
    got, _ = decide(seqs["gaps"], MIN_LEVEL, hold, hold + 1)
    assert got.count(False) == 1 + (2 * hold + 2)           # one column of the hold + 1 gap, all but `hold` of the long one
    assert not any(decide(seqs["all quiet"], MIN_LEVEL, hold, hold + 1)[0])
    assert decide(seqs["lead-in"], MIN_LEVEL, hold, hold + 1)[0] == [False] * 7 + [True] * 4 + [hold >= 1, hold >= 2]
    nan_pass = decide(seqs["nan"], MIN_LEVEL, hold, hold + 1)[0]
    assert nan_pass[2] == (hold >= 1) and nan_pass[4 + hold:4 + hold + 2] == [False, False] and nan_pass[-1]


def test_stream_model_levels_ordinals_diff_rule_and_restart():
    L, hop, hold = 8, 4, 1
    rs = np.random.RandomState(3)
    x = rs.standard_normal(8 + 4 * 15).astype(np.float32)
    quiet_cols = {0, 1, 5, 6, 7, 11}
    for m in range(16):
        if m in quiet_cols:
            x[m * hop:m * hop + L] = 0
    # columns next to a zeroed one keep half their samples: loud.  So quiet = fully zeroed frames only
    quiet = [not x[m * hop:m * hop + L].any() for m in range(16)]
    for diff in (False, True):
        g = GateStreamModel(L, hop, 1e-6, hold, diff=diff)
        for a in range(0, len(x), 7):
            g.feed(x[a:a + 7])
        assert g.seen == 16 and g.levels[3] == math.fsum(float(v) * float(v) for v in x[12:20]) / L
        passes = passes_closed_form([not z for z in quiet], hold)
        assert g.passes == passes and sum(n for n, _ in g.per_feed) == 16
        want = [m for m in range(16) if passes[m] and (not diff or (m > 0 and passes[m - 1]))]
        assert g.ordinals == want == sum((h for _, h in g.per_feed), []) and g.passed == len(want)
        assert g.open == passes[-1] and g.level == g.levels[-1]
        g.restart()
        assert (g.seen, g.passed, g.open, g.q) == (0, 0, False, hold + 1) and math.isnan(g.level)
        g.feed(x[2 * hop:2 * hop + L + hop])                     # two loud columns straight away
        assert g.passes == [True, True] and g.ordinals == ([1] if diff else [0, 1])
    g = GateStreamModel(L, hop, 1e-6, 0)
    bad = x[2 * hop:2 * hop + L].copy()
    bad[3] = np.nan
    g.feed(bad)
    assert math.isnan(g.level) and g.passes == [False] and math.isnan(frame_level(bad))


# ---- the cases of the GPU tests ---------------------------------------------------------------------------------------------

class Case(object):
    pass


def _first_pass(L, hop, feeds):
    """Every stream's columns under the ungated loop: [(feed index, first sample among all samples fed)], the restart
    included; and the samples fed before the restart."""
    from oracle.chroma_oracle import LiveLoopModel
    models = [LiveLoopModel(L, hop) for _ in range(B)]
    cols = [[] for _ in range(B)]
    since, pos, fed_at_restart = [0] * B, [0] * B, None
    for i, f in enumerate(feeds):
        if i == RESTART_AT:
            fed_at_restart = list(pos)
            for b in RESTART_STREAMS:
                models[b].restart()
                since[b] = pos[b]
        if f["refused"]:
            continue
        for b in range(B):
            k0 = len(models[b].slices)
            models[b].feed([0.0] * f["counts"][b])
            pos[b] += f["counts"][b]
            cols[b] += [(i, since[b] + s) for s in models[b].starts[k0:]]
    return cols, fed_at_restart, pos


def _envelope(L, hop, hold, feeds, base):
    """Gains per stream [B][samples fed], and where the NaN sample of the float32 runs goes (stream, sample).  ``base``:
    the streams' audio before the envelope, looked at only to keep a gap's ends where its neighbours stay loud."""
    cols, fed_at_restart, fed = _first_pass(L, hop, feeds)
    gain = [np.ones(fed[b] + 1) for b in range(B)]
    r = -(-L // hop)                                  # frames that hold one sample

    def quiet(b, a, k):                               # columns [a, a + k) of stream b
        gain[b][cols[b][a][1]:cols[b][a + k - 1][1] + L] = QUIET

    def place(b, a, k):
        """A run of exactly k quiet columns at a, or a little later: where hop < fft_len the columns next to it keep only
        the samples one hop brings (at hop = 1 a single one), which must carry 100 thresholds by themselves."""
        for a in range(a, a + 40):
            lo, hi = cols[b][a][1], cols[b][a + k - 1][1] + L
            edges = [base[b][cols[b][a - 1][1]:lo], base[b][hi:cols[b][a + k][1] + L]]
            if all(float((e * e).sum()) >= 100 * MIN_LEVEL * L for e in edges):
                quiet(b, a, k)
                return a
        raise AssertionError("no place for a gap of %d columns" % k)

    gain[S_ZERO][:] = 0.0
    # stream 1: closed first two columns; in the feed that completes cols_cap columns loud, hold + 1 quiet, loud; later a
    # gap of exactly `hold`
    quiet(S_EDGE, 0, 2)
    cols_cap = (max_pending(L, hop) - L) // hop + 1
    per_feed = {}
    for i, _ in cols[S_EDGE]:
        per_feed[i] = per_feed.get(i, 0) + 1
    full = [i for i, n in per_feed.items() if n == cols_cap][0]
    f0 = [k for k, (i, _) in enumerate(cols[S_EDGE]) if i == full][0]
    at = place(S_EDGE, f0 + 1, hold + 1)
    assert at + hold + 1 < f0 + cols_cap
    if hold:
        place(S_EDGE, f0 + cols_cap + 2 * r + 2, hold)
    # stream 2: its first column is closed
    quiet(S_FIRST, 0, 1)
    # stream 5: the first quarter is a lead-in; a gap that ends two columns before the stream does, of at least
    # hold + r + 3 columns and with three feeds wholly in its dropped part; the NaN is the first sample of its column
    # hold + r (the frames that hold it are columns hold + 1 .. hold + r of the gap)
    k5 = len(cols[S_LEAD])
    quiet(S_LEAD, 0, k5 // 4)
    by_feed = {}
    for idx, (i, _) in enumerate(cols[S_LEAD]):
        by_feed.setdefault(i, []).append(idx)
    k = max(hold + r + 3, 3 * hold + 2)
    while sum(1 for v in by_feed.values() if v[0] >= k5 - 2 - k + hold and v[-1] < k5 - 2) < 3:
        k += 1
    a = k5 - 2 - k
    assert a >= k5 // 4 + r + 2
    quiet(S_LEAD, a, k)
    nan_at = (S_LEAD, cols[S_LEAD][a + hold + r][1])
    # stream 4: quiet from hold + 2 columns before the restart to the second column after it
    before = [k for k, (i, _) in enumerate(cols[S_RESTART]) if i < RESTART_AT]
    gain[S_RESTART][cols[S_RESTART][before[-(hold + 2)]][1]:cols[S_RESTART][len(before) + 1][1] + L] = QUIET
    return gain, nan_at


@functools.lru_cache(maxsize=None)
def build_gate_case(L, hop, hold, dtype="float32", diff=False):
    """Schedule, audio and the gate models run through the whole schedule."""
    from oracle import chroma_oracle as co
    c = Case()
    c.L, c.hop, c.hold, c.cap = L, hop, hold, max_pending(L, hop)
    c.cols_cap = (c.cap - L) // hop + 1
    c.feeds = build_schedule(L, hop, seed=7 * L + hop)
    c.restart_at = RESTART_AT
    totals = [sum(f["counts"][b] for f in c.feeds if not f["refused"]) for b in range(B)]
    base = [synth(totals[b] + 1, max(hop, 16), 1000 * b + L + hop).astype(np.float64) for b in range(B)]
    gain, c.nan_at = _envelope(L, hop, hold, c.feeds, base)
    c.pcm, c.live = [], []
    for b in range(B):
        x = base[b] * gain[b]
        c.pcm.append(np.round(x * 32768.0).astype(np.int16))
        c.live.append(c.pcm[b].astype(np.float32) / np.float32(32768.0))
    if dtype == "float32":
        c.live[c.nan_at[0]][c.nan_at[1]] = np.nan
    else:
        c.nan_at = None
    c.models = [GateStreamModel(L, hop, MIN_LEVEL, hold, diff) for _ in range(B)]
    c.pending, c.since, pos = [], [0] * B, [0] * B
    c.all_levels = [[] for _ in range(B)]       # of every column, the runs before the restart included
    c.feed_log = []                             # per feed: [B] (columns completed, columns handed on)
    c.at_restart = None
    c.run_slices = [[m.loop.slices] for m in c.models]   # [b][run] the frames of every chroma column, by ordinal
    c.feed_handed = []                          # per feed: [B] (run, ordinals handed on)
    c.snap = []                                 # after every entry of the schedule: [B] (seen, passed, open, level)
    for i, f in enumerate(c.feeds):
        if i == c.restart_at:
            c.at_restart = [(m.q, m.seen, m.passed, list(m.passes)) for m in c.models]
            c.ordinals_at_restart = [list(m.ordinals) for m in c.models]
            for b in RESTART_STREAMS:
                c.all_levels[b] += c.models[b].levels
                c.models[b].restart()
                c.run_slices[b].append(c.models[b].loop.slices)
                c.since[b] = pos[b]
        if not f["refused"]:
            for b in range(B):
                n = f["counts"][b]
                c.models[b].feed(c.live[b][pos[b]:pos[b] + n])
                pos[b] += n
            c.feed_log.append([(m.per_feed[-1][0], len(m.per_feed[-1][1])) for m in c.models])
            c.feed_handed.append([(len(c.run_slices[b]) - 1, list(c.models[b].per_feed[-1][1])) for b in range(B)])
        c.snap.append([(m.seen, m.passed, m.open, m.level) for m in c.models])
        c.pending.append([len(m.loop.buf) for m in c.models])
    for b in range(B):
        c.all_levels[b] += c.models[b].levels
    c.fed = pos
    c.n_cols = [m.seen for m in c.models]       # chroma columns of the current run (sizes the trackers, as ungated)
    c.kept = [list(m.ordinals) for m in c.models]
    # oracle chroma of every column of the current run
    c.oracle_all = [co.live_loop_columns(m.loop.slices, L, FS) if m.loop.slices else np.zeros((0, 12)) for m in c.models]
    return c


def kept_oracle_columns(c, b):
    """What the oracle hands stream b's tracker: the kept chroma columns."""
    return c.oracle_all[b][c.kept[b]] if c.kept[b] else np.zeros((0, 12))


def runs(flags):
    """Lengths of the maximal runs of False between two True."""
    out, n, seen_true = [], 0, False
    for f in flags:
        if f:
            if seen_true and n:
                out.append(n)
            n, seen_true = 0, True
        else:
            n += 1
    return out


@pytest.mark.parametrize("L,hop,hold,dtype", CASES)
def test_no_level_lies_at_the_threshold(L, hop, hold, dtype):
    c = build_gate_case(L, hop, hold, dtype)
    n = 0
    for b in range(B):
        for lv in c.all_levels[b]:
            n += 1
            assert math.isnan(lv) or not (MIN_LEVEL * (1 - 1e-9) <= lv <= MIN_LEVEL * (1 + 1e-9)), (b, lv)
    assert n == sum(len(x) for x in c.all_levels) > 100


@pytest.mark.parametrize("L,hop,hold,dtype", CASES)
def test_schedule_contains_every_gate_case(L, hop, hold, dtype):
    c = build_gate_case(L, hop, hold, dtype)
    m = c.models
    loud = [[lv >= MIN_LEVEL for lv in c.all_levels[b]] for b in range(B)]
    # always loud / never opens (exact zeros)
    assert all(loud[S_LOUD]) and len(loud[S_LOUD]) > 10
    assert m[S_LOUD].ordinals == list(range(m[S_LOUD].seen))
    assert not any(c.all_levels[S_ZERO]) and len(c.all_levels[S_ZERO]) > 10 and m[S_ZERO].passed == 0
    assert c.at_restart[S_ZERO][2] == 0
    # a quiet lead-in (not zeros), then music
    lead = loud[S_LEAD].index(True)
    assert lead >= 3 and all(0 < lv < MIN_LEVEL for lv in c.all_levels[S_LEAD][:lead]) and m[S_LEAD].ordinals[0] == lead
    # gaps of exactly hold, hold + 1 and more columns
    gaps = sum((runs(loud[b]) for b in range(B)), [])
    assert hold + 1 in gaps and max(gaps) >= 3 * hold + 2 and (hold == 0 or hold in gaps), gaps
    # a feed in which one stream completes >= 3 columns with a pass / drop / pass pattern
    found = False
    for b in range(B):
        k = 0
        mm = m[b]
        for n, handed in mm.per_feed:
            flags = [(k + i) in handed for i in range(n)]
            k += n
            s = "".join("p" if x else "d" for x in flags)
            found = found or (n >= 3 and re.search("pd+p", s) is not None)
    assert found
    # a feed that completes columns and hands none on for any stream
    assert any(sum(n for n, _ in row) > 0 and sum(h for _, h in row) == 0 for row in c.feed_log)
    # a gap that spans at least 3 feeds (feeds in which the stream completes dropped columns only, in a row, with a
    # passing column before and after)
    spans = 0
    for b in (S_LEAD, S_RESTART):
        run = best = 0
        opened = False
        for n, handed in m[b].per_feed:
            if n == 0:
                continue
            if handed:
                opened, run = True, 0
            elif opened:
                run += 1
                best = max(best, run)
        spans = max(spans, best)
    assert spans >= 3
    # the restart falls inside a gap: the stream was closed (q > hold) and stays closed for its first columns afterwards
    q, seen, passed, passes = c.at_restart[S_RESTART]
    assert q == hold + 1 and seen > passed > 0 and not passes[-1]
    assert m[S_RESTART].passes[:2] == [False, False] and any(m[S_RESTART].passes) and m[S_RESTART].ordinals[0] >= 2
    # one NaN sample, float32 only; every frame that holds it is dropped
    if dtype == "float32":
        b, at = c.nan_at
        assert np.isnan(c.live[b]).sum() == 1 and np.isnan(c.live[b][at])
        bad = [k for k, lv in enumerate(m[b].levels) if math.isnan(lv)]
        assert len(bad) == (-(-L // hop) if hop <= L else 1) and not set(bad) & set(m[b].ordinals)
        assert not np.isnan(kept_oracle_columns(c, b)).any() and np.isnan(c.oracle_all[b][bad]).any(axis=1).all()
    else:
        assert not any(np.isnan(x).any() for x in c.live)
    assert 50 <= len(c.feed_log) <= 400


@pytest.mark.parametrize("L,hop,hold,dtype", CASES)
def test_trackers_stay_running_on_the_kept_columns(L, hop, hold, dtype):
    import oracle
    c = build_gate_case(L, hop, hold, dtype)
    ref = wtw_refs(c)
    windows = 0
    for b in range(B):
        log = [(0, len(h), 0) for _, h in c.models[b].per_feed]
        o = run_wtw_oracle(ref, log, kept_oracle_columns(c, b))
        assert o.state["status"] == oracle.RUNNING and o.state["chroma_ptr"] == len(c.kept[b]) <= 2 * ref.shape[1]
        windows += o.counters["windows"]
    assert windows > B - 1
    if (L, hop) in OTW_GEOMETRIES:
        kinds, o = otw_step_kinds(otw_ref(c), kept_oracle_columns(c, S_LOUD))
        assert kinds == {"row", "column", "both"}, kinds
