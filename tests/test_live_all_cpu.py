"""What the script of tests/live_all_model.py reaches, from the oracle and the models alone: tests/test_live_all_gpu.py
claims to cover a stream paused by the gate over several feeds, a tracker that has stopped while the others run, feeds
that bring nothing, the diff-mode feed whose only chroma column becomes a carry, a member of a consensus group that goes
out and is heard again, and a restart whose offset shows in the beat.  These are conditions on the inputs: if one fails,
the input (seeds, silence placement, cut sizes) changes, not the condition.  Each case prints what it found on an
OBSERVED line."""
import numpy as np
import pytest

import annot_model as am
import live_all_model as lam


def runs(flags):
    """Maximal runs of true entries -> [(first index, length)]."""
    out, start = [], None
    for i, f in enumerate(list(flags) + [False]):
        if f and start is None:
            start = i
        if not f and start is not None:
            out.append((start, i - start))
            start = None
    return out


@pytest.fixture(scope="module")
def sims():
    """Every case run to just before its reset(), with the published out / strikes words after every feed."""
    out = {}
    for cid in lam.CASES:
        case = lam.build_case(cid)
        sim = lam.Sim(case)
        hist = dict(out=[], strikes=[], restarts=[], offset_beat=None)
        pos, i = [0] * case.B, 0
        for ev in case.script[:-1]:
            if ev[0] == "feed":
                sim.feed(lam.cut(case, pos, ev[1]))
                hist["out"].append(list(sim.model.out_pub))
                hist["strikes"].append(list(sim.model.strikes_pub))
                b = lam.S_RESTART
                p = sim.trk[b].path
                if i > lam.F_RESTART and hist["offset_beat"] is None and len(p):   # the restarted stream's first beat
                    t = case.tables[sim.model.piece[b]]
                    hist["offset_beat"] = (sim.model.sticky[b].beat, am.lookup(int(p[-1][1]), t[0], t[1], lam.FRAME_SECONDS, 0)[0])
                i += 1
            else:
                if ev[0] == "restart":
                    carried = (sim.model.strikes[ev[1]], sim.model.out[ev[1]])
                sim.apply(ev)
                if ev[0] == "restart":                          # (strikes, out) the ensemble carried before and after
                    hist["restarts"].append((ev[1], sim.model.ens_on, carried, (sim.model.strikes[ev[1]], sim.model.out[ev[1]])))
        assert i == lam.N_FEEDS
        out[cid] = (case, sim, hist)
    return out


@pytest.mark.parametrize("cid", list(lam.CASES))
def test_the_script_reaches_the_states_the_gpu_test_covers(sims, cid):
    case, sim, hist = sims[cid]
    log = sim.log
    B, F = case.B, lam.N_FEEDS
    # the gate: paused over >= 3 consecutive feeds and open again; a silence longer than hold; a rest within hold, kept
    paused = {}
    for b in range(B):
        for first, n in runs([r[b][0] > 0 and r[b][1] == 0 and not r[b][2] for r in log]):
            if n >= 3 and any(r[b][1] > 0 for r in log[first + n:]):
                paused[b] = (first, n)
    assert paused, "no stream is paused by the gate for three feeds and opens again"
    kept_rest = cut_silence = None
    for b in (lam.S_SILENT, lam.S_REST):                        # (neither is restarted: their gate models hold the whole run)
        g = sim.gates[b]
        for lv in g.levels:
            assert not (lam.MIN_LEVEL * (1 - 1e-6) <= lv <= lam.MIN_LEVEL * (1 + 1e-6)), (b, lv)   # no decision hangs on rounding
        for first, n in runs([lv < lam.MIN_LEVEL for lv in g.levels]):
            if first == 0 or first + n == len(g.levels):
                continue
            if n <= lam.HOLD and all(g.passes[first:first + n]):
                kept_rest = (b, first, n)
            if n > lam.HOLD:
                assert g.passes[first:first + n] == [True] * lam.HOLD + [False] * (n - lam.HOLD), (b, first)
                cut_silence = (b, first, n)
    assert kept_rest and cut_silence, (kept_rest, cut_silence)
    # a tracker at the end of its reference >= 3 feeds before the end, the others still running
    stopped_at = {b: min(i for i in range(F) if log[i][b][3]) for b in range(B) if log[-1][b][3]}
    early = {b: i for b, i in stopped_at.items() if i <= F - 4 and not any(log[i][o][3] for o in range(B) if o != b)}
    assert early, stopped_at
    # feeds that bring nothing, and a feed with a count of 0 next to a count of 1
    nothing = [i for i in range(F) if all(r[0] == 0 for r in log[i])]
    zero_one = [i for i in range(F) if any(r[1] == 0 for r in log[i]) and any(r[1] == 1 for r in log[i])]
    assert nothing and zero_one
    assert log[lam.F_NOTHING] == [(0, 0, r[2], r[3], 0) for r in log[lam.F_NOTHING]]
    carry_only = [i for i in range(F) if max(r[0] for r in log[i]) > 0 and max(r[4] for r in log[i]) == 0]
    if case.diff:                                               # n_max > 0 and n_max_diff == 0: rows n_max apart, no push
        assert carry_only == [lam.F_RESTART], carry_only
        assert [r[0] for r in log[lam.F_RESTART]] == [1 if b == lam.S_RESTART else 0 for b in range(B)]
    else:
        assert not carry_only
    # a member out for >= 2 feeds and heard again without a restart in between
    heard = {}
    restarts = {lam.S_RESTART: lam.F_RESTART, lam.S_LATE: lam.F_UNBOUND}
    if case.kind == "otw":
        restarts[lam.S_REACQ] = lam.F_REACQ
    for b in range(B):
        for first, n in runs([o[b] == 1 for o in hist["out"]]):
            back = first + n
            if n >= 2 and back < F and not first < restarts.get(b, -1) <= back and hist["strikes"][back][b] == 0:
                heard.setdefault(b, (first, n))
    assert heard, hist["out"]
    # the scripted restart: its offset shows in the beat, and it clears strikes that were there (live_restart_kernel's
    # ens_state line has something to clear); the restart while consensus is off finds strikes too, and they stay
    with_offset, without = hist["offset_beat"]
    assert with_offset is not None and without is not None and with_offset != without, hist["offset_beat"]
    (b0, on0, before0, after0), (b1, on1, before1, after1) = hist["restarts"]
    assert (b0, on0, after0) == (lam.S_RESTART, True, (0, 0)) and before0[0] > 0, hist["restarts"]
    assert (b1, on1) == (lam.S_LATE, False) and before1 == after1 and before1[0] > 0, hist["restarts"]
    if case.kind == "otw":                                      # the scripted reacquire finds a place and moves the stream
        assert sim.direct[lam.S_REACQ] == lam.M_EXCERPT
    print("OBSERVED live_all %s: paused (stream: first feed, feeds) %s; kept rest %s, cut silence %s (stream, first column, "
          "columns); stopped at feed %s; no column in feeds %s; 0 next to 1 in feeds %s; carry-only feeds %s; out and heard "
          "again (stream: first feed, feeds) %s; restarts (stream, consensus on, strikes/out before, after) %s; beat with / "
          "without the offset %s"
          % (cid, paused, kept_rest, cut_silence, stopped_at, nothing, zero_one, carry_only, heard, hist["restarts"],
             hist["offset_beat"]))


def test_composed_restart_and_switches():
    """The composition's own rules, on made-up paths: a restart clears one stream's words and carried strikes, a switched-off
    publisher keeps its words, consensus waits for annotations, and a restart while consensus is off leaves the unbound
    ensemble's state alone."""
    case = lam.build_case("wtw")                                # no watch: the words need no history
    m = lam.Composed(case)
    paths = [[(t, t + 3 * b) for t in range(20)] for b in range(case.B)]
    m.feed(paths)
    first = (m.beats(), m.tempo_words(), m.consensus())
    assert np.isfinite(first[0]["beat"]).all() and np.isfinite(first[1]["bpm"]).all() and np.isfinite(first[2]["consensus"]).all()
    m.feed(paths)
    assert any(m.strikes) and m.consensus()["strikes"].tolist() == [s if g >= 0 else 0 for s, g in zip(m.strikes, case.groups)]
    b = next(b for b in range(case.B) if m.strikes[b])
    m.restart(b)
    assert np.isnan(m.beats()["beat"][b]) and m.beats()["ref_frame"][b] == -1 and m.tempo_words()["n"][b] == 0
    assert m.strikes[b] == 0 and np.isnan(m.consensus()["dev"][b]) and m.consensus()["consensus"].tolist() == first[2]["consensus"].tolist()
    m.annotate(False)
    kept = (m.beats(), m.consensus())
    longer = [p + [(20, p[-1][1] + 9)] for p in paths]
    m.feed(longer)
    assert m.beats()["beat"].tobytes() == kept[0]["beat"].tobytes() and m.consensus()["dev"].tobytes() == kept[1]["dev"].tobytes()
    assert np.isnan(m.tempo_words()["bpm"]).all() and np.isfinite(m.tempo_words()["slope"]).all()
    m.annotate(True)
    m.follow_consensus(False)
    other = next(o for o in range(case.B) if m.strikes[o])
    carried = m.strikes[other]
    m.restart(other)
    assert m.strikes[other] == carried and m.consensus()["strikes"][other] == 0
    m.follow_tempo(False)
    kept = m.tempo_words()
    m.feed(longer)
    assert m.tempo_words()["slope"].tobytes() == kept["slope"].tobytes() and m.beats()["ref_frame"][0] == longer[0][-1][1]
    m.reset()
    assert np.isnan(m.beats()["beat"]).all() and np.isnan(m.consensus()["consensus"]).all() and m.strikes[other] == carried
