"""Digital silence (all-zero chroma columns), the CPU half: what the inputs of tests/silence_inputs.py do to the trackers
is pinned here from the oracle alone, and the oracle is held to what the reference's own code gave on such inputs
(tests/golden/silence_golden.npz, made by tests/golden/make_silence_golden.py).

The census constants are pinned the way HIT_IF_COUNTS is: a later change of synth.py or of the inputs that removed the
ties or the NaN windows fails here, on the CPU, instead of quietly emptying the GPU modules that rely on them
(test_otw_ties_gpu.py, test_wtw_silence_gpu.py)."""
import hashlib
import os

import numpy as np
import pytest

import oracle
import silence_inputs as si
from conftest import GOLDEN, parse_case
from oracle import otw_numpy
from real_time_audio_sync_amd import synth

KEYS = ("inserts", "tied_fill", "tied_steady", "largest", "equal_minima")

# band_tie_census of the full stream of silent_pair(2 c + 100, c, otw_seed(c), True), OTW, max_run_count 3:
# (inserts, inserts with a tied band minimum at t < c, at t >= c, largest tie in cells, inserts with rmin == cmin)
OTW_CENSUS = {
    20: (137, 19, 82, 21, 44),
    116: (290, 115, 159, 117, 172),
    117: (293, 116, 160, 118, 173),
    244: (461, 243, 201, 245, 342),
    245: (461, 244, 211, 246, 343),
    500: (1147, 499, 647, 501, 515),
    501: (1153, 500, 636, 502, 516),
    1013: (2149, 1012, 1136, 1014, 1028),
}
# the three pieces of silent_pieces(245, otw_seed(245) + 1) against the full stream, LiveNoteV2
PIECES_CENSUS = [(629, 244, 362, 246, 260), (633, 244, 362, 246, 258), (635, 244, 362, 246, 254)]
# the same silences under the dot cost: whole rows cost exactly 1.0 and no band minimum is ever shared
DOT_CENSUS = {20: (60, 0, 0, 1, 20), 245: (526, 0, 0, 1, 245)}
# synth_tie: (n_frames, seed, c) of test_exact_ties_on_the_512_cell_window / test_exact_ties_in_the_fill
TIE_DOT_CENSUS = {(700, 11, 400): (700, 0, 0, 1, 578), (590, 13, 245): (590, 0, 0, 1, 485)}
TIE_EUCLID_CENSUS = {(700, 11, 400): (620, 399, 219, 118, 479), (590, 13, 245): (525, 244, 279, 100, 337)}

# wtw_silence_case(**wtw_cases()[name]): per stream (windows, windows with 0 < NaN share < 1, windows entirely NaN,
# final status, live_ptr, ref_ptr)
WTW_RECORDS = {
    'w16_rows': [(25, 5, 2, 1, 200, 239), (10, 3, 2, 0, 80, 104), (30, 0, 0, 1, 240, 244)],
    'w33_cols': [(26, 4, 1, 1, 390, 508), (10, 4, 1, 0, 150, 227), (26, 4, 1, 1, 390, 497)],
    'w64_both': [(19, 9, 2, 1, 570, 969), (10, 7, 2, 0, 300, 589), (28, 4, 1, 1, 840, 969)],
    'w65_rows': [(23, 7, 1, 1, 736, 991), (10, 5, 1, 0, 320, 491), (30, 0, 0, 1, 960, 985)],
    'w100_cols': [(26, 4, 1, 1, 1274, 1540), (10, 4, 1, 0, 490, 734), (26, 4, 1, 1, 1274, 1538)],
    'w128_both': [(20, 9, 2, 1, 1240, 1944), (10, 7, 2, 0, 620, 1164), (26, 4, 1, 1, 1612, 1984)],
    'w100_rows': [(27, 8, 1, 1, 999, 1503), (12, 5, 1, 0, 444, 809), (40, 0, 0, 1, 1480, 1512)],
    'w33_both': [(22, 10, 4, 1, 242, 498), (14, 7, 4, 0, 154, 357), (36, 4, 1, 1, 396, 503)],
    'w128_cols': [(25, 4, 2, 1, 1600, 1958), (10, 4, 2, 0, 640, 1015), (25, 4, 2, 1, 1600, 1947)],
    'w64_lastcol': [(27, 4, 1, 1, 783, 971), (10, 4, 1, 0, 290, 488), (27, 4, 1, 1, 783, 974)],
    'w65_lastcol': [(25, 4, 1, 1, 800, 986), (10, 4, 1, 0, 320, 522), (26, 4, 2, 1, 832, 997)],
    'w128_lastcol': [(27, 4, 1, 1, 1647, 1920), (10, 4, 1, 0, 610, 922), (28, 4, 1, 1, 1708, 1971)],
    'w129_both': [(20, 9, 2, 1, 1280, 1937), (10, 7, 2, 0, 640, 1228), (27, 4, 1, 1, 1728, 2003)],
    'w130_rows': [(24, 7, 1, 1, 1536, 1994), (10, 5, 1, 0, 640, 977), (30, 0, 0, 1, 1920, 1970)],
    'w200_cols': [(25, 4, 1, 1, 2450, 3036), (10, 4, 1, 0, 980, 1512), (25, 4, 1, 1, 2450, 3029)],
    'w130_lastcol': [(26, 4, 1, 1, 1664, 1971), (10, 4, 1, 0, 640, 972), (27, 4, 1, 1, 1728, 1959)],
    'w768_both': [(16, 6, 1, 1, 6224, 8608), (9, 4, 1, 0, 3501, 5054), (4, 2, 0, 0, 1556, 2380)],
    'w800_both': [(16, 6, 1, 1, 6480, 8878), (9, 4, 1, 0, 3645, 5113), (4, 2, 0, 0, 1620, 2275)],
}


def _census(ref, live, c, variant, euclid):
    d = si.band_tie_census(ref, live, c, 3, variant, euclid)
    return tuple(d[k] for k in KEYS)


def _ties_enough(census, c):
    """What every Euclidean silence input must do: at least half of the full stream's inserts leave a tied band minimum,
    some tie covers the whole band of c + 1 cells, and ties occur both in the fill (t < c) and after it."""
    inserts, fill, steady, largest, _ = census
    assert 2 * (fill + steady) >= inserts, census
    assert largest == c + 1, census
    assert fill >= 1 and steady >= 1, census


def test_existing_dot_cost_tie_inputs_never_tie_a_band_minimum():
    """synth_tie under the dot cost ties the three predecessors of a cell, never the minimum of a band: what
    test_exact_ties_on_the_512_cell_window and test_exact_ties_in_the_fill do NOT cover.  The same frames through
    abs(x - 0.2) under the Euclidean cost tie a band minimum after nearly every insert."""
    for (n, seed, c), want in TIE_DOT_CENSUS.items():
        ref, live = synth.synth_tie(n, seed=seed)
        got = _census(ref, live, c, "otw", False)
        assert got == want and got[1] == got[2] == 0, (n, seed, c, got)
    for (n, seed, c), want in TIE_EUCLID_CENSUS.items():
        ref, live = si.tie_euclid(n, seed)
        got = _census(ref, live, c, "livenote_v2", True)
        assert got == want, (n, seed, c, got)
        assert 2 * (got[1] + got[2]) >= got[0] and got[1] >= 1 and got[2] >= 1


@pytest.mark.parametrize("c", si.OTW_BOUNDARY_C + si.OTW_WIDE_C)
def test_silent_pairs_tie_the_band_minima(c):
    ref, lives = si.silent_pair(2 * c + 100, c, si.otw_seed(c), True)
    assert len(lives) == 3 and c < lives[1].shape[1] < c + 55 and lives[2].shape[1] > lives[0].shape[1]
    assert not ref[:, : c + 48].any() and ref[:, c + 48].any() and not lives[0][:, : c + 55].any()
    got = _census(ref, lives[0], c, "otw", True)
    assert got == OTW_CENSUS[c], got
    _ties_enough(got, c)
    # the cut stream ends inside the first silence, after the crossing of t = c: all of its inserts but the first tie
    cut = _census(ref, lives[1], c, "otw", True)
    assert cut[0] == lives[1].shape[1] and cut[1] == c - 1 and cut[2] == cut[0] - c, cut


def test_silent_pieces_tie_the_band_minima():
    c = 245
    refs, lives = si.silent_pieces(c, si.otw_seed(c) + 1)
    assert len({r.shape[1] for r in refs}) > 1
    for b, r in enumerate(refs):
        assert not r[:, : c + 48 - (0, 7, 19)[b]].any() and r[:, c + 48 - (0, 7, 19)[b]].any()
        got = _census(r, lives[0], c, "livenote_v2", True)
        assert got == PIECES_CENSUS[b], (b, got)
        _ties_enough(got, c)


@pytest.mark.parametrize("c", si.OTW_DOT_C)
def test_silence_under_the_dot_cost_has_no_ties(c):
    ref, lives = si.silent_pair(2 * c + 100, c, si.otw_seed(c), False)
    got = _census(ref, lives[0], c, "otw", False)
    assert got == DOT_CENSUS[c], got
    o = oracle.OtwOracle(ref, c, 3, keep_cost=True)
    o.run(lives[0][:, :5])
    assert (o.cost()[:5, : min(c, 5)] == 1.0).all()      # a zero frame costs exactly 1.0 against everything


@pytest.mark.parametrize("name", sorted(si.wtw_cases()))
def test_wtw_silence_cases_hold_nan_windows(name):
    kw = si.wtw_cases()[name]
    ref, lives, recs = si.wtw_silence_case(**kw)
    got = []
    for r in recs:
        sh = [w[2] for w in r["windows"]]
        got.append((len(sh), sum(0 < s < 1 for s in sh), sum(s == 1 for s in sh), r["status"], r["live_ptr"], r["ref_ptr"]))
    assert got == WTW_RECORDS[name], got
    assert 2 <= len(lives) <= 3 and lives[-1].all(), "the last stream holds no silent frame"
    if name.endswith("lastcol") or kw["W"] >= 768:
        # the first window's only silent column is its last: the one placement where a cell has a NaN above it and
        # finite neighbours to its left, on the column the path climbs
        assert recs[0]["windows"][0][:2] == (0, 0) and kw["cols"] == (kw["W"] - 1,)
        assert ref[:, : kw["W"] - 1].any(axis=0).all() and not ref[:, kw["W"] - 1].any()
    free_after_nan = stopped = False
    for b, r in enumerate(recs):
        sh = [w[2] for w in r["windows"]]
        assert len(sh) >= 3, (name, b)
        # a stream whose own frames and whose reference hold no silence cannot meet a NaN: the last stream of the cases
        # with silent live frames only.  Every other stream has a partly and a wholly NaN window.
        if lives[b].all() and ref.all():
            assert b == len(lives) - 1 and not any(sh)
        elif lives[b].all() and kw.get("clean_len"):
            assert any(0 < s < 1 for s in sh)             # the short third stream of the 12- and 13-strip windows
        else:
            assert any(0 < s < 1 for s in sh) and any(s == 1 for s in sh), (name, b, sh)
        nan_at = [i for i, s in enumerate(sh) if s > 0]
        free_after_nan |= bool(nan_at) and nan_at[-1] < len(sh) - 1 and sh[-1] == 0
        stopped |= r["status"] == oracle.STOP_REF_END
    assert free_after_nan and stopped, name


@pytest.mark.parametrize("c", [20, 70])
def test_numpy_restatement_equals_the_oracle_on_silence(c):
    """oracle/otw_numpy.py (dot cost, OTW) on the small silent inputs: whole rows of cost exactly 1.0."""
    ref, lives = si.silent_pair(2 * c + 100, c, si.otw_seed(c), False)
    for live in lives:
        n = otw_numpy.NumpyOTW(ref, c, 3)
        o = oracle.OtwOracle(ref, c, 3)
        assert n.run(live) == o.run(live)
        so = o.state
        assert np.array_equal(np.array(n.path, dtype=np.int32).reshape(-1, 2), o.path)
        assert (n.t, n.j, n.status) == (so["t"], so["j"], so["status"])
        if so["status"] == oracle.RUNNING:
            assert (n.direction, n.run_count) == (so["direction"], so["run_count"])
        rb, cb = n.bands()
        orb, ocb = o.bands()
        assert np.array_equal(rb, orb, equal_nan=True) and np.array_equal(cb, ocb, equal_nan=True)


# ---- the oracle against what the reference's own code gave (silence_golden.npz) --------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "silence_golden.npz"))


def test_golden_inputs_are_the_silent_pairs(golden):
    for c in (20, 70):
        for euclid in (False, True):
            grp = "c%d_%s" % (c, "euclid" if euclid else "dot")
            ref, lives = si.silent_pair(2 * c + 100, c, si.otw_seed(c), euclid)
            assert np.array_equal(golden[grp + "/ref"].astype(np.float64), ref)
            assert np.array_equal(golden[grp + "/live"].astype(np.float64), lives[0])


def test_oracle_equals_the_reference_on_silent_otw_inputs(golden):
    g = golden
    seen = set()
    for meta in g["cases"]:
        case = parse_case(meta)
        cid = case["cid"]
        grp = "c%d_%s" % (case["c"], "euclid" if case["euclid"] else "dot")
        ref, live = g[grp + "/ref"].astype(np.float64), g[grp + "/live"].astype(np.float64)
        o = oracle.OtwOracle(ref, case["c"], case["mrc"], si.VARIANTS[case["variant"]],
                             oracle.COST_EUCLID if case["euclid"] else oracle.COST_DOT)
        if case["mode"] == "set_live":
            o.set_live(live)
        else:
            assert o.run(live) == int(g[cid + "/consumed"]), cid
            assert (o.state["status"] == oracle.STOP_REF_END) == bool(g[cid + "/stopped"]), cid
        st = o.state
        assert np.array_equal(o.path, g[cid + "/path"]), cid
        assert (st["t"], st["j"]) == (int(g[cid + "/t"]), int(g[cid + "/j"])), cid
        assert (st["previous"], st["run_count"]) == (int(g[cid + "/previous"]), int(g[cid + "/run_count"])), cid
        if case["mode"] == "insert":
            assert st["direction"] == int(g[cid + "/direction"]), cid
            rb, cb = o.bands()
            assert np.array_equal(rb, g[cid + "/row_band"], equal_nan=True), cid
            assert np.array_equal(cb, g[cid + "/col_band"], equal_nan=True), cid
        seen.add((case["variant"], case["mode"], case["euclid"], case["c"]))
    assert len(seen) == 16


def _same_as_digest(A, g, key):
    Z = np.where(np.isnan(A), 0.0, A)
    assert np.array_equal(np.packbits(np.isnan(A)), g[key + "_nan"]), key
    assert np.array_equal(A[-1], g[key + "_last_row"], equal_nan=True), key
    assert np.array_equal(A[:, -1], g[key + "_last_col"], equal_nan=True), key
    assert np.array_equal(A[::7, ::5], g[key + "_grid"], equal_nan=True), key
    assert hashlib.sha256(np.ascontiguousarray(Z).tobytes()).hexdigest() == str(g[key + "_sha"]), key


def test_oracle_equals_the_reference_on_silent_wtw_windows(golden):
    g = golden
    assert len(g["windows"]) == 8
    for cid in g["windows"]:
        cid = str(cid)
        x, y = g[cid + "/x"].astype(np.float64), g[cid + "/y"].astype(np.float64)
        with np.errstate(all="ignore"):
            C = oracle.wtw_cost_matrix(x, y)
            D, B = oracle.wtw_run_dtw(C)
        sub = oracle.wtw_find_path(B)
        assert np.isnan(C).any(), cid
        if cid + "/C" in g.files:
            assert np.array_equal(C, g[cid + "/C"], equal_nan=True), cid
            assert np.array_equal(D, g[cid + "/D"], equal_nan=True), cid
        else:
            _same_as_digest(C, g, cid + "/C")
            _same_as_digest(D, g, cid + "/D")
        assert np.array_equal(B, g[cid + "/B"]), cid
        assert np.array_equal(sub, g[cid + "/sub"]), cid
