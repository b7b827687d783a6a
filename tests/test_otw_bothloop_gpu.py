"""Both steps in wave 0's hit-step loop (pipelined W = 512 kernel, csrc/otw.hip): while the band fills (t < c) every step is
a Both step whose two strips are the two speculated shadows, and with a full band a Both step is one if the column
speculation's flag allows ("hit if").  The loop settles such a step itself -- three cells, the dropped cell's sentinel
store, two wave reductions side by side -- and leaves it to the general loop when an argmin falls outside the step's
window.  Every stream must match the dense CPU oracle bit for bit: path, end state and (insert mode) both bands.

The library has no test-visible counter that tells the loop's Both path from the general loop's (the state words count
strips, cells and band reductions, which are the same either way); that the path runs is shown by the stamped profile
(tools/otw_phase_profile.py, level 2, by step kind)."""
import numpy as np
import pytest

from test_otw_hitloop_gpu import _check, mods  # noqa: F401  (mods: the module fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _streams(synth, c, seed):
    """Reference of 2c + 100 frames and three streams: one ends inside the fill, one crosses t = c-2, c-1, c and stops right
    behind, one runs past the reference end (stop; in set_live to the end of its frames)."""
    ref, lives = synth.synth_batch(2 * c + 100, 3, seed=seed)
    lives[0] = lives[0][:, : c - 7]
    lives[1] = lives[1][:, : c + 2]
    lives[2] = synth._as_f32_values(np.concatenate([lives[2], np.repeat(lives[2][:, -1:], 40, axis=1)], axis=1))
    return ref, lives


@pytest.mark.parametrize("variant", ["otw", "livenote", "livenote_v2"])
@pytest.mark.parametrize("mode", ["insert", "set_live"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("c", [245, 300])
def test_fill_every_policy(mods, variant, mode, dtype, c):
    oracle, ob, synth = mods
    ref, lives = _streams(synth, c, 5200 + c + len(variant) + (7 if mode == "set_live" else 0))
    tdt = torch.float32 if dtype == "f32" else torch.float64
    for mrc in (1, 3):
        _check(oracle, ob, ref, lives, c, mrc, variant, mode, tdt)


@pytest.mark.parametrize("mode", ["insert", "set_live"])
@pytest.mark.parametrize("c", [245, 300])
def test_reference_shorter_than_the_band(mods, mode, c):
    """The reference ends inside the fill: the stop falls on a Both step with t < c."""
    oracle, ob, synth = mods
    ref, lives = synth.synth_batch(c - 20, 3, seed=61 + c)
    lives[1] = lives[1][:, : lives[1].shape[1] // 2]
    lives[2] = synth._as_f32_values(np.concatenate([lives[2], np.repeat(lives[2][:, -1:], 60, axis=1)], axis=1))
    for variant in ("otw", "livenote_v2"):
        _check(oracle, ob, ref, lives, c, 3, variant, mode, torch.float32)


@pytest.mark.parametrize("variant", ["otw", "livenote_v2"])
@pytest.mark.parametrize("c", [245, 300])
def test_exact_ties_in_the_fill(mods, variant, c):
    """synth_tie: exactly equal costs, so the three predecessors of a cell tie (56 436 of the 226 676 cells at c = 245) and
    the order of the candidates decides.  Under the dot cost the minimum of a band is never tied, after none of the
    inserts (tests/test_silence_cpu.py pins that); tied band minima, where np.argmin's first-minimum rule decides, are in
    tests/test_otw_ties_gpu.py."""
    oracle, ob, synth = mods
    ref, live = synth.synth_tie(2 * c + 100, seed=13)
    lives = [live, live[:, : c - 3].copy(), live[:, : c + 1].copy()]
    for mode in ("insert", "set_live"):
        _check(oracle, ob, ref, lives, c, 3, variant, mode, torch.float64)


def test_euclidean_cost_in_the_fill(mods):
    oracle, ob, synth = mods
    ref, lives = _streams(synth, 245, 977)
    ref = synth._as_f32_values(np.abs(ref - 0.2))
    lives = [synth._as_f32_values(np.abs(l - 0.2)) for l in lives]
    _check(oracle, ob, ref, lives, 245, 2, "livenote_v2", "insert", torch.float64, euclid=True)


# ---- full band: "hit if" -------------------------------------------------------------------------------------------
HIT_IF_SEED, HIT_IF_N, HIT_IF_C = 77, 900, 245
# Both steps with a full band in the oracle's step sequence of the three streams (OTW, max_run_count 3), and how many
# of them find the column speculation's flag set / clear (_full_band_both_steps)
HIT_IF_COUNTS = [(75, 66, 9), (74, 63, 11), (81, 76, 5)]


def _full_band_both_steps(oracle, ref, live, c, mrc):
    """(Both steps with t >= c, flag set, flag clear) of the OTW policy, from the CPU oracle alone.  An insert that adds
    one path point fewer than it computes strips began with a Both step, (t, j) -> (t+1, j+1).  The flag restated on the dense
    matrices: the speculated column strip starts one row above the Both step's, at (t+1-c, j+1), and dropping that cell
    changes nothing iff the chain through it, (acc[t+1-c][j] + d(t+1-c, j+1)) + d(t+2-c, j+1), does not beat the value
    the oracle computed for (t+2-c, j+1)."""
    o = oracle.OtwOracle(ref, c, mrc, oracle.OTW, keep_cost=True)
    steps, last = [], None
    for t in range(live.shape[1]):
        o.insert(live[:, t])
        s, n = o.state, len(o.path)
        if s["status"] != 0:
            break
        if last is not None and (s["t"] - last[0]) + (s["j"] - last[1]) - (n - last[2]) == 1 and last[0] >= c - 1:
            steps.append((last[0] + 1, last[1] + 1))
        last = (s["t"], s["j"], n)
    acc, cost = o.acc_cost(), o.cost()
    n_set = n_clear = 0
    for pt, jn in steps:
        d0 = 1.0 - oracle.dot_strided(live[:, pt - c], ref[:, jn])
        if (acc[pt - c, jn - 1] + d0) + cost[pt - c + 1, jn] < acc[pt - c + 1, jn]:
            n_clear += 1
        else:
            n_set += 1
    return len(steps), n_set, n_clear


@pytest.fixture(scope="module")
def hit_if_streams(mods):
    oracle, ob, synth = mods
    ref, lives = synth.synth_batch(HIT_IF_N, 3, seed=HIT_IF_SEED)
    counts = [_full_band_both_steps(oracle, ref, l, HIT_IF_C, 3) for l in lives]
    return ref, lives, counts


def test_hit_if_inputs_have_both_steps_of_each_kind(hit_if_streams):
    ref, lives, counts = hit_if_streams
    assert counts == HIT_IF_COUNTS
    assert all(n_set > 0 and n_clear > 0 for _, n_set, n_clear in counts)


@pytest.mark.parametrize("variant", ["otw", "livenote", "livenote_v2"])
@pytest.mark.parametrize("mode", ["insert", "set_live"])
def test_hit_if_full_band(mods, hit_if_streams, variant, mode):
    oracle, ob, synth = mods
    ref, lives, _ = hit_if_streams
    for mrc, dtype in ((3, torch.float32), (1, torch.float64)):
        _check(oracle, ob, ref, lives, HIT_IF_C, mrc, variant, mode, dtype)
