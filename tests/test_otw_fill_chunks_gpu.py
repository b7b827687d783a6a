"""The chunked, skewed schedule of otw_bandfill_kernel (csrc/otw_fill.h): wave w runs K w stages behind wave 0, a chunk of K
stages between two barriers, and lane 63's values travel to the wave below through a ring of 2K + 1 slots per wave.

The schedule can go wrong at a chunk boundary (the last chunk of 1 .. K stages, the first slot of a chunk read from the
chunk before the previous one), at a wave boundary (the ring, the row band of the last wave) and where the two meet.  The
cases are the band widths that move those boundaries against each other; every one goes through ``_ab`` of
tests/test_otw_fill_gpu.py: the dense oracle, the RTS_OTW_FILL=1 / =0 pair bit for bit, the segmented handle with all 16
state words.  Two streams of c + 6 frames, a reference of 2c + 40 frames.

Two rows per thread: wave w owns rows 128 w .. 128 w + 127, so the wave boundaries sit at c = 128, 256, 384."""
import numpy as np
import pytest

from test_otw_fill_gpu import _ab, _silenced, mods  # noqa: F401  (mods: the module fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MODES = ["insert", "set_live"]
WAVE_EDGES = list(range(124, 135)) + list(range(252, 263)) + list(range(380, 391)) + [499]


def _inputs(synth, c, seed, n=2):
    ref, lives = synth.synth_batch(2 * c + 40, n, seed=seed)
    return ref, [l[:, : c + 6].copy() for l in lives]


@pytest.mark.parametrize("c", list(range(2, 71)))
def test_every_stage_count_in_one_wave(mods, c):
    """c = 2 .. 70: the stage count ceil(c / 2) + c - 1 passes through every residue modulo K for K <= 32, so the last
    chunk has 1, K - 1 and K stages."""
    oracle, ob, synth = mods
    ref, lives = _inputs(synth, c, 8000 + c)
    assert _ab(oracle, ob, ref, lives, c, 3, "otw", "insert", torch.float32) == [1, 1]


@pytest.mark.parametrize("c", WAVE_EDGES)
def test_wave_boundaries_against_chunk_boundaries(mods, c):
    """The last wave owns 1 .. 7 rows, or the wave above it ends 1 .. 4 rows short; 499: four waves, the longest sweep."""
    oracle, ob, synth = mods
    ref, lives = _inputs(synth, c, 8100 + c)
    assert _ab(oracle, ob, ref, lives, c, 3, "otw", "insert", torch.float32) == [1, 1]


@pytest.mark.parametrize("c", [128, 130, 257, 386])
def test_wave_boundaries_every_policy(mods, c):
    """set_live, the filtered variant, float64 features and the Euclidean cost at the wave boundaries."""
    oracle, ob, synth = mods
    ref, lives = _inputs(synth, c, 8600 + c)
    assert _ab(oracle, ob, ref, lives, c, 3, "otw", "set_live", torch.float32) == [1, 1]
    assert _ab(oracle, ob, ref, lives, c, 3, "livenote_v2", "insert", torch.float32) == [1, 1]
    assert _ab(oracle, ob, ref, lives, c, 1, "livenote_v2", "set_live", torch.float64) == [1, 1]
    refe, livese = synth._as_f32_values(np.abs(ref - 0.2)), [synth._as_f32_values(np.abs(l - 0.2)) for l in lives]
    assert _ab(oracle, ob, refe, livese, c, 3, "otw", "insert", torch.float64, euclid=True) == [1, 1]


@pytest.mark.parametrize("c", [130, 258])
def test_tied_minima_across_the_ring(mods, c):
    """All-zero frames 0, 63, 64 and c-1 on both sides: whole rows and columns cost exactly 1.0, so the column argmin that
    travels through the ring (value and index) ties with the rows below, and a stale slot shows as a wrong first minimum."""
    oracle, ob, synth = mods
    ref, lives = _inputs(synth, c, 8700 + c, n=1)
    ref, live = _silenced(ref, lives[0], c)
    for mode in MODES:
        assert _ab(oracle, ob, ref, [live], c, 3, "otw", mode, torch.float32) == [1]
    assert _ab(oracle, ob, ref, [live], c, 3, "livenote_v2", "insert", torch.float64) == [1]


@pytest.mark.parametrize("mode", MODES)
def test_nan_crosses_the_ring(mods, mode):
    """c = 130: a NaN feature in live frame 127 (the last row of wave 0: every value it publishes is NaN) and, in the other
    stream, in frame 128 (the first row of wave 1).  No oracle (OTW has no defined NaN behaviour): the step loop's bits."""
    oracle, ob, synth = mods
    c = 130
    ref, lives = _inputs(synth, c, 8800)
    lives[0][4, 127] = np.nan
    lives[1][7, 128] = np.nan
    for variant in ("otw", "livenote_v2"):
        assert _ab(oracle, ob, ref, lives, c, 3, variant, mode, torch.float64, with_oracle=False) == [1, 1]


def test_mixed_eligibility_in_one_batch(mods):
    """c = 130, streams of c-1, c, c+1 and c+6 frames: the first workgroup returns before the first barrier, the others
    sweep; ``_ab`` asserts ``took`` against ``_expect``."""
    oracle, ob, synth = mods
    c = 130
    ref, lives = synth.synth_batch(2 * c + 40, 4, seed=8900)
    lives = [lives[0][:, : c - 1].copy(), lives[1][:, :c].copy(), lives[2][:, : c + 1].copy(), lives[3][:, : c + 6].copy()]
    assert _ab(oracle, ob, ref, lives, c, 3, "otw", "insert", torch.float32) == [0, 1, 1, 1]
    assert _ab(oracle, ob, ref, lives, c, 3, "livenote_v2", "set_live", torch.float32) == [0, 0, 1, 1]
