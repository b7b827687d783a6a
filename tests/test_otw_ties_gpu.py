"""Tied band minima on the OTW kernels: digital silence under the Euclidean cost (tests/silence_inputs.py).

A zero live column against a zero reference column costs exactly 0, so accumulated costs repeat along the whole band and
both band minima are tied after nearly every insert -- tests/test_silence_cpu.py pins how often.  The kernel keeps both
argmins incrementally, and every one of its tie rules then decides the path: a kept minimum survives until it slides out
of the window, the appended corner cell wins only if strictly smaller, the full reduction and the per-lane parts of the
speculative strips return np.argmin's FIRST minimum across lanes and waves, and ``rmin < cmin`` chooses between the
bands.  Every configuration must equal the dense CPU oracle: path, end state and, in insert mode, the direction and both
accumulated-cost bands, all compared with ==.

Operands are never NaN here: a silent chroma column is all zeros, and OTW has no defined NaN behaviour."""
import numpy as np
import pytest

import silence_inputs as si
from test_otw_hitloop_gpu import _check

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import oracle
    from real_time_audio_sync_amd import otw_batch
    return oracle, otw_batch


@pytest.fixture(scope="module")
def pair245():
    return si.silent_pair(2 * 245 + 100, 245, si.otw_seed(245), True)


def _oracles(oracle, refs, lives, c, mrc, variant, euclid=True, mode="insert"):
    out = []
    for ref, live in zip(refs, lives):
        o = oracle.OtwOracle(ref, c, mrc, si.VARIANTS[variant], oracle.COST_EUCLID if euclid else oracle.COST_DOT)
        (o.set_live if mode == "set_live" else o.run)(live)
        out.append(o)
    return out


def _same(eng, oracles, tag, mode="insert"):
    for b, o in enumerate(oracles):
        st, so = eng.state(b), o.state
        assert np.array_equal(eng.path(b), o.path), (tag, b)
        for key in ("t", "j", "previous", "run_count", "status"):
            assert st[key] == so[key], (tag, b, key)
        if mode == "insert":
            assert st["direction"] == so["direction"], (tag, b)
            rb, cb = eng.bands(b)
            orb, ocb = o.bands()
            assert np.array_equal(rb, orb, equal_nan=True) and np.array_equal(cb, ocb, equal_nan=True), (tag, b)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("mode", ["insert", "set_live"])
@pytest.mark.parametrize("variant", ["otw", "livenote_v2"])
@pytest.mark.parametrize("c", si.OTW_BOUNDARY_C)
def test_silence_at_the_window_boundaries(mods, c, variant, mode, dtype):
    """The last and the first band width of each LDS window (32, 128, 256, 512 cells), three ragged streams."""
    oracle, ob = mods
    ref, lives = si.silent_pair(2 * c + 100, c, si.otw_seed(c), True)
    tdt = torch.float32 if dtype == "f32" else torch.float64
    for mrc in (1, 3):
        _check(oracle, ob, ref, lives, c, mrc, variant, mode, tdt, euclid=True)


@pytest.mark.parametrize("c,variant", [(501, "livenote_v2"), (1013, "otw")])
def test_silence_on_the_wide_windows(mods, c, variant):
    """The 1024- and 2048-cell windows at their first band width."""
    oracle, ob = mods
    ref, lives = si.silent_pair(2 * c + 100, c, si.otw_seed(c), True)
    _check(oracle, ob, ref, lives, c, 3, variant, "insert", torch.float32, euclid=True)


@pytest.mark.parametrize("flavour", ["default", "spec0", "tp_from0", "waves8"])
def test_silence_on_every_kernel_flavour(mods, pair245, monkeypatch, flavour):
    """c = 245: the pipelined kernel, the plain one (RTS_OTW_SPEC=0), the residency flavour (RTS_OTW_TP_FROM=0) and
    the wave count passed explicitly."""
    oracle, ob = mods
    ref, lives = pair245
    if flavour == "spec0":
        monkeypatch.setenv("RTS_OTW_SPEC", "0")
    if flavour == "tp_from0":
        monkeypatch.setenv("RTS_OTW_TP_FROM", "0")
    waves = int(flavour[5:]) if flavour.startswith("waves") else None
    for variant, mode in (("livenote_v2", "insert"), ("otw", "set_live")):
        eng = ob.BatchedOTW(ref, 245, 3, batch=3, variant=variant, euclid=True, dtype=torch.float32, waves=waves)
        lv, ln = eng.pack(lives)
        eng.run(lv, ln, mode=mode)
        _same(eng, _oracles(oracle, [ref] * 3, lives, 245, 3, variant, mode=mode), (flavour, variant, mode), mode)
        eng.close()


def test_silence_through_per_call_ingestion(mods, pair245):
    """The same streams one frame per call (insert) and in uneven per-stream chunks (push): a tie then straddles
    launches, with the kept argmins persisted in the state.  Both must equal the run and the oracle."""
    oracle, ob = mods
    ref, lives = pair245
    oracles = _oracles(oracle, [ref] * 3, lives, 245, 3, "livenote_v2")
    eng = ob.BatchedOTW(ref, 245, 3, batch=3, variant="livenote_v2", euclid=True, dtype=torch.float64)
    dev = eng.device
    lv, ln = eng.pack(lives)
    eng.run(lv, ln)
    _same(eng, oracles, "run")
    run_paths = eng.paths()
    lens = [l.shape[1] for l in lives]
    eng.reset()
    for i in range(max(lens)):
        frames = np.zeros((3, 12))
        for b, l in enumerate(lives):
            if i < lens[b]:
                frames[b] = l[:, i]
        active = torch.tensor([int(i < n) for n in lens], dtype=torch.uint8)
        eng.insert(torch.from_numpy(frames).to(dev), active.to(dev))
    _same(eng, oracles, "insert")
    assert all(np.array_equal(p, q) for p, q in zip(eng.paths(), run_paths))
    eng.reset()
    rs = np.random.RandomState(245)
    done = [0, 0, 0]
    while any(d < n for d, n in zip(done, lens)):
        take = [min(int(rs.choice([0, 1, 2, 7, 64, 100])), n - d) for d, n in zip(done, lens)]
        if not any(take):
            continue
        buf = np.zeros((3, max(take), 12))
        for b, l in enumerate(lives):
            buf[b, : take[b]] = l[:, done[b]: done[b] + take[b]].T
            done[b] += take[b]
        eng.push(torch.from_numpy(buf).to(dev), torch.tensor(take, dtype=torch.int32).to(dev))
    _same(eng, oracles, "push")
    assert all(np.array_equal(p, q) for p, q in zip(eng.paths(), run_paths))
    eng.close()


@pytest.mark.parametrize("variant", ["otw", "livenote", "livenote_v2"])
@pytest.mark.parametrize("c", si.OTW_DOT_C)
def test_silence_under_the_dot_cost(mods, c, variant):
    """No ties here: a zero frame costs exactly 1.0 against everything, whole rows and columns of it."""
    oracle, ob = mods
    ref, lives = si.silent_pair(2 * c + 100, c, si.otw_seed(c), False)
    for mode, dt in (("insert", torch.float32), ("set_live", torch.float64)):
        _check(oracle, ob, ref, lives, c, 3, variant, mode, dt)


def test_silence_with_per_stream_references(mods):
    """One create_refs handle whose pieces begin with different lengths of silence."""
    oracle, ob = mods
    c = 245
    refs, lives = si.silent_pieces(c, si.otw_seed(c) + 1)
    lives = [lives[0], lives[2], lives[0]]
    for variant, mode in (("livenote_v2", "insert"), ("otw", "set_live")):
        eng = ob.BatchedOTW.with_references(refs, c, 3, variant=variant, euclid=True, dtype=torch.float32)
        lv, ln = eng.pack(lives)
        eng.run(lv, ln, mode=mode)
        _same(eng, _oracles(oracle, refs, lives, c, 3, variant, mode=mode), (variant, mode), mode)
        eng.close()


@pytest.mark.parametrize("n,seed,c", [(590, 13, 245), (700, 11, 400)])
def test_tie_generator_under_the_euclidean_cost(mods, n, seed, c):
    """synth_tie's repeated frames cost exactly 0 against each other under the Euclidean cost: the inputs of
    test_exact_ties_in_the_fill and test_exact_ties_on_the_512_cell_window, which under the dot cost never tie a band
    minimum, tie one after nearly every insert."""
    oracle, ob = mods
    ref, live = si.tie_euclid(n, seed)
    lives = [live, live[:, : live.shape[1] // 2].copy()]
    for variant in ("otw", "livenote_v2"):
        for mode in ("insert", "set_live"):
            _check(oracle, ob, ref, lives, c, 3, variant, mode, torch.float64, euclid=True)
