"""The wide forms of the pipelined W = 512 step kernel (12 and 16 waves per stream, csrc/otw_plan.h: threads): the further
waves are helpers, so every strided loop over "the helper threads" -- the cost strips of a step, the launch prologue's
otw_costs_prime, the LDS clearing, the band reload and the epilogue -- runs with another thread count, and the cost strips
take the one-cell loop.  RTS_OTW_WAVES forces each width in turn; every run first asserts through ``BatchedOTW.kernel`` that
it got that width, then must equal the 8-wave kernel bit for bit -- path, both bands, every state word but
RTS_ST_BAND_RECOMPUTES -- and the dense CPU oracle.

Shapes: c = 245 (the smallest W = 512 band: a strip of 247 cells, most helpers of either wide form have none) and c = 500
(502 cells: one per thread for most of the 576 helpers of the 12-wave form, none for the rest; two per thread on the 320
of the 8-wave form), references of 260 and 600 frames with live streams around 1.3 N, so that strips are clipped at
column 0, at N - 1 and at the live end; stream 1 ends early, stream 2 runs on to the reference's end."""
import contextlib
import os

import numpy as np
import pytest

import silence_inputs as si

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WIDTHS = (8, 12, 16)
VARIANTS = ("otw", "livenote", "livenote_v2")
MODES = ("insert", "set_live")
SHAPES = ((245, 260), (245, 600), (500, 260), (500, 600))   # (c, N)


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import oracle
    from real_time_audio_sync_amd import _native, otw_batch, synth
    return oracle, otw_batch, synth, _native


@contextlib.contextmanager
def env(**kw):
    """RTS_OTW_* as rts_otw_create reads them."""
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def streams(synth, N, seed, euclid):
    """-> (ref (12, N), [full, cut, extended]): renditions at 0.55 .. 1.0 reference frames per live frame, about 1.3 N long."""
    ref = synth.synth_ref(N, seed)
    lives = [synth.synth_live(ref, seed + 1 + b, lo=0.55, hi=1.0) for b in range(3)]
    assert all(1.2 * N < l.shape[1] < 1.4 * N for l in lives)
    lives[1] = lives[1][:, : (3 * lives[1].shape[1]) // 5].copy()
    lives[2] = synth._as_f32_values(np.concatenate([lives[2], np.repeat(lives[2][:, -1:], N // 2, axis=1)], axis=1))
    if euclid:
        ref = synth._as_f32_values(np.abs(ref - 0.2))
        lives = [synth._as_f32_values(np.abs(l - 0.2)) for l in lives]
    return ref, lives


def snapshot(eng, B):
    """Everything a launch leaves behind: the paths, both bands and the state words (without RTS_ST_BAND_RECOMPUTES, which
    counts how often a kept band minimum had to be reduced again and is allowed to depend on the kernel)."""
    st = eng.states()
    return dict(paths=[eng.path(b) for b in range(B)], bands=[eng.bands(b) for b in range(B)], state=np.delete(st, 15, axis=1))


def same_snapshot(a, b, tag):
    assert np.array_equal(a["state"], b["state"]), (tag, "state")
    for p, q in zip(a["paths"], b["paths"]):
        assert np.array_equal(p, q), (tag, "path")
    for (r0, c0), (r1, c1) in zip(a["bands"], b["bands"]):
        # bit for bit, NaN slots (never evaluated) in the same places
        assert np.array_equal(r0.view(np.int64), r1.view(np.int64)) and np.array_equal(c0.view(np.int64), c1.view(np.int64)), (tag, "bands")


def same_as_oracle(oracle, eng, oracles, mode, tag):
    for b, o in enumerate(oracles):
        st, so = eng.state(b), o.state
        assert np.array_equal(eng.path(b), o.path), (tag, b, "path")
        for key in ("t", "j", "previous", "run_count", "status"):
            assert st[key] == so[key], (tag, b, key)
        if mode == "insert":
            assert st["direction"] == so["direction"], (tag, b)
            cnt = o.counters
            assert (st["cells"], st["row_strips"], st["col_strips"]) == (cnt["cells"], cnt["row_strips"], cnt["col_strips"]), (tag, b)
            rb, cb = eng.bands(b)
            orb, ocb = o.bands()
            assert np.array_equal(rb, orb, equal_nan=True) and np.array_equal(cb, ocb, equal_nan=True), (tag, b, "bands")


def run_oracles(oracle, ref, lives, c, mrc, variant, mode, euclid):
    out = []
    for live in lives:
        o = oracle.OtwOracle(ref, c, mrc, si.VARIANTS[variant], oracle.COST_EUCLID if euclid else oracle.COST_DOT)
        (o.set_live if mode == "set_live" else o.run)(live)
        out.append(o)
    return out


def every_width(ob, ref, c, mrc, variant, euclid, tdt, fill, drive, kernel_dtype, tag):
    """`drive(eng)` on a handle of each width; -> the snapshots by width, after asserting each handle's width and that the
    wide ones left what the 8-wave one left."""
    snaps = {}
    for waves in WIDTHS:
        with env(RTS_OTW_WAVES=waves, RTS_OTW_FILL=fill):
            eng = ob.BatchedOTW(ref, c, mrc, batch=3, variant=variant, euclid=euclid, dtype=tdt)
        try:
            got = eng.kernel(kernel_dtype, with_waves=True)
            assert got["waves"] == waves and got["pipelined"] and got["window"] == 512 and got["fill"] == bool(fill), (tag, waves, got)
            assert got["ring"] == ("float" if tdt == torch.float32 and kernel_dtype == torch.float32 else "double"), (tag, got)
            drive(eng, waves)
            snaps[waves] = snapshot(eng, 3)
        finally:
            eng.close()
        if waves != 8:
            same_snapshot(snaps[8], snaps[waves], (tag, waves))
    return snaps


@pytest.mark.parametrize("euclid", [False, True], ids=["dot", "euclid"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("c,N", SHAPES)
def test_every_width_matches_the_8_wave_kernel_and_the_oracle(mods, c, N, dtype, euclid):
    """Every variant, mode and run-count limit of tests/test_otw_hitloop_gpu.py, band fill on (the step loop resumes at
    t = c - 1 through the prologue) and off (the step loop from the first frame)."""
    oracle, ob, synth, _ = mods
    tdt = torch.float32 if dtype == "f32" else torch.float64
    ref, lives = streams(synth, N, 5200 + c + N, euclid)
    stopped = False
    for variant in VARIANTS:
        for mode in MODES:
            for mrc, fill in ((1, 1), (3, 1), (3, 0)):
                tag = (c, N, dtype, euclid, variant, mode, mrc, fill)
                oracles = run_oracles(oracle, ref, lives, c, mrc, variant, mode, euclid) if fill else oracles

                def drive(eng, waves):
                    lv, ln = eng.pack(lives, dtype=tdt)
                    eng.run(lv, ln, mode=mode)
                    same_as_oracle(oracle, eng, oracles, mode, (tag, waves))

                every_width(ob, ref, c, mrc, variant, euclid, tdt, fill, drive, tdt, tag)
                stopped = stopped or oracles[2].state["status"] == oracle.STOP_REF_END
    assert stopped, "no configuration ran stream 2 to the reference's end"


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("c,N", [(245, 260), (500, 600)])
def test_a_run_resumed_in_three_pieces(mods, c, N, dtype):
    """rts_otw_push three times: every launch goes through the prologue's otw_costs_prime at the width's thread count,
    the second and third from persisted bands in mid-piece.  The history is float64, so this is the double ring."""
    oracle, ob, synth, _ = mods
    tdt = torch.float32 if dtype == "f32" else torch.float64
    ref, lives = streams(synth, N, 6100 + c, False)
    oracles = run_oracles(oracle, ref, lives, c, 3, "otw", "insert", False)
    lens = [l.shape[1] for l in lives]
    cuts = [(0, n // 3, (2 * n) // 3 + 1, n) for n in lens]

    def drive(eng, waves):
        for piece in range(3):
            take = [cuts[b][piece + 1] - cuts[b][piece] for b in range(3)]
            buf = np.zeros((3, max(take), 12))
            for b, l in enumerate(lives):
                buf[b, : take[b]] = l[:, cuts[b][piece]: cuts[b][piece + 1]].T
            eng.push(torch.from_numpy(buf).to(tdt).to(eng.device), torch.tensor(take, dtype=torch.int32).to(eng.device))
        same_as_oracle(oracle, eng, oracles, "insert", ("push", c, N, dtype, waves))

    every_width(ob, ref, c, 3, "otw", False, tdt, 1, drive, None, ("push", c, N, dtype))


def test_digital_silence_at_every_width(mods):
    """Tied band minima (tests/silence_inputs.py): np.argmin's first-minimum rule decides nearly every step."""
    oracle, ob, _, _ = mods
    ref, lives = si.silent_pair(2 * 245 + 100, 245, si.otw_seed(245), True)
    for variant, mode in (("livenote_v2", "insert"), ("otw", "set_live")):
        oracles = run_oracles(oracle, ref, lives, 245, 3, variant, mode, True)

        def drive(eng, waves):
            lv, ln = eng.pack(lives)
            eng.run(lv, ln, mode=mode)
            same_as_oracle(oracle, eng, oracles, mode, ("silence", variant, mode, waves))

        every_width(ob, ref, 245, 3, variant, True, torch.float32, 1, drive, torch.float32, ("silence", variant, mode))


def test_what_a_handle_takes_by_itself(mods):
    """Without RTS_OTW_WAVES: the default of otw_plan.h where every stream has a compute unit to itself, 8 waves from
    B = cus + 1 on and on every kernel that has no wide form; a value that is no wave count is refused at create."""
    oracle, ob, synth, nat = mods
    from test_otw_wide_plan_cpu import AUTO_WAVES
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ref = synth.synth_ref(600, 77)
    os.environ.pop("RTS_OTW_WAVES", None)

    def waves_of(B, c=500, dtype=torch.float32, live=torch.float32):
        eng = ob.BatchedOTW(ref, c, 3, batch=B, dtype=dtype)
        try:
            return eng.kernel(live, with_waves=True)["waves"]
        finally:
            eng.close()

    assert [waves_of(B) for B in (1, cus, cus + 1)] == [AUTO_WAVES, AUTO_WAVES, 8]
    assert [waves_of(B, dtype=torch.float64, live=None) for B in (cus, cus + 1)] == [AUTO_WAVES, 8]
    with env(RTS_OTW_WAVES=16):
        assert waves_of(3) == 16 and waves_of(cus + 1) == 16          # the override holds at any batch size ...
        assert waves_of(3, c=244) == 8 and waves_of(3, c=501) == 8     # ... on the kernels that have the form
        assert waves_of(2 * cus) == 8                                  # the residency flavour
        with env(RTS_OTW_SPEC=0):
            assert waves_of(3) == 8
    for bad in ("10", "0", "sixteen", "1024"):
        with env(RTS_OTW_WAVES=bad):
            with pytest.raises(nat.RtsyncError, match="RTS_OTW_WAVES"):
                ob.BatchedOTW(ref, 500, 3, batch=3, dtype=torch.float32)
