"""Wave 0's hit-step loop of the pipelined W = 512 kernel (csrc/otw.hip) after its restructuring: the step kind comes
from the plan instead of being decoded from its flags, the speculated strip's first position from the plan instead of
LDS, and decide() / the next plan sit behind each kind's settle.  What such a loop can get wrong is where it leaves and
re-enters, where a launch stops inside it, and the words it hands back: every case here is compared bit for bit with the
dense CPU oracle (path, end state, counters, both bands in insert mode), and with the plain kernel (RTS_OTW_SPEC=0),
which has no hit-step loop, for the words the oracle does not keep.

Streams (reference of 2c + 60 frames, c = 245 -- the smallest band on the 512-cell window -- and c = 500):
  0  dwells: a run of repeated live frames, so that Row-only runs make the column band's kept minimum slide out of its
     window (RTS_ST_BAND_RECOMPUTES > 0: the loop hands that step to the general loop and comes back);
  1  runs past the reference end (stop at the reference end; in set_live to the end of its frames);
  2  runs out of live frames inside the loop, with the band full."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

from test_otw_bothloop_gpu import _full_band_both_steps

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VMAP = {"otw": "OTW", "livenote": "LIVENOTE", "livenote_v2": "LIVENOTE_V2"}
WORD_BAND_RECOMPUTES = 15   # launch-dependent: left out of every state comparison


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


_STREAMS = {}


def streams(synth, c):
    """-> (ref (12, 2c + 60), [dwelling, past the reference end, cut inside the loop]); made once per band width."""
    if c not in _STREAMS:
        N = 2 * c + 60
        ref, lives = synth.synth_batch(N, 3, seed=9100 + c)
        at = c + 30   # the dwell starts with the band full and lasts longer than the band is wide
        lives[0] = np.concatenate([lives[0][:, :at], np.repeat(lives[0][:, at:at + 1], c + 50, axis=1), lives[0][:, at:]], axis=1)
        lives[0] = synth._as_f32_values(lives[0][:, : 2 * N - 8])
        lives[1] = synth._as_f32_values(np.concatenate([lives[1], np.repeat(lives[1][:, -1:], 40, axis=1)], axis=1))
        lives[2] = lives[2][:, : c + 137].copy()
        _STREAMS[c] = (ref, lives)
    return _STREAMS[c]


_ORACLES = {}


def oracles(oracle, ref, lives, c, mrc, variant, mode, key):
    """The oracle's end state per stream, computed once per configuration and shared by the tests that need it."""
    k = (key, c, mrc, variant, mode)
    if k not in _ORACLES:
        out = []
        for live in lives:
            o = oracle.OtwOracle(ref, c, mrc, getattr(oracle, VMAP[variant]))
            consumed = (o.set_live if mode == "set_live" else o.run)(live)
            out.append(dict(path=o.path, state=o.state, counters=o.counters, bands=o.bands(), consumed=consumed))
        _ORACLES[k] = out
    return _ORACLES[k]


def same_as_oracle(eng, want, mode, tag):
    for b, o in enumerate(want):
        st, so = eng.state(b), o["state"]
        assert np.array_equal(eng.path(b), o["path"]), (tag, b, "path")
        for key in ("t", "j", "previous", "run_count", "status"):
            assert st[key] == so[key], (tag, b, key)
        assert st["n_path"] == len(o["path"]) and st["path_truncated"] == 0, (tag, b, "n_path")
        if mode == "insert":
            assert st["direction"] == so["direction"], (tag, b)
            cnt = o["counters"]
            got = (st["cells"], st["row_strips"], st["col_strips"], st["consumed"])
            assert got == (cnt["cells"], cnt["row_strips"], cnt["col_strips"], o["consumed"]), (tag, b, "counters")
            rb, cb = eng.bands(b)
            assert np.array_equal(rb, o["bands"][0], equal_nan=True) and np.array_equal(cb, o["bands"][1], equal_nan=True), (tag, b)


def snapshot(eng, B):
    st = eng.states()
    return dict(paths=[eng.path(b) for b in range(B)], bands=[eng.bands(b) for b in range(B)],
                state=np.delete(st, WORD_BAND_RECOMPUTES, axis=1))


def same_snapshot(a, b, tag):
    assert np.array_equal(a["state"], b["state"]), (tag, "state", a["state"], b["state"])
    for p, q in zip(a["paths"], b["paths"]):
        assert np.array_equal(p, q), (tag, "path")
    for (r0, c0), (r1, c1) in zip(a["bands"], b["bands"]):
        assert np.array_equal(r0.view(np.int64), r1.view(np.int64)) and np.array_equal(c0.view(np.int64), c1.view(np.int64)), (tag, "bands")


def make(ob, ref, c, mrc, variant, tdt, kernel_dtype, waves=None, spec=1):
    kw = dict(RTS_OTW_SPEC=spec)
    if waves:
        kw["RTS_OTW_WAVES"] = waves
    with env(**kw):
        eng = ob.BatchedOTW(ref, c, mrc, batch=3, variant=variant, dtype=tdt)
    got = eng.kernel(kernel_dtype, with_waves=True)
    assert got["window"] == 512 and got["pipelined"] == bool(spec), got
    if waves and spec:
        assert got["waves"] == waves, got
    return eng


# ---- every policy copy, every exit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["otw", "livenote", "livenote_v2"])
@pytest.mark.parametrize("mode", ["insert", "set_live"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("c", [245, 500])
def test_every_policy_against_the_oracle(mods, c, dtype, mode, variant):
    oracle, ob, synth, _ = mods
    ref, lives = streams(synth, c)
    tdt = torch.float32 if dtype == "f32" else torch.float64
    for mrc in (1, 3):
        want = oracles(oracle, ref, lives, c, mrc, variant, mode, "main")
        eng = make(ob, ref, c, mrc, variant, tdt, tdt)
        try:
            lv, ln = eng.pack(lives, dtype=tdt)
            eng.run(lv, ln, mode=mode)
            same_as_oracle(eng, want, mode, (c, dtype, mode, variant, mrc))
            st = [eng.state(b) for b in range(3)]
        finally:
            eng.close()
        # the exits are taken: the dwelling stream's kept minimum slid out (a step handed to the general loop in the middle
        # of a run of hits), stream 1 stopped at the reference end, stream 2 ran out of frames with the band full
        if mrc == 3:
            assert st[0]["band_recomputes"] > 0, (c, dtype, mode, variant, st[0])
        assert st[1]["status"] == oracle.STOP_REF_END or mode == "set_live", st[1]
        assert st[2]["status"] == 0 and st[2]["t"] >= c, st[2]


@pytest.mark.parametrize("waves", [8, 12, 16])
@pytest.mark.parametrize("variant", ["otw", "livenote_v2"])
@pytest.mark.parametrize("mode", ["insert", "set_live"])
def test_every_width_at_the_smallest_band(mods, mode, variant, waves):
    oracle, ob, synth, _ = mods
    c = 245
    ref, lives = streams(synth, c)
    for mrc, tdt in ((3, torch.float32), (1, torch.float64)):
        want = oracles(oracle, ref, lives, c, mrc, variant, mode, "main")
        eng = make(ob, ref, c, mrc, variant, tdt, tdt, waves=waves)   # asserts the width that runs
        try:
            lv, ln = eng.pack(lives, dtype=tdt)
            eng.run(lv, ln, mode=mode)
            same_as_oracle(eng, want, mode, (waves, mode, variant, mrc))
        finally:
            eng.close()


# ---- Both steps with a full band, both outcomes of the column speculation's flag ------------------------------------------
@pytest.fixture(scope="module")
def hit_if_streams(mods):
    """As tests/test_otw_bothloop_gpu.py builds its own: plain renditions, whose full-band Both steps find the flag set in
    most cases and clear in some (counted from the oracle's dense matrices)."""
    oracle, ob, synth, _ = mods
    c = 245
    ref, lives = synth.synth_batch(2 * c + 60, 3, seed=77)
    counts = [_full_band_both_steps(oracle, ref, l, c, 3) for l in lives]
    return c, ref, lives, counts


def test_hit_if_inputs_have_both_outcomes(hit_if_streams):
    _, _, _, counts = hit_if_streams
    assert sum(n_set for _, n_set, _ in counts) > 0 and sum(n_clear for _, _, n_clear in counts) > 0, counts


@pytest.mark.parametrize("variant", ["otw", "livenote", "livenote_v2"])
@pytest.mark.parametrize("mode", ["insert", "set_live"])
def test_hit_if_both_outcomes(mods, hit_if_streams, variant, mode):
    oracle, ob, synth, _ = mods
    c, ref, lives, _ = hit_if_streams
    for mrc, tdt in ((3, torch.float32), (1, torch.float64)):
        want = oracles(oracle, ref, lives, c, mrc, variant, mode, "hit_if")
        eng = make(ob, ref, c, mrc, variant, tdt, tdt)
        try:
            lv, ln = eng.pack(lives, dtype=tdt)
            eng.run(lv, ln, mode=mode)
            same_as_oracle(eng, want, mode, ("hit_if", mode, variant, mrc))
        finally:
            eng.close()


# ---- resumption at arbitrary steps ---------------------------------------------------------------------------------------
def push_in_pieces(eng, lives, first, piece):
    dev = eng.device
    lens = [l.shape[1] for l in lives]
    pos = 0
    while pos < max(lens):
        n = first if pos == 0 else piece
        buf = torch.zeros((3, n, 12), dtype=torch.float64)
        cnt = []
        for b, l in enumerate(lives):
            k = max(0, min(n, lens[b] - pos))
            buf[b, :k] = torch.from_numpy(np.ascontiguousarray(l[:, pos:pos + k].T))
            cnt.append(k)
        eng.push(buf.to(dev), torch.tensor(cnt, dtype=torch.int32, device=dev))
        pos += n


@pytest.mark.parametrize("piece", [1, 7, 64])
@pytest.mark.parametrize("variant", ["otw", "livenote_v2"])
def test_push_in_pieces_equals_one_run(mods, variant, piece):
    """The loop is left at the end of every launch and entered again by the next: after a first piece of c + 3 frames the
    same streams in pieces of 1, 7 and 64 frames leave every word but the launch-dependent one, the path and both bands as
    one rts_otw_run does (and that as the oracle)."""
    oracle, ob, synth, _ = mods
    c = 245
    ref, lives = streams(synth, c)
    want = oracles(oracle, ref, lives, c, 3, variant, "insert", "main")
    one = make(ob, ref, c, 3, variant, torch.float64, torch.float64)
    try:
        lv, ln = one.pack(lives, dtype=torch.float64)
        one.run(lv, ln, mode="insert")
        same_as_oracle(one, want, "insert", ("run", variant))
        snap_run = snapshot(one, 3)
    finally:
        one.close()
    eng = make(ob, ref, c, 3, variant, torch.float64, None)
    try:
        push_in_pieces(eng, lives, c + 3, piece)
        same_snapshot(snap_run, snapshot(eng, 3), ("pieces", variant, piece))
    finally:
        eng.close()


# ---- the words the oracle does not keep: against the plain kernel ------------------------------------------------------------
@pytest.mark.parametrize("variant", ["otw", "livenote", "livenote_v2"])
@pytest.mark.parametrize("mode", ["insert", "set_live"])
@pytest.mark.parametrize("c", [245, 500])
def test_state_words_equal_the_plain_kernel(mods, c, mode, variant):
    """RTS_ST_ROW_STRIPS, COL_STRIPS, CONSUMED, CELLS_HI / LO and N_PATH (all sixteen words but the launch-dependent one) of
    the pipelined kernel against the plain one, which has no hit-step loop; set_live included, where the oracle counts
    nothing."""
    oracle, ob, synth, _ = mods
    ref, lives = streams(synth, c)
    snaps = []
    for spec in (1, 0):
        eng = make(ob, ref, c, 3, variant, torch.float32, torch.float32, spec=spec)
        try:
            lv, ln = eng.pack(lives, dtype=torch.float32)
            eng.run(lv, ln, mode=mode)
            snaps.append(snapshot(eng, 3))
        finally:
            eng.close()
    same_snapshot(snaps[0], snaps[1], (c, mode, variant))


def _views(nat, eng):
    """The handle's device views: (path buffer [B][capacity][2] int32, capacity, state words [B][16] int32)."""
    path_dev, state_dev, cap = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int32()
    nat.check(nat.lib.rts_otw_device_views(eng._h, ctypes.byref(path_dev), ctypes.byref(cap), ctypes.byref(state_dev)))
    torch.cuda.synchronize(eng.device)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return hip, path_dev.value, cap.value, state_dev.value


def _poke_n_path(nat, eng, b, back):
    """Set stream b's RTS_ST_N_PATH to `back` points below the path capacity, through the handle's device view of its state
    words (the capacity, 3 N + 8, bounds the tracker's decisions: no input reaches it).  -> the capacity."""
    hip, _, cap, state_dev = _views(nat, eng)
    word = ctypes.c_int32(cap - back)
    assert hip.hipMemcpy(state_dev + 4 * (b * nat.STATE_LEN + nat.ST_N_PATH), ctypes.byref(word), 4, 1) == 0   # host to device
    return cap


def _path_slot_tail(nat, eng, b, back):
    """The last `back` pairs of stream b's path slot (rts_otw_read_path hands out n_path pairs, which is past the slot here)."""
    hip, path_dev, cap, _ = _views(nat, eng)
    out = np.empty((back, 2), dtype=np.int32)
    assert hip.hipMemcpy(out.ctypes.data, path_dev + 8 * (b * cap + cap - back), 8 * back, 2) == 0   # device to host
    return out


@pytest.mark.parametrize("variant", ["otw", "livenote_v2"])
def test_path_capacity_reached_inside_the_loop(mods, variant):
    """A path that reaches its capacity while the loop runs: the truncation flag is set, nothing is stored past the last
    slot and n_path counts on, as in the plain kernel.  Both handles get the same first piece, then stream 1's n_path is set
    25 points below the capacity, then the rest."""
    oracle, ob, synth, nat = mods
    c, back = 245, 25
    ref, lives = streams(synth, c)
    got = []
    for spec in (1, 0):
        eng = make(ob, ref, c, 3, variant, torch.float64, None, spec=spec)
        try:
            first = [l[:, : c + 3] for l in lives]
            rest = [l[:, c + 3:] for l in lives]
            push_in_pieces(eng, first, c + 3, 64)
            cap = _poke_n_path(nat, eng, 1, back)
            push_in_pieces(eng, rest, max(l.shape[1] for l in rest), 64)
            st = eng.states()
            got.append((np.delete(st, WORD_BAND_RECOMPUTES, axis=1), _path_slot_tail(nat, eng, 1, back), eng.path(0), eng.path(2)))
            s1 = eng.state(1)
            assert s1["path_truncated"] == 1 and s1["n_path"] > cap, (variant, spec, s1, cap)
            assert eng.state(0)["path_truncated"] == 0 and eng.state(2)["path_truncated"] == 0
        finally:
            eng.close()
    assert np.array_equal(got[0][0], got[1][0]), (variant, "state")
    for a, b in zip(got[0][1:], got[1][1:]):
        assert np.array_equal(a, b), (variant, "path")
