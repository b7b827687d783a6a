"""The band fill of a fresh stream as a dense wavefront (otw_bandfill_kernel, csrc/otw_fill.h): while t < c every step is a
Both step, so a stream that is fresh and receives at least c frames in one call has the square [0, c-1] x [0, c-1]
evaluated by that kernel, which leaves state, bands and path as the step loop leaves them after c frames; the step loop
resumes from there.

Every case is held to the dense CPU oracle (``_check`` of tests/test_otw_hitloop_gpu.py: path, end state, bands) and, bit
for bit, to a second handle created under RTS_OTW_FILL=0, which runs the step loop alone: the state words, both bands
(bytes, so NaN payloads and signed zeros count) and the path.  The diagnostic word 15 depends on where launches begin
(``_same_handles``): it is compared, with all the others, against a step-loop handle launched at the same frames.  ``rts_otw_read_fill`` says per stream whether the kernel
filled its band, and the tests assert it for every stream: a case that silently fell back to the step loop fails.

Shapes are the smallest at which the kernel can go wrong: c = 2 (three stages), 5, 63 / 64 / 65 (one wave, its last lane,
the lane-63 -> lane-0 hand-over), 129 (two hand-overs) and 500 once (the largest band, all eight waves)."""

import numpy as np
import pytest

import silence_inputs as si
from guarded import guarded, same_bytes
from scoped_env import Env
from test_otw_hitloop_gpu import _check, mods  # noqa: F401  (mods: the module fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
VARIANTS = ["otw", "livenote", "livenote_v2"]
MODES = ["insert", "set_live"]


def _pair(make):
    """The same handle twice: with the fill kernel (RTS_OTW_FILL is read at create) and with the step loop alone."""
    with Env(RTS_OTW_FILL=1):
        on = make()
    with Env(RTS_OTW_FILL=0):
        off = make()
    return on, off


def _same_handles(on, off, tag, all_words=False):
    """Every stream of the two handles, bit for bit: the state words (14 is kernel-private and read as 0), both bands, the
    path.  Word 15, RTS_ST_BAND_RECOMPUTES, is a diagnostic that depends on where launches begin: a Both step with a full
    band counts a reduction when it runs as a hit whose speculated argmin lies outside its window (otw_settle_hit_both)
    and none when it runs as a regular step, and the first step of a launch is always a regular one.  So rts_otw_run and
    the same frames through rts_otw_push differ in it, and so does a run that resumes at the hand-over.  It is compared
    (``all_words``) where the other handle's launches begin at the same frames -- ``_segmented`` -- and left out
    otherwise."""
    s_on, s_off = on.states(), off.states()
    if not all_words:
        s_on[:, 15] = s_off[:, 15] = 0
    assert np.array_equal(s_on, s_off), (tag, s_on, s_off)
    for b in range(on.B):
        assert np.array_equal(on.path(b), off.path(b)), (tag, b)
        for x, y in zip(on.bands(b), off.bands(b)):
            assert same_bytes(x, y), (tag, b)


def _segmented(make, lv, lens, took, c):
    """A step-loop handle (RTS_OTW_FILL=0) whose launches begin where the fill handle's kernels do: the packed frames
    ``lv`` through rts_otw_push, c frames first for the streams that took the fill (everything for the others), then the
    rest.  Insert mode only (push is the insert loop)."""
    with Env(RTS_OTW_FILL=0):
        seg = make()
    first = [c if t else n for t, n in zip(took, lens)]
    for lo, hi in (([0] * len(lens), first), (first, lens)):
        counts = [h - l for l, h in zip(lo, hi)]
        if max(counts) == 0:
            continue
        buf = torch.zeros((len(lens), max(counts), 12), dtype=torch.float64, device=lv.device)
        for b in range(len(lens)):
            buf[b, : counts[b]] = lv[b, lo[b]: hi[b]].double()
        seg.push(buf, torch.tensor(counts, dtype=torch.int32).to(lv.device))
    return seg


def _expect(lens, ref_lens, c, mode):
    """Eligibility as the header states it, for fresh streams of a handle without a dense mirror."""
    need = c + (1 if mode == "set_live" else 0)
    return [int(c <= 500 and n >= need and nr >= c) for n, nr in zip(lens, ref_lens)]


def _ab(oracle, ob, ref, lives, c, mrc, variant, mode, dtype, euclid=False, expect=None, with_oracle=True):
    """Oracle comparison on a default handle, then the FILL=1 / FILL=0 pair; -> the streams that took the fill."""
    if with_oracle:
        _check(oracle, ob, ref, lives, c, mrc, variant, mode, dtype, euclid=euclid)
    def make():
        return ob.BatchedOTW(ref, c, mrc, batch=len(lives), variant=variant, euclid=euclid, dtype=dtype)

    on, off = _pair(make)
    lv, ln = on.pack(lives, dtype=dtype)
    on.run(lv, ln, mode=mode)
    off.run(lv, ln, mode=mode)
    tag = (variant, mode, c, mrc, str(dtype), euclid)
    _same_handles(on, off, tag)
    took = on.fill_taken().tolist()
    assert off.fill_taken().tolist() == [0] * len(lives), tag
    if expect is None:
        expect = _expect([l.shape[1] for l in lives], [ref.shape[1]] * len(lives), c, mode)
    assert took == expect, (tag, took, expect)
    if mode == "insert":   # all 16 words against the step loop launched at the same frames
        seg = _segmented(make, lv, [l.shape[1] for l in lives], took, c)
        _same_handles(on, seg, (tag, "segmented"), all_words=True)
        seg.close()
    if with_oracle:   # the step-loop handle against the oracle as well: the pair is compared on the oracle's own path
        vmap = {"otw": oracle.OTW, "livenote": oracle.LIVENOTE, "livenote_v2": oracle.LIVENOTE_V2}
        for b, live in enumerate(lives):
            o = oracle.OtwOracle(ref, c, mrc, vmap[variant], oracle.COST_EUCLID if euclid else oracle.COST_DOT)
            (o.set_live if mode == "set_live" else o.run)(live)
            assert np.array_equal(off.path(b), o.path), (tag, b)
    on.close()
    off.close()
    return took


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", [2, 5, 63, 64, 65, 129])
def test_small_bands_every_policy(mods, c, mode, variant):
    """Reference of 2c + 40 frames, streams of c + 6 frames; float32 and float64 features."""
    oracle, ob, synth = mods
    ref, lives = synth.synth_batch(2 * c + 40, 2, seed=6100 + c + len(variant) + (7 if mode == "set_live" else 0))
    lives = [l[:, : c + 6].copy() for l in lives]
    for mrc, dtype in ((3, torch.float32), (1, torch.float64)):
        took = _ab(oracle, ob, ref, lives, c, mrc, variant, mode, dtype)
        assert took == [1, 1]


def test_the_largest_band(mods):
    """c = 500: all eight waves, seven hand-overs."""
    oracle, ob, synth = mods
    c = 500
    ref, lives = synth.synth_batch(2 * c + 40, 3, seed=6500)
    lives = [l[:, : c + 3].copy() for l in lives]
    assert _ab(oracle, ob, ref, lives, c, 3, "otw", "insert", torch.float32) == [1, 1, 1]


def test_the_first_band_of_the_wide_window_is_never_filled(mods):
    """c = 501 runs on the 1024-cell window: the step loop alone."""
    oracle, ob, synth = mods
    c = 501
    ref, lives = synth.synth_batch(2 * c + 40, 2, seed=6501)
    lives = [l[:, : c + 3].copy() for l in lives]
    assert _ab(oracle, ob, ref, lives, c, 3, "otw", "insert", torch.float32) == [0, 0]


@pytest.mark.parametrize("mode", MODES)
def test_live_length_edges_in_one_batch(mods, mode):
    """c = 65, streams of c-1, c, c+1 and 0 frames: the first and the last keep the step loop; the second ends exactly at
    the hand-over (insert; set_live leaves t one past the last frame there, which the step loop does); the third hands
    one frame over."""
    oracle, ob, synth = mods
    c = 65
    ref, lives = synth.synth_batch(2 * c + 40, 4, seed=6600)
    lives = [lives[0][:, : c - 1].copy(), lives[1][:, :c].copy(), lives[2][:, : c + 1].copy(), lives[3][:, :0].copy()]
    want = [0, 1, 1, 0] if mode == "insert" else [0, 0, 1, 0]
    for variant in VARIANTS:
        # (the oracle has no stream of zero frames to compare: the pair's bit-for-bit comparison covers it)
        _check(oracle, ob, ref, lives[:3], c, 3, variant, mode, torch.float64)
        assert _ab(oracle, ob, ref, lives, c, 3, variant, mode, torch.float64, with_oracle=False) == want


def test_the_hand_over_state_is_the_oracles_after_c_frames(mods):
    """A stream of exactly c frames: what the fill kernel alone leaves is the oracle after c inserts."""
    oracle, ob, synth = mods
    c = 65
    ref, lives = synth.synth_batch(2 * c + 40, 1, seed=6601)
    live = lives[0][:, :c].copy()
    with Env(RTS_OTW_FILL=1):
        eng = ob.BatchedOTW(ref, c, 3, batch=1, dtype=torch.float64)
    lv, ln = eng.pack([live])
    eng.run(lv, ln)
    assert eng.fill_taken().tolist() == [1]
    o = oracle.OtwOracle(ref, c, 3)
    o.run(live)
    st, so, cnt = eng.state(0), o.state, o.counters
    assert (st["t"], st["j"]) == (c - 1, c - 1) == (so["t"], so["j"])
    for key in ("direction", "previous", "run_count", "status"):
        assert st[key] == so[key], key
    assert (st["cells"], st["row_strips"], st["col_strips"]) == (cnt["cells"], cnt["row_strips"], cnt["col_strips"])
    assert st["cells"] == c * c and st["consumed"] == c and st["n_path"] == c - 1 and st["first_insert"] == 0
    assert np.array_equal(eng.path(0), o.path)
    for x, y in zip(eng.bands(0), o.bands()):
        assert np.array_equal(x, y, equal_nan=True)
    eng.close()


@pytest.mark.parametrize("mode", MODES)
def test_reference_length_edges(mods, mode):
    """Per-stream references of c-1 (stops inside the fill: step loop), c (filled; the very next step stops at the
    reference's end) and 2c frames."""
    oracle, ob, synth = mods
    c = 65
    ref, lives = synth.synth_batch(2 * c, 3, seed=6700)
    refs = [ref[:, : c - 1].copy(), ref[:, :c].copy(), ref]
    lives = [l[:, : c + 6].copy() for l in lives]
    for variant in ("otw", "livenote_v2"):
        on, off = _pair(lambda: ob.BatchedOTW.with_references(refs, c, 3, variant=variant, dtype=torch.float64))
        lv, ln = on.pack(lives)
        on.run(lv, ln, mode=mode)
        off.run(lv, ln, mode=mode)
        _same_handles(on, off, (variant, mode))
        assert on.fill_taken().tolist() == [0, 1, 1] and off.fill_taken().tolist() == [0, 0, 0]
        for b in range(3):
            o = oracle.OtwOracle(refs[b], c, 3, si.VARIANTS[variant])
            (o.set_live if mode == "set_live" else o.run)(lives[b])
            for eng in (on, off):
                st, so = eng.state(b), o.state
                assert np.array_equal(eng.path(b), o.path), (variant, mode, b)
                for key in ("t", "j", "previous", "run_count", "status"):
                    assert st[key] == so[key], (variant, mode, b, key)
        assert on.state(0)["status"] != oracle.RUNNING and on.state(1)["status"] != oracle.RUNNING  # both stopped
        on.close()
        off.close()


def _silenced(ref, live, c):
    ref, live = ref.copy(), live.copy()
    for f in (0, 63, 64, c - 1):
        ref[:, f] = 0.0
        live[:, f] = 0.0
    return ref, live


@pytest.mark.parametrize("variant", ["otw", "livenote_v2"])
@pytest.mark.parametrize("mode", MODES)
def test_ties_and_silence_inside_the_square(mods, variant, mode):
    """c = 65.  synth_tie: the three predecessors of a cell tie.  All-zero frames 0, 63, 64 and c-1 of the live stream and of
    the reference: cost exactly 1.0 along whole rows and columns under the dot cost, exactly 0 where two of them meet under
    the Euclidean cost, so band minima tie and np.argmin's first-minimum rule and ``rmin < cmin`` decide (as in
    tests/test_otw_ties_gpu.py; OTW costs are never NaN on finite features).  A whole silent opening (silent_pair) ties
    every band minimum of the square."""
    oracle, ob, synth = mods
    c = 65
    ref, live = synth.synth_tie(2 * c + 40, seed=13)
    _ab(oracle, ob, ref, [live[:, : c + 6].copy(), live[:, : c + 1].copy()], c, 3, variant, mode, torch.float64)
    ref, live = si.tie_euclid(2 * c + 40, 13)
    _ab(oracle, ob, ref, [live[:, : c + 6].copy()], c, 3, variant, mode, torch.float64, euclid=True)
    ref, lives = synth.synth_batch(2 * c + 40, 1, seed=6800)
    ref, live = _silenced(ref, lives[0][:, : c + 6], c)
    _ab(oracle, ob, ref, [live], c, 3, variant, mode, torch.float32)
    refe, livee = _silenced(synth._as_f32_values(np.abs(ref - 0.2)), synth._as_f32_values(np.abs(live - 0.2)), c)
    _ab(oracle, ob, refe, [livee], c, 3, variant, mode, torch.float64, euclid=True)
    ref, lives = si.silent_pair(2 * c + 100, c, si.otw_seed(c), True)
    _ab(oracle, ob, ref, lives, c, 3, variant, mode, torch.float32, euclid=True)


@pytest.mark.parametrize("mode", MODES)
def test_nan_features_spread_as_in_the_step_loop(mods, mode):
    """NaN chroma (no oracle: OTW has no defined NaN behaviour): the cell expression and the argmins are the step
    loop's own instructions and comparisons, so both handles hold the same bits."""
    oracle, ob, synth = mods
    c = 65
    ref, lives = synth.synth_batch(2 * c + 40, 2, seed=6900)
    lives = [l[:, : c + 6].copy() for l in lives]
    ref = ref.copy()
    ref[:, 10] = np.nan
    lives[0][:, [3, 64]] = np.nan
    lives[1][5, 20] = np.nan
    for variant in ("otw", "livenote_v2"):
        assert _ab(oracle, ob, ref, lives, c, 3, variant, mode, torch.float64, with_oracle=False) == [1, 1]


def test_push_catches_a_restarted_stream_up(mods):
    """A running batch, one stream restarted: c + 4 frames pushed to it in one call fill its band, the others (no new
    frames) are left alone; five more frames, one per call, never launch the kernel."""
    oracle, ob, synth = mods
    c = 65
    ref, lives = synth.synth_batch(2 * c + 40, 3, seed=7000)
    on, off = _pair(lambda: ob.BatchedOTW(ref, c, 3, batch=3, dtype=torch.float64))
    dev = on.device

    def push(frames, counts):
        buf = np.zeros((3, max(counts), 12))
        for b, f in enumerate(frames):
            buf[b, : counts[b]] = f.T
        for eng in (on, off):
            eng.push(torch.from_numpy(buf).to(dev), torch.tensor(counts, dtype=torch.int32).to(dev))

    push([l[:, :10] for l in lives], [10, 10, 10])
    assert on.fill_taken().tolist() == [0, 0, 0]          # 10 < c: not launched
    on.restart([1])
    off.restart([1])
    again = lives[1][:, 30: 30 + c + 9]                    # the restarted stream hears another part of the piece
    push([lives[0][:, :0], again[:, : c + 4], lives[2][:, :0]], [0, c + 4, 0])
    assert on.fill_taken().tolist() == [0, 1, 0] and off.fill_taken().tolist() == [0, 0, 0]
    _same_handles(on, off, "catch-up")
    for i in range(5):
        push([lives[0][:, 10 + i: 11 + i], again[:, c + 4 + i: c + 5 + i], lives[2][:, 10 + i: 11 + i]], [1, 1, 1])
        assert on.fill_taken().tolist() == [0, 0, 0]
    _same_handles(on, off, "one by one")
    heard = [lives[0][:, :15], again, lives[2][:, :15]]
    for b in range(3):
        o = oracle.OtwOracle(ref, c, 3)
        o.run(heard[b])
        st, so = on.state(b), o.state
        assert np.array_equal(on.path(b), o.path), b
        for key in ("t", "j", "direction", "previous", "run_count", "status"):
            assert st[key] == so[key], (b, key)
        for x, y in zip(on.bands(b), o.bands()):
            assert np.array_equal(x, y, equal_nan=True), b
    on.close()
    off.close()


@pytest.mark.parametrize("fill", [0x00, 0xFF, 0x55])
def test_caller_owned_memory_is_only_read(mods, fill):
    """The caller's live frames [B][T][12] and lengths [B] between guards (tests/guarded.py), the last stream as long as
    the buffer so that its last frame is the buffer's last 48 bytes: no guard byte and no frame changes.  The handle's own
    state, bands and paths cannot be bracketed from outside; every stream of them, the last one included, is compared
    with the step-loop handle instead."""
    oracle, ob, synth = mods
    c = 65
    ref, lives = synth.synth_batch(2 * c + 40, 3, seed=7100)
    lives = [lives[0][:, : c + 2].copy(), lives[1][:, : c - 3].copy(), lives[2][:, : c + 6].copy()]
    on, off = _pair(lambda: ob.BatchedOTW(ref, c, 3, batch=3, dtype=torch.float32))
    lv0, ln0 = on.pack(lives)
    lv, check_lv = guarded(tuple(lv0.shape), torch.float32, DEV, fill)
    ln, check_ln = guarded((3,), torch.int32, DEV, fill)
    lv.copy_(lv0)
    ln.copy_(ln0)
    on.run(lv, ln)
    torch.cuda.synchronize()
    check_lv("live frames")
    check_ln("live lengths")
    assert torch.equal(lv, lv0) and torch.equal(ln, ln0)
    assert on.fill_taken().tolist() == [1, 0, 1]
    off.run(lv0, ln0)
    _same_handles(on, off, fill)
    on.close()
    off.close()
