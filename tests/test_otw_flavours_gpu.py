"""The float64 no-ring instantiations of the pipelined step kernel at W <= 512 (``LiveFromGlobal``): what a handle takes when
its features are not float32 on both sides and its batch lies strictly between one and two streams per compute unit
(csrc/otw_plan.h) -- every rts_otw_insert / rts_otw_push and every live session of such a batch, whose frames come from the
handle's float64 history.  The tests reach it the way callers do, by batch size: B_lo = cus + 1 and B_hi = 2 cus - 1
streams, K = 16 distinct ones tiled (tests/otw_padded.py), the dense CPU oracle once per distinct stream and all B
streams compared with it bit for bit.  Every test first asserts through ``BatchedOTW.kernel`` that the launch it is about
to make gets ring kind 'none' on the pipelined kernel: on a device or after a change of the rule where it would not, the
test fails instead of passing on another kernel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import otw_padded as op
    n = op.cus()
    if n < 2:
        pytest.skip("a device of %d compute unit(s) has no batch between one and two streams per CU" % n)
    return op, n + 1, 2 * n - 1


# ---- 1. the rule on the device -------------------------------------------------------------------------------------------
def test_the_selection_rule_on_this_device(env):
    op, B_lo, B_hi = env
    cus, c = B_lo - 1, 20
    ref, lives = op.streams16(c, 8100)
    for B, ring in ((cus, "double"), (B_lo, "none"), (B_hi, "none"), (2 * cus, "none-lean")):
        op.check_padded(ref, lives, B, c, 3, "otw", "insert", F64, want=dict(ring=ring, pipelined=True, window=64, fill=True))
    # a float32 reference: the float ring for float32 live input, no ring for what push reads (the float64 history)
    op.check_padded(ref, lives, B_lo, c, 3, "otw", "insert", F32, want=dict(ring="float", pipelined=True))
    op.check_padded(ref, lives, B_lo, c, 3, "otw", "insert", F32, F64, want=op.NO_RING)
    eng = op.ob.BatchedOTW(ref, c, 3, batch=B_lo, dtype=F32)
    try:
        assert eng.kernel(F32)["ring"] == "float"
        op.assert_kernel(eng, None, op.NO_RING)
        lv, ln = eng.pack(op.tile(lives, B_lo))
        eng.push(lv, ln)
        op.same_batch(eng, [op.snapshot(ref, l, c, 3, "otw") for l in lives], "insert", "push")
    finally:
        eng.close()


def test_the_plain_kernel_and_the_refusal_are_reported(env):
    """RTS_OTW_SPEC=0: the plain kernel with its ring whatever the batch; no entry at the wide windows, where
    rts_otw_read_kernel refuses as the launch does (RTS_ERR_UNSUPPORTED = -2).  With a dense mirror attached every launch
    runs the plain kernel and none the band fill."""
    from scoped_env import Env
    op, B_lo, _ = env
    ref, lives = op.streams16(20, 8100)
    with Env(RTS_OTW_SPEC=0):
        plain = op.ob.BatchedOTW(ref, 20, 3, batch=B_lo, dtype=F64)
        wide = op.ob.BatchedOTW(ref, 501, 3, batch=2, dtype=F64)
    mirror = op.ob.BatchedOTW(ref, 20, 3, batch=2, dtype=F64)
    try:
        assert plain.kernel() == dict(window=64, ring="double", pipelined=False, fill=True)
        with pytest.raises(op.nat.RtsyncError, match="rtsync error -2"):
            wide.kernel()
        lv, ln = wide.pack(lives[7:9])
        with pytest.raises(op.nat.RtsyncError, match="rtsync error -2"):
            wide.run(lv, ln)
        assert mirror.kernel() == dict(window=64, ring="double", pipelined=True, fill=True)
        mirror.enable_dense()
        assert mirror.kernel() == dict(window=64, ring="double", pipelined=False, fill=False)
    finally:
        for eng in (plain, wide, mirror):
            eng.close()


# ---- 2. every window, every policy -----------------------------------------------------------------------------------
DD, FD, DF = (F64, F64), (F32, F64), (F64, F32)           # (reference, live) dtypes; none of them float32 on both sides
# c, variant, Euclidean cost, mode, max_run_count, dtypes.  Written out so that each of the four windows (64: c <= 52, 128:
# <= 116, 256: <= 244, 512: <= 500) sees every variant, the Euclidean cost, set_live and max_run_count 1 and 3, and every
# band width all three dtype pairs or the two mixed ones (test_the_rotation_covers_what_it_claims).
ROTATION = [
    (1, "otw", False, "insert", 1, DD), (1, "livenote", False, "set_live", 3, FD),
    (2, "livenote_v2", True, "insert", 3, DF), (2, "otw", False, "set_live", 1, DD),
    (52, "livenote", False, "insert", 3, FD), (52, "livenote_v2", True, "set_live", 1, DF),
    (53, "otw", False, "insert", 1, DD), (53, "livenote", False, "set_live", 3, FD), (53, "livenote_v2", True, "insert", 3, DF),
    (116, "livenote_v2", True, "set_live", 1, DD), (116, "otw", False, "insert", 3, FD), (116, "livenote", False, "insert", 1, DF),
    (117, "livenote", False, "insert", 1, DD), (117, "livenote_v2", True, "insert", 3, FD), (117, "otw", False, "set_live", 3, DF),
    (244, "otw", False, "insert", 3, DD), (244, "livenote_v2", False, "set_live", 1, FD), (244, "livenote", False, "insert", 1, DF),
    (245, "livenote_v2", True, "insert", 1, DD), (245, "otw", False, "set_live", 3, FD), (245, "livenote", False, "insert", 3, DF),
    (500, "otw", False, "insert", 3, DD), (500, "livenote", False, "set_live", 1, FD), (500, "livenote_v2", True, "insert", 1, DF),
]


def _window(c):
    return next(w for last, w in ((52, 64), (116, 128), (244, 256), (500, 512)) if c <= last)


def _rot_id(r):
    return "c%d-%s-%s-%s-mrc%d-%s" % (r[0], r[1], "euclid" if r[2] else "dot", r[3], r[4],
                                      "_".join(str(d).split(".")[-1] for d in r[5]))


def test_the_rotation_covers_what_it_claims():
    assert sorted({r[0] for r in ROTATION}) == [1, 2, 52, 53, 116, 117, 244, 245, 500]
    for W in (64, 128, 256, 512):
        rows = [r for r in ROTATION if _window(r[0]) == W]
        assert {r[1] for r in rows} == {"otw", "livenote", "livenote_v2"}, W
        assert any(r[2] and r[1] == "livenote_v2" for r in rows) and {r[3] for r in rows} == {"insert", "set_live"}, W
        assert {r[4] for r in rows} == {1, 3} and {r[5] for r in rows} == {DD, FD, DF}, W
    assert all(not r[2] or r[1] == "livenote_v2" for r in ROTATION)


@pytest.mark.parametrize("row", ROTATION, ids=_rot_id)
def test_every_window_and_policy_at_one_stream_over_a_cu_each(env, row):
    op, B_lo, _ = env
    c, variant, euclid, mode, mrc, (rdt, ldt) = row
    ref, lives = op.streams16(c, 8200 + c, euclid=euclid)
    op.check_padded(ref, lives, B_lo, c, mrc, variant, mode, rdt, ldt, euclid=euclid,
                    want=dict(op.NO_RING, window=_window(c), fill=c >= 2))


# ---- 3. the upper end ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [100, 500])
def test_one_stream_short_of_two_per_cu(env, c):
    op, _, B_hi = env
    ref, lives = op.streams16(c, 8300 + c)
    op.check_padded(ref, lives, B_hi, c, 3, "otw", "insert", F64, want=dict(op.NO_RING, window=_window(c)))


# ---- 4. the W = 512 hit loop with live frames from global memory -----------------------------------------------------------
@pytest.mark.parametrize("variant", ["otw", "livenote", "livenote_v2"])
@pytest.mark.parametrize("mode", ["insert", "set_live"])
@pytest.mark.parametrize("c", [245, 300])
def test_hit_loop_through_the_fill(env, variant, mode, c):
    """The streams of tests/test_otw_bothloop_gpu.py: one ends inside the fill, one crosses t = c and stops right behind, one
    runs past the reference end."""
    from test_otw_bothloop_gpu import _streams
    op, B_lo, _ = env
    ref, lives = _streams(op.synth, c, 5200 + c + len(variant) + (7 if mode == "set_live" else 0))
    for mrc in (1, 3):
        op.check_padded(ref, lives, B_lo, c, mrc, variant, mode, F64, want=dict(op.NO_RING, window=512))


@pytest.mark.parametrize("mode", ["insert", "set_live"])
@pytest.mark.parametrize("c", [245, 300])
def test_hit_loop_reference_shorter_than_the_band(env, mode, c):
    """The reference ends inside the fill: the stop falls on a Both step with t < c."""
    op, B_lo, _ = env
    ref, lives = op.synth.synth_batch(c - 20, 3, seed=61 + c)
    lives[1] = lives[1][:, : lives[1].shape[1] // 2]
    lives[2] = op.synth._as_f32_values(np.concatenate([lives[2], np.repeat(lives[2][:, -1:], 60, axis=1)], axis=1))
    for variant in ("otw", "livenote_v2"):
        op.check_padded(ref, lives, B_lo, c, 3, variant, mode, F64, want=dict(op.NO_RING, window=512))


@pytest.mark.parametrize("variant", ["otw", "livenote_v2"])
@pytest.mark.parametrize("c", [245, 300])
def test_hit_loop_exact_ties(env, variant, c):
    """synth_tie: exactly equal costs, the three predecessors of a cell tie and the order of the candidates decides."""
    op, B_lo, _ = env
    ref, live = op.synth.synth_tie(2 * c + 100, seed=13)
    lives = [live, live[:, : c - 3].copy(), live[:, : c + 1].copy()]
    for mode in ("insert", "set_live"):
        op.check_padded(ref, lives, B_lo, c, 3, variant, mode, F64, want=dict(op.NO_RING, window=512))


# ---- 5. tied band minima ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["silence", "tie_euclid"])
@pytest.mark.parametrize("c", [245, 500])
def test_tied_band_minima(env, c, kind):
    """Digital silence and repeated frames under the Euclidean cost (tests/test_otw_ties_gpu.py at batch 3): both band
    minima are tied after nearly every insert, and np.argmin's first-minimum rule decides the path."""
    import silence_inputs as si
    op, B_lo, _ = env
    if kind == "silence":
        ref, lives = si.silent_pair(2 * c + 100, c, si.otw_seed(c), True)
    else:
        ref, live = si.tie_euclid(2 * c + 100, 13)
        lives = [live, live[:, : live.shape[1] // 2].copy()]
    for variant, mode in (("livenote_v2", "insert"), ("otw", "set_live")):
        op.check_padded(ref, lives, B_lo, c, 3, variant, mode, F64, euclid=True, want=dict(op.NO_RING, window=512))


# ---- 6. the ingestion paths of a live session ----------------------------------------------------------------------------
def _feed(eng, lives, done, take, dtype):
    """One push of take[b] frames of stream b from position done[b]."""
    buf = np.zeros((eng.B, max(max(take), 1), 12))
    for b, n in enumerate(take):
        if n:
            buf[b, :n] = lives[b][:, done[b]: done[b] + n].T
    eng.push(torch.from_numpy(buf).to(dtype).to(eng.device), torch.tensor(take, dtype=torch.int32).to(eng.device))


@pytest.mark.parametrize("fill", [1, 0])
@pytest.mark.parametrize("c", [52, 245])
def test_ingestion_paths_on_a_float32_reference(env, c, fill):
    """run with float32 lives (float ring); insert for 60 frames, then push; push in uneven per-stream chunks: the last two
    read the float64 history and so run the no-ring kernel on a handle whose own features are float32."""
    from scoped_env import Env
    op, B_lo, _ = env
    ref, k_lives = op.streams16(c, 8600 + c)
    lives = op.tile(k_lives, B_lo)
    lens = [l.shape[1] for l in lives]
    snaps = [op.snapshot(ref, l, c, 3, "otw") for l in k_lives]
    with Env(RTS_OTW_FILL=fill):
        eng = op.ob.BatchedOTW(ref, c, 3, batch=B_lo, dtype=F32)
    try:
        assert eng.kernel(F32) == dict(window=_window(c), ring="float", pipelined=True, fill=bool(fill))
        op.assert_kernel(eng, None, dict(op.NO_RING, window=_window(c), fill=bool(fill)))
        lv, ln = eng.pack(lives)
        eng.run(lv, ln)
        op.same_batch(eng, snaps, "insert", "run")
        assert eng.fill_taken().tolist() == [int(bool(fill) and n >= c) for n in lens]
        run_paths = eng.paths()

        eng.reset()
        dev = eng.device
        for i in range(60):
            frames = np.zeros((B_lo, 12), dtype=np.float32)
            for b, l in enumerate(lives):
                if i < lens[b]:
                    frames[b] = l[:, i]
            eng.insert(torch.from_numpy(frames).to(dev), torch.tensor([int(i < n) for n in lens], dtype=torch.uint8).to(dev))
        done = [min(60, n) for n in lens]
        _feed(eng, lives, done, [n - d for n, d in zip(lens, done)], F32)
        assert not eng.fill_taken().any()                  # no stream was fresh any more
        op.same_batch(eng, snaps, "insert", "insert+push")
        assert all(np.array_equal(p, q) for p, q in zip(eng.paths(), run_paths))

        eng.reset()
        rs = np.random.RandomState(8600 + c)
        done, fresh, filled = [0] * B_lo, [True] * B_lo, [0] * B_lo
        while any(d < n for d, n in zip(done, lens)):
            draw = rs.choice([0, 1, 2, 7, 64, c], size=B_lo)
            draw[3::op.K] = c                                  # the streams of exactly c frames: all at once
            take = [min(int(v), n - d) for v, d, n in zip(draw, done, lens)]
            if not any(take):
                continue
            _feed(eng, lives, done, take, F32)
            # the band fill takes a stream whose first frames are at least c, in a call that can bring that many
            want = [int(bool(fill) and fresh[b] and take[b] >= c) for b in range(B_lo)]
            assert eng.fill_taken().tolist() == want, (c, fill)
            for b, n in enumerate(take):
                done[b] += n
                filled[b] |= want[b]
                fresh[b] = fresh[b] and n == 0
        assert (sum(filled) > 0) == bool(fill) and sum(filled) < B_lo
        op.same_batch(eng, snaps, "insert", "push")
        assert all(np.array_equal(p, q) for p, q in zip(eng.paths(), run_paths))
    finally:
        eng.close()


# ---- 7. per-stream references and restart ----------------------------------------------------------------------------------
def test_per_stream_references_and_restart(env):
    """Four pieces of different lengths (two begin with silence, one is shorter than the band), the Euclidean cost.  After
    half of every stream's frames every seventh stream is restarted, stream 7 onto another piece, and the rest is pushed:
    a restarted stream is a fresh tracker that hears the second half only."""
    import silence_inputs as si
    op, B_lo, _ = env
    c, synth = 245, op.synth
    srefs, slives = si.silent_pieces(c, si.otw_seed(c) + 1)
    short, other = op.as_euclid(synth.synth_ref(c - 20, 8701)), op.as_euclid(synth.synth_ref(c + 60, 8702))
    pieces = [srefs[0], srefs[1], short, other]
    assert len({p.shape[1] for p in pieces}) == 4 and short.shape[1] < c and not srefs[0][:, :c].any()
    k_lives = []
    for k in range(op.K):
        p = k % 4
        if p < 2:
            k_lives.append(slives[(k // 4 + p) % 3])
        else:
            raw = synth.synth_live(synth.synth_ref(pieces[p].shape[1], 8701 + p - 2), 8710 + k)
            k_lives.append(op.as_euclid(np.concatenate([raw, np.repeat(raw[:, -1:], 30 if p == 2 else 0, axis=1)], axis=1)))
    piece_of = [b % 4 for b in range(B_lo)]
    lives = op.tile(k_lives, B_lo)
    lens = [l.shape[1] for l in lives]
    half = [n // 2 for n in lens]
    restarted = list(range(0, B_lo, 7))
    new_piece = {b: piece_of[b] for b in restarted}
    new_piece[7] = 0                                           # from the last piece onto the first silent one
    assert piece_of[7] != new_piece[7]
    eng = op.ob.BatchedOTW.with_references([pieces[p] for p in piece_of], c, 3, variant="livenote_v2", euclid=True, dtype=F64)
    try:
        op.assert_kernel(eng, None, dict(op.NO_RING, window=512))
        _feed(eng, lives, [0] * B_lo, half, F64)
        eng.restart(restarted, refs=[pieces[new_piece[b]] for b in restarted])
        _feed(eng, lives, half, [n - h for n, h in zip(lens, half)], F64)
        states, cache = eng.states(), {}
        for b in range(B_lo):
            key = (b % op.K, new_piece.get(b))
            if key not in cache:
                heard = lives[b][:, half[b]:] if b in new_piece else lives[b]
                cache[key] = op.snapshot(pieces[new_piece.get(b, piece_of[b])], heard, c, 3, "livenote_v2", euclid=True)
            op.same_stream(eng, b, states[b], cache[key], "insert", ("restart", key))
    finally:
        eng.close()


# ---- 8. the soak --------------------------------------------------------------------------------------------------------
def test_soak_reaches_the_no_ring_kernels(env):
    """tests/otw_soak.py, short form: seeded float64 configurations at c <= 500, each tiled up to B_lo streams."""
    import otw_soak
    op, B_lo, _ = env
    assert otw_soak.run(24, seed=41, verbose=False, pad_to=B_lo, max_c=500, f64_only=True, expect=op.NO_RING) >= 24 * B_lo
