"""rts_otw_restart / rts_wtw_restart (BatchedOTW.restart, BatchedWTW.restart): single streams of a batched handle go back
to the start -- optionally onto another range of the reference pool -- while the others keep running.

Three-way equality, everything compared with ==: streams that were not restarted equal a control handle that saw the
same pushes and no restart; restarted streams equal a fresh single-stream handle fed only what came after the restart,
and the CPU oracle on those frames."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CHUNKS = (7, 23, 1, 40, 13, 64)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class Feeder:
    """Pushes per-stream sequences ((12, T_b) arrays) into handles in uneven chunks with per-stream counts, and remembers
    the counts, so that a stream's pushes can be repeated on a handle of its own."""

    def __init__(self, seqs, tdt, chunks=CHUNKS):
        self.seqs, self.tdt, self.chunks = list(seqs), tdt, chunks
        self.pos = [0] * len(seqs)
        self.log = [[] for _ in seqs]
        self.k = 0

    def done(self):
        return all(p >= s.shape[1] for p, s in zip(self.pos, self.seqs))

    def _buf(self, counts, chunk, seqs, pos):
        buf = np.zeros((len(seqs), chunk, 12))
        for b, n in enumerate(counts):
            buf[b, :n] = seqs[b][:, pos[b]:pos[b] + n].T
        return (torch.from_numpy(buf).to(self.tdt).to("cuda:0"),
                torch.tensor(counts, dtype=torch.int32, device="cuda:0"))

    def round(self, engines):
        chunk = self.chunks[self.k % len(self.chunks)]
        self.k += 1
        counts = [max(0, min(chunk - (b % 3), s.shape[1] - p)) for b, (p, s) in enumerate(zip(self.pos, self.seqs))]
        buf, n_new = self._buf(counts, chunk, self.seqs, self.pos)
        for e in engines:
            e.push(buf, n_new)
        for b, n in enumerate(counts):
            self.pos[b] += n
            self.log[b].append((chunk, n))

    def new_sequence(self, b, seq):
        self.seqs[b], self.pos[b], self.log[b] = seq, 0, []

    def repeat_on(self, b, engine):
        """Stream b's pushes since its last new_sequence, on a one-stream handle."""
        p = 0
        for chunk, n in self.log[b]:
            buf, n_new = self._buf([n], chunk, [self.seqs[b]], [p])
            engine.push(buf, n_new)
            p += n


def _same_stream(a, ba, b, bb, tag, bands=True):
    assert np.array_equal(a.states()[ba], b.states()[bb]), (tag, "state")
    assert np.array_equal(a.path(ba), b.path(bb)), (tag, "path")
    if bands:
        ra, ca = a.bands(ba)
        rb, cb = b.bands(bb)
        assert np.array_equal(ra, rb, equal_nan=True) and np.array_equal(ca, cb, equal_nan=True), (tag, "bands")


def _otw_vs_oracle(eng, b, ref, live, c, variant, euclid, tag):
    import oracle
    vmap = {"otw": oracle.OTW, "livenote": oracle.LIVENOTE, "livenote_v2": oracle.LIVENOTE_V2}
    o = oracle.OtwOracle(ref, c, 3, vmap[variant], oracle.COST_EUCLID if euclid else oracle.COST_DOT)
    n = o.run(live)
    st, so = eng.state(b), o.state
    assert np.array_equal(eng.path(b), o.path), (tag, "oracle path")
    for k in ("t", "j", "direction", "previous", "run_count", "status"):
        assert st[k] == so[k], (tag, k, st[k], so[k])
    assert st["consumed"] == n, tag
    cnt = o.counters
    assert (st["cells"], st["row_strips"], st["col_strips"]) == (cnt["cells"], cnt["row_strips"], cnt["col_strips"]), tag
    rb, cb = eng.bands(b)
    orb, ocb = o.bands()
    assert np.array_equal(rb, orb, equal_nan=True) and np.array_equal(cb, ocb, equal_nan=True), (tag, "oracle bands")


# ---- 1. OTW, three-way equality ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["default", "spec0", "tp0", "c600"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("euclid", [False, True], ids=["dot", "euclid"])
@pytest.mark.parametrize("variant", ["otw", "livenote", "livenote_v2"])
def test_otw_three_way(monkeypatch, variant, euclid, dtype, flavour):
    from real_time_audio_sync_amd import _native as nat, synth
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    if flavour == "spec0":
        monkeypatch.setenv("RTS_OTW_SPEC", "0")
    if flavour == "tp0":
        monkeypatch.setenv("RTS_OTW_TP_FROM", "0")
    c, n_ref = (600, 640) if flavour == "c600" else (40, 260)
    tdt = torch.float32 if dtype == "f32" else torch.float64
    prep = (lambda x: synth._as_f32_values(np.abs(x - 0.2))) if euclid else (lambda x: x)
    ref, lives = synth.synth_batch(n_ref, 6, seed=40)
    fresh_lives = {1: synth.synth_live(ref, seed=77, lo=0.9, hi=1.4), 4: synth.synth_live(ref, seed=78)[:, :n_ref // 3]}
    ref, lives = prep(ref), [prep(l) for l in lives]
    fresh_lives = {b: prep(l) for b, l in fresh_lives.items()}
    kw = dict(variant=variant, euclid=euclid, dtype=tdt)
    tag = (variant, euclid, dtype, flavour)
    eng, ctl = BatchedOTW(ref, c, 3, batch=6, **kw), BatchedOTW(ref, c, 3, batch=6, **kw)
    fe, fc = Feeder(lives, tdt), Feeder(lives, tdt)
    while fe.pos[0] < lives[0].shape[1] // 2:
        fe.round([eng])
        fc.round([ctl])
    assert eng.state(1)["n_path"] > 0 and eng.state(4)["consumed"] > 0
    eng.restart([1, 4])
    one = BatchedOTW(ref, c, 3, batch=1, **kw)
    for b in (1, 4):   # right after the restart: the state of a handle that has seen nothing
        assert np.array_equal(eng.states()[b], one.states()[0]), (tag, b)
        assert len(eng.path(b)) == 0 and eng.state(b)["status"] == nat.RUNNING, (tag, b)
        for got, want in zip(eng.bands(b), one.bands(0)):   # no bands yet: NaN, as on the fresh handle
            assert np.isnan(want).all() and np.array_equal(got, want, equal_nan=True), (tag, b)
    one.close()
    for b in (1, 4):
        fe.new_sequence(b, fresh_lives[b])
    while not (fe.done() and fc.done()):
        fe.round([eng])
        fc.round([ctl])
    for b in (0, 2, 3, 5):
        _same_stream(eng, b, ctl, b, (tag, "untouched", b))
    for b in (1, 4):
        one = BatchedOTW(ref, c, 3, batch=1, **kw)
        fe.repeat_on(b, one)
        _same_stream(eng, b, one, 0, (tag, "restarted", b))
        one.close()
        _otw_vs_oracle(eng, b, ref, fresh_lives[b], c, variant, euclid, (tag, b))
    eng.close()
    ctl.close()


# ---- 2. dead slots come back ------------------------------------------------------------------------------------------
def test_stopped_and_overflowed_streams_restart(otw_golden):
    """Golden inputs F (runs into the end of its reference: "stop") and E (runs past its 2N live frames), one stream each
    plus a bystander; both dead streams are restarted and follow the beginning of their recording again."""
    from real_time_audio_sync_amd import _native as nat
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    g = otw_golden
    refs = [g["F/ref"].astype(np.float64), g["E/ref"].astype(np.float64), g["F/ref"].astype(np.float64)[:, :60]]
    lives = [g["F/live"].astype(np.float64), g["E/live"].astype(np.float64), g["F/live"].astype(np.float64)[:, :25]]
    eng, ctl = BatchedOTW.with_references(refs, 10, 3), BatchedOTW.with_references(refs, 10, 3)
    fe = Feeder(lives, torch.float64)
    while not fe.done():
        fe.round([eng, ctl])
    st = eng.states()
    assert st[0][nat.ST_STATUS] == nat.STOP_REF_END and st[1][nat.ST_STATUS] == nat.LIVE_OVERFLOW
    eng.restart([0, 1])
    again = [lives[0][:, :30], lives[1][:, :50], lives[2][:, 25:25]]
    for b in (0, 1):
        fe.new_sequence(b, again[b])
    fe.seqs[2] = lives[2]            # nothing more for the bystander
    while not fe.done():
        fe.round([eng])
    for b in (0, 1):
        one = BatchedOTW(refs[b], 10, 3, batch=1, dtype=torch.float64)
        fe.repeat_on(b, one)
        _same_stream(eng, b, one, 0, ("dead slot", b))
        assert eng.state(b)["status"] == nat.RUNNING and eng.state(b)["n_path"] > 0
        one.close()
        _otw_vs_oracle(eng, b, refs[b], again[b], 10, "otw", False, ("dead slot", b))
    _same_stream(eng, 2, ctl, 2, "bystander")
    eng.close()
    ctl.close()


# ---- 3. re-reference and offset ---------------------------------------------------------------------------------------
def test_otw_rereference_and_offset():
    from real_time_audio_sync_amd import synth
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    lens = [200, 150, 240, 120, 180]
    refs = [synth.synth_ref(n, seed=500 + b) for b, n in enumerate(lens)]
    extra = synth.synth_ref(300, seed=599)                      # the longest piece: the handle's N_max
    lives = [synth.synth_live(r, seed=600 + b) for b, r in enumerate(refs)]
    c, off = 30, 70
    eng = BatchedOTW.with_references(refs, c, 3, extra_refs=[extra])
    ctl = BatchedOTW.with_references(refs, c, 3, extra_refs=[extra])
    assert eng.N == 300 and list(eng.ref_lens) == lens and eng.ref.shape[0] == sum(lens) + 300
    fe = Feeder(lives, torch.float64)
    for _ in range(5):
        fe.round([eng, ctl])
    # stream 0 moves on to the extra piece (a range as long as N_max), stream 2 starts again from frame `off` of its own
    # piece, stream 3 is put on the last frame of its piece (a range of length 1)
    eng.restart([0, 2, 3], refs=[extra, refs[2], refs[3]], offsets=[0, off, lens[3] - 1])
    assert list(eng.ref_lens) == [300, 150, 240 - off, 1, 180]
    new_refs = {0: extra, 2: np.ascontiguousarray(refs[2][:, off:]), 3: np.ascontiguousarray(refs[3][:, -1:])}
    new_lives = {0: synth.synth_live(extra, seed=700), 2: synth.synth_live(new_refs[2], seed=702),
                 3: synth.synth_live(refs[3], seed=703)[:, :9]}
    for b in new_lives:
        fe.new_sequence(b, new_lives[b])
    # (the control goes on with the old recordings of streams 1 and 4 only; what it does with 0, 2, 3 is not looked at)
    fc = Feeder(lives, torch.float64)
    fc.pos, fc.k = [lives[b].shape[1] if b in new_lives else fe.pos[b] for b in range(5)], fe.k
    while not (fe.done() and fc.done()):
        fe.round([eng])
        fc.round([ctl])
    for b in (1, 4):
        _same_stream(eng, b, ctl, b, ("untouched", b))
    for b in (0, 2, 3):
        one = BatchedOTW.with_references([new_refs[b]], c, 3)
        fe.repeat_on(b, one)
        _same_stream(eng, b, one, 0, ("re-referenced", b))
        one.close()
        _otw_vs_oracle(eng, b, new_refs[b], new_lives[b], c, "otw", False, ("re-referenced", b))
    # "same piece, from this frame": offsets alone
    eng.restart([2], offsets=[off + 5])
    assert eng.ref_lens[2] == 240 - off - 5
    r2 = np.ascontiguousarray(refs[2][:, off + 5:])
    l2 = synth.synth_live(r2, seed=710)[:, :60]
    buf = np.zeros((5, l2.shape[1], 12))
    buf[2] = l2.T
    eng.push(torch.from_numpy(buf).to("cuda:0"), torch.tensor([0, 0, l2.shape[1], 0, 0], dtype=torch.int32, device="cuda:0"))
    _otw_vs_oracle(eng, 2, r2, l2, c, "otw", False, "offset only")
    with pytest.raises(ValueError):
        eng.restart([1], refs=[np.zeros((12, 5))])              # not uploaded at create
    with pytest.raises(ValueError):
        eng.restart([1], offsets=[150])                          # outside its piece
    eng.close()
    ctl.close()


# ---- 4. dense mirror and dense replay ---------------------------------------------------------------------------------
def test_dense_mirror_and_replay_after_restart():
    from real_time_audio_sync_amd import synth
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    ref, lives = synth.synth_batch(60, 3, seed=11)
    again = synth.synth_live(ref, seed=99)[:, :35]
    c = 12
    for mirror in (True, False):
        eng, ctl, one = (BatchedOTW(ref, c, 3, batch=n, dtype=torch.float64) for n in (3, 3, 1))
        if mirror:
            for e in (eng, ctl, one):
                e.enable_dense()
        fe, fc = Feeder(lives, torch.float64), Feeder(lives, torch.float64)
        for _ in range(3):
            fe.round([eng])
            fc.round([ctl])
        eng.restart([1])
        if mirror:   # at once: the restarted stream's matrices are those of a fresh handle, the others' are untouched
            torch.cuda.synchronize()
            assert torch.equal(eng.dense_acc[1], one.dense_acc[0]) and torch.equal(eng.dense_cost[1], one.dense_cost[0])
            assert bool((eng.dense_acc[1] == 1e10).all()) and bool((eng.dense_cost[1] == -1.0).all())
            for b in (0, 2):
                assert torch.equal(eng.dense_acc[b], ctl.dense_acc[b]) and torch.equal(eng.dense_cost[b], ctl.dense_cost[b])
        fe.new_sequence(1, again)
        while not (fe.done() and fc.done()):
            fe.round([eng])
            fc.round([ctl])
        fe.repeat_on(1, one)
        if mirror:
            torch.cuda.synchronize()
            got, want_ctl, want_one = (eng.dense_acc, eng.dense_cost), (ctl.dense_acc, ctl.dense_cost), (one.dense_acc, one.dense_cost)
        else:
            got, want_ctl, want_one = eng.replay_dense(), ctl.replay_dense(), one.replay_dense()
        for m in (0, 1):
            assert torch.equal(got[m][1], want_one[m][0]), (mirror, m, "restarted")
            for b in (0, 2):
                assert torch.equal(got[m][b], want_ctl[m][b]), (mirror, m, b)
        import oracle
        o = oracle.OtwOracle(ref, c, 3, keep_cost=True)
        o.run(again)
        assert np.array_equal(got[0][1].cpu().numpy(), o.acc_cost()) and np.array_equal(got[1][1].cpu().numpy(), o.cost())
        _same_stream(eng, 1, one, 0, ("dense", mirror))
        for e in (eng, ctl, one):
            e.close()


# ---- 5. WTW -----------------------------------------------------------------------------------------------------------
def _wtw_vs_oracle(eng, b, ref, live, log, W, hopf, tag):
    import oracle
    o = oracle.WtwOracle(ref, W, hopf)
    p, alive = 0, True
    for _, n in log:
        if not alive:
            break
        alive = o.insert_precheck() == oracle.RUNNING
        for q in range(p, p + n):
            if not alive:
                break
            alive = o.push_col(live[:, q]) == oracle.RUNNING
        p += n
    st, so = eng.state(b), o.state
    assert np.array_equal(eng.path(b), o.path), (tag, "oracle path")
    assert (st["live_ptr"], st["ref_ptr"], st["status"]) == (so["live_ptr"], so["ref_ptr"], so["status"]), tag
    assert (st["windows"], st["cells"]) == (o.counters["windows"], o.counters["cells"]), tag


def _same_wtw_stream(a, ba, b, bb, tag):
    assert np.array_equal(a.states()[ba], b.states()[bb]), (tag, "state")
    assert np.array_equal(a.path(ba), b.path(bb)), (tag, "path")


@pytest.mark.parametrize("W,hopf,keep_d", [(20, 10, False), (100, 50, True), (200, 100, False)])
@pytest.mark.parametrize("per_stream", [False, True], ids=["shared", "refs"])
def test_wtw_three_way(W, hopf, keep_d, per_stream):
    """W = 20 and 100 run the one-workgroup window kernels, W = 200 the strip-DP pipeline (wtw_big_*)."""
    from real_time_audio_sync_amd import synth
    from real_time_audio_sync_amd.wtw import BatchedWTW
    dev = torch.device("cuda:0")
    B = 6
    to_dev = lambda r: torch.from_numpy(np.ascontiguousarray(r.T)).to(dev)
    scale = lambda l, s: l * (0.5 + np.random.RandomState(s).rand(1, l.shape[1]))
    if per_stream:
        Ms = [5 * W + 10, 4 * W + 3, 6 * W, 5 * W, 4 * W + 40, 5 * W + 7]
        refs = [synth.synth_ref(m, seed=800 + b) for b, m in enumerate(Ms)]
        extra = synth.synth_ref(7 * W, seed=899)
        tens, tex = [to_dev(r) for r in refs], to_dev(extra)
        mk = lambda: BatchedWTW.with_references(tens, W, hopf, keep_last_d=keep_d, extra_refs=[tex])
        off = 2 * W + 3
        new_refs = {1: extra, 4: np.ascontiguousarray(refs[4][:, off:])}
    else:
        ref = synth.synth_ref(5 * W + 10, seed=800)
        refs = [ref] * B
        t = to_dev(ref)
        mk = lambda: BatchedWTW(t, W, hopf, batch=B, keep_last_d=keep_d)
        new_refs = {1: ref, 4: ref}
    lives = [scale(synth.synth_live(r, seed=810 + b), b) for b, r in enumerate(refs)]
    new_lives = {1: scale(synth.synth_live(new_refs[1], seed=821), 21),
                 4: scale(synth.synth_live(new_refs[4], seed=824), 24)[:, : 2 * W + hopf + 3]}
    chunks = (hopf + 3, 2 * W + 1, 5, hopf, 3 * hopf + 1)
    eng, ctl = mk(), mk()
    if per_stream:
        assert eng.M == 7 * W and list(eng.ref_lens) == Ms
    fe, fc = Feeder(lives, torch.float64, chunks), Feeder(lives, torch.float64, chunks)
    while fe.pos[0] < lives[0].shape[1] // 2:
        fe.round([eng])
        fc.round([ctl])
    assert eng.state(1)["windows"] > 0 and eng.state(4)["windows"] > 0
    if per_stream:
        eng.restart([1, 4], refs=[tex, tens[4]], offsets=[0, off])
        assert list(eng.ref_lens) == [Ms[0], 7 * W, Ms[2], Ms[3], Ms[4] - off, Ms[5]]
    else:
        eng.restart([1, 4])
    st = eng.states()
    assert not st[1].any() and not st[4].any() and len(eng.path(1)) == 0
    for b in (1, 4):
        fe.new_sequence(b, new_lives[b])
    while not (fe.done() and fc.done()):
        fe.round([eng])
        fc.round([ctl])
    tag = (W, hopf, per_stream)
    for b in (0, 2, 3, 5):
        _same_wtw_stream(eng, b, ctl, b, (tag, "untouched", b))
        if keep_d:
            assert np.array_equal(eng.last_d(b), ctl.last_d(b)), (tag, "D", b)
    for b in (1, 4):
        one = BatchedWTW(to_dev(new_refs[b]), W, hopf, batch=1, keep_last_d=keep_d)
        fe.repeat_on(b, one)
        _same_wtw_stream(eng, b, one, 0, (tag, "restarted", b))
        if keep_d and eng.state(b)["windows"] > 0:
            assert np.array_equal(eng.last_d(b), one.last_d(0)), (tag, "D", b)
        one.close()
        _wtw_vs_oracle(eng, b, new_refs[b], new_lives[b], fe.log[b], W, hopf, (tag, b))
    eng.close()
    ctl.close()


def _device_to_host(ptr, shape):
    """Copy of library-owned device memory (a *_device_views pointer), through the HIP runtime the process already uses."""
    path = [l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l][0]
    hip = ctypes.CDLL(path)
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    out = np.empty(shape, dtype=np.float64)
    torch.cuda.synchronize()
    assert hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0      # hipMemcpyDeviceToHost
    return out


def test_wtw_history_reads_zero_after_restart():
    """wtw.py:55: a restarted stream's live chroma history is zeros again; its neighbours' is untouched."""
    from real_time_audio_sync_amd import _native as nat, synth
    from real_time_audio_sync_amd.wtw import BatchedWTW
    dev = torch.device("cuda:0")
    ref = synth.synth_ref(90, seed=1)
    eng = BatchedWTW(torch.from_numpy(np.ascontiguousarray(ref.T)).to(dev), 20, 10, batch=3)
    cols = torch.rand((3, 50, 12), dtype=torch.float64, device=dev) + 0.1
    eng.push(cols)
    lc, cap = ctypes.c_void_p(), ctypes.c_int()
    nat.check(nat.lib.rts_wtw_device_views(eng._h, ctypes.byref(lc), ctypes.byref(cap), None))
    assert cap.value == 180
    eng.restart([1])
    out = _device_to_host(lc.value, (3, 180, 12))
    want = cols.cpu().numpy()
    assert not out[1].any()
    for b in (0, 2):
        assert np.array_equal(out[b, :50], want[b]) and not out[b, 50:].any()
    eng.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------
def _tables(B, mask, first=None, lens=None):
    m = np.array(mask, dtype=np.uint8)
    f = None if first is None else np.array(first, dtype=np.int64)
    n = None if lens is None else np.array(lens, dtype=np.int32)
    return m, f, n


@pytest.mark.parametrize("kind", ["otw", "wtw", "live"])
def test_refusals_change_nothing(kind):
    """Every refusal is RTS_ERR_INVALID, names the stream at fault, and leaves every stream as it was."""
    from real_time_audio_sync_amd import _native as nat, synth
    from real_time_audio_sync_amd.live import LiveSession
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    from real_time_audio_sync_amd.wtw import BatchedWTW
    dev = torch.device("cuda:0")
    lens = [80, 60, 90, 70]
    pool = sum(lens)
    refs = [synth.synth_ref(n, seed=30 + b) for b, n in enumerate(lens)]
    lives = [synth.synth_live(r, seed=40 + b)[:, :40] for b, r in enumerate(refs)]
    to_dev = lambda r: torch.from_numpy(np.ascontiguousarray(r.T)).to(dev)
    sess = None
    if kind == "otw":
        multi, single = BatchedOTW.with_references(refs, 10, 3), BatchedOTW(refs[0], 10, 3, batch=4, dtype=torch.float64)
        fn, hm, hs = nat.lib.rts_otw_restart, multi._h, single._h
    elif kind == "wtw":
        multi, single = BatchedWTW.with_references([to_dev(r) for r in refs], 10, 5), BatchedWTW(to_dev(refs[0]), 10, 5, batch=4)
        fn, hm, hs = nat.lib.rts_wtw_restart, multi._h, single._h
    else:
        sess, sess_single = LiveSession(refs, batch=4, c=10), LiveSession(refs[0], batch=4, c=10)
        for s in (sess, sess_single):   # 5000 samples each: one column consumed, 2952 samples stay pending
            s.feed_block((np.random.RandomState(3).rand(4, 5000) - 0.5).astype(np.float32))
        multi, single = sess.otw, sess_single.otw
        fn, hm, hs = nat.lib.rts_live_restart, sess._h, sess_single._h
    fe = Feeder(lives, torch.float64)
    while not fe.done():
        fe.round([multi, single])
    before_m, before_s = multi.states(), single.states()
    paths = [multi.path(b) for b in range(4)]
    assert before_m[:, 0].any()
    stream = multi._stream()
    if sess is not None:
        assert list(sess.pending()) == [2952] * 4

    def refused(h, mask, first=None, lens_=None, names=None):
        m, f, n = _tables(4, mask, first, lens_)
        rc = fn(h, m.ctypes.data, None if f is None else f.ctypes.data, None if n is None else n.ctypes.data, stream)
        msg = nat.lib.rts_last_error()
        assert rc == -1 and msg, (rc, msg)
        if names is not None:
            assert (b"stream %d" % names) in msg, msg

    ok_f, ok_n = [0, 80, 140, 230], list(lens)
    assert fn(None, np.ones(4, np.uint8).ctypes.data, None, None, stream) == -1                    # NULL handle
    assert fn(hm, None, None, None, stream) == -1 and b"mask" in nat.lib.rts_last_error()         # NULL mask
    refused(hm, [0, 1, 0, 0], first=ok_f)                                                          # only one table
    refused(hm, [0, 1, 0, 0], lens_=ok_n)
    refused(hm, [0, 0, 1, 0], ok_f, [80, 60, 0, 70], names=2)                                      # len < 1
    refused(hm, [0, 0, 1, 0], [0, 80, -1, 230], ok_n, names=2)                                     # first < 0
    refused(hm, [0, 1, 0, 1], ok_f, [80, 60, 90, pool - 230 + 1], names=3)                         # range past the pool
    refused(hm, [1, 0, 0, 0], [100, 80, 140, 230], [91, 60, 90, 70], names=0)                      # len above N_max / M_max
    if hs is not None:
        refused(hs, [0, 1, 0, 0], ok_f, ok_n)                                                      # no per-stream references
    assert np.array_equal(multi.states(), before_m) and np.array_equal(single.states(), before_s)
    # entries of unselected streams are not read: nonsense there is fine, and an all-zero mask does nothing
    m, f, n = _tables(4, [0, 0, 0, 0], [-5, -5, -5, -5], [0, 0, 0, 0])
    assert fn(hm, m.ctypes.data, f.ctypes.data, n.ctypes.data, stream) == 0
    assert fn(hm, m.ctypes.data, None, None, stream) == 0
    assert np.array_equal(multi.states(), before_m)
    for b in range(4):
        assert np.array_equal(multi.path(b), paths[b])
    if sess is not None:   # the host mirror of the pending counts is part of "nothing changed"
        assert list(sess.pending()) == [2952] * 4 and list(sess_single.pending()) == [2952] * 4
    if torch.cuda.device_count() > 1:                                                              # wrong current device
        with torch.cuda.device(1):
            refused(hm, [0, 1, 0, 0])
        assert np.array_equal(multi.states(), before_m)
    # and the same call with nothing wrong goes through
    m, f, n = _tables(4, [0, 1, 0, 0], [0, 5, 0, 0], [1, 90, 1, 1])
    assert fn(hm, m.ctypes.data, f.ctypes.data, n.ctypes.data, stream) == 0
    after = multi.states()
    assert not np.array_equal(after[1], before_m[1]) and np.array_equal(after[[0, 2, 3]], before_m[[0, 2, 3]])
    if sess is not None:
        assert list(sess.pending()) == [2952, 0, 2952, 2952]
        sess.close()
        sess_single.close()
    else:
        multi.close()
        single.close()


# ---- 6b. more selected streams than one launch carries -----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["otw", "wtw", "live"])
def test_restart_of_more_streams_than_one_launch_carries(kind):
    """B = 300 with 203 streams selected: the selection travels in chunks of 128 streams per launch.  Every selected stream
    must be fresh and on its new range, every other one untouched."""
    from real_time_audio_sync_amd import _native as nat, synth
    from real_time_audio_sync_amd.live import LiveSession
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    from real_time_audio_sync_amd.wtw import BatchedWTW
    dev = torch.device("cuda:0")
    B = 300
    ref_a, ref_b = synth.synth_ref(90, seed=1), synth.synth_ref(70, seed=2)
    live = synth.synth_live(ref_a, seed=3)[:, :40]
    sel = [b for b in range(B) if b % 3 != 1 or b > 290]
    assert len(sel) == 203
    rest = [b for b in range(B) if b not in sel]
    sess = None
    if kind == "wtw":
        ta, tb = (torch.from_numpy(np.ascontiguousarray(r.T)).to(dev) for r in (ref_a, ref_b))
        eng = BatchedWTW.with_references([ta] * B, 10, 5, extra_refs=[tb])
        new_ref, slen = tb, nat.WTW_STATE_LEN
    elif kind == "otw":
        eng = BatchedOTW.with_references([ref_a] * B, 10, 3, extra_refs=[ref_b])
        new_ref, slen = ref_b, nat.STATE_LEN
    else:
        sess = LiveSession([ref_a] * B, batch=B, c=10, extra_refs=[ref_b], max_pending=3 * 4096)
        sess.feed_block((np.random.RandomState(5).rand(B, 5000) - 0.5).astype(np.float32))
        eng, new_ref, slen = sess.otw, ref_b, nat.STATE_LEN
    cols = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(live.T, (B,) + live.T.shape))).to(dev)
    eng.push(cols)
    before = eng.states()
    assert before[:, 0].all()
    (sess or eng).restart(sel, refs=[new_ref] * len(sel), offsets=[b % 7 for b in sel])
    after = eng.states()
    fresh = after[sel[0]]
    assert fresh[0] == 0 and (after[sel] == fresh).all() and np.array_equal(after[rest], before[rest])
    assert list(eng.ref_lens) == [70 - b % 7 if b in sel else 90 for b in range(B)]
    if sess is not None:
        assert list(sess.pending()) == [0 if b in sel else 2952 for b in range(B)]
    # the new ranges arrived: every restarted stream now follows ref_b from its own offset
    eng.push(torch.from_numpy(np.ascontiguousarray(np.broadcast_to(live.T[:12], (B, 12, 12)))).to(dev))
    if kind != "wtw":
        import oracle
        for b in (sel[0], sel[127], sel[128], sel[202]):
            o = oracle.OtwOracle(np.ascontiguousarray(ref_b[:, b % 7:]), 10, 3)
            o.run(live[:, :12])
            assert np.array_equal(eng.path(b), o.path), b
    else:
        assert (eng.states()[sel][:, 0] == 12).all()
    (sess or eng).close()


# ---- 7. graph capture -------------------------------------------------------------------------------------------------
def test_restart_and_push_captured_in_a_graph():
    """rts_otw_restart + rts_otw_push captured on a side stream and replayed once: the same states as the eager sequence.
    A synchronisation or an allocation inside the restart would fail the capture."""
    from real_time_audio_sync_amd import synth
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    ref, lives = synth.synth_batch(120, 4, seed=21)
    dev = torch.device("cuda:0")
    first = torch.from_numpy(np.ascontiguousarray(np.stack([l[:, :30].T for l in lives]))).to(dev)
    second = torch.from_numpy(np.ascontiguousarray(np.stack([l[:, 30:50].T for l in lives]))).to(dev)
    n_new = torch.tensor([20, 17, 20, 3], dtype=torch.int32, device=dev)
    eager, graphed = BatchedOTW(ref, 20, 3, batch=4, dtype=torch.float64), BatchedOTW(ref, 20, 3, batch=4, dtype=torch.float64)
    eager.push(first)
    eager.restart([1, 3])
    eager.push(second, n_new)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        graphed.push(first)          # (the first push allocates the history: before the capture)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        graphed.restart([1, 3])
        graphed.push(second, n_new)
    assert graphed.state(1)["consumed"] == 30        # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(graphed.states(), eager.states())
    for b in range(4):
        assert np.array_equal(graphed.path(b), eager.path(b)), b
    assert eager.state(1)["consumed"] == 17 and eager.state(3)["consumed"] == 3
    del g
    eager.close()
    graphed.close()
