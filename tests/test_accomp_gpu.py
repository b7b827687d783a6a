"""The live accompaniment on the device against its model (tests/accomp_model.py), bit for bit, at the geometry of
tests/live_all_model.py: L = 512, hop 128, a reference of 119 frames framed 160 samples apart (hop_track = 160), c = 10.  The
track is the reference's own audio, float32 or PCM16; the warp plans are N = 64, delta = 16 and N = 128, delta = 0.

Six streams per session, OTW and WTW: a microphone playing the reference; one playing it at tempo 0.8; one that never
receives a sample (it waits for ever); one restarted mid-way at an offset, which re-arms it; one without a track, whose row
of every chunk must stay as it was made; one more ordinary one, slower fed.  (The stream with A_max = 4 is a session of its
own below: A_max belongs to the session.)  The script: a first feed before the accompaniment is on, then 30 ragged feeds
with a feed of nothing, a feed below H, one large enough to exceed chunk_blocks = 3 (LATE, and the catch-up behind it), and
the accompaniment switched off for one feed and on again.

After every feed each stream's path is read from the device and drives the model; anchors and renderer state
(rts_live_accomp_map), every published word and the chunk's audio (warp_model on the model's anchors) are compared as
bytes.  One case drives the model from the composed oracle session (live_all_model.Sim) instead of the device's paths.  A
consumer that never synchronises and trusts feeds_done alone collects the same audio."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import accomp_model as acm  # noqa: E402
import live_all_model as lam  # noqa: E402
from guarded import same_bytes  # noqa: E402

DEV = "cuda:0"
B = 6
S_REF, S_SLOW, S_SILENT, S_RESTART, S_NONE, S_PLAIN = range(B)
HOP_TRACK = lam.REF_HOP
K, GLIDE, LEAD, RATES, CHUNK_BLOCKS, A_MAX = 6, 100, -30, (0.5, 2.0), 3, 64
PRE_FEED = 1500                     # samples before the accompaniment is on: the trackers (WTW too) have points by then
N_FEEDS, F_NOTHING, F_SMALL, F_LARGE, F_RESTART, F_OFF = 30, 3, 5, 8, 12, 20
RESTART_OFFSET = 40
CASES = {"otw_n64": ("otw", 64, 16, False, False), "wtw_n128_pcm": ("wtw", 128, 0, True, False),
         "otw_n128_pcm_oracle": ("otw", 128, 0, True, True)}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def material():
    """The reference, the track (its own audio), the microphones' audio and the feed counts: computed once, never changed."""
    ref = lam.reference(300, 0, False)
    track = lam.music(lam.N_CLEAN, lam.RATE, 300, 0)
    m = dict(ref=ref, track=track, track_pcm=np.round(track.astype(np.float64) * 32768.0 * 0.5).astype(np.int16))
    total = PRE_FEED + 200 * N_FEEDS + 1000
    m["audio"] = [lam.music(total, lam.RATE, 300, 0), lam.music(total, lam.RATE * 1.25, 300, 0), np.zeros(0, np.float32),
                  lam.music(total, lam.RATE, 301, 0), lam.music(total, lam.RATE, 302, 0), lam.music(total, lam.RATE, 303, 0)]
    for a in m["audio"] + [track, m["track_pcm"]]:          # (the reference goes to torch, which wants it writable)
        a.setflags(write=False)
    return m


def feed_counts(H):
    """30 ragged feeds of at most chunk_blocks * H samples on average, so that a stream can catch up."""
    rs = np.random.RandomState(7)
    rows = []
    for i in range(N_FEEDS):
        row = [int(rs.randint(H, 3 * H - H // 2)) for _ in range(B)]
        row[S_PLAIN] = int(rs.randint(1, 2 * H))
        if i == F_NOTHING:
            row = [0] * B
        if i == F_SMALL:
            row = [H - 5] * B
        if i == F_LARGE:
            row = [3 * H * 4 + 7] * B
        row[S_SILENT] = 0
        rows.append(row)
    return rows


def open_session(kind, ref, **kw):
    from real_time_audio_sync_amd.live import LiveSession
    wtw = {'dtw_win_size': lam.WTW_W * lam.HOP, 'dtw_hop_size': lam.WTW_HOPF * lam.HOP} if kind == "wtw" else None
    return LiveSession([ref] * B, batch=B, c=lam.C, max_run_count=lam.MRC, variant="otw", fft_len=lam.L, hop_size=lam.HOP,
                       fs=lam.RATE, max_pending=1 << 14, wtw_params=wtw, device=DEV, **kw)


def sim_case(ref):
    c = lam.Case()
    c.__dict__.update(id="accomp", kind="otw", variant="otw", euclid=False, features="chroma", diff=False, fs_in=None, pcm=False,
                      watch=False, refs=False, B=B, groups=[-1] * B, pool=[ref], ref_of=[0] * B, extra=[],
                      tables=lam.synth_tables(1, 1.0, 17))
    return c


class Script(object):
    """One session and the model of its six streams, moved in lock-step."""

    def __init__(self, sess, material, N, D, pcm, sim=None, max_anchors=A_MAX, rates=RATES, origins=None):
        self.sess, self.m, self.N, self.H, self.D, self.sim = sess, material, N, N // 2, D, sim
        self.track = material["track_pcm"] if pcm else material["track"]
        self.tracks = [self.track] * B
        self.tracks[S_NONE] = None
        self.origins = [0, 0, 0, 0, 0, 3 * HOP_TRACK] if origins is None else origins
        self.max_anchors, self.rates = max_anchors, rates
        self.p = acm.Params(H=self.H, hop=lam.HOP, hop_track=HOP_TRACK, K=K, glide=GLIDE, lead=LEAD,
                            rate_min_pm=int(round(rates[0] * 1000)), rate_max_pm=int(round(rates[1] * 1000)),
                            chunk_blocks=CHUNK_BLOCKS, A_max=max_anchors)
        self.shadow, self.ring_at = None, None           # what the whole ring must hold, and where it lies
        self.streams = [acm.Stream(self.p) for _ in range(B)]
        self.state = [(0, 0)] * B
        self.pos = [0] * B
        self.offset = [0] * B
        self.on = self.ever_on = False
        self.seen = [0] * B
        self.collected = [[] for _ in range(B)]
        self.raw = []                                    # per feed: (words, audio) as the readers returned them

    def accompany(self, streams=None):
        self.sess.accompany(self.tracks, origins=self.origins, warp_N=self.N, delta=self.D, hop_track=HOP_TRACK, K=K, glide=GLIDE,
                            lead=LEAD, rates=self.rates, chunk_seconds=CHUNK_BLOCKS * self.H / float(lam.RATE), max_anchors=self.max_anchors)
        self.on = self.ever_on = True
        for b in range(B):
            self.arm(b)

    def arm(self, b):
        if self.tracks[b] is not None:
            self.streams[b].arm(self.origins[b] + self.offset[b] * HOP_TRACK, len(self.track))
            self.state[b] = (0, 0)

    def off(self):
        self.sess.accompany(None)
        self.on = False
        for s in self.streams:
            s.disarm()

    def restart(self, b, offset):
        self.sess.restart([b], offsets=[offset])
        self.offset[b] = offset
        if self.sim is not None:
            self.sim.restart(b, 0, offset)
        self.streams[b].disarm()
        if self.on:
            self.arm(b)

    def bufs(self, counts):
        out = []
        for b, n in enumerate(counts):
            out.append(self.m["audio"][b][self.pos[b]:self.pos[b] + n])
            self.pos[b] += n
        return out

    def ring(self):
        """The whole ring [4][B][row], found from the newest chunk as the C call hands it out, and that chunk's feed."""
        import ctypes
        from real_time_audio_sync_amd import _native as nat
        chunk, stride, done = ctypes.c_void_p(), ctypes.c_longlong(), ctypes.c_int()
        nat.check(nat.lib.rts_live_accompaniment(self.sess._h, ctypes.byref(chunk), ctypes.byref(stride), None, None, None, None, None,
                                                 None, ctypes.byref(done)))
        assert stride.value == CHUNK_BLOCKS * self.H and chunk.value % 16 == 0
        base = chunk.value - (done.value % acm.SLOTS) * B * stride.value * 4
        if base != self.ring_at:                         # a ring just made (the first call, or a rebuild): all zeros
            self.ring_at, self.shadow = base, np.zeros((acm.SLOTS, B, stride.value), np.float32)
        return np.ctypeslib.as_array(ctypes.cast(base, ctypes.POINTER(ctypes.c_float)), shape=(acm.SLOTS, B, stride.value)), done.value

    def feed(self, counts, where, sync=True):
        """One feed on the device and in the model; with ``sync`` everything is compared."""
        sess = self.sess
        bufs = self.bufs(counts)
        sess.feed(bufs)
        f = sess.poll()["feeds_submitted"]
        if self.sim is not None:
            self.sim.feed(bufs)
        if sync:
            sess.sync()
        if not self.ever_on:
            return None
        if not sync:                                     # only feeds_done is trusted
            t0 = time.time()
            while sess.accompaniment()[1]["feeds_done"] < f:
                assert time.time() - t0 < 20.0, "feed %d was never published" % f
        audio, words = sess.accompaniment()
        assert words["feeds_done"] == f, where
        self.raw.append((words, [a.copy() for a in audio]))
        if not sync:
            return words
        eng = sess.otw or sess.wtw
        ring, done = self.ring()
        assert done == f, where
        for b in range(B):
            s = self.streams[b]
            if not self.on:                              # nothing was published for this feed
                assert (words["blocks"][b], words["status"][b], words["warp_status"][b], words["out_total"][b]) == (0, 0, 0, 0), (where, b)
                assert np.isnan(words["rate"][b]) and len(audio[b]) == 0
                continue
            path = self.sim.trk[b].path if self.sim is not None else sess.path(b)
            Nb = int(eng.ref_lens[b]) if hasattr(eng, "ref_lens") else self.m["ref"].shape[1]
            blocks = s.steer(counts[b], [(int(t), int(j)) for t, j in path], 2 * Nb, Nb)
            y, self.state[b], wst = s.render(self.track, self.N, self.D, self.state[b], w=None)
            w = s.words
            self.seen[b] |= w["status"]
            got = dict((k, words[k][b]) for k in ("out_total", "in_pos", "blocks", "status", "warp_status"))
            want = dict(out_total=w["out_total"], in_pos=w["in_pos"], blocks=blocks, status=w["status"], warp_status=wst)
            assert got == want, (where, b, got, want)
            assert same_bytes(np.float64(words["rate"][b]), np.float64(w["rate"])), (where, b, words["rate"][b], w["rate"])
            assert len(audio[b]) == blocks * self.H and audio[b].tobytes() == y.tobytes(), (where, b, blocks)
            self.collected[b].append(audio[b].copy())
            self.shadow[f % acm.SLOTS, b, :len(y)] = y
            anchors, state = sess.accompaniment_map(b)
            if s.armed:
                assert anchors[:, 0].tolist() == s.out_pos and anchors[:, 1].tolist() == s.in_pos, (where, b)
                assert state == tuple(int(v) for v in self.state[b]), (where, b, state, self.state[b])
                assert s.out_pos[-1] == state[0] * self.H                           # the invariant o0 == k H
            else:
                assert len(anchors) == 0, (where, b)
        # guard regions: every sample of the ring that this feed's due blocks do not cover is what it was -- the rows of the
        # stream without a track (zeros for ever), the rows behind blocks * H, the three other chunks
        assert not ring[:, S_NONE].any(), (where, "the row of the stream without a track was written")
        assert ring.tobytes() == self.shadow.tobytes(), (where, np.argwhere(ring != self.shadow)[:5])
        return words

    def run(self, sync=True):
        self.feed([PRE_FEED if b != S_SILENT else 0 for b in range(B)], "pre", sync=sync)    # before it is on: nothing to look at
        self.accompany()
        for i, counts in enumerate(feed_counts(self.H)):
            if i == F_RESTART:
                self.restart(S_RESTART, RESTART_OFFSET)
            if i == F_OFF:
                self.off()
            if i == F_OFF + 1:
                self.accompany()
            self.feed(counts, "feed %d" % i, sync=sync)


@pytest.fixture(scope="module")
def runs(material):
    """Every case run once, synchronised after each feed; the tests below look at what it left."""
    out = {}
    for cid, (kind, N, D, pcm, oracle) in CASES.items():
        sess = open_session(kind, material["ref"])
        try:
            sim = None
            if oracle:
                old, lam.MIN_LEVEL = lam.MIN_LEVEL, 0.0      # the composed session has a gate: level >= 0 lets every column through
                try:
                    sim = lam.Sim(sim_case(material["ref"]))
                finally:
                    lam.MIN_LEVEL = old
            r = Script(sess, material, N, D, pcm, sim)
            if sim is not None:
                old, lam.MIN_LEVEL = lam.MIN_LEVEL, 0.0      # Sim.restart makes a fresh gate model
                try:
                    r.run()
                finally:
                    lam.MIN_LEVEL = old
                for b in range(B):                           # the oracle's paths are the device's
                    assert np.array_equal(sess.path(b), sim.trk[b].path), b
            else:
                r.run()
            out[cid] = r
            r.sess = None
        finally:
            sess.close()
    return out


@pytest.mark.parametrize("cid", sorted(CASES))
def test_every_feed_matches_the_model(runs, cid):
    """The comparisons happened feed by feed inside the run; here: what the script was meant to reach, it reached."""
    r = runs[cid]
    seen = r.seen
    assert seen[S_SILENT] == acm.ON | acm.WAIT                     # never a sample: waiting for ever
    assert seen[S_NONE] == 0 and not any(len(a) for a in r.collected[S_NONE])
    for b in (S_REF, S_SLOW, S_RESTART, S_PLAIN):
        assert seen[b] & acm.ON and sum(len(a) for a in r.collected[b]) > 0, b
    assert seen[S_REF] & acm.LATE and seen[S_RESTART] & acm.WAIT    # the large feed; the restarted stream waits for its first point
    assert r.streams[S_RESTART].in_pos[0] == RESTART_OFFSET * HOP_TRACK
    assert r.streams[S_PLAIN].in_pos[0] == 3 * HOP_TRACK


def test_a_consumer_that_trusts_feeds_done_collects_the_same_audio(runs, material):
    kind, N, D, pcm, _ = CASES["otw_n64"]
    sess = open_session(kind, material["ref"])
    try:
        r = Script(sess, material, N, D, pcm)
        r.run(sync=False)                                # never synchronises: no path is read, the model does not run
    finally:
        sess.close()
    want = runs["otw_n64"].raw                           # the same script, synchronised and held against the model feed by feed
    assert len(r.raw) == len(want) == N_FEEDS
    for i, ((w0, a0), (w1, a1)) in enumerate(zip(r.raw, want)):
        assert w0.keys() == w1.keys() and all(same_bytes(np.asarray(w0[k]), np.asarray(w1[k])) for k in w0), i
        assert [a.tobytes() for a in a0] == [a.tobytes() for a in a1], i
    assert sum(len(a) for _, audio in r.raw for a in audio) > 0


def test_full_anchor_list(material):
    """A_max = 4: three rendering feeds, then FULL with nothing rendered, the words those of the last anchor."""
    sess = open_session("otw", material["ref"])
    try:
        r = Script(sess, material, 64, 16, False, max_anchors=4)
        r.feed([PRE_FEED if b != S_SILENT else 0 for b in range(B)], "pre")
        r.accompany()
        rs = np.random.RandomState(3)
        for i in range(8):
            words = r.feed([int(rs.randint(40, 90)) if b != S_SILENT else 0 for b in range(B)], "feed %d" % i)
        assert words["status"][S_REF] & acm.FULL and words["blocks"][S_REF] == 0 and len(r.streams[S_REF].out_pos) == 4
        assert r.seen[S_REF] & acm.FULL and not r.seen[S_SILENT] & acm.FULL
        # the same call with another A_max rebuilds everything: every stream from output sample 0 again
        r.max_anchors, r.p.A_max, r.ring_at = A_MAX, A_MAX, None     # (a new ring, wherever it lies)
        r.accompany()
        words = r.feed([60 if b != S_SILENT else 0 for b in range(B)], "after the rebuild")
        assert words["out_total"][S_REF] == 32 and not words["status"][S_REF] & acm.FULL
    finally:
        sess.close()


def test_rate_limits_the_end_of_the_track_and_a_fit_without_a_slope(material):
    """What the main script does not reach: a band of rates so narrow that the steering leaves it on both sides (LO, HI), a
    stream armed 300 samples before the end of its track (END), and streams armed with one path point stored (FREE) -- each
    held against the model feed by feed like everything else."""
    sess = open_session("otw", material["ref"])
    try:
        n = len(material["track"])
        fast = dict(material)                            # one microphone plays the music 1.43 times as fast: above the band
        fast["audio"] = list(material["audio"])
        fast["audio"][S_RESTART] = lam.music(4000, lam.RATE * 0.7, 300, 0)
        r = Script(sess, fast, 64, 16, False, rates=(0.9, 0.95), origins=[0, 0, 0, 0, 0, n - 300])
        r.feed([600 if b != S_SILENT else 0 for b in range(B)], "pre")      # one chroma column each
        r.accompany()
        rs = np.random.RandomState(9)
        for i in range(24):
            r.feed([int(rs.randint(40, 95)) if b != S_SILENT else 0 for b in range(B)], "feed %d" % i)
    finally:
        sess.close()
    union = 0
    for b in (S_REF, S_SLOW, S_RESTART, S_PLAIN):
        union |= r.seen[b]
    assert r.seen[S_REF] & acm.FREE and r.seen[S_PLAIN] & acm.END
    assert union & acm.LO and union & acm.HI, [bin(v) for v in r.seen]
    assert r.streams[S_PLAIN].in_pos[-1] == n


def test_refusals(material):
    from real_time_audio_sync_amd import _native as nat
    track = material["track"]
    sess = open_session("otw", material["ref"])
    try:
        sess.gate(-50.0, 2)
        with pytest.raises(nat.RtsyncError, match="error -2.*gate"):
            sess.accompany(track, warp_N=64, delta=16, hop_track=HOP_TRACK)
        sess.gate(None)
        for kw, code in ((dict(K=1), -1), (dict(K=1025), -1), (dict(hop_track=0), -1), (dict(hop_track=65537), -1), (dict(glide=-1), -1),
                         (dict(glide=2 ** 31), -1), (dict(lead=2 ** 31), -1), (dict(rates=(2.0, 1.0)), -1), (dict(rates=(0.5, 4.001)), -1),
                         (dict(rates=(0.0, 0.0)), -1), (dict(max_anchors=1), -1), (dict(chunk_seconds=97400.0), -2)):
            args = dict(warp_N=64, delta=16, hop_track=HOP_TRACK)
            args.update(kw)
            with pytest.raises(nat.RtsyncError, match="error %d" % code):
                sess.accompany(track, **args)
        with pytest.raises(nat.RtsyncError, match="error -1"):
            sess.accompaniment_map(0)                     # nothing was ever made: every call above was refused
        sess.accompany(track, warp_N=64, delta=16, hop_track=HOP_TRACK, max_anchors=8)
        with pytest.raises(nat.RtsyncError, match="error -2.*accompaniment"):
            sess.export_streams([0])
        with pytest.raises(nat.RtsyncError, match="error -2.*accompaniment"):
            sess.gate(-50.0, 2)
        sess.accompany(None)
        sess.export_streams([0])                          # off again: allowed
    finally:
        sess.close()
    rs = open_session("otw", material["ref"], fs_in=48000)
    try:
        with pytest.raises(nat.RtsyncError, match="error -2.*resampl"):
            rs.accompany(track, warp_N=64, delta=16, hop_track=HOP_TRACK)
    finally:
        rs.close()
