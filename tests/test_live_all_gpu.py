"""A live session with every publisher on -- gate, watch, annotate, follow_tempo, follow_consensus, in diff mode and behind
the resampler too -- against the composition of the models (tests/live_all_model.py), the oracle trackers, and twin
sessions that have the gate and one publisher each.  tests/test_live_all_cpu.py pins what the script reaches (a stream
paused by the gate over several feeds, a stopped tracker, feeds without a column, the carry-only feed of diff mode, members
out and heard again, a restart that clears strikes and whose offset shows in the beat).

| id       | tracker             | features    | extras                                                            |
| otw      | otw, dot            | chroma      | watch                                                             |
| v2_diff  | livenote_v2, euclid | chroma_diff | watch                                                             |
| wtw      | WTW                 | chroma      | (WTW refuses the watch and has no reacquire step in the script)   |
| otw_48k  | otw                 | chroma      | fs_in = 48000, PCM16 input, watch                                 |
| otw_refs | otw                 | chroma      | a reference per stream and one extra piece; the restart goes onto |
|          |                     |             | the extra piece with an offset, piece_of names eight tables       |

Every case gives its references as a list (the single-reference cases the same array seven times, uploaded once):
``restart(offsets=...)`` and ``reacquire`` need a tracker made from a list.

After every feed, bit for bit: (a) every reader's words equal ``Composed`` on the paths read back, seen / passed / open
and frame_columns equal the gate model; (b) paths and published positions equal the oracle trackers fed the chroma
oracle's columns of the frames the gate model lets through, and each feed hands on as many columns as the model says;
(c) every publisher's words equal those of the twin that has only this publisher, paths and states() those of the
gate-only twin; (d) feeds_done is the same from all six readers and is the number of feeds submitted.  (e) after a restart
or reacquire the stream's words are the cleared ones for every publisher and nobody else's moved; (f) after reset()
everything is cleared, the bound ensemble's strikes / out are zero, and two feeds reproduce the first two.

The script (live_all_model.build_case): 36 ragged feeds; a restart with an offset of a member that carries strikes; a
reacquire (OTW cases); annotate, follow_tempo and follow_consensus switched off for two feeds each, one after the other; a
second restart while consensus is off, of a member whose strikes the unbound ensemble must keep until it is bound again;
reset().

Three mutations of csrc/live.hip were run against this module, once each, all five cases failing in check (a) on the
consensus words: the consensus launch moved in front of the tracker push (feed 0; feed 1 for WTW, which has no path
point before), the ens_state line dropped from live_restart_kernel (feed 12, strikes / out of the restarted member), and
rts_live_follow_consensus(NULL) leaving ens_state set (feed 31, the strikes the unbound ensemble should have kept).
tests/test_ensemble_gpu.py notices the first two as well, no older module the third.

Two words are not the models' to the bit and are held to the twin instead: ``levels()['level']`` (the device's sum of
squares is not the correctly rounded one; tests/test_live_gate_gpu.py bounds it) and the confidence model's history, which
is the columns the session itself handed on (``last_columns``), as in tests/test_reacquire_gpu.py -- the chroma oracle's
columns agree with them only within the chroma gate."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import live_all_model as lam  # noqa: E402
from guarded import same_bytes  # noqa: E402

DEV = "cuda:0"
ALL = ("watch", "annotate", "tempo", "consensus")
TWINS = ((), ("annotate",), ("annotate", "tempo"), ("annotate", "consensus"), ("watch",))
READER_OF = {"annotate": "beats", "tempo": "tempo", "consensus": "consensus", "watch": "confidence"}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def open_session(case):
    from real_time_audio_sync_amd.live import LiveSession
    wtw = {'dtw_win_size': lam.WTW_W * lam.HOP, 'dtw_hop_size': lam.WTW_HOPF * lam.HOP} if case.kind == "wtw" else None
    return LiveSession([case.pool[p] for p in case.ref_of], batch=case.B, c=lam.C, max_run_count=lam.MRC,
                       variant=case.variant or "otw", fft_len=lam.L, hop_size=lam.HOP, fs=lam.RATE, max_pending=1 << 14,
                       wtw_params=wtw, extra_refs=[case.pool[p] for p in case.extra], features=case.features,
                       euclid=case.euclid, fs_in=case.fs_in, device=DEV)


def enable(sess, what, case, tab):
    if what == "gate":
        sess.gate(lam.MIN_DB, lam.HOLD)
    elif what == "watch":
        sess.watch(lam.K_WATCH)
    elif what == "annotate":
        sess.annotate(tab, piece_of=[(ref, p) for p, ref in enumerate(case.pool)])
    elif what == "tempo":
        sess.follow_tempo(lam.K_TEMPO, lam.AHEAD)
    elif what == "consensus":
        sess.follow_consensus(case.groups, lam.MAX_DEV, lam.PATIENCE)


def read(sess, has):
    """-> ({reader: {word: array}}, {reader: feeds_done}) of the readers this session has."""
    got = dict(poll=sess.poll(), levels=sess.levels())
    for what in has:
        got[READER_OF[what]] = getattr(sess, READER_OF[what])()
    done = {k: v.pop("feeds_done") for k, v in got.items()}
    got["poll"].pop("feeds_submitted")
    got["levels"]["open"] = got["levels"]["open"].astype(np.int32)
    if "beats" in got:
        got["beats"].pop("label_text")
    return got, done


def same(a, b):
    return a.keys() == b.keys() and all(same_bytes(np.asarray(a[k]), np.asarray(b[k])) for k in a)


def differing(a, b):
    return {k: (a[k], b[k]) for k in a if not same_bytes(np.asarray(a[k]), np.asarray(b[k]))}


class Run(object):
    """The all-on session, its twins, the CPU session and the composition on the device's own paths, moved in lock-step."""

    def __init__(self, case, tab):
        self.case, self.tab = case, tab
        self.has = tuple(w for w in ALL if w != "watch" or case.watch)
        self.twins = [t for t in TWINS if t != ("watch",) or case.watch]
        self.sessions = []

    def open(self):
        for has in [self.has] + self.twins:
            s = open_session(self.case)
            self.sessions.append((s, has))
            for what in ("gate",) + has:
                enable(s, what, self.case, self.tab)
        self.all = self.sessions[0][0]
        self.eng = self.all.otw or self.all.wtw
        self.fresh()

    def fresh(self):
        self.sim = lam.Sim(self.case)
        self.model = lam.Composed(self.case)
        self.hist = [np.zeros((0, 12)) for _ in range(self.case.B)]
        self.pos, self.feeds = [0] * self.case.B, 0

    def close(self):
        for s, _ in self.sessions:
            s.close()

    def each(self, what=None):
        return [s for s, has in self.sessions if what is None or what in has]

    def sync(self):
        for s in self.each():
            s.sync()

    def ranges(self):
        return [np.ascontiguousarray(self.sim.ref_range(b).T) for b in range(self.case.B)]

    # ---- one feed and everything that must hold after it
    def feed(self, counts, where):
        import oracle
        case, B = self.case, self.case.B
        bufs = lam.cut(case, self.pos, counts)
        for s in self.each():
            s.feed(bufs)
        self.feeds += 1
        handed = self.sim.feed(bufs)
        self.sync()
        got, done = read(self.all, self.has)
        assert set(done.values()) == {self.feeds}, (where, done)                                        # (d)
        assert self.all.poll()["feeds_submitted"] == self.feeds
        cols, n = self.all.last_columns()
        n = n.cpu().numpy()
        assert n.tolist() == [len(h) for h in handed], (where, n, [len(h) for h in handed])          # (b) the gate model's counts
        for b in range(B):
            self.hist[b] = np.concatenate([self.hist[b], cols[b, :int(n[b])].cpu().numpy().reshape(-1, 12)])
        paths = [self.all.path(b) for b in range(B)]
        self.model.feed(paths, self.hist, self.ranges())
        self.check_model(got, where)                                                                    # (a)
        for b in range(B):                                                                              # (b)
            t = self.sim.trk[b]
            assert np.array_equal(paths[b], t.path), (where, b, paths[b][-3:], t.path[-3:])
            assert (got["poll"]["status"][b],) + tuple(got["poll"]["positions"][b]) == t.position(), (where, b)
            assert (got["poll"]["status"][b] == oracle.STOP_REF_END) == t.stopped, (where, b)
        self.check_twins(got, paths, where)                                                             # (c)
        return got, paths

    def check_model(self, got, where):
        m, sim = self.model, self.sim
        want = dict(beats=m.beats(), tempo=m.tempo_words(), consensus=m.consensus())
        if self.case.watch:
            want["confidence"] = m.confidence()
        for reader, words in want.items():
            assert same(got[reader], words), (where, reader, differing(got[reader], words))
        lv = got["levels"]
        assert lv["seen"].tolist() == [g.seen for g in sim.gates] and lv["passed"].tolist() == [g.passed for g in sim.gates], where
        assert lv["open"].tolist() == [int(g.open) for g in sim.gates], where
        assert [np.isnan(v) for v in lv["level"]] == [g.seen == 0 for g in sim.gates], where
        for b in range(self.case.B):
            assert self.all.frame_columns(b).tolist() == sim.frame_columns(b), (where, b)

    def check_twins(self, got, paths, where):
        states = self.eng.states()
        for s, has in self.sessions[1:]:
            theirs, done = read(s, has)
            assert set(done.values()) == {self.feeds}, (where, has, done)
            for reader in theirs:
                assert same(got[reader], theirs[reader]), (where, has, reader, differing(got[reader], theirs[reader]))
            if not has:                                          # the gate-only twin: the tracker did the same work
                for b in range(self.case.B):
                    assert np.array_equal(paths[b], s.path(b)), (where, b)
                assert np.array_equal(states, (s.otw or s.wtw).states()), where

    # ---- the events between feeds
    def after_restart(self, b, before, where):
        """(e): the all-on session's words are the composition's -- cleared for stream b by every publisher -- and every
        other stream's, and the groups', are the bytes they were."""
        import oracle
        self.sync()
        got, done = read(self.all, self.has)
        assert set(done.values()) == {self.feeds}, (where, done)                  # feeds_done does not go backwards
        self.check_model(got, where)
        assert np.isnan(got["beats"]["beat"][b]) and got["beats"]["label"][b] == -1 and got["beats"]["ref_frame"][b] == -1
        assert np.isnan(got["tempo"]["slope"][b]) and np.isnan(got["tempo"]["pos"][b]) and np.isnan(got["tempo"]["bpm"][b])
        assert got["tempo"]["n"][b] == 0 and np.isnan(got["consensus"]["dev"][b])
        assert got["consensus"]["strikes"][b] == 0 and got["consensus"]["out"][b] == 0
        if self.case.watch:
            assert np.isnan(got["confidence"]["mean"][b]) and got["confidence"]["n"][b] == 0
        lv = got["levels"]
        assert (lv["seen"][b], lv["passed"][b], lv["open"][b]) == (0, 0, 0) and np.isnan(lv["level"][b])
        fresh = lam.Tracker(self.case, self.sim.ref_range(b))
        assert (got["poll"]["status"][b],) + tuple(got["poll"]["positions"][b]) == fresh.position() and fresh.position()[0] == oracle.RUNNING
        others = [o for o in range(self.case.B) if o != b]
        for reader in got:
            for key, v in got[reader].items():
                per_stream = len(v) == self.case.B and not (reader == "consensus" and key in ("consensus", "spread", "n_in", "n_valid"))
                keep = others if per_stream else slice(None)
                assert same_bytes(np.asarray(v)[keep], np.asarray(before[reader][key])[keep]), (where, reader, key)
        self.check_twins(got, [self.all.path(o) for o in range(self.case.B)], where)

    def restart(self, b, pool_index, offset, where):
        before, _ = read(self.all, self.has)
        if pool_index is None:                                   # the same range again
            for s in self.each():
                s.restart([b])
            self.model.restart(b)
        else:
            kw = dict(refs=[self.case.pool[pool_index]]) if self.case.refs else {}
            for s in self.each():
                s.restart([b], offsets=[offset], **kw)
            self.model.restart(b, pool_index, offset, self.case.pool[pool_index].shape[1] - offset)
        self.sim.restart(b, pool_index, offset)
        self.hist[b] = np.zeros((0, 12))
        self.after_restart(b, before, where)

    def reacquire(self, b, where):
        before, _ = read(self.all, self.has)
        assert self.eng.state(b)["consumed"] == len(self.hist[b]) >= lam.M_EXCERPT     # still running: it took every column
        want = self.sim.reacquire(b)
        found = [s.reacquire([b], M=lam.M_EXCERPT) for s in self.each()]
        for f in found:
            assert set(f) == {b} and f[b][0] is self.case.pool[want[0]] and f[b][1:3] == want[1:3], (where, f, want)
            assert f[b][1:] == found[0][b][1:], where            # every session found the same place at the same cost
        self.model.restart(b, want[0], want[1], self.case.pool[want[0]].shape[1] - want[1])
        self.hist[b] = self.hist[b][-lam.M_EXCERPT:]             # the excerpt comes first in the new run's history
        # the tracker was pushed the excerpt itself: the position words stay a fresh stream's until the next feed
        self.after_restart(b, before, where)
        assert np.array_equal(self.all.path(b), self.sim.trk[b].path), where
        assert self.all.frame_columns(b).tolist() == [-1] * lam.M_EXCERPT

    def switch(self, what, on):
        getattr(self.model, {"annotate": "annotate", "tempo": "follow_tempo", "consensus": "follow_consensus"}[what])(on)
        self.sim.apply((what, on))
        for s in self.each(what):
            if what == "annotate":
                enable(s, what, self.case, self.tab) if on else s.annotate(None)
            elif what == "tempo":
                enable(s, what, self.case, self.tab) if on else s.follow_tempo(0)
            else:
                s.follow_consensus(s._ens if on else None)      # the ensemble bound before: its strikes are carried

    def reset(self):
        """(f), first half: every word cleared, feeds_done 0, the ensemble's carried state zero."""
        for s in self.each():
            s.reset()
        self.sync()
        moved = [b for b in range(self.case.B) if self.sim.range_of[b] != (self.case.ref_of[b], 0)]
        assert lam.S_RESTART in moved
        self.fresh()
        got, done = read(self.all, self.has)
        assert set(done.values()) == {0}, done
        self.check_model(got, "reset")
        assert np.isnan(got["consensus"]["consensus"]).all() and not got["consensus"]["n_valid"].any()
        assert np.isnan(got["beats"]["beat"]).all() and not got["levels"]["seen"].any() and not got["tempo"]["n"].any()
        # one fusion step of the bound ensemble from the (empty) paths: nobody has a beat, so nobody's strikes move, and the
        # step publishes what the handle carries
        carried = self.eng.consensus(self.all._ens, self.tab, [0] * self.case.B, [0] * self.case.B)
        assert not carried["strikes"].any() and not carried["out"].any() and np.isnan(carried["dev"]).all()
        # reset keeps every stream on the range it was moved to (like its piece and frame0): back to the script's start
        for b in moved:
            kw = dict(refs=[self.case.pool[self.case.ref_of[b]]]) if self.case.refs else {}
            for s in self.each():
                s.restart([b], offsets=[0], **kw)
        self.sync()


@pytest.mark.parametrize("cid", list(lam.CASES))
def test_every_publisher_on(cid):
    from real_time_audio_sync_amd.annotate import AnnotationTables
    case = lam.build_case(cid)
    tab = AnnotationTables(case.tables, frame_seconds=lam.FRAME_SECONDS, device=DEV)
    run = Run(case, tab)
    first = []
    try:
        run.open()
        start, done = read(run.all, run.has)
        assert set(done.values()) == {0}
        run.check_model(start, "before the first feed")
        i = 0
        for ev in case.script:
            if ev[0] == "feed":
                got, paths = run.feed(ev[1], i)
                if i < 2:
                    first.append((got, paths))
                i += 1
            elif ev[0] == "restart":
                run.restart(ev[1], ev[2], ev[3], "restart before feed %d" % i)
            elif ev[0] == "reacquire":
                run.reacquire(ev[1], "reacquire before feed %d" % i)
            elif ev[0] == "reset":
                run.reset()
            else:
                run.switch(ev[0], ev[1])
        assert i == lam.N_FEEDS
        print("OBSERVED live_all %s: %d feeds into %d sessions, path points %s, stopped %s, out %s, consensus %s"
              % (cid, i, len(run.sessions), [len(p) for p in paths], np.nonzero(got["poll"]["status"])[0].tolist(),
                 got["consensus"]["out"].tolist(), got["consensus"]["consensus"].tolist()))
        for k in range(2):                                      # (f), second half: the script's first two feeds again
            got, paths = run.feed(case.feeds[k], "after the reset, feed %d" % k)
            for reader in got:
                assert same(got[reader], first[k][0][reader]), (k, reader, differing(got[reader], first[k][0][reader]))
            assert all(np.array_equal(p, q) for p, q in zip(paths, first[k][1])), k
    finally:
        run.close()
        tab.close()


def test_enable_order_does_not_matter():
    """Two all-on sessions of the ``otw`` case whose publishers were enabled in different orders publish the same bytes."""
    from real_time_audio_sync_amd import _native as nat
    from real_time_audio_sync_amd.annotate import AnnotationTables
    case = lam.build_case("otw")
    tab = AnnotationTables(case.tables, frame_seconds=lam.FRAME_SECONDS, device=DEV)
    a, b = open_session(case), open_session(case)
    try:
        for what in ("gate", "watch", "annotate", "tempo", "consensus"):
            enable(a, what, case, tab)
        enable(b, "tempo", case, tab)                            # before annotate; the gate last
        with pytest.raises(nat.RtsyncError, match="before any rts_live_annotate"):
            enable(b, "consensus", case, tab)
        for what in ("watch", "annotate", "consensus", "gate"):
            enable(b, what, case, tab)
        pos = [0] * case.B
        for i in range(10):
            bufs = lam.cut(case, pos, case.feeds[i])
            a.feed(bufs)
            b.feed(bufs)
            a.sync()
            b.sync()
            (mine, done), (theirs, done_b) = read(a, ALL), read(b, ALL)
            assert set(done.values()) == set(done_b.values()) == {i + 1}
            for reader in mine:
                assert same(mine[reader], theirs[reader]), (i, reader, differing(mine[reader], theirs[reader]))
            for s in range(case.B):
                assert np.array_equal(a.path(s), b.path(s)), (i, s)
        assert np.isfinite(mine["consensus"]["consensus"]).all() and np.isfinite(mine["tempo"]["bpm"]).any()
        assert np.isfinite(mine["confidence"]["mean"]).any() and mine["levels"]["passed"].any()
    finally:
        a.close()
        b.close()
        tab.close()


def test_restart_across_launch_chunks_clears_every_block():
    """A restart of 129 of 130 streams -- the selection reaches the device in launches of 128 and 1 (kRestartChunk) -- with
    every publisher on: the restarted streams' words in every block are the empty values of csrc/live_pub.h bit for bit and
    their status words a fresh tracker's, stream 64 and the consensus group words keep their bytes, feeds_done stays, and
    the next feed fills the words again."""
    from real_time_audio_sync_amd.annotate import AnnotationTables
    from real_time_audio_sync_amd.live import LiveSession
    B, KEPT = 130, 64
    case = lam.Case()
    case.kind, case.variant, case.euclid = "otw", "otw", False
    ref = lam.reference(300, 0, False)
    groups = [lam.GROUPS[b % len(lam.GROUPS)] for b in range(B)]
    counts = (1500, 900, 1500)                                   # 8, 7 and (a fresh stream) 8 chroma columns
    sounds = [lam.music(sum(counts), lam.RATE, 500 + s) for s in range(len(lam.GROUPS))]
    audio = [sounds[b % len(sounds)] for b in range(B)]
    tab = AnnotationTables(lam.synth_tables(1, 1.0, 17), frame_seconds=lam.FRAME_SECONDS, device=DEV)
    sess = LiveSession([ref] * B, batch=B, c=lam.C, max_run_count=lam.MRC, variant="otw", fft_len=lam.L, hop_size=lam.HOP,
                       fs=lam.RATE, max_pending=1 << 14, device=DEV)
    try:
        sess.gate(lam.MIN_DB, lam.HOLD)
        sess.watch(lam.K_WATCH)
        sess.annotate(tab, piece_of=[(ref, 0)])
        sess.follow_tempo(lam.K_TEMPO, lam.AHEAD)
        sess.follow_consensus(groups, lam.MAX_DEV, lam.PATIENCE)
        at = 0
        for n in counts[:2]:
            sess.feed([x[at:at + n] for x in audio])
            at += n
        sess.sync()
        before, done = read(sess, ALL)
        assert set(done.values()) == {2}, done
        # there is something to clear in every block, for every stream
        assert (before["confidence"]["n"] > 0).all() and (before["tempo"]["n"] > 0).all() and (before["levels"]["seen"] > 0).all()
        assert (before["beats"]["ref_frame"] >= 0).all() and (before["poll"]["positions"][:, 0] > 0).all()
        assert np.isfinite(before["consensus"]["dev"]).any()
        assert np.isfinite(before["consensus"]["consensus"]).all() and (before["consensus"]["n_in"] > 0).all()

        gone = [b for b in range(B) if b != KEPT]
        sess.restart(gone)
        sess.sync()
        got, done = read(sess, ALL)
        assert set(done.values()) == {2}, done                   # feeds_done does not move
        qnan = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]
        empty = dict(confidence=dict(mean=qnan, n=0), beats=dict(beat=qnan, label=-1, ref_frame=-1),
                     tempo=dict(slope=qnan, pos=qnan, bpm=qnan, n=0), consensus=dict(dev=qnan, strikes=0, out=0),
                     levels=dict(level=qnan, open=0, seen=0, passed=0))
        for reader, words in empty.items():
            for key, value in words.items():
                v = np.asarray(got[reader][key])
                assert same_bytes(v[gone], np.full(len(gone), value, dtype=v.dtype)), (reader, key, v[gone])
        status, t, j = lam.Tracker(case, ref).position()         # a fresh tracker's
        assert same_bytes(got["poll"]["status"][gone], np.full(len(gone), status, dtype=np.int32))
        assert same_bytes(got["poll"]["positions"][gone], np.tile(np.array([t, j], dtype=np.int32), (len(gone), 1)))
        group_words = ("consensus", "spread", "n_in", "n_valid")
        for reader in got:
            for key, v in got[reader].items():
                keep = slice(None) if reader == "consensus" and key in group_words else [KEPT]
                assert same_bytes(np.asarray(v)[keep], np.asarray(before[reader][key])[keep]), (reader, key)

        sess.feed([x[at:at + counts[2]] for x in audio])
        sess.sync()
        got, done = read(sess, ALL)
        assert set(done.values()) == {3}, done
        assert (got["confidence"]["n"][gone] > 0).all() and (got["tempo"]["n"][gone] > 0).all()
        assert (got["levels"]["seen"][gone] == 8).all() and got["levels"]["seen"][KEPT] == 8 + 7 + 12
    finally:
        sess.close()
        tab.close()
