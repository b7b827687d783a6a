"""One live session with every publisher on, composed from the models the suite already trusts -- CPU only, no torch.

A feed is one chain (live_enqueue, csrc/live.hip): resampler, append, chroma, difference, gate, tracker push, watch, beat,
tempo, consensus, compaction.  Every link has a bit-exact model of its own; this module composes them and holds the event
script that tests/test_live_all_cpu.py (the census of what the script's inputs reach) and tests/test_live_all_gpu.py (the
device against the composition) both run:

  * ``Composed``: the per-stream state the publishers carry, driven by the paths of the trackers after every feed --
    annot_model.Sticky (beats), tempo_model.tail / bpm (tempo), ensemble_model.member_beat / fuse_step (consensus),
    path_cost_ref of tests/test_reacquire_cpu.py (confidence).  Restart, reset and the three switches change it the way
    live_restart_kernel, rts_live_reset and the rts_live_* setters change the device.
  * ``Sim``: what reaches the trackers and what they make of it -- resample_model (fs_in != fs), live_gate_model.GateStreamModel
    on oracle.chroma_oracle.LiveLoopModel (framing, levels, the gate, the difference rule), the chroma oracle's columns
    of the frames the gate lets through, oracle.OtwOracle / WtwOracle fed with them, restart onto a range, and reacquire
    as locate_ref (tests/test_locate_cpu.py) over the pool in upload order.  It carries a ``Composed`` fed by the oracle's
    paths, so the whole session exists without a GPU.
  * ``build_case(id)``: geometry, references, tables, audio and the script of one case of the table in the GPU module.

Every float here is a Python float or a float64 produced in the operation order of the definitions, so the GPU module
compares bytes."""
import numpy as np

import annot_model as am
import ensemble_model as em
import tempo_model as tm
from live_gate_model import GateStreamModel
from resample_model import as_float32, avail_closed, ratio, resample_model_fast

L, HOP, RATE = 512, 128, 22050
FRAME_SECONDS = HOP / float(RATE)
REF_HOP = HOP * 5 // 4                      # the references are the same music framed 1.25 hops apart
N_CLEAN = L + 148 * HOP                     # samples behind one reference: 119 chroma frames at REF_HOP
C, MRC = 10, 3
WTW_W, WTW_HOPF = 8, 4
MIN_DB, HOLD = -50.0, 2
MIN_LEVEL = 10.0 ** (MIN_DB / 10.0)
K_WATCH, K_TEMPO, AHEAD = 16, 16, 4.0
MAX_DEV, PATIENCE = 0.05, 2
GROUPS = [0, 1, 0, 1, -1, 0, 1]             # two groups of three, interleaved, and one stream in none
B = len(GROUPS)
M_EXCERPT = 32                              # frames reacquire() locates
ONE_COLUMN = 560                            # samples (at RATE) that complete exactly one chroma column of a fresh stream

S_FAST, S_SILENT, S_RESTART, S_REACQ, S_FREE, S_REST, S_LATE = range(B)
N_FEEDS = 36
F_NOTHING, F_RESTART, F_REACQ = 7, 12, 20   # the feed without a column; the feeds a restart / reacquire comes before
F_ANNOT, F_TEMPO, F_ENS = (23, 25), (26, 28), (29, 31)     # (off before this feed, on again before that one)
F_UNBOUND = 30                              # S_LATE restarts before this feed, while consensus is off: its strikes stay
RESTART_OFFSET = 48

CASES = {
    "otw": dict(kind="otw", variant="otw", euclid=False, features="chroma", fs_in=None, pcm=False, watch=True, refs=False),
    "v2_diff": dict(kind="otw", variant="livenote_v2", euclid=True, features="chroma_diff", fs_in=None, pcm=False, watch=True,
                    refs=False),
    "wtw": dict(kind="wtw", variant=None, euclid=False, features="chroma", fs_in=None, pcm=False, watch=False, refs=False),
    "otw_48k": dict(kind="otw", variant="otw", euclid=False, features="chroma", fs_in=48000, pcm=True, watch=True, refs=False),
    "otw_refs": dict(kind="otw", variant="otw", euclid=False, features="chroma", fs_in=None, pcm=False, watch=True, refs=True),
}


def clip_diff(cols):
    """np.clip(np.diff(chroma), 0, inf) for frame-major columns [K][12] (chroma.py:89-90)."""
    return np.clip(np.diff(np.asarray(cols, dtype=np.float64).reshape(-1, 12), axis=0), 0, np.inf)


def music(n, rate, seed, shift=0):
    """A few drifting tones over noise (test_tempo_gpu.live_audio): the same music at any rate, the noise by seed."""
    rs = np.random.RandomState(seed)
    t = np.arange(n) / float(rate)
    x = 0.05 * rs.randn(n)
    for k in range(4):
        x += 0.2 * np.sin(2 * np.pi * (220.0 * 2 ** ((3 * k + shift + 2 * t) / 12.0)) * t)
    return x.astype(np.float32)


def reference(seed, shift, diff):
    """(12, N) oracle chroma of N_CLEAN samples of the music framed REF_HOP apart; difference features for ``diff``."""
    from oracle import chroma_oracle as co
    x = music(N_CLEAN, RATE, seed, shift)
    n = (len(x) - L) // REF_HOP + 1
    cols = co.live_loop_columns([x[m * REF_HOP:m * REF_HOP + L] for m in range(n)], L, RATE)
    return np.ascontiguousarray((clip_diff(cols) if diff else cols).T)


def synth_tables(P, seconds, seed):
    """One table per piece: the same beats at slightly different times (test_ensemble_gpu.synth_tables), at this
    geometry's frame time; the first row sits at 0 s like test_ensemble_gpu.SYNTH's."""
    rs = np.random.RandomState(seed)
    base = np.cumsum(rs.uniform(0.05, 0.14, size=int(seconds / 0.05)))
    base = base[base < seconds]
    out = []
    for _ in range(P):
        times = np.sort(base * rs.uniform(0.97, 1.03) + rs.uniform(-0.01, 0.01, size=len(base)))
        out.append(([0.0] + [float(t) for t in times], list(range(3, 4 + len(times)))))
    return out


class Case(object):
    pass


def build_case(cid):
    """Everything one case runs on.  ``script``: ("feed", counts[B]) in input samples, ("restart", b, pool index | None, offset),
    ("reacquire", b), ("annotate" | "tempo" | "consensus", on) and a final ("reset",)."""
    cfg = CASES[cid]
    c = Case()
    c.id, c.B, c.groups = cid, B, list(GROUPS)
    c.__dict__.update(cfg)
    c.diff = cfg["features"] == "chroma_diff"
    c.rate_in = cfg["fs_in"] or RATE
    if cfg["refs"]:                                              # a recording per stream and one more piece
        c.pool = [reference(300 + b, 0, c.diff) for b in range(B)] + [reference(399, 5, c.diff)]
        c.ref_of = list(range(B))
        c.extra = [B]
    else:
        c.pool = [reference(300, 0, c.diff)]
        c.ref_of = [0] * B
        c.extra = []
    c.tables = synth_tables(len(c.pool), 1.0, 17)                # table p belongs to pool entry p
    c.restart_to = (B if cfg["refs"] else 0, RESTART_OFFSET)     # (pool index, offset) of the scripted restart
    scale = (lambda n: int(round(n * c.rate_in / float(RATE)))) if cfg["fs_in"] else (lambda n: n)
    rs = np.random.RandomState(5)
    feeds = []
    for i in range(N_FEEDS):
        row = []
        for b in range(B):
            n = int(rs.randint(700, 1300)) if b == S_FAST else int(rs.randint(300, 900))
            r = rs.rand()
            row.append(0 if r < 0.08 else 1 if r < 0.14 else n)
        feeds.append(row)
    feeds[F_NOTHING] = [1, 0, 1, 0, 0, 1, 0]
    feeds[F_RESTART] = [ONE_COLUMN if b == S_RESTART else 0 for b in range(B)]
    c.feeds = [[scale(n) if n > 1 else n for n in row] for row in feeds]
    c.script = []
    for i, row in enumerate(c.feeds):
        if i == F_RESTART:
            c.script.append(("restart", S_RESTART) + c.restart_to)
        if i == F_REACQ and cfg["kind"] == "otw":
            c.script.append(("reacquire", S_REACQ))
        for name, (off, on) in (("annotate", F_ANNOT), ("tempo", F_TEMPO), ("consensus", F_ENS)):
            if i == off:
                c.script.append((name, False))
            if i == on:
                c.script.append((name, True))
        if i == F_UNBOUND:
            c.script.append(("restart", S_LATE, None, 0))        # the same range again
        c.script.append(("feed", row))
    c.script.append(("reset",))
    # audio: the same music into every microphone, its own noise, digital silence spliced in at RATE positions
    silences = {S_SILENT: [(40 * HOP, 34 * HOP)], S_REST: [(55 * HOP, L + HOP + 64)],
                S_LATE: [(30 * HOP, L + 40), (90 * HOP, 30 * HOP)]}
    c.audio = []
    for b in range(B):
        total = sum(row[b] for row in c.feeds) + 1
        x = music(total, c.rate_in, 500 + b)
        for at, n in silences.get(b, ()):
            at, n = scale(at), scale(n)
            x = np.concatenate([x[:at], np.zeros(n, dtype=np.float32), x[at:]])[:total]
        if cfg["pcm"]:
            x = np.round(x.astype(np.float64) * 32768.0 * 0.5).astype(np.int16)
        c.audio.append(x)
    return c


def cut(case, pos, counts):
    bufs = []
    for b, n in enumerate(counts):
        bufs.append(case.audio[b][pos[b]:pos[b] + n])
        pos[b] += n
    return bufs


# ---- the publishers ------------------------------------------------------------------------------------------------

class Composed(object):
    """The words of beats(), tempo(), consensus() and confidence() of a session whose publishers were all enabled before
    the first feed, from the trackers' paths after every feed."""

    def __init__(self, case):
        self.case, self.B, self.groups = case, case.B, case.groups
        self.G = max(self.groups) + 1
        self.annot_on = self.tempo_on = self.ens_on = True
        self.true_piece = list(case.ref_of)                      # what every stream follows (a pool index = its table)
        self.true_frame0 = [0] * self.B
        self.piece, self.frame0 = list(self.true_piece), list(self.true_frame0)   # as the last rts_live_annotate set them
        self.ref_len = [case.pool[p].shape[1] for p in self.true_piece]
        self.sticky = [am.Sticky() for _ in range(self.B)]
        self.strikes, self.out = [0] * self.B, [0] * self.B      # the ensemble handle's carried state
        self._clear(range(self.B), groups=True)

    def _clear(self, streams, groups=False):
        if groups:
            self.tempo = [None] * self.B
            self.conf = [None] * self.B
            self.dev, self.strikes_pub, self.out_pub = [em.NAN] * self.B, [0] * self.B, [0] * self.B
            self.cons, self.spread = [em.NAN] * self.G, [em.NAN] * self.G
            self.n_in, self.n_valid = [0] * self.G, [0] * self.G
        for b in streams:
            self.sticky[b].clear()
            self.tempo[b] = (tm.NAN, tm.NAN, tm.NAN, 0)
            self.conf[b] = (tm.NAN, 0)
            self.dev[b], self.strikes_pub[b], self.out_pub[b] = em.NAN, 0, 0

    # the setters
    def annotate(self, on):
        self.annot_on = on
        if on:                                                   # rts_live_annotate re-issued for every stream
            self.piece, self.frame0 = list(self.true_piece), list(self.true_frame0)

    def follow_tempo(self, on):
        self.tempo_on = on

    def follow_consensus(self, on):
        self.ens_on = on                                         # the same Ensemble bound again: its state is carried

    def restart(self, b, piece=None, frame0=None, ref_len=None):
        """live_restart_kernel for stream b; with a new range, the re-issued rts_live_annotate while annotations are on."""
        self._clear([b])
        if self.ens_on:                                          # ens_state is NULL while consensus is off
            self.strikes[b] = self.out[b] = 0
        if piece is not None:
            self.true_piece[b], self.true_frame0[b], self.ref_len[b] = piece, frame0, ref_len
            if self.annot_on:
                self.piece[b], self.frame0[b] = piece, frame0

    def reset(self):
        self._clear(range(self.B), groups=True)
        if self.ens_on:
            self.strikes, self.out = [0] * self.B, [0] * self.B

    def feed(self, paths, hists=None, ranges=None):
        """One feed's publisher launches.  ``paths[b]``: the stored (t, j) points of stream b after the push; ``hists[b]``
        [n][12]: the frames its tracker was given; ``ranges[b]`` [N][12]: the range it follows (both for the watch)."""
        case = self.case
        paths = [[(int(t), int(j)) for t, j in p] for p in paths]
        last = [p[-1][1] if p else None for p in paths]
        tabs = [case.tables[self.piece[b]] for b in range(self.B)]
        if case.watch:
            from test_reacquire_cpu import path_cost_ref
            for b in range(self.B):
                mean, n, _ = path_cost_ref(np.array(paths[b], dtype=np.int32).reshape(-1, 2), hists[b], ranges[b], K_WATCH,
                                           case.euclid)
                self.conf[b] = (mean, n)
        if self.annot_on:
            for b in range(self.B):
                self.sticky[b].feed(last[b], tabs[b][0], tabs[b][1], FRAME_SECONDS, self.frame0[b])
        if self.tempo_on:
            for b in range(self.B):
                s, q, n = tm.tail(paths[b], K_TEMPO, AHEAD, 2 * self.ref_len[b], self.ref_len[b])
                bpm = tm.NAN
                if paths[b] and self.annot_on:
                    bpm = tm.bpm(s, last[b], tabs[b][0], tabs[b][1], FRAME_SECONDS, self.frame0[b])
                self.tempo[b] = (s, q, bpm, n)
        if self.annot_on and self.ens_on:
            betas = [em.member_beat(last[b], tabs[b][0], tabs[b][1], FRAME_SECONDS, self.frame0[b]) for b in range(self.B)]
            for g in range(self.G):
                mem = [b for b in range(self.B) if self.groups[b] == g]
                s, o = [self.strikes[b] for b in mem], [self.out[b] for b in mem]
                cons, spread, n_in, n_valid, devs = em.fuse_step([betas[b] for b in mem], s, o, MAX_DEV, PATIENCE)
                for k, b in enumerate(mem):
                    self.strikes[b], self.out[b], self.dev[b] = s[k], o[k], devs[k]
                    self.strikes_pub[b], self.out_pub[b] = s[k], o[k]
                self.cons[g], self.spread[g], self.n_in[g], self.n_valid[g] = cons, spread, n_in, n_valid
            for b in range(self.B):
                if self.groups[b] < 0:
                    self.dev[b], self.strikes_pub[b], self.out_pub[b] = em.NAN, 0, 0

    # the words, shaped like the readers' dicts
    def beats(self):
        f = np.array([em.NAN if s.beat is None else s.beat for s in self.sticky], dtype=np.float64)
        return dict(beat=f, label=np.array([s.label for s in self.sticky], dtype=np.int32),
                    ref_frame=np.array([s.ref_frame for s in self.sticky], dtype=np.int32))

    def tempo_words(self):
        return dict(slope=np.array([w[0] for w in self.tempo], dtype=np.float64),
                    pos=np.array([w[1] for w in self.tempo], dtype=np.float64),
                    bpm=np.array([w[2] for w in self.tempo], dtype=np.float64),
                    n=np.array([w[3] for w in self.tempo], dtype=np.int32))

    def consensus(self):
        return dict(consensus=np.array(self.cons, dtype=np.float64), spread=np.array(self.spread, dtype=np.float64),
                    n_in=np.array(self.n_in, dtype=np.int32), n_valid=np.array(self.n_valid, dtype=np.int32),
                    dev=np.array(self.dev, dtype=np.float64), strikes=np.array(self.strikes_pub, dtype=np.int32),
                    out=np.array(self.out_pub, dtype=np.int32))

    def confidence(self):
        return dict(mean=np.array([w[0] for w in self.conf], dtype=np.float64), n=np.array([w[1] for w in self.conf], dtype=np.int32))


# ---- what reaches the trackers, and the trackers -------------------------------------------------------------------

class Tracker(object):
    """One stream's tracker as the oracle: fed like the device feeds it, a feed at a time."""

    def __init__(self, case, ref_range):
        import oracle
        self.wtw = case.kind == "wtw"
        if self.wtw:
            self.o = oracle.WtwOracle(ref_range, WTW_W, WTW_HOPF)
        else:
            variant = {"otw": oracle.OTW, "livenote": oracle.LIVENOTE, "livenote_v2": oracle.LIVENOTE_V2}[case.variant]
            self.o = oracle.OtwOracle(ref_range, C, MRC, variant=variant, cost=oracle.COST_EUCLID if case.euclid else oracle.COST_DOT)
        self.stopped = False
        self.taken = []                                          # the frames it consumed

    def feed(self, cols):
        import oracle
        if self.wtw and not self.stopped and self.o.insert_precheck() != oracle.RUNNING:   # wtw.py:76-77, every insert()
            self.stopped = True
        for col in cols:
            if self.stopped:
                break
            self.taken.append(np.asarray(col, dtype=np.float64))
            st = self.o.push_col(col) if self.wtw else self.o.insert(col)
            if st != oracle.RUNNING:
                self.stopped = True

    @property
    def path(self):
        return self.o.path

    def position(self):
        """(status, live position, reference position) as rts_live_poll publishes them."""
        st = self.o.state
        return (st["status"], st["live_ptr"], st["ref_ptr"]) if self.wtw else (st["status"], st["t"], st["j"])


class Sim(object):
    """The session of ``case`` without a GPU.  After every feed: ``gates[b]`` (levels, seen / passed / open, ordinals of
    the run), ``trk[b]`` (path, position), ``model`` (the publishers on the oracle's paths), ``log`` (per feed and stream:
    chroma columns completed, columns handed on, gate open, tracker stopped, columns before the gate))."""

    def __init__(self, case):
        self.case = case
        if case.fs_in:
            from real_time_audio_sync_amd import filters
            self.rs_L, self.rs_M = ratio(case.fs_in, RATE)
            self.taps = filters.resample_taps(case.fs_in, RATE)
            self.half = (len(self.taps) - 1) // 2
        self.range_of = [(p, 0) for p in case.ref_of]            # (pool index, offset) every stream follows
        self.model = Composed(case)
        self._fresh(range(case.B), first=True)
        self.log = []

    def ref_range(self, b):
        p, off = self.range_of[b]
        return self.case.pool[p][:, off:]

    def _fresh(self, streams, first=False):
        case = self.case
        if first:
            self.gates, self.run_in, self.n_out, self.cols = [None] * case.B, [None] * case.B, [0] * case.B, [None] * case.B
            self.trk, self.direct = [None] * case.B, [0] * case.B
        for b in streams:
            self.gates[b] = GateStreamModel(L, HOP, MIN_LEVEL, HOLD, case.diff)
            self.run_in[b] = np.zeros(0, dtype=np.float32)
            self.n_out[b] = 0
            self.cols[b] = np.zeros((0, 12))                     # oracle chroma of every column of the run
            self.trk[b] = Tracker(case, self.ref_range(b))
            self.direct[b] = 0

    def samples(self, b, buf):
        """The samples at RATE that the feed of ``buf`` appends to stream b's pending ones."""
        x = as_float32(buf)
        if not self.case.fs_in:
            return x
        self.run_in[b] = np.concatenate([self.run_in[b], x])
        n = avail_closed(len(self.run_in[b]), self.rs_L, self.rs_M, self.half)
        y = resample_model_fast(self.run_in[b], self.rs_L, self.rs_M, self.taps, ks=np.arange(self.n_out[b], n))
        self.n_out[b] = n
        return y

    def feed(self, bufs):
        """-> per stream the oracle's columns this feed hands its tracker."""
        from oracle import chroma_oracle as co
        case = self.case
        handed, row = [], []
        for b in range(case.B):
            g = self.gates[b]
            k0 = g.seen
            ords = g.feed(self.samples(b, bufs[b]))
            new = co.live_loop_columns(g.loop.slices[k0:], L, RATE)
            self.cols[b] = np.concatenate([self.cols[b], new.reshape(-1, 12)])
            if case.diff:
                cols = [np.clip(self.cols[b][m] - self.cols[b][m - 1], 0, np.inf) for m in ords]
            else:
                cols = [self.cols[b][m] for m in ords]
            self.trk[b].feed(cols)
            handed.append(cols)
            n_new = g.seen - k0
            n_diff = max(n_new - 1, 0) if case.diff and k0 == 0 else n_new    # what live_diff_kernel makes, before the gate
            row.append((n_new, len(ords), g.open, self.trk[b].stopped, n_diff))
        self.log.append(row)
        self.publish()
        return handed

    def hists(self):
        return [np.array(t.taken, dtype=np.float64).reshape(-1, 12) for t in self.trk]

    def publish(self):
        self.model.feed([t.path for t in self.trk], self.hists(), [np.ascontiguousarray(self.ref_range(b).T) for b in range(self.case.B)])

    def restart(self, b, pool_index=None, offset=0):
        if pool_index is not None:
            self.range_of[b] = (pool_index, offset)
        self._fresh([b])
        if pool_index is not None:
            self.model.restart(b, pool_index, offset, self.case.pool[pool_index].shape[1] - offset)
        else:
            self.model.restart(b)

    def locate(self, excerpt):
        """reacquire's search: the excerpt [M][12] on every piece of the pool, cheapest first, ties in upload order ->
        (pool index, start, end, cost)."""
        from test_locate_cpu import dot_cost, euclid_cost, locate_ref
        best = None
        for p, ref in enumerate(self.case.pool):
            cost, end, start = locate_ref((euclid_cost if self.case.euclid else dot_cost)(np.ascontiguousarray(excerpt.T), ref))[:3]
            if best is None or cost < best[3]:
                best = (p, int(start), int(end), float(cost))
        return best

    def reacquire(self, b):
        """-> (pool index, start, end, cost) | None.  The last M_EXCERPT frames the tracker consumed are located, the stream
        restarts there and its tracker is pushed the excerpt."""
        taken = self.hists()[b]
        if not len(taken):
            return None
        excerpt = taken[-M_EXCERPT:]
        found = self.locate(excerpt)
        self.restart(b, found[0], found[1])
        self.trk[b].feed(list(excerpt))
        self.direct[b] = len(self.trk[b].taken)
        return found

    def reset(self):
        self._fresh(range(self.case.B))
        self.model.reset()

    def frame_columns(self, b):
        cap = 2 * max(r.shape[1] for r in self.case.pool)
        return [-1] * self.direct[b] + self.gates[b].ordinals[:cap]

    def apply(self, ev):
        """An event of the script other than a feed."""
        if ev[0] == "restart":
            self.restart(ev[1], ev[2], ev[3])
        elif ev[0] == "reacquire":
            return self.reacquire(ev[1])
        elif ev[0] == "annotate":
            self.model.annotate(ev[1])
        elif ev[0] == "tempo":
            self.model.follow_tempo(ev[1])
        elif ev[0] == "consensus":
            self.model.follow_consensus(ev[1])
        elif ev[0] == "reset":
            self.reset()
        return None
