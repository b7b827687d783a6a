"""Ensemble following (csrc/ensemble.hip): one microphone followed against several recordings of its piece at once, the
group's position the median beat of its members -- beats being the scale the recordings share (the reference's harness
compares two performances the same way, tests.py:59-137).  A member that loses its place is outvoted, marked ``out`` after
``patience`` steps beyond ``max_dev`` beats from the consensus, and ``EnsembleSession.heal`` puts it back where the others
are (Arzt and Widmer, "Real-time music tracking using multiple performances as a reference", ISMIR 2015).

include/rtsync.h (rts_ensemble_create) has the definitions: the inverse lookup beat -> frame, the member beat, the fusion
step.  ``frames_of_beat`` is the host form of the first; every float64 operation is rounded on its own, in the order
written there, so host and device agree to the bit."""
import bisect
import ctypes
import math

import numpy as np
import torch

from . import _native as nat

INT32_MAX = 2 ** 31 - 1


def frames_of_beat(table, x, frame_seconds):
    """Beat ``x`` -> the frame of the piece with ``table = (times, beats)`` (one row per annotated beat, as
    ``evaluate.read_annotations`` returns them), or -1 where there is none: the host form of rts_annot_frames /
    ``AnnotationTables.frames``.  The round trip frame -> ``get_beat`` -> frame is the identity on every frame that has a
    beat."""
    times, beats = table[0], table[1]
    n = len(times)
    x = float(x)
    if x != x or n < 1 or any(int(beats[i]) <= int(beats[i - 1]) for i in range(1, n)):
        return -1
    i = bisect.bisect_left([float(int(v)) for v in beats], x)       # the first row with x <= beats[i]
    if i >= n:
        return -1
    beat = float(int(beats[i]))
    if x < beat - 1.0:
        return -1
    end = float(times[i])
    start = 0.0 if i == 0 else float(times[i - 1])
    time = end - (beat - x) * (end - start)
    q = time / float(frame_seconds) + 0.5
    if q != q or q == math.inf:
        return -1
    f = math.floor(q) if q != -math.inf else -1
    if f < 0:
        return 0
    return -1 if f > INT32_MAX else int(f)


class Ensemble(object):
    """The groups of a batch of B streams and the state of the vote (rts_ensemble_create).  ``groups[b]`` is the group of
    stream b in ``[0, n_groups)``, or -1 for a stream in no group; every group has 1 to 64 members.  ``max_dev``: beats
    a member may lie from the consensus (> 0, ``inf`` allowed: never out, the plain median); ``patience``: steps beyond
    it, 1..65535, after which the member is out of the vote until one step back within it."""

    def __init__(self, groups, max_dev=math.inf, patience=1, n_groups=None, device="cuda:0"):
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device(self.device.type, torch.cuda.current_device())
        self.groups = np.ascontiguousarray(np.asarray(groups, dtype=np.int32).reshape(-1))
        self.B = len(self.groups)
        self.n_groups = int(n_groups) if n_groups is not None else int(self.groups.max(initial=-1)) + 1
        self.max_dev, self.patience = float(max_dev), int(patience)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            nat.check(nat.lib.rts_ensemble_create(self.B, self.groups.ctypes.data, self.n_groups, self.max_dev,
                                                  self.patience, ctypes.byref(h)))
        self._h = h

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @nat.on_device
    def reset(self, streams=None):
        """Strikes and out of the listed streams (None: all) back to zero; asynchronous."""
        mask = None
        if streams is not None:
            mask = np.zeros(self.B, dtype=np.uint8)
            mask[[int(b) for b in streams]] = 1
        nat.check(nat.lib.rts_ensemble_reset(self._h, mask.ctypes.data if mask is not None else None, self._stream()))

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                torch.cuda.synchronize(self.device)
            except Exception:
                pass
            nat.destroy_on(self.device, nat.lib.rts_ensemble_destroy, h)

    __del__ = close


def tracker_consensus(handle, fn, ens, tables, pieces, frame0=None):
    """What ``BatchedOTW.consensus`` / ``BatchedWTW.consensus`` share: one fusion step from the tracker's paths as they
    stand.  Synchronises; returns the dict they document."""
    dev = handle.device
    B, G = ens.B, ens.n_groups
    pieces = tables._i32(pieces, B, "pieces")
    frame0 = tables._i32(frame0, B, "frame0") if frame0 is not None else None
    group = torch.empty((2, G), dtype=torch.float64, device=dev)
    group_n = torch.empty((2, G), dtype=torch.int32, device=dev)
    devn = torch.empty((B,), dtype=torch.float64, device=dev)
    member = torch.empty((2, B), dtype=torch.int32, device=dev)
    nat.check(fn(handle._h, ens._h, tables._h, pieces.data_ptr(), frame0.data_ptr() if frame0 is not None else None,
                 group.data_ptr(), group_n.data_ptr(), devn.data_ptr(), member.data_ptr(), handle._stream()))
    group, group_n, member = group.cpu().numpy(), group_n.cpu().numpy(), member.cpu().numpy()
    return dict(consensus=group[0].copy(), spread=group[1].copy(), n_in=group_n[0].copy(), n_valid=group_n[1].copy(),
                dev=devn.cpu().numpy(), strikes=member[0].copy(), out=member[1].copy())


def path_consensus(paths, groups, tables, pieces, T, frame0=None, max_dev=math.inf, patience=1, outputs=True):
    """The consensus curve of offline paths (rts_path_consensus): at every live frame ``t < T`` member b stands at the
    reference index of its last path point with live index <= t, and the fusion step runs frame by frame with state that
    starts at zero.  With ``max_dev=inf`` the curve is the plain median beat per frame.

    ``paths``: a list of B (P_k, 2) integer arrays of (live frame, reference frame) with a non-decreasing live index, or a
    device pair ``(path int32 [B][P_max][2], len int32 [B])`` as ``dtw.dtw_paths`` returns it.  ``groups`` as ``Ensemble``
    takes them, or an ``Ensemble`` (whose own state is left alone; ``max_dev`` / ``patience`` are then its).  ``tables``:
    an ``AnnotationTables``; ``pieces`` / ``frame0``: table and first frame inside it of every path's reference side.

    Returns device tensors ``(consensus float64 [n_groups][T], spread float64 [n_groups][T], n_in int32 [n_groups][T], out
    int32 [B][T])``, ``out[b][t]`` being member b's flag after step t; with ``outputs=False`` the consensus alone.
    Asynchronous for the device form."""
    ens = groups if isinstance(groups, Ensemble) else Ensemble(groups, max_dev, patience, device=tables.device)
    dev = tables.device
    if isinstance(paths, tuple) and len(paths) >= 2 and torch.is_tensor(paths[0]):
        path, plen = paths[0], paths[1]
    else:
        arrs = [np.asarray(p, dtype=np.int32).reshape(-1, 2) for p in paths]
        host = np.zeros((len(arrs), max([len(a) for a in arrs] + [1]), 2), dtype=np.int32)
        for k, a in enumerate(arrs):
            host[k, :len(a)] = a
        path = torch.from_numpy(host).to(dev)
        plen = torch.tensor([len(a) for a in arrs], dtype=torch.int32, device=dev)
    path = path.to(device=dev, dtype=torch.int32).contiguous()
    B, P_max, T = int(path.shape[0]), int(path.shape[1]), int(T)
    if B != ens.B:
        raise ValueError("%d paths for an ensemble of %d streams" % (B, ens.B))
    plen = tables._i32(plen, B, "path lengths")
    pieces = tables._i32(pieces, B, "pieces")
    frame0 = tables._i32(frame0, B, "frame0") if frame0 is not None else None
    G = ens.n_groups
    with torch.cuda.device(dev):
        cons = torch.empty((G, max(T, 0)), dtype=torch.float64, device=dev)
        spread = torch.empty((G, max(T, 0)), dtype=torch.float64, device=dev) if outputs else None
        n_in = torch.empty((G, max(T, 0)), dtype=torch.int32, device=dev) if outputs else None
        out = torch.empty((B, max(T, 0)), dtype=torch.int32, device=dev) if outputs else None
        nat.check(nat.lib.rts_path_consensus(
            ens._h, tables._h, path.data_ptr() if P_max else None, P_max, plen.data_ptr(), pieces.data_ptr(),
            frame0.data_ptr() if frame0 is not None else None, T, cons.data_ptr(),
            spread.data_ptr() if outputs else None, n_in.data_ptr() if outputs else None,
            out.data_ptr() if outputs else None, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        if ens is not groups:
            torch.cuda.current_stream(dev).synchronize()            # the private handle goes with this call
            ens.close()
    return (cons, spread, n_in, out) if outputs else cons


def annotate_recordings(recordings, table, annotated=0, device="cuda:0", frame_seconds=None):
    """One annotated recording of a piece and several that are not -> an ``annotate.AnnotationTables`` with a table for
    each of them.  ``recordings``: G chroma arrays (12, N_k); ``table``: the ground truth of ``recordings[annotated]``, a
    CSV path or a ``(times, beats[, labels])`` tuple.  Makes one ``dtw.align_pairs`` call, recording ``annotated`` against
    each of the others, and one ``AnnotationTables.transfer`` along those paths.  Table ``annotated`` of the result is the
    one given; the others hold its rows at the times the alignment puts them (rows in front of or behind the aligned
    stretch are dropped).  ``frame_seconds``: seconds per chroma frame (None: ``evaluate.FRAME_SECONDS``)."""
    from . import annotate, dtw
    recordings = list(recordings)
    G, annotated = len(recordings), int(annotated)
    if not 0 <= annotated < G:
        raise ValueError("annotated = %d with %d recordings" % (annotated, G))
    args = dict(device=device) if frame_seconds is None else dict(device=device, frame_seconds=frame_seconds)
    own = annotate._table(table)
    if G == 1:
        return annotate.AnnotationTables([own], **args)
    others = [k for k in range(G) if k != annotated]
    pairs = dtw.align_pairs(np.asarray(recordings[annotated]), [recordings[k] for k in others], device=device)
    source = annotate.AnnotationTables([own], **args)
    try:
        carried, _ = source.transfer([p for p, _ in pairs], [0] * len(others), 0)   # column 0 is the annotated recording
    finally:
        source.close()
    tables = dict(zip(others, carried))
    tables[annotated] = own
    return annotate.AnnotationTables([tables[k] for k in range(G)], **args)


class EnsembleSession(object):
    """``mics`` microphones, each followed against all ``G = len(recordings)`` recordings of one piece.

    ``recordings``: G chroma arrays (12, N_k) of the piece; ``tables``: an ``annotate.AnnotationTables`` with one table
    per recording, in the same order.  Wraps a ``LiveSession`` of ``mics * G`` streams, stream ``mic * G + k`` following
    recording k (each recording is uploaded once), with ``annotate(tables)`` and ``follow_consensus`` on, one group per
    microphone.  The inner session stays reachable as ``.live``: gate, watch, tempo and backward are its own.  Further
    keyword arguments go to ``LiveSession``."""

    def __init__(self, recordings, tables, mics, max_dev=2.0, patience=4, **live_args):
        from .live import LiveSession
        self.recordings = list(recordings)
        self.G, self.mics = len(self.recordings), int(mics)
        if self.G < 1 or self.G > nat.ENSEMBLE_MAX_MEMBERS:
            raise ValueError("1 to %d recordings per microphone (got %d)" % (nat.ENSEMBLE_MAX_MEMBERS, self.G))
        if tables.P != self.G:
            raise ValueError("%d tables for %d recordings" % (tables.P, self.G))
        self.tables = tables
        live_args.setdefault("device", str(tables.device))
        self.live = LiveSession([self.recordings[k] for _ in range(self.mics) for k in range(self.G)],
                                self.mics * self.G, **live_args)
        self.B = self.live.B
        self.live.annotate(tables, piece_of=[(r, k) for k, r in enumerate(self.recordings)])
        self.live.follow_consensus([b // self.G for b in range(self.B)], max_dev, patience)
        self.max_dev, self.patience = float(max_dev), int(patience)

    @classmethod
    def from_annotated(cls, recordings, table, mics, annotated=0, **kw):
        """A session from one ground-truth table: ``table`` belongs to ``recordings[annotated]``, the other recordings get
        theirs from ``annotate_recordings`` (on ``kw['device']``, default "cuda:0").  Everything else as the constructor."""
        tables = annotate_recordings(recordings, table, annotated, device=kw.get("device", "cuda:0"))
        return cls(recordings, tables, mics, **kw)

    def feed(self, buffers, wait=False):
        """``buffers``: one array of new samples per microphone (None / empty = nothing new), written G times into the
        staging slot, once per recording followed.  Otherwise ``LiveSession.feed``."""
        assert len(buffers) == self.mics
        return self.live.feed([x for x in buffers for _ in range(self.G)], wait=wait)

    def consensus(self):
        """Non-blocking: {'consensus', 'spread' float64 [mics], 'n_in', 'n_valid' int32 [mics], 'dev' float64 [mics][G],
        'strikes', 'out' int32 [mics][G], 'feeds_done'} as last published by the device (``LiveSession.consensus``)."""
        w = self.live.consensus()
        for k in ("dev", "strikes", "out"):
            w[k] = w[k].reshape(self.mics, self.G)
        return w

    def heal(self, back=0, streams=None):
        """Put the members that are out back where their group is, without synchronising: for every stream (or listed
        stream) that reads ``out == 1`` and whose group has a consensus, ``restart`` it at ``offset = clamp(
        frames_of_beat(its table, consensus) - back, 0, N - 1)`` of its recording; a beat its table does not reach leaves
        it alone.  ``back``: frames to start before the consensus, so that the tracker's band settles before "now".
        Returns ``{stream: offset}``."""
        w = self.live.consensus()
        moved = {}
        for b in (range(self.B) if streams is None else [int(s) for s in streams]):
            c = w["consensus"][b // self.G]
            if w["out"][b] != 1 or c != c:
                continue
            k = b % self.G
            f = frames_of_beat((self.tables.times[k], self.tables.beat_rows[k]), c, self.tables.frame_seconds)
            if f < 0:
                continue
            N = int(np.asarray(self.recordings[k]).shape[1])
            moved[b] = min(max(f - int(back), 0), N - 1)
        if moved:
            order = sorted(moved)
            self.live.restart(order, offsets=[moved[b] for b in order])
        return moved

    def sync(self):
        self.live.sync()

    def close(self):
        live = getattr(self, "live", None)
        if live is not None:
            live.close()
