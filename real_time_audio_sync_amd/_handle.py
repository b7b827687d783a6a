"""Host-side plumbing the batched tracker handles share (BatchedOTW in otw_batch.py, BatchedWTW in wtw.py): the pool of
per-stream references, the restart bookkeeping, and the calls that differ only in the ``rts_otw_`` / ``rts_wtw_``
prefix."""
import ctypes

import numpy as np
import torch

from . import _native as nat


def _concat_refs(refs, to_frames, extra=()):
    """Per-stream references -> (one device tensor [n_ref_frames][12], int64 first frames [B], int32 lengths [B], pool).
    A reference object that appears more than once is converted and uploaded once; its range is reused.  ``extra``:
    pieces uploaded behind them although no stream follows them yet.  ``pool`` maps id(object) -> (object, first frame,
    frames) for everything uploaded (what ``restart`` looks references up in)."""
    if len(refs) < 1:
        raise ValueError("at least one reference is needed")
    parts, seen, first, lens, off = [], {}, [], [], 0
    for k, r in enumerate(list(refs) + list(extra)):
        if id(r) not in seen:
            t = to_frames(r)
            if parts and t.dtype != parts[0].dtype:
                raise TypeError("all references must have the same dtype (%s, %s)" % (parts[0].dtype, t.dtype))
            seen[id(r)] = (r, off, int(t.shape[0]))
            parts.append(t)
            off += int(t.shape[0])
        if k < len(refs):
            first.append(seen[id(r)][1])
            lens.append(seen[id(r)][2])
    return torch.cat(parts).contiguous(), np.array(first, dtype=np.int64), np.array(lens, dtype=np.int32), seen


class _BatchedHandle:
    """What BatchedOTW and BatchedWTW share.  ``_abi`` ("otw" / "wtw") names the tracker: the handle ``_h`` is destroyed,
    restarted and read through ``rts_<_abi>_destroy``, ``_restart`` and ``_read_path``.  The bookkeeping for ``restart``:
    which range of the uploaded pool every stream follows; ``_pool`` is None on a single-reference handle."""

    def _fn(self, name):
        return getattr(nat.lib, "rts_%s_%s" % (self._abi, name))

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            nat.destroy_on(self.device, self._fn("destroy"), h)

    __del__ = close

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @nat.on_device
    def path(self, b=0):
        n = ctypes.c_int(0)
        nat.check(self._fn("read_path")(self._h, b, None, 0, ctypes.byref(n), self._stream()))
        out = np.empty((n.value, 2), dtype=np.int32)
        if n.value:
            nat.check(self._fn("read_path")(self._h, b, out.ctypes.data, n.value, ctypes.byref(n), self._stream()))
        return out

    @nat.on_device
    def tempo(self, K=64, ahead=0.0):
        """How fast is every stream going (rts_otw_tempo / rts_wtw_tempo)?  The least-squares line through the last
        ``n = min(K, path points)`` points of every stream's own path: numpy ``(slope float64 [B], pos float64 [B], n int32
        [B])``.  ``slope`` is reference frames per live frame (1.0: the reference's tempo); ``pos`` the line read at the
        newest live frame plus ``ahead`` frames, in reference frames.  NaN for a stream with fewer than two points, one
        whose live index did not move inside the window, and one with a point outside its reference.  ``2 <= K <= 1024``.
        The definition (exact integer sums, one rounding per float64 operation) is include/rtsync.h's; ``tempo.path_tempo``
        gives the whole curve of a path, whose entry i is this call's answer when point i was the newest.  Synchronises."""
        slope = torch.empty(self.B, dtype=torch.float64, device=self.device)
        pos = torch.empty(self.B, dtype=torch.float64, device=self.device)
        n = torch.empty(self.B, dtype=torch.int32, device=self.device)
        nat.check(self._fn("tempo")(self._h, int(K), float(ahead), slope.data_ptr(), pos.data_ptr(), n.data_ptr(),
                                    self._stream()))
        return slope.cpu().numpy(), pos.cpu().numpy(), n.cpu().numpy()

    @nat.on_device
    def consensus(self, ens, tables, pieces, frame0=None):
        """Where is every group of streams, in beats (rts_otw_consensus / rts_wtw_consensus)?  One fusion step of
        ``ens`` (an ``ensemble.Ensemble`` of this handle's B streams) from the paths as they stand: every member's beat is
        the lookup, in ``tables`` (an ``AnnotationTables``), of ``frame0[b]`` + the reference index of its last path point
        in table ``pieces[b]``; the group's consensus is the median of the members that are in.  ``pieces`` / ``frame0``:
        lists or int32 device tensors of B entries, like ``AnnotationTables.beats`` takes them.  Advances the strikes and
        out that ``ens`` carries.  Returns numpy ``dict(consensus, spread float64 [n_groups], n_in, n_valid int32
        [n_groups], dev float64 [B], strikes, out int32 [B])``; NaN / 0 / 0 for a stream in no group.  The definition is
        include/rtsync.h's (rts_ensemble_create).  Synchronises."""
        from .ensemble import tracker_consensus
        return tracker_consensus(self, self._fn("consensus"), ens, tables, pieces, frame0)

    @nat.on_device
    def restart(self, streams, refs=None, offsets=None):
        """Put the listed streams back to the start while the others keep running (the subclasses document ``refs`` and
        ``offsets``)."""
        mask, first, lens, pieces = self._restart_tables(streams, refs, offsets)
        nat.check(self._fn("restart")(self._h, mask.ctypes.data, first.ctypes.data if first is not None else None,
                                      lens.ctypes.data if lens is not None else None, self._stream()))
        self._restarted(first, lens, pieces)

    @nat.on_device
    def locate(self, queries, q_len=None, euclid=None, matches=1):
        """Where in the repertoire is each microphone?  ``queries``: the last frames every stream heard -- a device
        tensor [B][M_max][12] (frame-major like ``push`` takes them), or a list of B arrays (12, M_b) in the
        reference's layout; at most 256 frames.  ``q_len``: valid frames per stream for the tensor form (list of ints
        or int32 device tensor; a stream with 0 gets an empty answer).  ``euclid``: cost kind, None = the tracker's
        own.  Needs a handle made by ``with_references``.

        Returns, per stream, a list of ``(ref_object, start, end, cost)`` for every distinct piece uploaded at create
        (``refs`` + ``extra_refs``), cheapest first, ties in upload order: the excerpt matches frames start..end of
        that piece.  ``restart([b], refs=[ref_object], offsets=[start])`` puts the stream there.  Features must be
        finite (``locate.locate_batch``).  Synchronises.

        ``matches=K`` (2..32): up to K ranked, non-overlapping matches per piece instead of the first minimum alone
        (``locate.locate_matches``) -- an excerpt of a repeated section is found in every pass of the repeat.  Every
        stream's list then holds an entry for every rank of every piece, cheapest first, ties in upload order, then in
        rank order.  ``matches=1`` is the call above, unchanged."""
        from .locate import locate_batch, locate_matches
        if self._pool is None:
            raise ValueError("locate needs a handle made by with_references")
        if not torch.is_tensor(queries):
            lens = [int(q.shape[1]) for q in queries]
            buf = torch.zeros((len(queries), max(max(lens), 1), 12), dtype=self.ref.dtype)
            for b, q in enumerate(queries):
                q = torch.from_numpy(np.ascontiguousarray(q)) if isinstance(q, np.ndarray) else q
                buf[b, :lens[b]] = q.t().to(self.ref.dtype)
            queries, q_len = buf, lens
        queries = queries.to(self.device)
        if queries.dim() != 3 or queries.shape[0] != self.B or queries.shape[2] != 12:
            raise ValueError("queries must be [B][M_max][12] with B = %d" % self.B)
        if q_len is not None and not torch.is_tensor(q_len):
            q_len = torch.tensor([int(n) for n in q_len], dtype=torch.int32)
        if q_len is not None:
            q_len = q_len.to(self.device)
        pieces = list(self._pool.values())
        if getattr(self, "_piece_tables", None) is None:
            self._piece_tables = (torch.tensor([f for _, f, _ in pieces], dtype=torch.int64, device=self.device),
                                  torch.tensor([n for _, _, n in pieces], dtype=torch.int32, device=self.device))
        if euclid is None:
            euclid = bool(getattr(self, "euclid", False))
        if int(matches) != 1:
            cost, end, start, n = (t.cpu().numpy() for t in locate_matches(queries, q_len, self.ref, *self._piece_tables,
                                                                           int(matches), euclid=euclid))
            out = []
            for b in range(self.B):
                # n = -1 (pieces that share pool frames; with_references never builds such a pool): slot 0 alone
                ranks = [(p, r) for p in range(len(pieces)) for r in range(max(int(n[b, p]), -int(n[b, p])))
                         if np.isfinite(cost[b, p, r]) and end[b, p, r] >= 0]
                ranks.sort(key=lambda pr: (cost[b, pr[0], pr[1]], pr[0], pr[1]))
                out.append([(pieces[p][0], int(start[b, p, r]), int(end[b, p, r]), float(cost[b, p, r])) for p, r in ranks])
            return out
        cost, end, start = (t.cpu().numpy() for t in
                            locate_batch(queries, q_len, self.ref, *self._piece_tables, euclid=euclid))
        out = []
        for b in range(self.B):
            order = sorted((p for p in range(len(pieces)) if np.isfinite(cost[b, p]) and end[b, p] >= 0),
                           key=lambda p: (cost[b, p], p))
            out.append([(pieces[p][0], int(start[b, p]), int(end[b, p]), float(cost[b, p])) for p in order])
        return out

    @nat.on_device
    def recent(self, M=128, streams=None):
        """The last frames every stream heard, from the tracker's own history (rts_otw_recent / rts_wtw_recent): device
        tensors ``(frames [B][M][12] float64, lens int32 [B])``, ``frames[b, :lens[b]]`` being the last ``lens[b] =
        min(M, consumed)`` frames of stream b in order and zeros behind them -- what ``locate`` takes as ``queries`` /
        ``q_len``.  ``streams``: only these (the others get lens 0 and zeros).  Frames consumed since create, ``reset`` or
        the stream's last ``restart``; at most 256.  Asynchronous, nothing is read back."""
        M = int(M)
        frames = torch.empty((self.B, max(M, 0), 12), dtype=torch.float64, device=self.device)
        lens = torch.empty(self.B, dtype=torch.int32, device=self.device)
        mask = None
        if streams is not None:
            mask = self._restart_tables(streams, None, None)[0]
            mask = torch.from_numpy(mask).to(self.device)
        nat.check(self._fn("recent")(self._h, M, frames.data_ptr(), lens.data_ptr(),
                                     mask.data_ptr() if mask is not None else None, self._stream()))
        return frames, lens

    def locate_recent(self, M=128, streams=None, euclid=None, matches=1):
        """``locate`` on what the streams heard last: ``recent(M, streams)`` handed to ``locate``.  Same return value;
        streams not listed get ``[]``."""
        frames, lens = self.recent(M, streams)
        return self.locate(frames, lens, euclid, matches)

    def reacquire(self, streams, M=128, matches=1, choose=None):
        """This microphone is lost: put it where it really is.  For the listed streams: take the last ``M`` frames each
        heard (``recent``, before anything is cleared), ``locate`` them in the repertoire, ``restart`` every stream
        that got an answer onto the cheapest ``(piece, start)``, and ``push`` its excerpt into the restarted tracker, so
        that it re-follows those frames from ``start`` and stands at "now" instead of M frames behind.  One restart
        and one push in all; the other streams receive no frame and no restart.  Returns ``{b: (piece, start, end,
        cost) | None}`` (None: nothing heard yet, nothing changed).  Whether a stream is lost is the caller's decision:
        compare ``path_cost`` with ``cost / (M + end - start + 1)`` of a ``locate_recent``.  Synchronises (locate).

        A piece that repeats a section holds several equally good matches, and the cheapest entry is the earliest of
        them.  ``matches=K`` searches with ``locate(..., matches=K)``; ``choose(b, candidates) -> index | None`` picks the
        candidate stream b is restarted on (``candidates``: its list, a ``locate.Candidates`` whose ``M`` is the number
        of frames the excerpt has; None: leave this stream alone, it is reported as None).  Without ``choose`` the first
        candidate is taken; ``locate.nearest_to`` builds one that prefers the pass nearest to where the stream was."""
        return self._reacquire(streams, M, self.restart, matches, choose)

    def _reacquire(self, streams, M, restart, matches=1, choose=None):
        streams = list(dict.fromkeys(int(b) for b in streams))
        frames, lens = self.recent(M, streams)
        found = self.locate(frames, lens, None, matches)
        if choose is None:
            out = {b: (found[b][0] if found[b] else None) for b in streams}
        else:
            from .locate import Candidates
            heard, out = lens.cpu().numpy(), {}
            for b in streams:
                cand = Candidates(found[b])
                cand.M = int(heard[b])
                k = choose(b, cand) if cand else None
                out[b] = cand[int(k)] if k is not None else None
        moved = [b for b in streams if out[b] is not None]
        if moved:
            restart(moved, refs=[out[b][0] for b in moved], offsets=[out[b][1] for b in moved])
            keep = torch.from_numpy(self._restart_tables(moved, None, None)[0]).to(self.device)
            self.push(frames, lens * keep.to(torch.int32))
        return out

    # ---- snapshots -----------------------------------------------------------------------------
    def _range_of(self, b):
        """(first pool frame, frames) of the range stream b follows, and (frames of its piece, offset inside it)."""
        if self._pool is None:
            n = int(self.ref.shape[0])
            return 0, n, n, 0
        f, n = self._piece[b]
        rl = int(self.ref_lens[b])
        return f + n - rl, rl, n, n - rl

    @nat.on_device
    def export_streams(self, streams, verify=False, blob=None):
        """The carried state of the listed streams as a ``snapshot.Snapshot`` (rts_otw_export / rts_wtw_export): record
        i is ``streams[i]``.  Asynchronous on the current stream; the handle is only read.  ``verify``: also record a
        digest of every stream's reference range (synchronises), which ``import_streams`` holds against the slot it is
        given.  ``blob``: a uint8 device tensor [n][>= rts_*_snapshot_bytes] to write into instead of a new one.
        BatchedOTW: not after ``run`` (those frames are the caller's) and not with the dense mirror attached."""
        from .snapshot import export_streams
        return export_streams(self, streams, verify, blob)

    @nat.on_device
    def import_streams(self, snap, slots, refs=None, offsets=None, verify=True, status=None):
        """Record i of ``snap`` into slot ``slots[i]`` (rts_otw_import / rts_wtw_import): from here on the slot is that
        stream, bit for bit, whatever this handle's batch size, longest reference, slot layout or kernel flavour; the
        tracker's own parameters must be the exporter's.  ``refs`` / ``offsets``: one entry per slot, as in ``restart``
        -- the range the slot moves to (handles made by ``with_references``); without them every slot keeps its range,
        whose length must be the record's.  ``verify``: compare the digests of a snapshot exported with ``verify``.
        Reads the per-stream status back and raises ``RtsyncError`` naming the first stream that refused its record and
        why; such a slot is unchanged, the others are imported.  Synchronises."""
        from .snapshot import import_streams
        return import_streams(self, snap, slots, refs, offsets, verify, status)

    def _init_refs(self, pool, first, lens):
        self._pool = pool
        self._piece = None if pool is None else [(int(f), int(n)) for f, n in zip(first, lens)]

    def _grow_to_pool(self, first, lens):
        """The handle's buffers are sized by the longest range given at create.  When a piece nobody follows yet is the
        longest, stream 0 is created on it and put on its own reference by a restart right away (bit for bit a fresh
        stream, by that call's contract)."""
        f, n = max(((f, n) for _, f, n in self._pool.values()), key=lambda x: x[1])
        if n <= int(lens.max()):
            return first, lens, None
        first0, lens0 = first.copy(), lens.copy()
        first0[0], lens0[0] = f, n

        def fix():
            mask = np.zeros(self.B, dtype=np.uint8)
            mask[0] = 1
            nat.check(self._fn("restart")(self._h, mask.ctypes.data, first.ctypes.data, lens.ctypes.data, self._stream()))
        return first0, lens0, fix

    def _restart_tables(self, streams, refs, offsets):
        """-> (mask uint8 [B], first int64 [B] | None, lens int32 [B] | None, new (first, frames) of the pieces)."""
        streams = [int(b) for b in streams]
        for b in streams:
            if not 0 <= b < self.B:
                raise IndexError("stream %d out of range [0, %d)" % (b, self.B))
        mask = np.zeros(self.B, dtype=np.uint8)
        mask[streams] = 1
        if refs is None and offsets is None:
            return mask, None, None, {}
        if self._pool is None:
            raise ValueError("refs / offsets need a handle made by with_references")
        if refs is not None and len(refs) != len(streams) or offsets is not None and len(offsets) != len(streams):
            raise ValueError("refs / offsets need one entry per listed stream")
        first, lens, pieces = np.zeros(self.B, dtype=np.int64), np.ones(self.B, dtype=np.int32), {}
        for k, b in enumerate(streams):
            if refs is None:
                f, n = self._piece[b]
            else:
                if id(refs[k]) not in self._pool:
                    raise ValueError("stream %d: this reference was not uploaded at create (refs / extra_refs)" % b)
                _, f, n = self._pool[id(refs[k])]
            o = int(offsets[k]) if offsets is not None else 0
            if not 0 <= o < n:
                raise ValueError("stream %d: offset %d outside its reference of %d frames" % (b, o, n))
            first[b], lens[b], pieces[b] = f + o, n - o, (f, n)
        return mask, first, lens, pieces

    def _restarted(self, first, lens, pieces):
        for b, piece in pieces.items():
            self._piece[b] = piece
            self.ref_lens[b] = lens[b]
