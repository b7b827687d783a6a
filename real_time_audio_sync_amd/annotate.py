"""Beats and labels on the device: the ground-truth tables of a repertoire (``AnnotationTables``), the lookup of the
reference's ``get_beat`` / ``get_beat_and_label`` for whole batches of frames, and its accuracy metric
(tests.py:59-137, ``evaluate.AlignmentError.stats``) for a whole corpus of paths in one launch.

``evaluate.py`` stays the host form and the definition: every number here equals its number bit for bit, the squared beat
error included (one float64 addition after the other, in path order).  ``LiveSession.annotate`` binds tables to a live
session; the device then publishes beat and bar label of every microphone with each feed (csrc/annot.hip).
``AnnotationTables.transfer`` carries a table along an alignment path onto the other recording (csrc/pathmap.hip)."""
import ctypes

import numpy as np
import torch

from . import _native as nat
from . import evaluate

THRESHOLDS = evaluate.AlignmentError.THRESHOLDS


def _table(t):
    """(times float64, beats int32, labels list | None) of a CSV path or a (times, beats[, labels]) tuple."""
    if isinstance(t, str):
        t = evaluate.read_annotations(t)
    times = np.asarray(t[0], dtype=np.float64).reshape(-1)
    beats = np.asarray(t[1]).reshape(-1)
    if len(beats) and not np.array_equal(beats, beats.astype(np.int32)):
        raise ValueError("beats must be integers that fit int32")
    labels = t[2] if len(t) > 2 else None
    if len(times) != len(beats) or (labels is not None and len(labels) != len(times)):
        raise ValueError("times, beats and labels of a table must have one length")
    return times, beats.astype(np.int32), (None if labels is None else [str(s) for s in labels])


class AnnotationTables(object):
    def __init__(self, tables, frame_seconds=evaluate.FRAME_SECONDS, device="cuda:0"):
        """``tables``: one entry per piece, each a ground-truth CSV path (``time_seconds,beat[,label]``) or a tuple
        ``(times, beats[, labels])``.  Times must be finite and non-decreasing, beats >= 0, every table needs a row
        (rts_annot_create refuses anything else, naming piece and row).  ``labels[piece]`` holds the label strings of a
        piece (None for a piece without a label column); only "is the label non-empty" goes to the device.
        ``frame_seconds``: seconds per chroma frame, hop_size / fs."""
        self.device = self.dev = torch.device(device)
        if self.device.index is None:
            self.device = self.dev = torch.device(self.device.type, torch.cuda.current_device())
        parsed = [_table(t) for t in tables]
        self.P = len(parsed)
        self.times = [p[0] for p in parsed]
        self.beat_rows = [p[1] for p in parsed]
        self.labels = [p[2] for p in parsed]
        self.frame_seconds = float(frame_seconds)
        lens = np.array([len(t) for t in self.times], dtype=np.int32)
        first = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)]).astype(np.int64) if self.P else np.zeros(0, np.int64)
        times = np.ascontiguousarray(np.concatenate(self.times)) if self.P else np.zeros(0)
        beats = np.ascontiguousarray(np.concatenate(self.beat_rows)) if self.P else np.zeros(0, np.int32)
        flags = None
        if any(l is not None for l in self.labels):   # a piece without a label column: every row counts as labelled
            flags = np.ascontiguousarray(np.concatenate(
                [np.ones(n, np.uint8) if l is None else np.array([1 if s else 0 for s in l], dtype=np.uint8).reshape(-1)
                 for n, l in zip(lens, self.labels)]))
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            nat.check(nat.lib.rts_annot_create(self.P, len(times), first.ctypes.data, lens.ctypes.data, times.ctypes.data,
                                               beats.ctypes.data, flags.ctypes.data if flags is not None else None,
                                               self.frame_seconds, ctypes.byref(h)))
        self._h = h

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _i32(self, v, n, what):
        t = v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, dtype=np.int32).reshape(-1))
        t = t.to(device=self.device, dtype=torch.int32).contiguous()
        if t.numel() != n:
            raise ValueError("%s: %d entries for %d streams / pairs" % (what, t.numel(), n))
        return t

    # ---- lookup -----------------------------------------------------------------------------------------------
    @nat.on_device
    def beats(self, frames, pieces, frame0=None, n=None):
        """``get_beat`` of many frames.  ``frames``: a list of B integer arrays (one per stream, any lengths), or an
        int32 device tensor [B][n_max] with ``n`` (valid entries per stream; None = all).  ``pieces``: the table of
        every stream; ``frame0``: added to every frame of the stream (where its reference range starts inside its
        piece).  A negative frame or a piece that does not exist has no beat.

        List form: synchronises and returns a list of ``(beat float64 (NaN = none), seg int32 (-1 = none))`` arrays.
        Tensor form: asynchronous; returns device tensors ``(beat [B][n_max], seg [B][n_max])`` whose entries behind
        ``n[b]`` are not written."""
        as_list = not torch.is_tensor(frames)
        if as_list:
            rows = [np.asarray(f, dtype=np.int32).reshape(-1) for f in frames]
            B, n_max = len(rows), max([len(r) for r in rows] + [0])
            host = np.zeros((B, max(n_max, 1)), dtype=np.int32)
            for b, r in enumerate(rows):
                host[b, :len(r)] = r
            frames = torch.from_numpy(host).to(self.device)
            n = [len(r) for r in rows]
        frames = frames.to(device=self.device, dtype=torch.int32).contiguous()
        B, n_max = int(frames.shape[0]), int(frames.shape[1])
        pieces = self._i32(pieces, B, "pieces")
        frame0 = self._i32(frame0, B, "frame0") if frame0 is not None else None
        n = self._i32(n, B, "n") if n is not None else None
        beat = torch.empty((B, n_max), dtype=torch.float64, device=self.device)
        seg = torch.empty((B, n_max), dtype=torch.int32, device=self.device)
        nat.check(nat.lib.rts_annot_beats(self._h, frames.data_ptr(), n_max, n.data_ptr() if n is not None else None,
                                          pieces.data_ptr(), frame0.data_ptr() if frame0 is not None else None, B,
                                          beat.data_ptr(), seg.data_ptr(), self._stream()))
        if not as_list:
            return beat, seg
        beat, seg = beat.cpu().numpy(), seg.cpu().numpy()
        return [(beat[b, :len(r)].copy(), seg[b, :len(r)].copy()) for b, r in enumerate(rows)]

    @nat.on_device
    def frames(self, beats, pieces, n=None):
        """The way back, beat -> frame of a piece (rts_annot_frames; ``ensemble.frames_of_beat`` is the host form): the
        frame whose ``beats()`` lookup is nearest to the beat, -1 where there is none -- a NaN beat, a piece that does not
        exist or whose beats are not strictly increasing, a beat behind the table's last, in a gap of it, or more than
        one beat before its first row.  ``beats``: a list of B float arrays (one per stream, any lengths), or a float64
        device tensor [B][n_max] with ``n`` (valid entries per stream; None = all).  ``pieces``: the table of every stream.

        List form: synchronises and returns a list of int32 arrays.  Tensor form: asynchronous; returns an int32 device
        tensor [B][n_max] whose entries behind ``n[b]`` are not written."""
        as_list = not torch.is_tensor(beats)
        if as_list:
            rows = [np.asarray(x, dtype=np.float64).reshape(-1) for x in beats]
            B, n_max = len(rows), max([len(r) for r in rows] + [0])
            host = np.zeros((B, max(n_max, 1)), dtype=np.float64)
            for b, r in enumerate(rows):
                host[b, :len(r)] = r
            beats = torch.from_numpy(host).to(self.device)
            n = [len(r) for r in rows]
        beats = beats.to(device=self.device, dtype=torch.float64).contiguous()
        B, n_max = int(beats.shape[0]), int(beats.shape[1])
        pieces = self._i32(pieces, B, "pieces")
        n = self._i32(n, B, "n") if n is not None else None
        out = torch.empty((B, n_max), dtype=torch.int32, device=self.device)
        nat.check(nat.lib.rts_annot_frames(self._h, beats.data_ptr(), n_max, n.data_ptr() if n is not None else None,
                                           pieces.data_ptr(), B, out.data_ptr(), self._stream()))
        if not as_list:
            return out
        out = out.cpu().numpy()
        return [out[b, :len(r)].copy() for b, r in enumerate(rows)]

    @nat.on_device
    def bpm(self, frames, slopes, pieces, frame0=None, n=None):
        """Slopes of a path (reference frames per live frame: ``tempo.path_tempo``, ``BatchedOTW.tempo``) in beats per
        minute (rts_annot_bpm): ``(slope * 60.0) / (times[i] - start)`` with ``i`` and ``start`` what ``beats()`` uses for
        the same frame, one beat per table segment.  NaN where the frame has no row, the row has no width, or the slope is
        NaN.  ``frames`` / ``slopes``: lists of B arrays of equal lengths per stream (synchronises, returns a list of
        float64 arrays), or device tensors int32 / float64 [B][n_max] with ``n`` (asynchronous, returns a device tensor
        whose entries behind ``n[b]`` are not written).  ``pieces`` / ``frame0`` as for ``beats()``."""
        as_list = not torch.is_tensor(frames)
        if as_list:
            rows = [np.asarray(f, dtype=np.int32).reshape(-1) for f in frames]
            srows = [np.asarray(s, dtype=np.float64).reshape(-1) for s in slopes]
            if len(rows) != len(srows) or any(len(r) != len(s) for r, s in zip(rows, srows)):
                raise ValueError("frames and slopes must have the same lengths")
            B, n_max = len(rows), max([len(r) for r in rows] + [0])
            host, shost = np.zeros((B, max(n_max, 1)), dtype=np.int32), np.zeros((B, max(n_max, 1)), dtype=np.float64)
            for b, (r, s) in enumerate(zip(rows, srows)):
                host[b, :len(r)] = r
                shost[b, :len(s)] = s
            frames, slopes = torch.from_numpy(host).to(self.device), torch.from_numpy(shost).to(self.device)
            n = [len(r) for r in rows]
        frames = frames.to(device=self.device, dtype=torch.int32).contiguous()
        slopes = slopes.to(device=self.device, dtype=torch.float64).contiguous()
        if tuple(frames.shape) != tuple(slopes.shape) or frames.dim() != 2:
            raise ValueError("frames and slopes must both be [B][n_max]")
        B, n_max = int(frames.shape[0]), int(frames.shape[1])
        pieces = self._i32(pieces, B, "pieces")
        frame0 = self._i32(frame0, B, "frame0") if frame0 is not None else None
        n = self._i32(n, B, "n") if n is not None else None
        out = torch.empty((B, n_max), dtype=torch.float64, device=self.device)
        nat.check(nat.lib.rts_annot_bpm(self._h, frames.data_ptr(), slopes.data_ptr(), n_max,
                                        n.data_ptr() if n is not None else None, pieces.data_ptr(),
                                        frame0.data_ptr() if frame0 is not None else None, B, out.data_ptr(), self._stream()))
        if not as_list:
            return out
        out = out.cpu().numpy()
        return [out[b, :len(r)].copy() for b, r in enumerate(rows)]

    # ---- transfer ---------------------------------------------------------------------------------------------
    @nat.on_device
    def transfer_times(self, path, path_len, pieces, from_side, offsets=None):
        """The raw transfer (rts_annot_transfer): device tensors ``path`` int32 [B][P_max][2] and ``path_len`` int32 [B]
        -> device tensors ``(times float64 [B][rows_max], n_rows int32 [B], status int32 [B])``, rows_max the longest table
        of the handle; entries behind ``n_rows[b]`` are not written.  Asynchronous."""
        from . import pathmap
        path, path_len = pathmap.pack_paths((path, path_len), self.device)
        B, P_max = int(path.shape[0]), int(path.shape[1])
        pieces = self._i32(pieces, B, "pieces")
        off = pathmap.pack_offsets(offsets, B, self.device)
        rows_max = max([len(t) for t in self.times] + [1])
        times = torch.empty((B, rows_max), dtype=torch.float64, device=self.device)
        n_rows = torch.empty((B,), dtype=torch.int32, device=self.device)
        status = torch.empty((B,), dtype=torch.int32, device=self.device)
        nat.check(nat.lib.rts_annot_transfer(self._h, path.data_ptr() if P_max else None, P_max, path_len.data_ptr(),
                                             off.data_ptr() if off is not None else None, int(from_side), pieces.data_ptr(),
                                             B, rows_max, times.data_ptr(), n_rows.data_ptr(), status.data_ptr(),
                                             self._stream()))
        return times, n_rows, status

    def transfer(self, paths, pieces, from_side, offsets=None):
        """Carry tables along alignment paths: pair k's table ``pieces[k]`` belongs to the recording in column
        ``from_side`` of ``paths[k]``, and the result is that table on the time axis of the recording in the other column
        (include/rtsync.h, rts_path_map: the time of every row, in frames, mapped along the path).  ``paths`` as
        ``path_errors`` takes them; ``offsets``: None or two integers per pair, added to column 0 and column 1 of its path.

        Returns ``(tables, dropped)``: ``tables[k]`` a tuple ``(times, beats, labels)`` ready for ``AnnotationTables([...])``
        -- the rows with an image, beat numbers and label strings unchanged (labels None for a piece without a label
        column), times replaced -- and ``dropped[k]`` the indices of the rows that lie before the first or behind the last
        aligned frame.  The map does not decrease, so a kept table passes rts_annot_create's rules.  Raises ValueError for
        a refused path, a piece that does not exist or a pair with no row left, naming the pairs.  Synchronises."""
        from . import pathmap
        path, plen = pathmap.pack_paths(paths, self.device)
        if int(path.shape[0]) < 1:
            return [], []
        pieces = [int(p) for p in (pieces.tolist() if torch.is_tensor(pieces) else pieces)]
        missing = [k for k, p in enumerate(pieces) if p < 0 or p >= self.P]
        if missing:
            raise ValueError("transfer: pair%s %s: no such piece" % ("s" if len(missing) > 1 else "",
                                                                     ", ".join(str(k) for k in missing)))
        times, n_rows, status = self.transfer_times(path, plen, pieces, from_side, offsets)
        times, n_rows, status = times.cpu().numpy(), n_rows.cpu().numpy(), status.cpu().numpy()
        bad = pathmap.refusals(status)
        if bad:
            raise ValueError("transfer: " + pathmap.refusal_message(bad))
        tables, dropped = [], []
        for k, p in enumerate(pieces):
            new = times[k, :int(n_rows[k])]
            keep = np.flatnonzero(np.isfinite(new))
            tables.append((new[keep].copy(), self.beat_rows[p][keep].copy(),
                           None if self.labels[p] is None else [self.labels[p][r] for r in keep]))
            dropped.append([int(r) for r in np.flatnonzero(~np.isfinite(new))])
        empty = [k for k, t in enumerate(tables) if len(t[0]) == 0]
        if empty:
            raise ValueError("transfer: pair%s %s: no row of the table lies on the aligned stretch"
                             % ("s" if len(empty) > 1 else "", ", ".join(str(k) for k in empty)))
        return tables, dropped

    # ---- metric -----------------------------------------------------------------------------------------------
    @nat.on_device
    def path_error_counts(self, path, path_len, pieces0, pieces1):
        """The raw metric (rts_annot_path_error): device tensors ``path`` int32 [B][P_max][2] and ``path_len`` int32 [B]
        (the layout of ``dtw.dtw_paths``: column 0 the live side, column 1 the reference side) -> device tensors
        ``(squared_beat_error float64 [B], counts int32 [B][10])``, counts being count, points off by more than 1, 3,
        5, 10 beats, by more than 1, 3, 5, 10 seconds, index errors.  Asynchronous."""
        path = path.to(device=self.device, dtype=torch.int32).contiguous()
        B, P_max = int(path.shape[0]), int(path.shape[1])
        path_len = self._i32(path_len, B, "path_len")
        pieces0, pieces1 = self._i32(pieces0, B, "pieces0"), self._i32(pieces1, B, "pieces1")
        sq = torch.empty((B,), dtype=torch.float64, device=self.device)
        counts = torch.empty((B, nat.ANNOT_COUNTS), dtype=torch.int32, device=self.device)
        nat.check(nat.lib.rts_annot_path_error(self._h, path.data_ptr() if P_max else None, P_max, path_len.data_ptr(),
                                               pieces0.data_ptr(), pieces1.data_ptr(), B, sq.data_ptr(), counts.data_ptr(),
                                               self._stream()))
        return sq, counts

    def path_errors(self, paths, pieces0, pieces1):
        """``evaluate.AlignmentError(ref_csv, live_csv, path).stats()`` of many recording pairs in one launch.
        ``paths``: a list of (P_k, 2) integer arrays of path points (live frame, reference frame), or the device triple
        ``(path, path_len, total)`` that ``dtw.dtw_paths`` returns (a pair, or ``dtw_subseq_paths``' longer tuple, does
        as well: the first two entries are used).  ``pieces0[k]`` is the table of pair k's live side (column 0),
        ``pieces1[k]`` that of its reference side.

        Returns one dict per pair, shaped like ``stats()`` and equal to it (``count``, ``squared_beat_error``,
        ``pct_off_beats``, ``pct_off_seconds``), or None for a pair none of whose points counted (where ``stats()``
        raises ZeroDivisionError).  Raises IndexError, naming the pairs, when the integer part of a beat is no row of the
        live side's table (``get_time``'s list index, tests.py:130-134).  Synchronises."""
        if isinstance(paths, tuple) and len(paths) >= 2 and torch.is_tensor(paths[0]):
            path, plen = paths[0], paths[1]
        else:
            arrs = [np.asarray(p, dtype=np.int32).reshape(-1, 2) for p in paths]
            host = np.zeros((len(arrs), max([len(a) for a in arrs] + [1]), 2), dtype=np.int32)
            for k, a in enumerate(arrs):
                host[k, :len(a)] = a
            path = torch.from_numpy(host).to(self.device)
            plen = torch.tensor([len(a) for a in arrs], dtype=torch.int32, device=self.device)
        sq, counts = self.path_error_counts(path, plen, pieces0, pieces1)
        sq, counts = sq.cpu().numpy(), counts.cpu().numpy()
        bad = [k for k in range(len(sq)) if counts[k, 9] > 0]
        if bad:
            raise IndexError("pair%s %s: the integer part of a beat is no row of the live side's table (%s path points)"
                             % ("s" if len(bad) > 1 else "", ", ".join(str(k) for k in bad),
                                ", ".join(str(int(counts[k, 9])) for k in bad)))
        out = []
        for k in range(len(sq)):
            count = int(counts[k, 0])
            if count == 0:
                out.append(None)
                continue
            out.append(dict(count=count, squared_beat_error=float(sq[k]),
                            pct_off_beats={t: float(v) / count * 100 for t, v in zip(THRESHOLDS, counts[k, 1:5].tolist())},
                            pct_off_seconds={t: float(v) / count * 100 for t, v in zip(THRESHOLDS, counts[k, 5:9].tolist())}))
        return out

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                torch.cuda.synchronize(self.device)
            except Exception:
                pass
            nat.destroy_on(self.device, nat.lib.rts_annot_destroy, h)

    __del__ = close
