"""Many live audio streams followed against one reference (or one reference each), entirely on the device.

This is the batched form of the reference's microphone loops (livenote_live.py:161-209 for the OTW family,
wtw.py:71-93 for WTW): audio arrives in buffers of arbitrary size; whenever a stream has at least ``fft_len``
pending samples, every complete hop becomes a chroma column (un-padded framing, chroma.py:35-42) and is inserted
into that stream's alignment state; ``hop_size`` samples are dropped per column (livenote_live.py:208).

All of it happens behind ``rts_live_*`` (csrc/live.hip): per feed ONE host-to-device copy from a pinned staging slot
and a fixed chain of launches, nothing read back -- the pending samples live in per-stream device buffers, and the
device publishes status and position of every stream into host-mapped memory, which ``poll()`` reads without
touching the stream.  The host only mirrors the pending-sample counts (integer arithmetic).

``features="chroma_diff"`` hands the trackers the half-wave rectified difference of consecutive chroma columns instead
(chroma.py:77-90): with ``variant="livenote_v2", euclid=True`` and a ``wav_to_chroma_diff`` reference this is the
reference's headline configuration (tests.py:145-163) from microphones."""
import ctypes

import numpy as np
import torch

from . import _native as nat
from .chroma import ChromaPlan, ResamplePlan
from .otw_batch import BatchedOTW

_KINDS = {np.dtype(np.float32): nat.F32, np.dtype(np.int16): nat.I16}
_FEATURES = {"chroma": nat.FEATURE_CHROMA, "chroma_diff": nat.FEATURE_CHROMA_DIFF}


class _DeviceView(object):
    """Library-owned device memory as something torch.as_tensor wraps without a copy."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2)


class LiveSession(object):
    def __init__(self, ref_chroma, batch, c=500, max_run_count=3, variant="otw", fft_len=4096, hop_size=2048,
                 fs=22050, max_pending=1 << 16, device="cuda:0", wtw_params=None, extra_refs=(), features="chroma",
                 euclid=False, fs_in=None, tuning=None):
        """``ref_chroma``: (12, N) reference chroma (e.g. chroma.wav_to_chroma(ref_path)), or a list of ``batch`` such
        arrays, one per stream (one piece per microphone; a list entry that repeats is uploaded once).  With
        ``wtw_params`` ({'dtw_win_size', 'dtw_hop_size'} in samples, like wtw.py:29-30) the streams are followed by
        windowed time warping instead of ``variant`` ('otw' | 'livenote' | 'livenote_v2').  ``extra_refs`` (with a list
        of references only): further pieces uploaded at create, which ``restart`` may move a microphone on to.

        ``features``: 'chroma' (the normalised chroma columns) or 'chroma_diff': column m handed to the tracker is
        ``np.clip(np.diff(chroma), 0, inf)[:, m]`` of the columns the ingestion makes, so a stream's tracker gets its
        first frame with the stream's second chroma column, and ``ref_chroma`` must itself be difference features
        (chroma.wav_to_chroma_diff).  The previous chroma column of every stream is carried on the device; ``restart``
        drops it for the listed streams and ``reset`` for all, like their pending samples.  Not available with
        ``wtw_params`` (the reference never runs WTW on difference features; its cosine cost is NaN on their zero
        columns).  ``euclid``: the OTW family's Euclidean cost (livenote_v2.py:168) instead of 1 - dot; the reference
        pairs it with either feature kind (tests.py:156).

        ``fs_in``: the microphones' own sample rate.  None or ``fs`` gives the ordinary session.  Anything else puts the
        device resampler (chroma.ResamplePlan) in front of the chain: ``feed``, ``feed_block`` and ``staging`` then take
        samples at ``fs_in``, ``max_pending`` and ``pending()`` stay in samples at ``fs``, and a stream that has been
        fed n samples has handed ``resampler.avail(n)`` samples on, the same ones however the input was cut.

        ``tuning``: the microphones' offset from A4 = 440 Hz in cents (``chroma.estimate_tuning_batch`` of a sound
        check finds it), handed to the session's ``ChromaPlan``; None is the 440 Hz filterbank.  One offset per
        session -- the chroma kernels share one filterbank among the streams of a pass -- reported as
        ``session.tuning``.  It changes the table the plan uploads and nothing a feed enqueues."""
        if features not in _FEATURES:
            raise ValueError("features must be 'chroma' or 'chroma_diff', not %r" % (features,))
        if features == "chroma_diff" and wtw_params is not None:
            raise ValueError("features='chroma_diff' is not available with wtw_params (WTW's cosine cost is NaN on the "
                             "zero columns of difference features)")
        if euclid and wtw_params is not None:
            raise ValueError("euclid selects the OTW family's cost; WTW has its own (wtw_params)")
        self.features = features
        self.plan = ChromaPlan(fft_len, hop_size, fs, device, tuning=tuning)
        self.tuning = self.plan.tuning
        self.dev = self.device = self.plan.device
        self.B, self.L, self.H = int(batch), int(fft_len), int(hop_size)
        self.cap = int(max_pending)
        per_stream = isinstance(ref_chroma, (list, tuple))
        self._conv = None   # per-stream references: id(object given) -> (object, what the tracker knows it as)
        if per_stream:
            if len(ref_chroma) != self.B:
                raise ValueError("%d references for %d streams" % (len(ref_chroma), self.B))
            conv = self._conv = {}
            for r in list(ref_chroma) + list(extra_refs):
                conv.setdefault(id(r), (r, np.asarray(r, dtype=np.float64)))
            refs = [conv[id(r)][1] for r in ref_chroma]
            extra = [conv[id(r)][1] for r in extra_refs]
        else:
            if len(extra_refs):
                raise ValueError("extra_refs need per-stream references (a list as ref_chroma)")
            ref = np.asarray(ref_chroma, dtype=np.float64)
        self.otw = self.wtw = None
        if wtw_params is None:
            if per_stream:
                self.otw = BatchedOTW.with_references(refs, c, max_run_count, variant=variant, euclid=euclid,
                                                      device=device, dtype=torch.float64, extra_refs=extra)
            else:
                self.otw = BatchedOTW(ref, c, max_run_count, batch=batch, variant=variant, euclid=euclid,
                                      device=device, dtype=torch.float64)
        else:
            from .wtw import BatchedWTW
            win, hopf = wtw_params['dtw_win_size'] // self.H, wtw_params['dtw_hop_size'] // self.H
            if per_stream:
                for k, (r, a) in list(conv.items()):
                    conv[k] = (r, torch.from_numpy(np.ascontiguousarray(a.T)).to(self.dev))
                self._ref_dev = [conv[id(r)][1] for r in ref_chroma]
                self.wtw = BatchedWTW.with_references(self._ref_dev, win, hopf,
                                                      extra_refs=[conv[id(r)][1] for r in extra_refs])
            else:
                self._ref_dev = torch.from_numpy(np.ascontiguousarray(ref.T)).to(self.dev)
                self.wtw = BatchedWTW(self._ref_dev, win, hopf, batch)
        self.resampler = None
        if fs_in is not None and int(fs_in) != int(fs):
            self.resampler = ResamplePlan(fs_in, fs, self.dev)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.dev):
            otw_h, wtw_h = self.otw._h if self.otw else None, self.wtw._h if self.wtw else None
            if self.resampler is None:
                nat.check(nat.lib.rts_live_create_features(self.plan._h, otw_h, wtw_h, self.B, self.cap,
                                                           _FEATURES[features], ctypes.byref(h)))
            else:
                nat.check(nat.lib.rts_live_create_resampled(self.plan._h, otw_h, wtw_h, self.B, self.cap,
                                                            _FEATURES[features], self.resampler._h, ctypes.byref(h)))
        self._h = h
        self._status = np.zeros(self.B, dtype=np.int32)
        self._pos = np.zeros((self.B, 2), dtype=np.int32)
        self.fs = int(fs)
        self._gated = False                                  # gate() has made the handle's gate buffers
        self._direct = np.zeros(self.B, dtype=np.int64)      # frames reacquire() pushed into the tracker since a restart
        self._annot = None                                   # the AnnotationTables annotate() bound, while they are on
        self._annot_of = self._annot_piece = self._last_tables = None   # pool frame -> table; table of each stream; for label_text
        # accompany(): the warp plan and the uploaded pool of tracks with the key they were made for, the objects given (kept
        # alive: the pool is recognised by their identity), per stream (first, len, origin) while it is on, the parameters,
        # and the arrays accompaniment() reads the words into
        self._acc_plan = self._acc_pool = self._acc_key = self._acc_tracks = self._acc_par = self._acc_words = None
        self._acc_given = {}

    # ---- feeding ----------------------------------------------------------------------------------------------
    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def staging(self, dtype=np.float32):
        """The next pinned staging slot as numpy views: (counts int32 [B], samples `dtype` [B * max_pending], or with
        ``fs_in`` the input-rate capacity rts_live_staging reports).  Write
        the new sample count of every stream and the samples of all streams packed back to back in stream order, then
        call ``submit(dtype)``.  A producer that writes here directly (an audio callback, a socket reader) saves the
        copy ``feed`` makes."""
        counts, samples, capn = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_longlong()
        nat.check(nat.lib.rts_live_staging(self._h, ctypes.byref(counts), ctypes.byref(samples), ctypes.byref(capn)))
        dt = np.dtype(dtype)
        cv = np.ctypeslib.as_array(ctypes.cast(counts.value, ctypes.POINTER(ctypes.c_int32)), shape=(self.B,))
        ctype = ctypes.c_float if dt == np.float32 else ctypes.c_int16
        sv = np.ctypeslib.as_array(ctypes.cast(samples.value, ctypes.POINTER(ctype)), shape=(capn.value,))
        return cv, sv

    @nat.on_device
    def submit(self, dtype=np.float32):
        """Enqueue the feed written into the staging slot (asynchronous; nothing is read back)."""
        nat.check(nat.lib.rts_live_submit(self._h, _KINDS[np.dtype(dtype)], self._stream()))

    def feed_block(self, block):
        """``block``: (B, n) float32 or int16 -- the same number of new samples for every stream (a multi-channel
        interface): one copy into the staging slot, one submit."""
        block = np.asarray(block)
        assert block.ndim == 2 and block.shape[0] == self.B and block.dtype in _KINDS
        cv, sv = self.staging(block.dtype)
        cv[:] = block.shape[1]
        sv[:block.size] = block.reshape(-1)
        self.submit(block.dtype)

    def feed(self, buffers, wait=False):
        """``buffers``: one array of new samples per stream (None / empty = nothing new), int16 (PCM16) or float; the
        feed goes out as int16 when every buffer is int16, else as float32 with the int16 buffers scaled by 1/32768
        (the value the device would have made of them).  Asynchronous: returns the
        streams known to have reached the end of the reference ("stop", livenote_live.py:188-190) according to what
        the device has published so far -- the result of this very feed shows up in a later call, or at once with
        ``wait=True`` (which synchronises the stream)."""
        assert len(buffers) == self.B
        dt = np.int16 if all(x is None or np.asarray(x).dtype == np.int16 for x in buffers) else np.float32
        cv, sv = self.staging(dt)
        off = 0
        for b, x in enumerate(buffers):
            n = 0 if x is None else len(x)
            cv[b] = n
            if n:
                if dt is np.float32 and np.asarray(x).dtype == np.int16:
                    # mixed feed: PCM16 next to float buffers goes out as float32, scaled like the device scales (exact)
                    x = np.asarray(x).astype(np.float32) / np.float32(32768.0)
                sv[off:off + n] = x
                off += n
        self.submit(dt)
        if wait:
            self.sync()
        return self.stopped()

    # ---- results ----------------------------------------------------------------------------------------------
    def poll(self):
        """Non-blocking: {'status' [B], 'positions' [B][2] (live frame, reference frame), 'feeds_done',
        'feeds_submitted'} as last published by the device."""
        done, sub = ctypes.c_int(), ctypes.c_int()
        nat.check(nat.lib.rts_live_poll(self._h, self._status.ctypes.data, self._pos.ctypes.data, ctypes.byref(done),
                                        ctypes.byref(sub)))
        return dict(status=self._status.copy(), positions=self._pos.copy(), feeds_done=done.value, feeds_submitted=sub.value)

    def stopped(self):
        st = self.poll()["status"]
        return [int(b) for b in np.nonzero(st == nat.STOP_REF_END)[0]]

    def pending(self):
        out = np.zeros(self.B, dtype=np.int64)
        nat.check(nat.lib.rts_live_pending(self._h, out.ctypes.data))
        return out

    def last_columns(self):
        """(cols [B][rows][12] float64, n_cols [B] int32): device tensors that view, without a copy, the columns the most
        recently submitted feed handed to the trackers and how many of them each stream had -- the chroma columns, or
        with ``features='chroma_diff'`` the difference columns.  ``rows`` is that feed's largest chroma column count of
        a stream (0 when it completed none); stream b's columns are ``cols[b, :n_cols[b]]``.  The contents belong to
        the last feed in stream order: ``sync()`` first, or consume them on the same stream.  The memory is the
        session's: the next feed overwrites it, and the views die with the session."""
        cols, n_cols, cap, rows = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int()
        nat.check(nat.lib.rts_live_columns_view(self._h, ctypes.byref(cols), ctypes.byref(cap), ctypes.byref(rows),
                                                ctypes.byref(n_cols)))
        n = torch.as_tensor(_DeviceView(n_cols.value, (self.B,), "<i4"), device=self.dev)
        if rows.value == 0:
            return torch.empty((self.B, 0, 12), dtype=torch.float64, device=self.dev), n
        return torch.as_tensor(_DeviceView(cols.value, (self.B, rows.value, 12), "<f8"), device=self.dev), n

    def sync(self):
        torch.cuda.current_stream(self.dev).synchronize()

    @nat.on_device
    def reset(self):
        """Every stream starts again: pending samples, the carried chroma column of ``features='chroma_diff'`` and the
        tracker state are dropped."""
        nat.check(nat.lib.rts_live_reset(self._h, self._stream()))
        self._direct[:] = 0

    @nat.on_device
    def restart(self, streams, refs=None, offsets=None):
        """Put the listed streams back to the start while the others keep running (rts_live_restart; asynchronous,
        ordered after the feeds already submitted): their pending samples are dropped, their tracker state is fresh,
        ``poll()`` shows them running at the start again.  With ``features='chroma_diff'`` their carried chroma column
        is dropped too: the first chroma column of the new run only becomes the new carry.  ``refs``: one entry per listed stream, each an object given
        at create (``ref_chroma`` list / ``extra_refs``, matched by identity); ``offsets``: first frame inside the
        piece; without ``refs``, "same piece, from this frame"."""
        if refs is not None:
            if self._conv is None or any(id(r) not in self._conv for r in refs):
                raise ValueError("a reference to restart on must have been given at create (ref_chroma list / extra_refs)")
            refs = [self._conv[id(r)][1] for r in refs]
        self._restart_known(streams, refs, offsets)

    @nat.on_device
    def _restart_known(self, streams, refs=None, offsets=None):
        """``restart`` with the references named as the bound tracker knows them."""
        eng = self.otw or self.wtw
        mask, first, lens, pieces = eng._restart_tables(streams, refs, offsets)
        nat.check(nat.lib.rts_live_restart(self._h, mask.ctypes.data, first.ctypes.data if first is not None else None,
                                           lens.ctypes.data if lens is not None else None, self._stream()))
        if self.otw:
            self.otw._version += 1
        eng._restarted(first, lens, pieces)
        self._direct[mask != 0] = 0
        if self._annot is not None and pieces:   # new piece / offset: the beats stay in the piece's own time
            self._annotate_streams(sorted(pieces))
        if self._acc_tracks is not None:   # rts_live_restart disarmed them: the track follows the offset
            self._accompany_streams([int(b) for b in streams])

    # ---- snapshots --------------------------------------------------------------------------------------------
    @nat.on_device
    def export_streams(self, streams, verify=False, blob=None):
        """The carried state of the listed streams as a ``snapshot.Snapshot`` (rts_live_export): the tracker's record, the
        pending samples and, with ``features='chroma_diff'``, the carried chroma column; ``Snapshot.mirror`` holds the two
        host mirror words per stream.  Asynchronous, behind the feeds already submitted; the session is only read.  Not
        for a session that resamples (``fs_in``) or has the gate on."""
        from .snapshot import export_live
        return export_live(self, streams, verify, blob)

    @nat.on_device
    def import_streams(self, snap, slots, refs=None, offsets=None, verify=True, status=None):
        """Record i of ``snap`` (a live session's snapshot) into slot ``slots[i]`` (rts_live_import): from the next feed on
        the slot is that stream, bit for bit.  fft_len, hop, features, max_pending and the tracker's parameters must be the
        exporter's; ``refs`` / ``offsets`` as in ``restart``.  All or nothing: if the device refuses one record the call
        raises ``RtsyncError`` naming the stream, and ``pending()``, ``poll()`` and the tracker are what they were.
        ``poll()`` shows the imported positions at once; confidence, beat and tempo words read empty until the next feed.
        Synchronises."""
        from .snapshot import import_streams
        if refs is not None:
            if self._conv is None or any(id(r) not in self._conv for r in refs):
                raise ValueError("a reference to import onto must have been given at create (ref_chroma list / extra_refs)")
            refs = [self._conv[id(r)][1] for r in refs]
        eng = self.otw or self.wtw
        got = import_streams(eng, snap, slots, refs, offsets, verify, status, live=self)
        if self.otw:
            self.otw._version += 1
        self._direct[[int(s) for s in slots]] = 0
        if self._annot is not None and (refs is not None or offsets is not None):   # the beats stay in the piece's own time
            self._annotate_streams(sorted(int(s) for s in slots))
        return got

    # ---- beats and labels -------------------------------------------------------------------------------------
    def _annotate_streams(self, streams):
        """rts_live_annotate for the listed streams, piece and frame offset taken from what the tracker follows now."""
        eng = self.otw or self.wtw
        mask, piece, frame0 = np.zeros(self.B, np.uint8), np.zeros(self.B, np.int32), np.zeros(self.B, np.int32)
        for b in streams:
            mask[b] = 1
            if self._conv is not None:
                f, n = eng._piece[b]
                if f not in self._annot_of:
                    raise ValueError("stream %d follows a reference that piece_of gives no table for" % b)
                piece[b], frame0[b] = self._annot_of[f], n - int(eng.ref_lens[b])
        nat.check(nat.lib.rts_live_annotate(self._h, self._annot._h, mask.ctypes.data, piece.ctypes.data,
                                            frame0.ctypes.data, self._stream()))
        self._annot_piece[mask != 0] = piece[mask != 0]

    @nat.on_device
    def annotate(self, tables, piece_of=None):
        """Beat and bar label of every microphone with each feed, without a read-back (rts_live_annotate): the last step of
        the reference's loop, ``get_beat_and_label(ln.path[-1][1])`` after every insert (livenote_live.py:197-202).
        ``tables``: an ``annotate.AnnotationTables`` of this device; it must stay open while it is in use here.
        ``piece_of``: with per-stream references, a list of ``(reference, table index)`` pairs, ``reference`` being an
        object given at create (``ref_chroma`` list / ``extra_refs``, matched by identity like ``restart`` does); every
        reference a stream follows needs an entry.  A single-reference session uses table 0.  ``restart`` with ``refs`` /
        ``offsets`` and ``reacquire`` re-issue the call for their streams with the new piece and the offset as the
        piece's frame at which the range starts, so beats stay in the piece's own time after "follow from bar 50".
        With annotations on, each feed enqueues one more small launch; ``beats()`` reads its words.  ``annotate(None)``
        switches annotations off: the words stay as they are.  Allowed at any time; ordered behind the feeds already
        submitted."""
        if tables is None:
            nat.check(nat.lib.rts_live_annotate(self._h, None, None, None, None, self._stream()))
            self._annot = None
            return
        of = {}
        if self._conv is not None:
            eng = self.otw or self.wtw
            for r, idx in (piece_of or ()):
                if id(r) not in self._conv:
                    raise ValueError("piece_of names a reference that was not given at create (ref_chroma list / extra_refs)")
                if not 0 <= int(idx) < tables.P:
                    raise ValueError("piece_of: table %d outside [0, %d)" % (int(idx), tables.P))
                of[eng._pool[id(self._conv[id(r)][1])][1]] = int(idx)
        elif piece_of is not None:
            raise ValueError("piece_of needs per-stream references (a list as ref_chroma)")
        prev = self._annot, self._annot_of
        self._annot, self._annot_of, self._last_tables = tables, of, tables
        if self._annot_piece is None:
            self._annot_piece = np.full(self.B, -1, dtype=np.int32)
            self._beat = np.zeros(self.B, dtype=np.float64)
            self._beat_words = np.zeros((2, self.B), dtype=np.int32)
        try:
            self._annotate_streams(range(self.B))
        except Exception:
            self._annot, self._annot_of = prev
            raise

    def beats(self):
        """Non-blocking: {'beat' float64 [B] (NaN: none yet), 'label' int32 [B] (index into the piece's labels, -1: none
        yet), 'label_text' list (the label string, None where there is none or the piece has no label column),
        'ref_frame' int32 [B] (the frame of the piece looked up last, -1 while the stream has no path point),
        'feeds_done'} as last published by the device.  Beat and label are sticky like the reference's display: a feed
        changes the beat only to a beat that is neither none nor 0.0, and the label only to a non-empty one.  Needs
        ``annotate(tables)`` first."""
        done = ctypes.c_int()
        have = self._annot_piece is not None
        nat.check(nat.lib.rts_live_beats(self._h, self._beat.ctypes.data if have else None,
                                         self._beat_words[0].ctypes.data if have else None,
                                         self._beat_words[1].ctypes.data if have else None, ctypes.byref(done)))
        label = self._beat_words[0].copy()
        tab = self._last_tables
        text = []
        for b in range(self.B):
            names = tab.labels[self._annot_piece[b]] if tab is not None and self._annot_piece[b] >= 0 else None
            text.append(names[label[b]] if names is not None and 0 <= label[b] < len(names) else None)
        return dict(beat=self._beat.copy(), label=label, label_text=text, ref_frame=self._beat_words[1].copy(),
                    feeds_done=done.value)

    def locate(self, queries, q_len=None, euclid=None, matches=1):
        """Where in the repertoire is each microphone?  ``BatchedOTW.locate`` / ``BatchedWTW.locate`` of the bound
        tracker (needs per-stream references: a list as ``ref_chroma``), with the pieces named by the objects given at
        create, so that every entry ``(ref, start, end, cost)`` goes straight into ``restart([b], refs=[ref],
        offsets=[start])``.  The session keeps no history of columns: ``queries`` are what the caller collected from
        ``last_columns()``.  ``matches=K``: up to K ranked non-overlapping matches per piece, as there."""
        found = (self.otw or self.wtw).locate(queries, q_len, euclid, matches)
        given = {id(conv): obj for obj, conv in self._conv.values()}
        return [[(given[id(r)], s, e, c) for r, s, e, c in entries] for entries in found]

    def _given(self, entry):
        """A ``(ref, start, end, cost)`` of the bound tracker with the piece named by the object given at create."""
        given = {id(conv): obj for obj, conv in self._conv.values()}
        return (given[id(entry[0])],) + tuple(entry[1:])

    def locate_recent(self, M=128, streams=None, euclid=None, matches=1):
        """``locate`` on the last ``M`` columns every stream (or the listed ones) handed to its tracker, taken from the
        tracker's own history on the device (``recent`` of the bound tracker): no column is collected on the host.  Same
        return value as ``locate``; streams not listed get ``[]``."""
        if self._conv is None:
            raise ValueError("locate needs per-stream references (a list as ref_chroma)")
        found = (self.otw or self.wtw).locate_recent(M, streams, euclid, matches)
        return [[self._given(e) for e in entries] for entries in found]

    def reacquire(self, streams, M=128, matches=1, choose=None):
        """This microphone is lost: put it where it really is (``BatchedOTW.reacquire`` / ``BatchedWTW.reacquire`` of the
        bound tracker, the pieces named by the objects given at create).  The restart goes through ``restart``: the
        listed streams' pending samples -- and with ``features='chroma_diff'`` their carried chroma column -- are
        dropped as documented there; the excerpt is then pushed into the bound tracker directly, so the position words
        ``poll()`` shows for these streams are those of a fresh stream until the next feed publishes the caught-up
        ones, and ``confidence()`` reads n = 0 until then.  Returns ``{b: (ref, start, end, cost) | None}``.
        ``matches`` / ``choose`` as ``BatchedOTW.reacquire``; ``choose`` sees the pieces as the objects given at create
        (``where`` of ``locate.nearest_to`` names them so)."""
        if self._conv is None:
            raise ValueError("reacquire needs per-stream references (a list as ref_chroma)")
        eng = self.otw or self.wtw
        def chosen(b, cand):   # the caller's choose on the caller's names for the pieces
            named = type(cand)(self._given(e) for e in cand)
            named.M = cand.M
            return choose(b, named)
        out = eng._reacquire(streams, M, self._restart_known, matches, chosen if choose is not None else None)
        if self._gated:   # frame_columns: the excerpt's frames come first in the restarted streams' trackers
            for b, e in out.items():
                if e is not None:
                    self._direct[b] = eng.state(b)["consumed" if self.otw else "chroma_ptr"]
        return {b: (self._given(e) if e is not None else None) for b, e in out.items()}

    # ---- the level gate ---------------------------------------------------------------------------------------
    @nat.on_device
    def gate(self, min_db, hold=0):
        """Keep silence away from the trackers (rts_live_gate): a chroma column is handed on iff the mean square of its
        frame is at least ``10 ** (min_db / 10)`` -- ``min_db`` on the scale of the reference's microphone meter,
        20 log10(rms) (livenote_live.py:170-177) -- or it is among the first ``hold`` columns of a rest.  Every stream
        starts closed and opens with its first loud column: a session may be opened before the downbeat and left
        running between two movements.  With ``features='chroma_diff'`` a difference column is handed on iff both its
        chroma columns passed.  ``gate(None)`` switches the gate off.  Only before the first feed, or right after
        ``reset()``; ``reset`` keeps the setting, ``restart`` closes the listed streams.  Two more small launches per
        feed; nothing is read back."""
        level = 0.0 if min_db is None else 10.0 ** (float(min_db) / 10.0)
        nat.check(nat.lib.rts_live_gate(self._h, level, int(hold)))
        self._gated = self._gated or level > 0.0

    def levels(self):
        """Non-blocking: {'level' float64 [B] (mean square of the frame of every stream's latest chroma column, NaN
        before its first), 'level_db' (10 log10 of it, clipped like the reference's meter clips the rms to
        [1e-10, 1]), 'open' bool [B] (that column passed), 'seen', 'passed' int32 [B] (chroma columns completed /
        columns handed to the tracker since create, reset or the stream's restart), 'feeds_done'} as last published by
        the device.  Needs ``gate(min_db)`` first."""
        level = np.zeros(self.B, dtype=np.float64)
        words = np.zeros((3, self.B), dtype=np.int32)
        done = ctypes.c_int()
        nat.check(nat.lib.rts_live_levels(self._h, level.ctypes.data, words[0].ctypes.data, words[1].ctypes.data,
                                          words[2].ctypes.data, ctypes.byref(done)))
        with np.errstate(invalid="ignore"):
            db = 10.0 * np.log10(np.clip(level, 1e-20, 1.0))
        return dict(level=level, level_db=db, open=words[0] != 0, seen=words[1].copy(), passed=words[2].copy(),
                    feeds_done=done.value)

    @nat.on_device
    def frame_columns(self, b=0):
        """int32 array aligned with the live frames of stream b's tracker: entry t is the ordinal, among the chroma
        columns the stream has completed since create, reset or its restart, of the column that became live frame t (for
        a difference column the later of its two), so that frame t ended ``(ordinal * hop_size + fft_len) / fs``
        seconds into the stream's run.  Frames that ``reacquire`` pushed into the tracker itself come first and read
        -1.  As long as the tracker's history at most.  Waits for the feeds in flight.  Needs ``gate(min_db)`` first."""
        n = ctypes.c_int()
        nat.check(nat.lib.rts_live_gate_columns(self._h, int(b), None, 0, ctypes.byref(n), self._stream()))
        history = 2 * (self.otw.N if self.otw else self.wtw.M)   # ordinals are kept for as many frames as the tracker keeps
        out = np.zeros(min(max(n.value, 0), history), dtype=np.int32)
        if len(out):
            nat.check(nat.lib.rts_live_gate_columns(self._h, int(b), out.ctypes.data, len(out), ctypes.byref(n),
                                                    self._stream()))
        return np.concatenate([np.full(int(self._direct[b]), -1, dtype=np.int32), out])

    @nat.on_device
    def watch(self, K):
        """Tracking confidence with every feed (rts_live_watch): K = 1..256 path points per stream, 0 = off (the
        default).  With watch on, each feed enqueues one more small launch, ``BatchedOTW.path_cost(K)`` of the bound
        tracker published into host-mapped memory; ``confidence()`` reads it.  OTW family only."""
        nat.check(nat.lib.rts_live_watch(self._h, int(K)))
        if getattr(self, "_conf_mean", None) is None:
            self._conf_mean = np.zeros(self.B, dtype=np.float64)
            self._conf_n = np.zeros(self.B, dtype=np.int32)

    def confidence(self):
        """Non-blocking: {'mean' float64 [B], 'n' int32 [B], 'feeds_done'} as last published by the device: the mean
        cell cost over the last ``n`` path points of every stream (NaN with n = 0: no path point yet, or just
        restarted) -- ``BatchedOTW.path_cost`` as of feed ``feeds_done`` or later.  Needs ``watch(K)`` first.  No
        threshold is applied: compare with ``cost / (M + end - start + 1)`` of a ``locate_recent`` entry."""
        done = ctypes.c_int()
        mean = getattr(self, "_conf_mean", None)
        nat.check(nat.lib.rts_live_confidence(self._h, mean.ctypes.data if mean is not None else None,
                                              self._conf_n.ctypes.data if mean is not None else None, ctypes.byref(done)))
        return dict(mean=self._conf_mean.copy(), n=self._conf_n.copy(), feeds_done=done.value)

    @nat.on_device
    def follow_tempo(self, K, ahead=0.0):
        """Tempo of every microphone with every feed (rts_live_follow_tempo): K = 2..1024 path points per stream, 0 = off
        (the default).  With it on, each feed enqueues one more small launch, ``tempo(K, ahead)`` of the bound tracker
        (OTW or WTW) published into host-mapped memory together with beats per minute through the tables of
        ``annotate``; ``tempo()`` reads it.  With the gate on, live indices count the columns the tracker received, so the
        slope is per column handed on; ``frame_columns`` maps them back."""
        nat.check(nat.lib.rts_live_follow_tempo(self._h, int(K), float(ahead)))
        if int(K) > 0 and getattr(self, "_tempo_words", None) is None:
            self._tempo_words = np.zeros((3, self.B), dtype=np.float64)
            self._tempo_n = np.zeros(self.B, dtype=np.int32)

    def tempo(self):
        """Non-blocking: {'slope' float64 [B], 'pos' float64 [B], 'bpm' float64 [B], 'n' int32 [B], 'feeds_done'} as last
        published by the device: slope (reference frames per live frame) and position of the regression line through the
        last ``n`` path points of every stream -- ``BatchedOTW.tempo`` / ``BatchedWTW.tempo`` as of feed ``feeds_done`` or
        later; NaN with n = 0 for a stream without a path point or just restarted.  ``bpm``: the slope in beats per
        minute at the frame ``beats()`` reports (``AnnotationTables.bpm``), NaN while annotations are off or the stream
        has no piece.  Needs ``follow_tempo(K)`` first."""
        done = ctypes.c_int()
        w = getattr(self, "_tempo_words", None)
        nat.check(nat.lib.rts_live_tempo(self._h, *([w[q].ctypes.data for q in range(3)] if w is not None else [None] * 3),
                                         self._tempo_n.ctypes.data if w is not None else None, ctypes.byref(done)))
        return dict(slope=w[0].copy(), pos=w[1].copy(), bpm=w[2].copy(), n=self._tempo_n.copy(), feeds_done=done.value)

    @nat.on_device
    def follow_consensus(self, groups, max_dev=2.0, patience=4):
        """Several streams vote on where a microphone is (rts_live_follow_consensus): ``groups[b]`` is the group of stream
        b (-1: none), 1 to 64 streams each -- the trackers that follow one microphone against different recordings of its
        piece (``ensemble.EnsembleSession`` sets this up).  With it on, each feed enqueues one more small launch: the
        median beat of every group, every member's distance from it, and ``out`` for a member that lay more than
        ``max_dev`` beats away ``patience`` feeds in a row (it is left out of the median until one feed back within it);
        ``consensus()`` reads the words.  Needs ``annotate(tables)`` first, and does nothing while annotations are off.
        ``groups`` may be an ``ensemble.Ensemble`` of this device; ``None`` switches consensus off (the words stay).
        ``restart`` clears the listed streams' strikes, ``reset`` everyone's."""
        from .ensemble import Ensemble
        if groups is None:
            nat.check(nat.lib.rts_live_follow_consensus(self._h, None))
            return
        ens = groups if isinstance(groups, Ensemble) else Ensemble(groups, max_dev, patience, device=self.dev)
        nat.check(nat.lib.rts_live_follow_consensus(self._h, ens._h))
        if getattr(self, "_ens", None) is not None and self._ens is not ens:
            self.sync()                                   # feeds in flight still vote with the ensemble bound before
        self._ens = ens                                   # held by reference on the device side: keep it alive
        self._ens_f = np.zeros((3, self.B), dtype=np.float64)
        self._ens_i = np.zeros((4, self.B), dtype=np.int32)

    def consensus(self):
        """Non-blocking: {'consensus', 'spread' float64 [n_groups], 'n_in', 'n_valid' int32 [n_groups], 'dev' float64 [B],
        'strikes', 'out' int32 [B], 'feeds_done'} as last published by the device: the groups' median beat (NaN: no member
        has a beat) and the range of the members that voted, how many voted and how many have a beat at all; per stream
        its beat minus the consensus (NaN: no beat, or in no group), its strikes and whether it is out.  Unlike ``beats()``
        nothing here is sticky.  Needs ``follow_consensus`` first."""
        done = ctypes.c_int()
        f, i = getattr(self, "_ens_f", None), getattr(self, "_ens_i", None)
        ptr = lambda a, q: a[q].ctypes.data if a is not None else None   # noqa: E731
        nat.check(nat.lib.rts_live_consensus(self._h, ptr(f, 0), ptr(f, 1), ptr(i, 0), ptr(i, 1), ptr(f, 2), ptr(i, 2), ptr(i, 3),
                                             ctypes.byref(done)))
        G = self._ens.n_groups
        return dict(consensus=f[0, :G].copy(), spread=f[1, :G].copy(), n_in=i[0, :G].copy(), n_valid=i[1, :G].copy(),
                    dev=f[2].copy(), strikes=i[2].copy(), out=i[3].copy(), feeds_done=done.value)

    # ---- accompaniment ----------------------------------------------------------------------------------------
    @nat.on_device
    def accompany(self, tracks, origins=None, warp_N=1024, delta=256, hop_track=None, K=64, glide=None, lead=0,
                  rates=(0.5, 2.0), chunk_seconds=0.25, max_anchors=1 << 14):
        """Play a track along every microphone (rts_live_accompany; include/rtsync.h has the steering law).  ``tracks``: one
        array of samples (float32, or int16 PCM) for every stream, or a list with one entry per stream -- an array, or None
        for a stream that gets no accompaniment; an array that repeats is uploaded once.  ``origins``: per stream, the track
        sample that belongs to frame 0 of the stream's piece (default 0); a stream that follows its piece from an offset
        (``restart(offsets=...)``) is armed ``offset * hop_track`` samples further on.  ``hop_track``: track
        samples per reference frame (default ``hop_size``: the track is the reference's own recording).  ``K``: path points
        in the regression window.  ``glide``: samples over which a correction is spread (default 0.2 s).  ``lead``: signed
        samples, what the output path adds between ``accompaniment()`` and the loudspeaker plus the offset between a live
        index and the microphone sample its frame is centred on.  ``rates``: limits of the playing rate.
        ``chunk_seconds``: the most audio a feed renders per stream (a multiple of the warp hop ``warp_N // 2``, at least
        one); it must exceed the length of a feed, or the output falls behind (status ``ACC_LATE``).  ``max_anchors``: one
        anchor per feed that renders; a stream whose list is full stops (``ACC_FULL``) until it is armed again.

        The tracks are uploaded once per object given and recognised by identity afterwards: hand over a new array to play
        other audio, one changed in place is not uploaded again.  A stream keeps its track when ``restart(refs=...)`` moves it
        onto another piece (it is armed again on the same track at the new offset): call ``accompany`` again with that
        piece's track.  With ``features='chroma_diff'`` a live index lags the microphone by one frame (the tracker's first
        frame is the stream's second chroma column): add ``hop_size`` to ``lead``.

        Each call arms the listed streams from output sample 0, with the next feed; calling it again with the same
        arguments re-arms them, with others it waits for the device and rebuilds.  ``accompany(None)`` switches it off.
        ``restart`` disarms the restarted streams and arms them again at ``origin + offset * hop_track``; ``reset`` disarms
        everyone.  Not with ``fs_in`` or the gate (live indices are not microphone time there), and ``export_streams`` /
        ``import_streams`` refuse while it is on.  Two more launches per feed; nothing is read back."""
        from .render import WarpPlan
        if tracks is None:
            nat.check(nat.lib.rts_live_accompany(self._h, None, None, nat.F32, None, None, None, None, None))
            self._acc_tracks = None
            return
        per = list(tracks) if isinstance(tracks, (list, tuple)) else [tracks] * self.B
        if len(per) != self.B:
            raise ValueError("%d tracks for %d streams" % (len(per), self.B))
        uniq, given = {}, {}
        for t in per:
            if t is not None:
                uniq.setdefault(id(t), np.ascontiguousarray(t))
                given[id(t)] = t
        if not uniq:
            raise ValueError("no stream has a track")
        pcm = all(a.dtype == np.int16 for a in uniq.values())
        gap = int(warp_N) + int(delta)                   # silence between tracks: a search window never meets a neighbour
        first, pieces, at = {}, [], 0
        for key, a in uniq.items():
            if a.ndim != 1:
                raise ValueError("a track must be a 1-D array of samples")
            first[key] = at
            a = a if pcm or a.dtype != np.int16 else a.astype(np.float32) * np.float32(1.0 / 32768.0)
            pieces += [a.astype(np.int16 if pcm else np.float32), np.zeros(gap, dtype=np.int16 if pcm else np.float32)]
            at += len(a) + gap
        key = (tuple(sorted(first.items())), pcm, int(warp_N), int(delta))
        if self._acc_key != key or any(self._acc_given.get(k) is not t for k, t in given.items()):   # another pool or plan
            if self._acc_plan is not None:
                self.sync()
                nat.check(nat.lib.rts_live_accompany(self._h, None, None, nat.F32, None, None, None, None, None))
                torch.cuda.synchronize(self.dev)
                self._acc_plan.close()
            self._acc_plan = WarpPlan(warp_N, delta, device=self.dev)
            self._acc_pool = torch.from_numpy(np.concatenate(pieces)).to(self.dev)
            self._acc_key, self._acc_given = key, given   # the objects given stay alive, so their ids stay theirs
        H = self._acc_plan.H
        org = [0] * self.B if origins is None else [int(o) for o in origins]
        par = nat.AccompParams(int(self.H if hop_track is None else hop_track), int(K),
                               int(self.fs // 5 if glide is None else glide), int(lead), int(round(rates[0] * 1000)),
                               int(round(rates[1] * 1000)), max(1, -(-int(round(chunk_seconds * self.fs)) // H)), int(max_anchors))
        self._acc_par = par
        self._acc_tracks = [None if t is None else (first[id(t)], len(uniq[id(t)]), org[b]) for b, t in enumerate(per)]
        self._accompany_streams([b for b in range(self.B) if per[b] is not None])
        self._acc_words = dict(blocks=np.zeros(self.B, np.int32), out_total=np.zeros(self.B, np.int64),
                               in_pos=np.zeros(self.B, np.int64), rate=np.zeros(self.B, np.float64),
                               status=np.zeros(self.B, np.int32), warp_status=np.zeros(self.B, np.int32))

    def _accompany_streams(self, streams):
        """rts_live_accompany for the listed streams, each origin moved to the frame of its piece at which the range the
        stream follows now begins (``restart(offsets=...)``), like ``_annotate_streams`` moves frame0."""
        eng = self.otw or self.wtw
        mask, first, lens, org = (np.zeros(self.B, np.uint8), np.zeros(self.B, np.int64), np.zeros(self.B, np.int64),
                                  np.zeros(self.B, np.int64))
        for b in streams:
            if self._acc_tracks[b] is None:
                continue
            mask[b] = 1
            first[b], lens[b], org[b] = self._acc_tracks[b]
            if self._conv is not None:
                org[b] += (eng._piece[b][1] - int(eng.ref_lens[b])) * self._acc_par.hop_track
        if not mask.any():
            return
        nat.check(nat.lib.rts_live_accompany(self._h, self._acc_plan._h, self._acc_pool.data_ptr(),
                                             nat.I16 if self._acc_pool.dtype == torch.int16 else nat.F32, mask.ctypes.data,
                                             first.ctypes.data, lens.ctypes.data, org.ctypes.data, ctypes.byref(self._acc_par)))

    def accompaniment(self):
        """Non-blocking: ``(audio, words)`` of the newest feed every stream has published.  ``audio[b]``: a float32 numpy
        view of stream b's row of that feed's chunk, cut to ``blocks[b] * (warp_N // 2)`` samples -- host-mapped memory the
        device wrote; copy it before three more feeds are submitted, the fourth writes over it.  ``words``: {'blocks',
        'out_total' (output samples made since the stream was armed, this chunk included), 'in_pos' (the track sample the
        map has reached, counted in the pool ``accompany`` uploaded), 'rate', 'status' (a sum of ``_native.ACC_*``),
        'warp_status', 'feeds_done'}.  A consumer appends ``audio[b]`` whenever ``feeds_done`` has moved on."""
        w = self._acc_words
        if w is None:
            raise nat.RtsyncError("accompaniment() needs accompany(tracks) first")
        chunk, stride, done = ctypes.c_void_p(), ctypes.c_longlong(), ctypes.c_int()
        nat.check(nat.lib.rts_live_accompaniment(self._h, ctypes.byref(chunk), ctypes.byref(stride), w["blocks"].ctypes.data,
                                                 w["out_total"].ctypes.data, w["in_pos"].ctypes.data, w["rate"].ctypes.data,
                                                 w["status"].ctypes.data, w["warp_status"].ctypes.data, ctypes.byref(done)))
        ring = np.ctypeslib.as_array(ctypes.cast(chunk.value, ctypes.POINTER(ctypes.c_float)), shape=(self.B, stride.value))
        H = self._acc_plan.H
        audio = [ring[b, :int(w["blocks"][b]) * H] for b in range(self.B)]
        words = dict((k, v.copy()) for k, v in w.items())
        words["feeds_done"] = done.value
        return audio, words

    @nat.on_device
    def accompaniment_map(self, b=0):
        """(anchors int64 [A][2] as (out_pos, in_pos), (k, p_prev)) of stream b's time map and renderer state
        (rts_live_accomp_map).  Waits for the feeds in flight: for tests and tools."""
        n, state = ctypes.c_int(), np.zeros(2, dtype=np.int64)
        cap = int(self._acc_par.A_max)
        out = np.zeros((cap, 2), dtype=np.int64)
        nat.check(nat.lib.rts_live_accomp_map(self._h, int(b), out.ctypes.data, cap, ctypes.byref(n), state.ctypes.data,
                                              self._stream()))
        return out[:max(0, min(n.value, cap))].copy(), (int(state[0]), int(state[1]))

    def backward(self, streams=None):
        """The backward path of every stream (or the listed ones) through the bound OTW tracker
        (``BatchedOTW.backward``): ``(paths, totals, ends)`` for everything the microphones' columns have brought the
        tracker so far; streams not listed get an empty path.  Waits for the feeds in flight.  OTW family only: a WTW
        window re-decides its own path."""
        if self.otw is None:
            raise nat.RtsyncError("backward needs an OTW tracker (this session is bound to WTW)")
        self.sync()
        paths, totals, ends = self.otw.backward()
        if streams is not None:
            keep = set(int(b) for b in streams)
            paths = [p if b in keep else p[:0] for b, p in enumerate(paths)]
        return paths, totals, ends

    def path(self, b=0):
        return (self.otw or self.wtw).path(b)

    def position(self, b=0):
        """(live_frame, ref_frame) of stream b's latest path point, or None."""
        p = self.path(b)
        return (int(p[-1, 0]), int(p[-1, 1])) if len(p) else None

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                torch.cuda.synchronize(self.dev)
            except Exception:
                pass
            nat.destroy_on(self.dev, nat.lib.rts_live_destroy, h)
        self._acc_pool = None                                # behind the handle that pointed at them
        for o in (getattr(self, "otw", None), getattr(self, "wtw", None), getattr(self, "plan", None),
                  getattr(self, "resampler", None), getattr(self, "_acc_plan", None)):
            if o is not None:
                o.close()

    __del__ = close
