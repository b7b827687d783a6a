"""Snapshots: the carried state of single streams as self-contained records (include/rtsync.h, rts_otw_export /
rts_otw_import, the rts_wtw_ and rts_live_ pairs).  ``export_streams`` of a ``BatchedOTW`` / ``BatchedWTW`` /
``LiveSession`` makes a ``Snapshot``, ``import_streams`` puts one into slots of another handle of the same kind -- of another batch size,
longest reference, slot layout, kernel flavour, device or process.  A continued stream is bit for bit the stream that was
never moved."""
import ctypes

import numpy as np
import torch

from . import _native as nat

# int32 words of a record's header (csrc/snapshot_plan.h, snap::Word)
W_MAGIC, W_VERSION, W_KIND, W_NB, W_MB, W_HIST_VALID, W_PATH_VALID, W_HIST_LEN, W_C = range(9)
W_USED = 13
HEADER_BYTES = 64
_DESC_FIELDS = tuple(k for k, _ in nat.SnapshotDesc._fields_)


def range_digest(frames):
    """The 64-bit integer sum of the bit patterns of a [n][12] float32 / float64 device tensor (modulo 2^64): exact and
    independent of the order of summation, so the same recording gives the same number on any device."""
    bits = frames.contiguous().view(torch.int32 if frames.dtype == torch.float32 else torch.int64)
    return int(bits.to(torch.int64).sum().item())


class Snapshot:
    """``desc``: dict of the rts_snapshot_desc fields.  ``blob``: uint8 tensor [n][rec_stride], one record per row.
    ``pieces``: int64 [n][2], what the exporter knew of each stream's reference: frames of its piece, and the offset
    inside the piece its range starts at.  ``digests``: int64 [n] of ``range_digest`` over each stream's range, or None
    (exported without ``verify``).  ``mirror``: int32 [n][2], a live session's host mirror words per stream (pending
    samples, carry flag), which ``rts_live_import`` takes; None for a tracker's snapshot.  A live record carries its
    tail (pending samples, diff carry) at the end of the stride: ``tail_bytes``."""

    def __init__(self, desc, blob, pieces, digests=None, mirror=None):
        self.desc = {k: int(desc[k]) for k in _DESC_FIELDS}
        self.blob, self.pieces, self.digests = blob, np.asarray(pieces, dtype=np.int64), digests
        self.mirror = None if mirror is None else np.ascontiguousarray(mirror, dtype=np.int32).reshape(-1, 2)
        if blob.dtype != torch.uint8 or tuple(blob.shape) != (self.n, self.rec_stride) or not blob.is_contiguous():
            raise ValueError("blob must be a contiguous uint8 tensor [n = %d][rec_stride = %d]" % (self.n, self.rec_stride))

    n = property(lambda self: self.desc["n"])
    rec_stride = property(lambda self: self.desc["rec_stride"])
    device = property(lambda self: self.blob.device)

    @property
    def tail_bytes(self):
        """Bytes of the live tail at the end of every record (0 for a tracker's snapshot)."""
        if self.desc["kind"] != nat.SNAPSHOT_LIVE:
            return 0
        return 16 + -(-4 * self.desc["max_pending"] // 16) * 16 + 96

    def c_desc(self):
        return nat.SnapshotDesc(**self.desc)

    def to(self, device):
        """The same snapshot with its blob on ``device`` (a GPU of this process, or "cpu" to park it)."""
        return Snapshot(self.desc, self.blob.to(device), self.pieces, self.digests, self.mirror)

    def select(self, i):
        """The records ``i`` (an index or a list of indices) as a snapshot of their own."""
        idx = [int(i)] if np.isscalar(i) else [int(k) for k in i]
        take = torch.as_tensor(idx, dtype=torch.long, device=self.blob.device)
        return Snapshot(dict(self.desc, n=len(idx)), self.blob.index_select(0, take).contiguous(), self.pieces[idx],
                        None if self.digests is None else np.asarray(self.digests)[idx],
                        None if self.mirror is None else self.mirror[idx])

    def headers(self):
        """int32 [n][16]: the header words of every record (synchronises)."""
        return self.blob[:, :HEADER_BYTES].cpu().numpy().view(np.int32).reshape(self.n, HEADER_BYTES // 4)

    def used_bytes(self):
        """int64 [n]: the bytes of each record that carry state; zeros lie behind them up to rec_stride."""
        return self.headers()[:, W_USED].astype(np.int64)

    def save(self, path):
        """One ``.npz`` file (no pickled objects): the desc fields and every record trimmed to its used bytes (a live
        record: those of its tracker, and its tail cut to the pending samples)."""
        used, tail = self.used_bytes(), self.tail_bytes
        if (used < HEADER_BYTES).any() or (used > self.rec_stride - tail).any():
            raise ValueError("the blob holds records that were never written")
        host = self.blob.cpu().numpy()
        data = np.concatenate([host[i, :used[i]] for i in range(self.n)]) if self.n else np.zeros(0, np.uint8)
        tails = host[:, self.rec_stride - tail:] if tail else np.zeros((self.n, 0), np.uint8)
        np.savez(path, tails=tails, has_mirror=np.array(self.mirror is not None),
                 mirror=np.zeros((self.n, 2), np.int32) if self.mirror is None else self.mirror,
                 desc_names=np.array(_DESC_FIELDS), desc_values=np.array([self.desc[k] for k in _DESC_FIELDS], np.int64),
                 used=used, data=data, pieces=self.pieces, has_digests=np.array(self.digests is not None),
                 digests=np.zeros(self.n, np.int64) if self.digests is None else np.asarray(self.digests, np.int64))

    @classmethod
    def load(cls, path, device):
        with np.load(path, allow_pickle=False) as z:
            desc = {str(k): int(v) for k, v in zip(z["desc_names"], z["desc_values"])}
            if set(desc) != set(_DESC_FIELDS):
                raise ValueError("%s: not the desc fields of this build" % path)
            used, data, pieces = z["used"], z["data"], z["pieces"]
            digests = z["digests"] if bool(z["has_digests"]) else None
            tails, mirror = z["tails"], (z["mirror"] if bool(z["has_mirror"]) else None)
        n, stride = desc["n"], desc["rec_stride"]
        if len(used) != n or (used < HEADER_BYTES).any() or (used > stride).any() or int(used.sum()) != len(data):
            raise ValueError("%s: record sizes do not add up" % path)
        host, at = np.zeros((n, stride), np.uint8), 0
        for i in range(n):
            host[i, :used[i]] = data[at:at + used[i]]
            at += int(used[i])
        if tails.shape[1]:
            if tails.shape[0] != n or tails.shape[1] > stride - int(used.max(initial=0)):
                raise ValueError("%s: the live tails do not fit behind the records" % path)
            host[:, stride - tails.shape[1]:] = tails
        return cls(desc, torch.from_numpy(host).to(device), pieces, digests, mirror)


def export_streams(eng, streams, verify=False, blob=None):
    """``export_streams`` of the batched handles."""
    idx = np.ascontiguousarray([int(b) for b in streams], dtype=np.int32)
    need = ctypes.c_size_t()
    nat.check(eng._fn("snapshot_bytes")(eng._h, ctypes.byref(need)))
    if blob is None:
        blob = torch.empty((len(idx), need.value), dtype=torch.uint8, device=eng.device)
    desc = nat.SnapshotDesc()
    nat.check(eng._fn("export")(eng._h, idx.ctypes.data, len(idx), blob.data_ptr(), int(blob.shape[1]), ctypes.byref(desc),
                                eng._stream()))
    return _exported(eng, idx, desc, blob, verify, None)


def _exported(eng, idx, desc, blob, verify, mirror):
    ranges = [eng._range_of(int(b)) for b in idx]
    pieces = [(n_piece, off) for _, _, n_piece, off in ranges]
    digests = np.array([range_digest(eng.ref[f:f + n]) for f, n, _, _ in ranges], np.int64) if verify else None
    return Snapshot({k: getattr(desc, k) for k in _DESC_FIELDS}, blob, pieces, digests, mirror)


def export_live(sess, streams, verify=False, blob=None):
    """``LiveSession.export_streams``."""
    idx = np.ascontiguousarray([int(b) for b in streams], dtype=np.int32)
    need = ctypes.c_size_t()
    nat.check(nat.lib.rts_live_snapshot_bytes(sess._h, ctypes.byref(need)))
    if blob is None:
        blob = torch.empty((len(idx), need.value), dtype=torch.uint8, device=sess.dev)
    desc, mirror = nat.SnapshotDesc(), np.zeros((len(idx), 2), dtype=np.int32)
    nat.check(nat.lib.rts_live_export(sess._h, idx.ctypes.data, len(idx), blob.data_ptr(), int(blob.shape[1]), ctypes.byref(desc),
                                      mirror.ctypes.data, sess._stream()))
    return _exported(sess.otw or sess.wtw, idx, desc, blob, verify, mirror)


def import_streams(eng, snap, slots, refs=None, offsets=None, verify=True, status=None, live=None):
    """``import_streams`` of the batched handles; ``live``: the LiveSession whose tracker ``eng`` is (rts_live_import)."""
    slots = [int(s) for s in slots]
    if len(slots) != snap.n:
        raise ValueError("%d slots for a snapshot of %d streams" % (len(slots), snap.n))
    if snap.blob.device != eng.device:
        raise ValueError("the snapshot is on %s, the handle on %s: use Snapshot.to" % (snap.blob.device, eng.device))
    first = lens = None
    pieces = {}
    if refs is not None or offsets is not None:
        _, first_b, lens_b, pieces = eng._restart_tables(slots, refs, offsets)
        first = np.ascontiguousarray(first_b[slots])
        lens = np.ascontiguousarray(lens_b[slots])
    if verify and snap.digests is not None:
        for i, s in enumerate(slots):
            f, n = (int(first[i]), int(lens[i])) if first is not None else eng._range_of(s)[:2]
            if range_digest(eng.ref[f:f + n]) != int(snap.digests[i]):
                raise nat.RtsyncError("stream %d: its reference range is not the recording record %d was exported against "
                                      "(digest mismatch)" % (s, i))
    idx = np.ascontiguousarray(slots, dtype=np.int32)
    if status is None:
        status = torch.empty(max(snap.n, 1), dtype=torch.int32, device=eng.device)
    desc = snap.c_desc()
    tables = (first.ctypes.data if first is not None else None, lens.ctypes.data if lens is not None else None,
              status.data_ptr())
    if live is None:
        nat.check(eng._fn("import")(eng._h, idx.ctypes.data, snap.n, snap.blob.data_ptr(), snap.rec_stride, ctypes.byref(desc),
                                    *tables, eng._stream()))
    else:   # all or nothing: a refused record raises here, with nothing of the session changed
        if snap.mirror is None:
            raise ValueError("a live session takes the snapshot of a live session")
        nat.check(nat.lib.rts_live_import(live._h, idx.ctypes.data, snap.n, snap.blob.data_ptr(), snap.rec_stride,
                                          ctypes.byref(desc), snap.mirror.ctypes.data, *tables, live._stream()))
    got = status[:snap.n].cpu().numpy()
    taken = {s: pieces[s] for i, s in enumerate(slots) if got[i] == 0 and s in pieces}
    if taken:   # the bookkeeping of restart(): which piece and range the slots that took their record follow now
        lens_b = np.ones(eng.B, dtype=np.int32)
        lens_b[slots] = lens
        eng._restarted(None, lens_b, taken)
    for i, s in enumerate(slots):
        if got[i] != 0:
            raise nat.RtsyncError("stream %d refused record %d: %s (status %d); the slot is unchanged"
                                  % (s, i, nat.SNAP_REASONS.get(int(got[i]), "unknown reason"), int(got[i])))
    return got
