"""Batched online time warping on one MI355X: B independent live streams against one reference, or each against its
own (``BatchedOTW.with_references``).

This is the host-side object behind the drop-in classes (otw_eran.OnlineTimeWarping,
livenote.LiveNote, livenote_v2.LiveNoteV2) and behind bench.py.  torch supplies device memory and
the stream; all computation happens in librtsync.so's HIP kernels (csrc/otw.hip)."""
import ctypes

import numpy as np
import torch

from . import _native as nat
from ._handle import _BatchedHandle, _concat_refs

_VARIANTS = {"otw": nat.VARIANT_OTW, "livenote": nat.VARIANT_LIVENOTE, "livenote_v2": nat.VARIANT_LIVENOTE_V2}


def _np_dtype_code(dt):
    if dt == torch.float32:
        return nat.F32
    if dt == torch.float64:
        return nat.F64
    raise TypeError("feature tensors must be float32 or float64, got %s" % dt)


def frames_tensor(x, device, dtype=None):
    """Reference layout (12, n) feature-major (numpy or torch) -> device tensor [n][12]."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if dtype is not None:
        x = x.to(dtype)
    return x.to(device).t().contiguous()


_on_device = nat.on_device


class BatchedOTW(_BatchedHandle):
    """``ref``: (12, N) feature-major array/tensor, or a device tensor already [N][12] with
    ``frame_major=True``.  ``variant``: 'otw' | 'livenote' | 'livenote_v2'."""
    _abi = "otw"

    def __init__(self, ref, c, max_run_count, batch=1, variant="otw", euclid=False, device="cuda:0",
                 dtype=None, frame_major=False, waves=None):
        self._set_device(device)
        if frame_major:
            self.ref = ref.to(self.device).contiguous()
        else:
            self.ref = frames_tensor(ref, self.device, dtype)
        self.N, F = self.ref.shape
        self.ref_lens = None
        self._init_refs(None, None, None)
        self.B, self.c = int(batch), int(c)
        self.variant = variant
        self.euclid = bool(euclid)
        h = ctypes.c_void_p()
        nat.check(nat.lib.rts_otw_create(self.ref.data_ptr(), _np_dtype_code(self.ref.dtype), F, self.N, self.B,
                                         self.c, int(max_run_count), _VARIANTS[variant],
                                         nat.COST_EUCLID if euclid else nat.COST_DOT, ctypes.byref(h)))
        self._finish(h, waves)

    @classmethod
    def with_references(cls, refs, c, max_run_count, variant="otw", euclid=False, device="cuda:0", dtype=None,
                        waves=None, extra_refs=()):
        """One reference per stream (one piece per microphone): ``refs`` is a list of ``batch`` (12, N_b) arrays or
        tensors.  Stream b behaves exactly like stream 0 of ``BatchedOTW(refs[b], ...)``.  A reference object that
        appears more than once is uploaded once.  ``extra_refs``: pieces uploaded as well although no stream follows
        them yet (the repertoire ``restart`` may move a microphone on to).  ``N`` is the longest of them all,
        ``ref_lens`` holds what each stream follows now.  The dense mirror is not available on such a handle
        (``enable_dense`` / ``replay_dense`` raise)."""
        self = cls.__new__(cls)
        self._set_device(device)
        self.ref, first, lens, pool = _concat_refs(refs, lambda r: frames_tensor(r, self.device, dtype), extra_refs)
        F = self.ref.shape[1]
        self.ref_lens = lens
        self._init_refs(pool, first, lens)
        self.B, self.c = len(refs), int(c)
        self.variant = variant
        self.euclid = bool(euclid)
        first0, lens0, fix = self._grow_to_pool(first, lens)
        self.N = int(lens0.max())
        h = ctypes.c_void_p()
        nat.check(nat.lib.rts_otw_create_refs(self.ref.data_ptr(), _np_dtype_code(self.ref.dtype), F, self.ref.shape[0],
                                              first0.ctypes.data, lens0.ctypes.data, self.B, self.c, int(max_run_count),
                                              _VARIANTS[variant], nat.COST_EUCLID if euclid else nat.COST_DOT,
                                              ctypes.byref(h)))
        self._finish(h, waves)
        if fix:
            fix()
        return self

    def _set_device(self, device):
        if not torch.cuda.is_available():
            raise RuntimeError("BatchedOTW needs a ROCm GPU (no CPU fallback)")
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        torch.cuda.set_device(self.device)

    def _finish(self, h, waves):
        self._h = h
        if waves is not None:
            nat.check(nat.lib.rts_otw_set_waves(self._h, int(waves)))
        self._keep = None
        self._version = 0  # bumped by everything that changes what the handle has consumed

    # ---- whole sequences -------------------------------------------------------------------
    def pack(self, lives, dtype=None):
        """List of (12, T_b) arrays -> (device [B][T_max][12], device int32 [B])."""
        assert len(lives) == self.B
        dtype = dtype or self.ref.dtype
        tmax = max(int(l.shape[1]) for l in lives)
        buf = torch.zeros((self.B, tmax, 12), dtype=dtype)
        for b, l in enumerate(lives):
            l = torch.from_numpy(np.ascontiguousarray(l)) if isinstance(l, np.ndarray) else l
            buf[b, : l.shape[1]] = l.t().to(dtype)
        lens = torch.tensor([int(l.shape[1]) for l in lives], dtype=torch.int32)
        return buf.to(self.device), lens.to(self.device)

    @_on_device
    def run(self, live_dev, live_len_dev, mode="insert"):
        """Asynchronous on the current stream.  live_dev: [B][T_max][12]; live_len_dev: int32 [B]."""
        assert live_dev.is_contiguous() and live_dev.shape[0] == self.B and live_dev.shape[2] == 12
        self._keep = (live_dev, live_len_dev)
        self._version += 1
        nat.check(nat.lib.rts_otw_run(self._h, live_dev.data_ptr(), _np_dtype_code(live_dev.dtype),
                                      int(live_dev.shape[1]), live_len_dev.data_ptr(),
                                      nat.MODE_SET_LIVE if mode == "set_live" else nat.MODE_INSERT_LOOP,
                                      self._stream()))

    @_on_device
    def insert(self, frames_dev, active_dev=None):
        """One frame per stream: frames_dev [B][12]; active_dev optional uint8 [B]."""
        assert frames_dev.is_contiguous() and tuple(frames_dev.shape) == (self.B, 12)
        self._version += 1
        nat.check(nat.lib.rts_otw_insert(self._h, frames_dev.data_ptr(), _np_dtype_code(frames_dev.dtype),
                                         active_dev.data_ptr() if active_dev is not None else None,
                                         self._stream()))

    @_on_device
    def push(self, frames_dev, n_new_dev=None):
        """Several frames per stream: frames_dev [B][n_max][12]; n_new_dev optional int32 [B]."""
        assert frames_dev.is_contiguous() and frames_dev.shape[0] == self.B and frames_dev.shape[2] == 12
        self._version += 1
        nat.check(nat.lib.rts_otw_push(self._h, frames_dev.data_ptr(), _np_dtype_code(frames_dev.dtype),
                                       int(frames_dev.shape[1]), n_new_dev.data_ptr() if n_new_dev is not None else None,
                                       self._stream()))

    @_on_device
    def reset(self):
        self._version += 1
        self._keep = None
        nat.check(nat.lib.rts_otw_reset(self._h, self._stream()))

    def restart(self, streams, refs=None, offsets=None):
        """Put the listed streams back to the start while the others keep running (rts_otw_restart; asynchronous on
        the current stream).  ``refs``: one entry per listed stream, each an object that was uploaded at create
        (``refs`` / ``extra_refs`` of ``with_references``, matched by identity): the stream moves on to that piece.
        ``offsets``: first frame inside the piece, the stream then follows ``ref[:, offset:]`` and its path indices
        count from there; without ``refs`` it means "same piece, from this frame"."""
        super().restart(streams, refs, offsets)
        self._version += 1

    def import_streams(self, snap, slots, refs=None, offsets=None, verify=True, status=None):
        """``_BatchedHandle.import_streams``; c, max_run_count, variant, cost kind and dtype must be the exporter's, batch
        size, N_max, slot layout and kernel flavour need not.  Not with the dense mirror attached."""
        got = super().import_streams(snap, slots, refs, offsets, verify, status)
        self._version += 1
        return got

    # ---- results ------------------------------------------------------------------------------
    @_on_device
    def path_cost(self, K=64, want_costs=False):
        """Tracking confidence (rts_otw_path_cost): the tracker's own cell cost at the last ``n = min(K, path points)``
        points of every stream's path.  Device tensors ``(mean float64 [B], n int32 [B])``, with ``want_costs`` also
        ``costs float64 [B][K]`` (NaN behind the n-th).  ``mean`` is NaN for a stream without a path point, and for one
        that heard a silent (NaN) column among those points.  It is in the unit of ``locate``'s normalised cost,
        ``cost / (M + end - start + 1)``; what value means "lost" depends on the features and the room.  At most 256
        points; not after ``run`` (those frames are the caller's).  Asynchronous, nothing is read back."""
        K = int(K)
        mean = torch.empty(self.B, dtype=torch.float64, device=self.device)
        n = torch.empty(self.B, dtype=torch.int32, device=self.device)
        costs = torch.empty((self.B, max(K, 0)), dtype=torch.float64, device=self.device) if want_costs else None
        nat.check(nat.lib.rts_otw_path_cost(self._h, K, mean.data_ptr(), n.data_ptr(),
                                            costs.data_ptr() if want_costs else None, self._stream()))
        return (mean, n, costs) if want_costs else (mean, n)

    @_on_device
    def states(self):
        out = np.zeros((self.B, nat.STATE_LEN), dtype=np.int32)
        nat.check(nat.lib.rts_otw_read_states(self._h, out.ctypes.data, self._stream()))
        return out

    def state(self, b=0):
        s = self.states()[b]
        cells = (int(np.uint32(s[nat.ST_CELLS_HI])) << 32) | int(np.uint32(s[nat.ST_CELLS_LO]))
        return dict(t=int(s[nat.ST_T]), j=int(s[nat.ST_J]), direction=int(s[nat.ST_DIRECTION]),
                    previous=int(s[nat.ST_PREVIOUS]), run_count=int(s[nat.ST_RUN_COUNT]),
                    status=int(s[nat.ST_STATUS]), first_insert=int(s[nat.ST_FIRST_INSERT]),
                    n_path=int(s[nat.ST_N_PATH]), consumed=int(s[nat.ST_CONSUMED]),
                    row_strips=int(s[nat.ST_ROW_STRIPS]), col_strips=int(s[nat.ST_COL_STRIPS]), cells=cells,
                    path_truncated=int(s[nat.ST_PATH_TRUNCATED]), band_recomputes=int(s[nat.ST_BAND_RECOMPUTES]))

    def paths(self):
        return [self.path(b) for b in range(self.B)]

    @_on_device
    def bands(self, b=0):
        rb = np.empty(self.c + 1)
        cb = np.empty(self.c + 1)
        nat.check(nat.lib.rts_otw_read_bands(self._h, b, rb.ctypes.data, cb.ctypes.data, self._stream()))
        return rb, cb

    @_on_device
    def fill_taken(self):
        """int32 [B]: 1 where the stream's band was filled by the dense wavefront kernel in the last run / insert / push
        (rts_otw_read_fill), 0 where the step loop ran alone."""
        out = np.zeros(self.B, dtype=np.int32)
        nat.check(nat.lib.rts_otw_read_fill(self._h, out.ctypes.data, self._stream()))
        return out

    @_on_device
    def enable_dense(self):
        """Allocate and attach the reference's dense (2N x N) acc_cost / cost matrices per stream
        (float64 device tensors [B][2N][N]); every evaluated cell is mirrored into them."""
        if self.ref_lens is not None:   # refused by the library: one [2N][N] layout per handle
            nat.check(nat.lib.rts_otw_set_dense(self._h, None, None, self._stream()))
        self.dense_acc = torch.empty((self.B, 2 * self.N, self.N), dtype=torch.float64, device=self.device)
        self.dense_cost = torch.empty((self.B, 2 * self.N, self.N), dtype=torch.float64, device=self.device)
        nat.check(nat.lib.rts_otw_set_dense(self._h, self.dense_acc.data_ptr(), self.dense_cost.data_ptr(),
                                            self._stream()))
        return self.dense_acc, self.dense_cost

    @_on_device
    def replay_dense(self):
        """The reference's dense (2N x N) acc_cost / cost matrices (float64 device tensors [B][2N][N]) for
        everything consumed since the last reset, recomputed on demand by a second pass over the kept frames
        (rts_otw_replay_dense); the tracker itself never pays for them."""
        if self.ref_lens is not None:   # refused by the library, before anything is allocated
            nat.check(nat.lib.rts_otw_replay_dense(self._h, None, nat.F64, 0, None, None, None, self._stream()))
        acc = torch.empty((self.B, 2 * self.N, self.N), dtype=torch.float64, device=self.device)
        cost = torch.empty((self.B, 2 * self.N, self.N), dtype=torch.float64, device=self.device)
        if self._keep is not None:   # the frames of the last run(): handed in again, the library keeps no pointer to them
            lv, ln = self._keep
            nat.check(nat.lib.rts_otw_replay_dense(self._h, lv.data_ptr(), _np_dtype_code(lv.dtype), int(lv.shape[1]),
                                                   ln.data_ptr(), acc.data_ptr(), cost.data_ptr(), self._stream()))
        else:                        # frames that came through insert() / push(): the handle's own history
            nat.check(nat.lib.rts_otw_replay_dense(self._h, None, nat.F64, 0, None, acc.data_ptr(), cost.data_ptr(),
                                                   self._stream()))
        return acc, cost

    @_on_device
    def backward(self, live_dev=None, live_len_dev=None, want_acc=False):
        """The backward path of every stream (rts_otw_backward): from its current best point back to (0, 0) over the
        cells the tracker has evaluated -- monotone, gap-free and optimal inside the explored band, where ``path`` is
        causal and may jump.  Returns ``(paths, totals, ends)``: a list of (n_b, 2) int32 arrays from (0, 0) to
        ``ends[b]``, float64 [B] accumulated cost at the end cell, int32 [B][2]; with ``want_acc`` also a list of
        float64 (n_b,) arrays, the accumulated cost at every path point.  A stream that has consumed nothing: an empty
        path, NaN, (-1, -1).  After ``run`` the frames are that call's (kept by this object; ``live_dev`` /
        ``live_len_dev`` override them); after ``insert`` / ``push`` they are the handle's history.  Works with
        per-stream references.  The tracker itself is not disturbed."""
        cap = 3 * self.N + 8
        need = ctypes.c_size_t()
        nat.check(nat.lib.rts_otw_backward_workspace_bytes(self.N, self.c, self.B, ctypes.byref(need)))
        ws = getattr(self, "_bw_ws", None)
        if ws is None or ws.numel() < need.value:
            ws = self._bw_ws = torch.empty(need.value, dtype=torch.uint8, device=self.device)
        path = torch.empty((self.B, cap, 2), dtype=torch.int32, device=self.device)
        plen = torch.empty(self.B, dtype=torch.int32, device=self.device)
        total = torch.empty(self.B, dtype=torch.float64, device=self.device)
        end = torch.empty((self.B, 2), dtype=torch.int32, device=self.device)
        acc = torch.empty((self.B, cap), dtype=torch.float64, device=self.device) if want_acc else None
        if live_dev is None and self._keep is not None:
            live_dev, live_len_dev = self._keep
        if live_dev is not None:
            src = (live_dev.data_ptr(), _np_dtype_code(live_dev.dtype), int(live_dev.shape[1]), live_len_dev.data_ptr())
        else:
            src = (None, nat.F64, 0, None)
        nat.check(nat.lib.rts_otw_backward(self._h, src[0], src[1], src[2], src[3], path.data_ptr(), plen.data_ptr(),
                                           total.data_ptr(), end.data_ptr(), acc.data_ptr() if want_acc else None,
                                           ws.data_ptr(), ws.numel(), self._stream()))
        n = plen.cpu().numpy()
        path_h = path.cpu().numpy()
        paths = [path_h[b, :n[b]].copy() for b in range(self.B)]
        out = (paths, total.cpu().numpy(), end.cpu().numpy())
        if want_acc:
            acc_h = acc.cpu().numpy()
            out += ([acc_h[b, :n[b]].copy() for b in range(self.B)],)
        return out

    @_on_device
    def set_waves(self, waves):
        nat.check(nat.lib.rts_otw_set_waves(self._h, int(waves)))

    @property
    def kernel_name(self):
        return nat.lib.rts_otw_kernel_name(self._h).decode()

    def kernel(self, live_dtype=None, with_waves=False):
        """What a launch with live input of ``live_dtype`` runs (rts_otw_read_kernel; no GPU call): ``dict(window, ring,
        pipelined, fill)`` with ``ring`` one of 'float', 'double', 'none', 'none-lean'.  ``None``: float64, the handle's
        own history, which ``insert`` and ``push`` read whatever dtype their frames come in; for ``run`` pass the live
        tensor's dtype.  ``with_waves``: also ``waves``, the waves per stream of that kernel (rts_otw_read_kernel_waves:
        8, or 12 / 16 for the wide forms a handle takes at ``batch <= CUs``; ``RTS_OTW_WAVES`` fixes it at create)."""
        out = (ctypes.c_int32 * 4)()
        code = nat.F64 if live_dtype is None else _np_dtype_code(live_dtype)
        nat.check(nat.lib.rts_otw_read_kernel(self._h, code, out))
        info = dict(window=int(out[0]), ring=nat.OTW_RINGS[out[1]], pipelined=bool(out[2]), fill=bool(out[3]))
        if with_waves:
            waves = ctypes.c_int32()
            nat.check(nat.lib.rts_otw_read_kernel_waves(self._h, code, ctypes.byref(waves)))
            info["waves"] = int(waves.value)
        return info
