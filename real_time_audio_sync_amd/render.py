"""Render one recording on another's time axis, along an alignment path (csrc/warp.hip).

``align_pairs`` says where two performances correspond; ``warp_pairs`` makes that audible: recording A stretched and
squeezed onto recording B's timeline (or the other way round), so that the two can be played together, mixed left and
right to hear whether a path is right, or used as an accompaniment that follows.  It is time-scale modification by
waveform-similarity overlap-add along a piecewise-linear integer time map; include/rtsync.h (rts_warp_run) has the
definition, to the bit, and tests/warp_model.py is that definition in numpy.

The pieces, all on device tensors and asynchronous: ``WarpPlan`` (frame length, search tolerance, window),
``anchors_from_paths`` (a time map per path, made on the device from the output of ``dtw.dtw_paths``) and ``warp`` (the
rendering, resumable block by block through a two-word state per stream)."""
import ctypes

import numpy as np
import torch

from . import _native as nat
from . import filters


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _i64(v, B, dev, name):
    t = torch.as_tensor(v).to(device=dev, dtype=torch.int64).contiguous().reshape(-1)
    if t.numel() != B:
        raise ValueError("%s: %d entries for %d streams" % (name, t.numel(), B))
    return t


def blocks(n_out, N):
    """Blocks of N / 2 samples that cover ``n_out`` output samples (rts_warp_blocks)."""
    k = int(nat.lib.rts_warp_blocks(int(n_out), int(N)))
    if k < 0:
        raise ValueError("N = %d is not a frame length a plan takes" % N)
    return k


class WarpPlan:
    """Frame length ``N`` (a multiple of 16 in [64, 4096]; the hop is N / 2), search tolerance ``delta`` in samples
    ([0, 1024]; 0 is plain overlap-add) and the window, N float64 values (default: the periodic Hann window, whose halves
    sum to one).  Belongs to ``device``."""

    def __init__(self, N=1024, delta=256, window=None, device="cuda:0"):
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device(self.device.type, torch.cuda.current_device())
        self.N, self.H, self.delta = int(N), int(N) // 2, int(delta)
        w = filters.hann_window_periodic(self.N) if window is None else np.ascontiguousarray(window, dtype=np.float64)
        if w.shape != (self.N,):
            raise ValueError("window must hold N = %d values, got shape %s" % (self.N, w.shape))
        self.window = w
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            nat.check(nat.lib.rts_warp_create(self.N, self.delta, w.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h)))
        self._h = h

    def close(self):
        if self._h:
            nat.destroy_on(self.device, nat.lib.rts_warp_destroy, self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def anchors_from_paths(path_dev, plen_dev, onto, hop, n_out, n_in, A_max=None):
    """Time maps from monotone paths, on the device (rts_warp_anchors).  ``path_dev`` int32 [B][P_max][2] and ``plen_dev``
    int32 [B] as ``dtw.dtw_paths`` returns them; ``onto`` in {0, 1} is the path column whose time axis the output gets;
    ``hop`` the samples per feature frame; ``n_out`` / ``n_in`` the output and input sample counts per stream.

    Returns device tensors ``(anchors int64 [B][A_max][2], n_anchor int32 [B], status int32 [B])``.  A stream whose path is
    refused has a non-zero status (a sum of ``_native.WARP_PATH_*``) and n_anchor 0.  ``A_max`` defaults to P_max + 1, which
    every path fits.  Asynchronous."""
    dev = path_dev.device
    path_dev = path_dev.to(torch.int32).contiguous()
    if path_dev.dim() != 3 or path_dev.shape[2] != 2:
        raise ValueError("path_dev must be [B][P_max][2]")
    B, P_max = int(path_dev.shape[0]), int(path_dev.shape[1])
    plen_dev = torch.as_tensor(plen_dev).to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
    if plen_dev.numel() != B:
        raise ValueError("plen_dev: %d entries for %d paths" % (plen_dev.numel(), B))
    n_out, n_in = _i64(n_out, B, dev, "n_out"), _i64(n_in, B, dev, "n_in")
    A_max = max(P_max + 1, 2) if A_max is None else int(A_max)
    anchors = torch.empty((B, A_max, 2), dtype=torch.int64, device=dev)
    n_anchor = torch.empty((B,), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib.rts_warp_anchors(path_dev.data_ptr() if P_max else None, P_max, plen_dev.data_ptr(), int(onto),
                                           int(hop), n_out.data_ptr(), n_in.data_ptr(), B, anchors.data_ptr(), A_max,
                                           n_anchor.data_ptr(), status.data_ptr(), _stream(dev)))
    return anchors, n_anchor, status


def warp(plan, samples, n_in, anchors, n_anchor, n_out, state=None, k_count=None, out=None, status=None):
    """Render up to ``k_count`` further blocks of every stream (rts_warp_run).  ``samples``: float32 or int16 (PCM16)
    device tensor [B][n_max]; ``n_in`` / ``n_out``: sample counts per stream; ``anchors`` int64 [B][A_max][2] and
    ``n_anchor`` int32 [B] as ``anchors_from_paths`` returns them, or made by the caller.

    ``state`` int64 [B][2] is (k, p of the block before) per stream and moves on; None starts at block 0.  ``k_count`` None
    renders everything that is left.  Block k goes to ``out[b, (k - k_start) * H:]``, k_start the stream's k when the call
    began; ``out`` None allocates zeros for ``k_count`` blocks (for a whole rendering, ``out[b, :n_out[b]]`` is the
    result; samples behind n_out are not written).  Returns ``(out, state, status)``, status int32 [B] non-zero for a stream
    that was skipped (``_native.WARP_NO_MAP`` / ``WARP_BAD_MAP`` / ``WARP_BAD_STATE``).  Asynchronous when ``k_count`` and
    ``out`` are given."""
    dev = samples.device
    if samples.dim() != 2 or samples.dtype not in (torch.float32, torch.int16):
        raise ValueError("samples must be a float32 or int16 tensor [B][n_max]")
    if samples.stride(1) != 1 and samples.shape[1] > 1:
        samples = samples.contiguous()
    B = int(samples.shape[0])
    n_in, n_out = _i64(n_in, B, dev, "n_in"), _i64(n_out, B, dev, "n_out")
    if anchors.dtype != torch.int64 or anchors.dim() != 3 or anchors.shape[0] != B or anchors.shape[2] != 2 or not anchors.is_contiguous():
        raise ValueError("anchors must be a contiguous int64 tensor [B][A_max][2]")
    n_anchor = torch.as_tensor(n_anchor).to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
    if n_anchor.numel() != B:
        raise ValueError("n_anchor: %d entries for %d streams" % (n_anchor.numel(), B))
    if state is None:
        state = torch.zeros((B, 2), dtype=torch.int64, device=dev)
    if state.dtype != torch.int64 or tuple(state.shape) != (B, 2) or not state.is_contiguous():
        raise ValueError("state must be a contiguous int64 tensor [B][2]")
    if k_count is None:
        k_count = max(blocks(int(n_out.max().item()), plan.N), 0) if out is None else out.shape[1] // plan.H
    k_count = int(k_count)
    if out is None:
        out = torch.zeros((B, k_count * plan.H), dtype=torch.float32, device=dev)
    if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B or (out.shape[1] > 1 and out.stride(1) != 1):
        raise ValueError("out must be a float32 tensor [B][>= k_count * H]")
    if out.shape[1] < k_count * plan.H:
        raise ValueError("out holds %d samples per stream, %d blocks need %d" % (out.shape[1], k_count, k_count * plan.H))
    if status is None:
        status = torch.empty((B,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib.rts_warp_run(plan._h, samples.data_ptr(),
                                       nat.I16 if samples.dtype == torch.int16 else nat.F32,
                                       samples.stride(0), n_in.data_ptr(),
                                       anchors.data_ptr(), n_anchor.data_ptr(), int(anchors.shape[1]), n_out.data_ptr(),
                                       state.data_ptr(), k_count, out.data_ptr() if out.numel() else None,
                                       out.stride(0), status.data_ptr(), B, _stream(dev)))
    return out, state, status


def warp_pairs(audio_a, audio_b, paths, onto="a", hop=2048, N=1024, delta=256, device="cuda:0"):
    """Every pair of recordings on one timeline.  ``audio_a`` / ``audio_b``: lists of sample arrays (float32, or int16
    PCM), ``paths``: what ``dtw.align_pairs(chroma_a, chroma_b)`` returned for them, [(path (P_k, 2), total), ...] or the
    bare paths, in feature frames of ``hop`` samples.  ``onto="a"`` renders B on A's time axis (the result has A's length),
    ``onto="b"`` renders A on B's.  Pads, uploads once, makes the two calls (``rts_warp_anchors``, ``rts_warp_run``) and one
    read-back.  Returns a list of float32 arrays.  Raises ``RtsyncError`` when a path is refused (the message names the
    pair and its status)."""
    if onto not in ("a", "b"):
        raise ValueError("onto must be 'a' or 'b'")
    if not torch.cuda.is_available():
        raise RuntimeError("warp_pairs needs a ROCm GPU (no CPU fallback)")
    B = len(paths)
    if len(audio_a) != B or len(audio_b) != B:
        raise ValueError("warp_pairs: %d paths for %d and %d recordings" % (B, len(audio_a), len(audio_b)))
    if B == 0:
        return []
    dev = torch.device(device)
    col = 0 if onto == "a" else 1
    srcs = [np.asarray(x) for x in (audio_b if onto == "a" else audio_a)]
    n_out = [len(x) for x in (audio_a if onto == "a" else audio_b)]
    pcm = all(s.dtype == np.int16 for s in srcs)
    n_in = [len(s) for s in srcs]
    host = np.zeros((B, max(n_in + [1])), dtype=np.int16 if pcm else np.float32)
    for k, s in enumerate(srcs):
        host[k, :n_in[k]] = s if pcm or s.dtype != np.int16 else s.astype(np.float32) * np.float32(1.0 / 32768.0)
    arrs = [np.asarray(p[0] if isinstance(p, tuple) else p, dtype=np.int32).reshape(-1, 2) for p in paths]
    phost = np.zeros((B, max([len(a) for a in arrs] + [1]), 2), dtype=np.int32)
    for k, a in enumerate(arrs):
        phost[k, :len(a)] = a
    plan = WarpPlan(N, delta, device=dev)
    try:
        with torch.cuda.device(plan.device):
            anchors, n_anchor, st_a = anchors_from_paths(torch.from_numpy(phost).to(dev),
                                                         torch.tensor([len(a) for a in arrs], dtype=torch.int32), col, hop,
                                                         n_out, n_in)
            K = blocks(max(n_out), N)
            # one buffer, so that one copy brings everything back: the samples, then the two status words as float32 bits
            # (four words behind the samples keep every row on a 16-byte boundary)
            buf = torch.zeros((B, K * plan.H + 4), dtype=torch.float32, device=dev)
            st_r = torch.empty((B,), dtype=torch.int32, device=dev)
            warp(plan, torch.from_numpy(host).to(dev), n_in, anchors, n_anchor, n_out, k_count=K, out=buf, status=st_r)
            buf[:, K * plan.H:K * plan.H + 2] = torch.stack([st_a, st_r], dim=1).view(torch.float32)
            got = buf.cpu().numpy()
    finally:
        plan.close()
    status = got[:, K * plan.H:K * plan.H + 2].copy().view(np.int32)
    for k in range(B):
        if status[k, 0] or status[k, 1]:
            raise nat.RtsyncError("warp_pairs: pair %d was not rendered (path status %d, run status %d; "
                                  "include/rtsync.h, RTS_WARP_*)" % (k, status[k, 0], status[k, 1]))
    return [got[k, :n_out[k]].copy() for k in range(B)]
