"""Tempo curves of alignment paths (csrc/tempo.hip): the slope of a path over a trailing window of K points, and the
position its regression line gives -- how fast the performer is going, next to where ``poll()`` / ``path()`` say they are.

A path is points ``(live frame, reference frame)``; the slope at point i is the least-squares slope of the reference index
over the live index through points ``max(0, i - K + 1) .. i`` (1.0: the live side moves at the reference's tempo), ``pos``
the line read at point i's live frame plus ``ahead`` frames.  The windows are trailing, so entry i of a curve is what
``BatchedOTW.tempo`` / ``LiveSession.tempo`` would have published when point i was the newest.  include/rtsync.h
(rts_path_tempo) has the definition: exact integer sums, one rounding per float64 operation, so every implementation
agrees to the bit.  ``AnnotationTables.bpm`` turns slopes into beats per minute."""
import ctypes

import numpy as np
import torch

from . import _native as nat


def path_tempo(path_dev, len_dev, K, ahead=0.0, x_limit=None, y_limit=None):
    """The tempo curves of B paths in one launch (rts_path_tempo).  ``path_dev`` int32 [B][P_max][2] and ``len_dev`` int32
    [B] are laid out like the outputs of ``dtw.dtw_paths``; lengths <= 0 (the -1 fault marker included) give no entry,
    larger than P_max are clamped.  ``x_limit`` / ``y_limit``: a point outside ``[0, x_limit) x [0, y_limit)`` makes every
    window that contains it NaN; None takes one maximum over the valid points of the buffer (which synchronises), so
    that only negative coordinates are bad.  ``2 <= K <= 1024``; ``K * K * x_limit * y_limit`` must stay below 2^63.

    Returns device tensors ``(slope, pos)`` float64 [B][P_max]; entries behind ``len_dev[b]`` are not written.  NaN where
    the window has fewer than two points or its live index does not move.  Asynchronous when both limits are given."""
    dev = path_dev.device
    path_dev = path_dev.to(torch.int32).contiguous()
    if path_dev.dim() != 3 or path_dev.shape[2] != 2:
        raise ValueError("path_dev must be [B][P_max][2]")
    B, P_max = int(path_dev.shape[0]), int(path_dev.shape[1])
    len_dev = torch.as_tensor(len_dev).to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
    if len_dev.numel() != B:
        raise ValueError("len_dev: %d entries for %d paths" % (len_dev.numel(), B))
    with torch.cuda.device(dev):
        if x_limit is None or y_limit is None:
            valid = torch.arange(P_max, device=dev, dtype=torch.int32)[None, :] < len_dev[:, None]
            top = int(path_dev.masked_fill(~valid[:, :, None], 0).max().item()) + 1 if B * P_max else 1
            x_limit = max(top, 1) if x_limit is None else x_limit
            y_limit = max(top, 1) if y_limit is None else y_limit
        slope = torch.empty((B, P_max), dtype=torch.float64, device=dev)
        pos = torch.empty((B, P_max), dtype=torch.float64, device=dev)
        nat.check(nat.lib.rts_path_tempo(path_dev.data_ptr() if P_max else None, P_max, len_dev.data_ptr(), B, int(K),
                                         float(ahead), int(x_limit), int(y_limit), slope.data_ptr(), pos.data_ptr(),
                                         ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return slope, pos


def tempo_curves(paths, K, ahead=0.0, device="cuda:0"):
    """``path_tempo`` for a list of numpy paths, (P_k, 2) integer arrays of (live frame, reference frame) such as
    ``BatchedOTW.paths()``, ``backward()`` or ``dtw.align_pairs`` return.  Returns a list of ``(slope, pos)`` float64 arrays
    of P_k entries each.  The limits come from the largest coordinate given.  Synchronises."""
    arrs = [np.asarray(p, dtype=np.int32).reshape(-1, 2) for p in paths]
    if not arrs:
        return []
    host = np.zeros((len(arrs), max([len(a) for a in arrs] + [1]), 2), dtype=np.int32)
    for k, a in enumerate(arrs):
        host[k, :len(a)] = a
    dev = torch.device(device)
    slope, pos = path_tempo(torch.from_numpy(host).to(dev), torch.tensor([len(a) for a in arrs], dtype=torch.int32), K, ahead)
    slope, pos = slope.cpu().numpy(), pos.cpu().numpy()
    return [(slope[k, :len(a)].copy(), pos[k, :len(a)].copy()) for k, a in enumerate(arrs)]
