"""The time map of an alignment path (csrc/pathmap.hip): read a position on one recording, say where that moment lies on
the other.  ``dtw.align_pairs`` / ``dtw_paths``, ``align_excerpts`` and ``BatchedOTW.backward()`` make the paths;
``map_frames`` maps positions along them and ``AnnotationTables.transfer`` carries a whole ground-truth table over.

include/rtsync.h (rts_path_map) has the definition: the knots are the distinct values of the ``from_side`` column, each
mapped to the middle of the other column's run there, with float64 linear interpolation in between and NaN outside the
first and last knot.  tests/pathmap_model.py is the same in plain Python; host and device agree to the bit."""
import ctypes

import numpy as np
import torch

from . import _native as nat


def pack_paths(paths, device):
    """``paths``: a list of (P_k, 2) integer arrays, or a device tuple ``(path int32 [B][P_max][2], path_len int32 [B],
    ...)`` as ``dtw.dtw_paths`` / ``dtw_subseq_paths`` return it -> device tensors (path, path_len)."""
    if isinstance(paths, tuple) and len(paths) >= 2 and torch.is_tensor(paths[0]):
        path, plen = paths[0], paths[1]
    else:
        arrs = [np.asarray(p, dtype=np.int32).reshape(-1, 2) for p in paths]
        host = np.zeros((len(arrs), max([len(a) for a in arrs] + [1]), 2), dtype=np.int32)
        for k, a in enumerate(arrs):
            host[k, :len(a)] = a
        path, plen = torch.from_numpy(host), torch.tensor([len(a) for a in arrs], dtype=torch.int32)
    path = path.to(device=device, dtype=torch.int32).contiguous()
    plen = plen.to(device=device, dtype=torch.int32).contiguous()
    if path.dim() != 3 or path.shape[2] != 2 or plen.dim() != 1 or plen.shape[0] != path.shape[0]:
        raise ValueError("paths must be [B][P_max][2] with one length per pair")
    return path, plen


def pack_offsets(offsets, B, device):
    """None, or (B, 2) integers -- offsets[k][c] is added to column c of pair k's path -> a device int32 [B][2] tensor."""
    if offsets is None:
        return None
    t = offsets if torch.is_tensor(offsets) else torch.as_tensor(np.asarray(offsets, dtype=np.int32))
    t = t.to(device=device, dtype=torch.int32).contiguous()
    if tuple(t.shape) != (B, 2):
        raise ValueError("offsets must hold two integers per pair (%d pairs), got shape %s" % (B, tuple(t.shape)))
    return t


def refusals(status):
    """{pair: reason} of the pairs whose status word (RTS_PATHMAP_*) is not 0."""
    return {k: ", ".join(text for bit, text in nat.PATHMAP_REASONS if int(s) & bit)
            for k, s in enumerate(status) if int(s) != 0}


def refusal_message(bad):
    return "pair%s %s: the path is refused (%s)" % ("s" if len(bad) > 1 else "", ", ".join(str(k) for k in sorted(bad)),
                                                     "; ".join("%d: %s" % (k, bad[k]) for k in sorted(bad)))


def map_frames(paths, positions, from_side=0, offsets=None, n=None, device="cuda:0"):
    """Positions on column ``from_side`` of every pair's path, in frames (fractions allowed), mapped onto the other column.

    List form -- ``paths`` a list of B (P_k, 2) integer arrays, ``positions`` a list of B float arrays of any lengths:
    synchronises and returns a list of float64 arrays, NaN where a position has no image (NaN itself, before the first or
    behind the last knot).  Raises ValueError naming the pairs whose path is refused and why (no point, a column that
    steps back, an index below 0 after the offsets).

    Tensor form -- ``paths`` the device triple of ``dtw.dtw_paths`` or a pair ``(path, path_len)``, ``positions`` a float64
    device tensor [B][n_max], ``n`` the valid entries per pair (None: all): asynchronous, nothing is read back; returns
    device tensors ``(y float64 [B][n_max], status int32 [B])``.  Entries behind ``n[b]`` are not written; a pair with a
    status other than 0 holds NaN in all of its valid entries.

    ``offsets``: None or two integers per pair, added to column 0 and column 1 of the pair's path (where a restarted
    stream's or an excerpt's own range begins)."""
    as_list = not torch.is_tensor(positions)
    if not torch.cuda.is_available():
        raise RuntimeError("map_frames needs a ROCm GPU (no CPU fallback)")
    if as_list:
        dev = torch.device(device)
        rows = [np.asarray(x, dtype=np.float64).reshape(-1) for x in positions]
        host = np.zeros((len(rows), max([len(r) for r in rows] + [1])), dtype=np.float64)
        for b, r in enumerate(rows):
            host[b, :len(r)] = r
        positions, n = torch.from_numpy(host), [len(r) for r in rows]
    else:
        dev = positions.device
    if dev.index is None:
        dev = torch.device(dev.type, torch.cuda.current_device())
    path, plen = pack_paths(paths, dev)
    B, P_max = int(path.shape[0]), int(path.shape[1])
    x = positions.to(device=dev, dtype=torch.float64).contiguous()
    if x.dim() != 2 or x.shape[0] != B:
        raise ValueError("%d paths, positions of shape %s" % (B, tuple(x.shape)))
    if B < 1:
        return [] if as_list else (x.clone(), torch.zeros((0,), dtype=torch.int32, device=dev))
    n_max = int(x.shape[1])
    off = pack_offsets(offsets, B, dev)
    if n is not None:
        n = (n if torch.is_tensor(n) else torch.as_tensor(np.asarray(n, dtype=np.int32).reshape(-1)))
        n = n.to(device=dev, dtype=torch.int32).contiguous()
        if n.numel() != B:
            raise ValueError("n: %d entries for %d pairs" % (n.numel(), B))
    with torch.cuda.device(dev):
        y = torch.empty((B, n_max), dtype=torch.float64, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        nat.check(nat.lib.rts_path_map(path.data_ptr() if P_max else None, P_max, plen.data_ptr(),
                                       off.data_ptr() if off is not None else None, int(from_side),
                                       x.data_ptr() if n_max else None, n_max, n.data_ptr() if n is not None else None, B,
                                       y.data_ptr() if n_max else None, status.data_ptr(),
                                       ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    if not as_list:
        return y, status
    y, status = y.cpu().numpy(), status.cpu().numpy()
    bad = refusals(status)
    if bad:
        raise ValueError("map_frames: " + refusal_message(bad))
    return [y[b, :len(r)].copy() for b, r in enumerate(rows)]
