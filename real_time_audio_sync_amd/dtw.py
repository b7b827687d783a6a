"""Drop-in for the reference's dtw.py: ``DTW(seq_a, seq_b) -> (cost, acc_cost, path)``, plus a
batched form over many pairs, a path-only form over pairs of different lengths (``dtw_paths``, ``align_pairs``) and its
subsequence form for excerpts against whole pieces (``dtw_subseq_paths``, ``align_excerpts``).
Computation: csrc/dtw.hip (reference: dtw.py:5-53)."""
import ctypes

import numpy as np
import torch

from . import _native as nat
from .otw_batch import frames_tensor, _np_dtype_code


def dtw_batch(a_dev, b_dev, want_back=True, check=False):
    """a_dev: [B][M][12] or [M][12] (shared), b_dev: [B][N][12] or [N][12] (shared); device
    tensors, float32/float64.  Returns device tensors (cost [B][M][N] f64, acc [B][M][N] f64,
    back [B][M][N] int8 -- None unless want_back --, path [B][M+N][2] int32, path_len [B] int32).
    Asynchronous.

    Fault contract: ``path_len[k] == -1`` means the device pipeline reported a fault (a bounded in-launch wait between
    workgroups ran out -- never expected); the other outputs of that call are then not to be used.  ``check=True``
    synchronises and raises RtsyncError instead of leaving that to the caller."""
    dev = a_dev.device
    sa = a_dev.dim() == 2
    sb = b_dev.dim() == 2
    B = 1 if (sa and sb) else (b_dev.shape[0] if sa else a_dev.shape[0])
    M, N = a_dev.shape[-2], b_dev.shape[-2]
    a_dev, b_dev = a_dev.contiguous(), b_dev.contiguous()
    cost = torch.empty((B, M, N), dtype=torch.float64, device=dev)
    acc = torch.empty((B, M, N), dtype=torch.float64, device=dev)
    back = torch.empty((B, M, N), dtype=torch.int8, device=dev) if want_back else None
    path = torch.empty((B, M + N, 2), dtype=torch.int32, device=dev)
    plen = torch.zeros((B,), dtype=torch.int32, device=dev)
    nbytes = ctypes.c_size_t(0)
    nat.check(nat.lib.rts_dtw_workspace_bytes(M, N, B, ctypes.byref(nbytes)))
    ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=dev)
    nat.check(nat.lib.rts_dtw(a_dev.data_ptr(), _np_dtype_code(a_dev.dtype), 0 if sa else M,
                              b_dev.data_ptr(), _np_dtype_code(b_dev.dtype), 0 if sb else N,
                              12, M, N, B, cost.data_ptr(), acc.data_ptr(),
                              back.data_ptr() if back is not None else None, path.data_ptr(),
                              plen.data_ptr(), ws.data_ptr(), nbytes.value,
                              ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    if check and int(plen.min().item()) < 1:
        raise nat.RtsyncError("rts_dtw: the device pipeline reported a fault (path_len = -1)")
    return cost, acc, back, path, plen


def DTW(seq_a, seq_b, device="cuda:0"):
    """seq_a (12, M), seq_b (12, N) feature-major like the reference; rows of the returned matrices
    index seq_a.  Returns (cost (M,N) float64, acc_cost (M,N) float64, path (P,2) int64)."""
    if not torch.cuda.is_available():
        raise RuntimeError("DTW needs a ROCm GPU (no CPU fallback)")
    dev = torch.device(device)
    a = frames_tensor(np.asarray(seq_a, dtype=np.float64), dev)
    b = frames_tensor(np.asarray(seq_b, dtype=np.float64), dev)
    cost, acc, _, path, plen = dtw_batch(a, b, want_back=False)
    n = int(plen[0].item())
    if n < 1:
        raise nat.RtsyncError("rts_dtw: the device pipeline reported a fault")
    return cost[0].cpu().numpy(), acc[0].cpu().numpy(), path[0, :n].cpu().numpy().astype(np.int64)


def _lengths(v, B, dev, name):
    """A per-pair length table as the C-ABI wants it: None, or a device int32 [B] tensor."""
    if v is None:
        return None
    t = torch.as_tensor(v).to(device=dev, dtype=torch.int32).contiguous()
    if t.dim() != 1 or t.shape[0] != B:
        raise ValueError("%s must hold one length per pair (%d), got shape %s" % (name, B, tuple(t.shape)))
    return t


def _infer_pairs(a_dev, b_dev, a_len, b_len):
    """The number of pairs of a path-only call: that of whichever side is batched; with both sides shared, the number of
    lengths given (a_len if given, else b_len), 1 without any.  ValueError when the two sides hold different numbers."""
    sa, sb = a_dev.dim() == 2, b_dev.dim() == 2
    if not sa and not sb and a_dev.shape[0] != b_dev.shape[0]:
        raise ValueError("a_dev holds %d pairs, b_dev %d" % (a_dev.shape[0], b_dev.shape[0]))
    if not sa:
        return a_dev.shape[0]
    if not sb:
        return b_dev.shape[0]
    given = a_len if a_len is not None else b_len
    return 1 if given is None else int(torch.as_tensor(given).numel())


def _paths_call(a_dev, b_dev, a_len, b_len, B, path, plen, total, start=None, end=None, row=None):
    """rts_dtw_paths, or with start / end (and optionally row) rts_dtw_subseq_paths: the same arguments but for those."""
    dev = a_dev.device
    M, N = a_dev.shape[-2], b_dev.shape[-2]
    name = "rts_dtw_paths" if start is None else "rts_dtw_subseq_paths"
    ends = () if start is None else (start.data_ptr(), end.data_ptr(), row.data_ptr() if row is not None else None)
    nbytes = ctypes.c_size_t(0)
    nat.check(getattr(nat.lib, name + "_workspace_bytes")(M, N, B, ctypes.byref(nbytes)))
    ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=dev)
    nat.check(getattr(nat.lib, name)(
        a_dev.data_ptr(), _np_dtype_code(a_dev.dtype), 0 if a_dev.dim() == 2 else M,
        a_len.data_ptr() if a_len is not None else None,
        b_dev.data_ptr(), _np_dtype_code(b_dev.dtype), 0 if b_dev.dim() == 2 else N,
        b_len.data_ptr() if b_len is not None else None,
        12, M, N, B, path.data_ptr(), plen.data_ptr(), total.data_ptr(), *ends, ws.data_ptr(), nbytes.value,
        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))


def _align(who, name, seqs_a, seqs_b, device, dtype, n_tables):
    """The body of align_pairs (n_tables = 1: path_len) and align_excerpts (3: path_len, start, end): pads, uploads once,
    makes one call and one read-back.  Returns (path [B][M+N][2], total [B] float64, the int32 tables), on the host."""
    if not torch.cuda.is_available():
        raise RuntimeError("%s needs a ROCm GPU (no CPU fallback)" % who)
    dev = torch.device(device)
    a_one, b_one = isinstance(seqs_a, (np.ndarray, torch.Tensor)), isinstance(seqs_b, (np.ndarray, torch.Tensor))
    B = 1 if (a_one and b_one) else (len(seqs_b) if a_one else len(seqs_a))
    if B < 1:
        return None
    a, a_len = _pad_frames(seqs_a, B, dtype, who)
    b, b_len = _pad_frames(seqs_b, B, dtype, who)
    a, b = a.to(dev), b.to(dev)
    M, N = a.shape[-2], b.shape[-2]
    # one int32 buffer for all outputs, so that one copy brings them back: total (as float64), then the int32 tables
    # (padded together to an even count: the path is written in 8-byte pairs), path
    head = 2 * B + n_tables * B + (n_tables * B & 1)

    def unpack(buf, view64):
        return (buf[head:].reshape(B, M + N, 2), view64(buf[:2 * B]),
                [buf[(2 + t) * B:(3 + t) * B] for t in range(n_tables)])

    out = torch.zeros((head + B * (M + N) * 2,), dtype=torch.int32, device=dev)
    path, total, tables = unpack(out, lambda x: x.view(torch.float64))
    _paths_call(a, b, _lengths(a_len, B, dev, "a_len"), _lengths(b_len, B, dev, "b_len"), B, path, tables[0], total,
                *tables[1:])
    path, total, tables = unpack(out.cpu().numpy(), lambda x: x.view(np.float64))
    if int(tables[0].min()) < 0:
        raise nat.RtsyncError("%s: the device pipeline reported a fault" % name)
    return path, total, tables


def dtw_paths(a_dev, b_dev, a_len=None, b_len=None, check=False):
    """Alignment paths and total costs only, for pairs of different lengths in one call: no cost or acc_cost matrix is
    written or allocated (about 0.45 bytes of workspace per cell instead of 16).

    a_dev: [B][M_max][12] or [M_max][12] (shared), b_dev: [B][N_max][12] or [N_max][12] (shared); device tensors,
    float32/float64, padded.  a_len / b_len: the pairs' own lengths -- device int32 tensors or anything torch.as_tensor
    takes; None = the maximum for every pair, larger values are clamped to it.  With both sequences shared, B is the
    number of lengths given (1 without any).  Pair k is ``dtw_batch`` of a[k, :a_len[k]] against b[k, :b_len[k]].

    Returns device tensors (path [B][M_max+N_max][2] int32, path_len [B] int32, total [B] float64): the first
    path_len[k] rows of path[k] run from (0, 0) to (a_len[k]-1, b_len[k]-1), the rows behind them are not written;
    total[k] is acc_cost[-1, -1].  A pair with a length < 1 has path_len 0 and total +inf.  Asynchronous.

    Fault contract as ``dtw_batch``: path_len[k] == -1 (and total NaN); ``check=True`` synchronises and raises.

    Errors: ValueError when a length table does not hold one length per pair (with both sequences shared that includes
    a_len and b_len of different sizes: B is the size of a_len if given, else of b_len) or when a_dev and b_dev hold
    different numbers of pairs.  Both sequences shared and no lengths is one pair, not an error."""
    dev = a_dev.device
    B = _infer_pairs(a_dev, b_dev, a_len, b_len)
    M, N = a_dev.shape[-2], b_dev.shape[-2]
    a_dev, b_dev = a_dev.contiguous(), b_dev.contiguous()
    a_len, b_len = _lengths(a_len, B, dev, "a_len"), _lengths(b_len, B, dev, "b_len")
    path = torch.empty((B, M + N, 2), dtype=torch.int32, device=dev)
    plen = torch.zeros((B,), dtype=torch.int32, device=dev)
    total = torch.empty((B,), dtype=torch.float64, device=dev)
    _paths_call(a_dev, b_dev, a_len, b_len, B, path, plen, total)
    if check and int(plen.min().item()) < 0:
        raise nat.RtsyncError("rts_dtw_paths: the device pipeline reported a fault (path_len = -1)")
    return path, plen, total


def _pad_frames(seqs, B, dtype, who="align_pairs"):
    """(12, n_k) feature-major arrays -> (host [B][n_max][12] or, for a single shared array, [n][12]; lengths or None)."""
    if isinstance(seqs, (np.ndarray, torch.Tensor)):
        x = torch.as_tensor(np.asarray(seqs)).to(dtype)
        return x.t().contiguous(), None
    if len(seqs) != B:
        raise ValueError("%s: %d sequences on one side, %d on the other" % (who, len(seqs), B))
    lens = [int(np.shape(x)[1]) for x in seqs]
    out = torch.zeros((B, max(max(lens), 1), 12), dtype=dtype)
    for k, x in enumerate(seqs):
        out[k, :lens[k]] = torch.as_tensor(np.asarray(x)).to(dtype).t()
    return out, lens


def align_pairs(seqs_a, seqs_b, device="cuda:0", dtype=torch.float64):
    """Offline DTW of many pairs of different lengths at once, for a corpus harness (the reference's tests.py:199-262
    aligns every recording of a piece against every other, one DTW call per pair).

    seqs_a, seqs_b: lists of feature-major (12, M_k) / (12, N_k) arrays like ``DTW()`` takes; a single array on either
    side is shared by all pairs.  Pads, uploads once, makes one ``rts_dtw_paths`` call and one read-back.
    Returns [(path (P_k, 2) int64 ndarray, total float), ...], each path what ``DTW(seqs_a[k], seqs_b[k])[2]`` is and
    ready for ``evaluate.AlignmentError(ref_csv, live_csv, path)``; total is acc_cost[-1, -1]."""
    got = _align("align_pairs", "rts_dtw_paths", seqs_a, seqs_b, device, dtype, 1)
    if got is None:
        return []
    path, total, (plen,) = got
    return [(path[k, :int(plen[k])].astype(np.int64), float(total[k])) for k in range(len(plen))]


def dtw_subseq_paths(a_dev, b_dev, a_len=None, b_len=None, want_row=False, check=False):
    """Subsequence DTW with paths: every a (an excerpt, matched entirely) against the stretch of its b (a whole piece,
    free at both ends) it fits best.  ``dtw_paths`` with the first row freed and the end taken at the first minimum of the
    last row; any excerpt length, same workspace (about 0.45 bytes per cell), no matrix written.

    a_dev, b_dev, a_len, b_len: as ``dtw_paths`` (B inferred the same way; a shared b_dev [N_max][12] is the common case:
    many excerpts against one piece).

    Returns device tensors (path [B][M_max+N_max][2] int32, path_len [B] int32, total [B] float64, start [B] int32,
    end [B] int32) and, with ``want_row``, row [B][N_max] float64: the first path_len[k] rows of path[k] run from
    (0, start[k]) to (a_len[k]-1, end[k]), the rows behind them are not written; total[k] is the accumulated cost of
    that path, equal to ``dtw_paths``' total of a[k] against b[k, start[k]:end[k]+1]; row[k, :b_len[k]] is the last row
    of the accumulated-cost matrix (its cells behind b_len[k] are not written).  A pair with a length < 1 has path_len 0,
    total +inf and start = end = -1.  Asynchronous.

    Fault contract as ``dtw_paths``: path_len[k] == -1 (total NaN, start = end = -1); ``check=True`` synchronises and
    raises.  Errors as ``dtw_paths``."""
    dev = a_dev.device
    B = _infer_pairs(a_dev, b_dev, a_len, b_len)
    M, N = a_dev.shape[-2], b_dev.shape[-2]
    a_dev, b_dev = a_dev.contiguous(), b_dev.contiguous()
    a_len, b_len = _lengths(a_len, B, dev, "a_len"), _lengths(b_len, B, dev, "b_len")
    path = torch.empty((B, M + N, 2), dtype=torch.int32, device=dev)
    plen = torch.zeros((B,), dtype=torch.int32, device=dev)
    total = torch.empty((B,), dtype=torch.float64, device=dev)
    start = torch.empty((B,), dtype=torch.int32, device=dev)
    end = torch.empty((B,), dtype=torch.int32, device=dev)
    row = torch.empty((B, N), dtype=torch.float64, device=dev) if want_row else None
    _paths_call(a_dev, b_dev, a_len, b_len, B, path, plen, total, start, end, row)
    if check and int(plen.min().item()) < 0:
        raise nat.RtsyncError("rts_dtw_subseq_paths: the device pipeline reported a fault (path_len = -1)")
    return (path, plen, total, start, end, row) if want_row else (path, plen, total, start, end)


def align_excerpts(excerpts, pieces, device="cuda:0", dtype=torch.float64):
    """``align_pairs`` for excerpts: each excerpt is aligned against the stretch of its piece it fits best (a stream
    restarted inside a piece, a re-acquired stream's history, a rehearsal take, a cut of a recording).

    excerpts, pieces: lists of feature-major (12, M_k) / (12, N_k) arrays; a single array on either side is shared by
    all pairs (typically one piece).  Pads, uploads once, makes one ``rts_dtw_subseq_paths`` call and one read-back.
    Returns [(path (P_k, 2) int64 ndarray, total float, start int, end int), ...]: path[:, 0] indexes the excerpt's
    frames, path[:, 1] the piece's, from (0, start) to (M_k-1, end) -- ready for
    ``evaluate.AlignmentError(excerpt_csv, piece_csv, path)``.  A pair without frames on either side gives an empty
    path, total inf and start = end = -1."""
    got = _align("align_excerpts", "rts_dtw_subseq_paths", excerpts, pieces, device, dtype, 3)
    if got is None:
        return []
    path, total, (plen, start, end) = got
    return [(path[k, :int(plen[k])].astype(np.int64), float(total[k]), int(start[k]), int(end[k]))
            for k in range(len(plen))]
