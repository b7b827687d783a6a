"""Locate: where in the repertoire is this microphone?  Subsequence DTW of short live excerpts against every piece of
a reference pool (csrc/locate.hip, ``rts_locate`` in include/rtsync.h).  The reference has no such function; the
recurrence is dtw.py's with the first row freed, so a match may begin and end anywhere on a piece."""
import ctypes

import torch

from . import _native as nat


def _dtype_code(dt):
    if dt == torch.float32:
        return nat.F32
    if dt == torch.float64:
        return nat.F64
    raise TypeError("feature tensors must be float32 or float64, got %s" % dt)


def _shapes(queries_dev, q_len_dev, pool_dev, first_dev, len_dev):
    """The checks locate_batch and locate_matches share -> (queries [B][M_max][F], pool, B, M_max, F, P, n_pool)."""
    if queries_dev.dim() == 2:
        queries_dev = queries_dev.unsqueeze(0)
    queries_dev, pool_dev = queries_dev.contiguous(), pool_dev.contiguous()
    B, M_max, F = queries_dev.shape
    P = int(first_dev.shape[0])
    if first_dev.dtype != torch.int64 or len_dev.dtype != torch.int32 or len_dev.shape[0] != P:
        raise TypeError("first_dev must be int64 [P] and len_dev int32 [P]")
    if q_len_dev is not None and (q_len_dev.dtype != torch.int32 or q_len_dev.shape[0] != B):
        raise TypeError("q_len_dev must be int32 [B]")
    return queries_dev, pool_dev, B, M_max, F, P, int(pool_dev.shape[0])


def locate_batch(queries_dev, q_len_dev, pool_dev, first_dev, len_dev, euclid=False, want_rows=False):
    """queries_dev: [B][M_max][12] (or [M_max][12] for one stream), M_max <= 256; q_len_dev: int32 [B] valid frames per
    stream or None; pool_dev: [n_pool][12]; first_dev int64 [P] / len_dev int32 [P]: piece p is frames
    [first[p], first[p] + len[p]) of the pool.  All device tensors, features float32 or float64.

    Returns device tensors ``(cost [B][P] float64, end [B][P] int32, start [B][P] int32)``: the cheapest warping of
    stream b's excerpt onto piece p covers frames start..end of the piece (both inclusive, relative to the piece) at
    accumulated cost ``cost``.  ``+inf, -1, -1`` where there is nothing to match: a piece with len < 1 or outside the
    pool, a stream with q_len 0.  With ``want_rows`` also ``row [B][n_pool] float64`` and ``rowstart [B][n_pool]
    int32``: the last row of the accumulated-cost matrix of every piece at its pool position and the start each of
    its cells carries (+inf / -1 where no piece lies; where pieces overlap, one of them).

    Features must be finite: a NaN frame (a silent microphone normalises to one) makes the results of the (stream,
    piece) pairs it takes part in unspecified.  Asynchronous on the current stream."""
    dev = pool_dev.device
    queries_dev, pool_dev, B, M_max, F, P, n_pool = _shapes(queries_dev, q_len_dev, pool_dev, first_dev, len_dev)
    cost = torch.empty((B, P), dtype=torch.float64, device=dev)
    end = torch.empty((B, P), dtype=torch.int32, device=dev)
    start = torch.empty((B, P), dtype=torch.int32, device=dev)
    row = torch.full((B, n_pool), float("inf"), dtype=torch.float64, device=dev) if want_rows else None
    rowstart = torch.full((B, n_pool), -1, dtype=torch.int32, device=dev) if want_rows else None
    nat.check(nat.lib.rts_locate(queries_dev.data_ptr(), _dtype_code(queries_dev.dtype), M_max,
                                 q_len_dev.data_ptr() if q_len_dev is not None else None, B,
                                 pool_dev.data_ptr(), _dtype_code(pool_dev.dtype), F, n_pool,
                                 first_dev.data_ptr(), len_dev.data_ptr(), P,
                                 nat.COST_EUCLID if euclid else nat.COST_DOT,
                                 cost.data_ptr(), end.data_ptr(), start.data_ptr(),
                                 row.data_ptr() if want_rows else None, rowstart.data_ptr() if want_rows else None,
                                 ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return (cost, end, start, row, rowstart) if want_rows else (cost, end, start)


def locate_matches(queries_dev, q_len_dev, pool_dev, first_dev, len_dev, K, max_cost=float("inf"), euclid=False):
    """Ranked non-overlapping matches per (stream, piece) (``rts_locate_matches`` in include/rtsync.h): an excerpt of a
    repeated section matches every pass of the repeat, and ``locate_batch`` reports the earliest only.  Arguments as
    ``locate_batch``; ``K``: ranks per (stream, piece), 1..32; ``max_cost``: the list of a pair ends in front of the
    first rank that costs more (+inf: no cut-off).

    Returns device tensors ``(cost [B][P][K] float64, end [B][P][K] int32, start [B][P][K] int32, n [B][P] int32)``:
    rank r of stream b on piece p covers frames start..end of the piece; rank 0 is ``locate_batch``'s answer bit for
    bit, costs do not decrease with the rank, ranges of one pair are disjoint.  ``n``: ranks written, the slots behind
    them hold ``+inf, -1, -1``; 0 where there is nothing to match; -1 for a piece whose pool range intersects that of
    another piece (slot 0 then holds ``locate_batch``'s answer and nothing else is known).  Allocates the workspace
    (12 bytes per stream and pool frame).  Asynchronous on the current stream."""
    dev = pool_dev.device
    queries_dev, pool_dev, B, M_max, F, P, n_pool = _shapes(queries_dev, q_len_dev, pool_dev, first_dev, len_dev)
    K = int(K)
    nbytes = ctypes.c_size_t()
    nat.check(nat.lib.rts_locate_matches_workspace_bytes(B, n_pool, ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    cost = torch.empty((B, P, max(K, 0)), dtype=torch.float64, device=dev)
    end = torch.empty((B, P, max(K, 0)), dtype=torch.int32, device=dev)
    start = torch.empty((B, P, max(K, 0)), dtype=torch.int32, device=dev)
    n = torch.empty((B, P), dtype=torch.int32, device=dev)
    nat.check(nat.lib.rts_locate_matches(queries_dev.data_ptr(), _dtype_code(queries_dev.dtype), M_max,
                                         q_len_dev.data_ptr() if q_len_dev is not None else None, B,
                                         pool_dev.data_ptr(), _dtype_code(pool_dev.dtype), F, n_pool,
                                         first_dev.data_ptr(), len_dev.data_ptr(), P,
                                         nat.COST_EUCLID if euclid else nat.COST_DOT, K, float(max_cost),
                                         cost.data_ptr(), end.data_ptr(), start.data_ptr(), n.data_ptr(),
                                         ws.data_ptr(), nbytes.value,
                                         ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return cost, end, start, n


class Candidates(list):
    """The list ``reacquire`` hands to ``choose``: ``(ref_object, start, end, cost)`` cheapest first, and ``M``, the
    frames of the excerpt they were found with."""
    M = None


def nearest_to(where, slack, M=None):
    """A ``choose`` for ``reacquire(streams, matches=K, choose=...)``: of equally good matches, the one nearest to where
    the stream was last known to be.  ``where = {b: (ref_object, frame)}``, e.g. from ``poll()`` / ``read_states``
    before the restart.  Among stream b's candidates on that piece, those whose cost per path step ``cost / (M + end -
    start + 1)`` is within ``slack`` of the best candidate's (of any piece) are considered, and the one whose ``start``
    is nearest to ``frame`` is chosen (the cheaper one on a tie); if there is none, or ``where`` does not name the
    stream, the overall best: the first candidate, as without ``choose``.  ``slack`` has no default: what "equally
    good" means depends on the material.  ``M``: the excerpt's frames, for hand-made lists; the lists ``reacquire``
    hands over carry their own."""
    slack = float(slack)

    def choose(b, candidates):
        if not candidates:
            return None
        m = getattr(candidates, "M", None) or M
        if m is None:
            raise ValueError("nearest_to needs the excerpt's length: give M, or a reacquire candidate list")
        step = [c / (m + e - s + 1) for _, s, e, c in candidates]
        best = min(range(len(step)), key=lambda k: (step[k], k))
        if b not in where:
            return 0
        piece, frame = where[b]
        near = [k for k, (r, _, _, _) in enumerate(candidates) if r is piece and step[k] <= step[best] + slack]
        if not near:
            return 0
        return min(near, key=lambda k: (abs(candidates[k][1] - frame), k))
    return choose
