"""The backward path of on-line time warping, stated in numpy on the reference's dense matrices.

``acc`` / ``cost`` are ``OtwOracle(..., keep_cost=True).acc_cost()`` / ``.cost()`` (otw_eran.py:23,27 /
livenote_v2.py:21-23: never-evaluated cells hold the sentinel, resp. -1) after everything the stream has consumed,
``(t, j)`` its end position and ``rows`` the number of live frames it was given.

  end cell     best_point (otw_eran.py:192-211, livenote_v2.py:219-236) at (t', j') with t' = min(t, rows consumed - 1)
               and j' = min(j, N - 1): a stop or an overflow leaves one index one past the end.  Row t' over columns
               [max(0, j'-c+1), j'], column j' over rows [max(0, t'-c+1), t'], first minima; the row wins only if
               strictly smaller.
  predecessor  of (x, y) != (0, 0), with d = cost[x][y]: the first of (x, y-1) with acc + d, (x-1, y) with acc + d and
               (x-1, y-1) with acc + 2 d -- in-range candidates only -- whose sum == acc[x][y].  The candidate order of
               eval_path_cost (otw_eran.py:228-234).
  path         the predecessors from the end cell down to (0, 0), in forward order; total = acc[end].
"""
import numpy as np


def end_cell(acc, t, j, c, rows):
    """-> (x, y), or None for a stream that has consumed no frame."""
    M, N = acc.shape
    rows = min(int(rows), M)
    if rows < 1:
        return None
    tt, jj = min(int(t), rows - 1), min(int(j), N - 1)
    j1, t1 = max(0, jj - c + 1), max(0, tt - c + 1)
    row, col = acc[tt, j1:jj + 1], acc[t1:tt + 1, jj]
    ri, ci = int(np.argmin(row)), int(np.argmin(col))
    if row[ri] < col[ci]:
        return tt, j1 + ri
    return t1 + ci, jj


def predecessor(acc, cost, x, y):
    """-> (x', y', weight), or None if no candidate reproduces acc[x][y]."""
    d = cost[x, y]
    a = acc[x, y]
    if y > 0 and acc[x, y - 1] + d == a:
        return x, y - 1, 1
    if x > 0 and acc[x - 1, y] + d == a:
        return x - 1, y, 1
    if x > 0 and y > 0 and acc[x - 1, y - 1] + 2 * d == a:
        return x - 1, y - 1, 2
    return None


def backward(acc, cost, t, j, c, rows):
    """-> dict(path (n, 2) int32 in forward order, total, end (2,) int32, acc (n,), weights (n,) int: the step weight
    that leads INTO each point, 1 for (0, 0)).  A stream without a frame: empty path, NaN, (-1, -1)."""
    e = end_cell(acc, t, j, c, rows)
    if e is None:
        return dict(path=np.zeros((0, 2), np.int32), total=np.float64("nan"), end=np.array([-1, -1], np.int32),
                    acc=np.zeros(0), weights=np.zeros(0, np.int64))
    x, y = e
    pts, w = [(x, y)], []
    while (x, y) != (0, 0):
        p = predecessor(acc, cost, x, y)
        assert p is not None, "no predecessor reproduces acc[%d][%d]" % (x, y)
        x, y, wk = p
        w.append(wk)
        pts.append((x, y))
    w.append(1)
    path = np.array(pts[::-1], dtype=np.int32).reshape(-1, 2)
    return dict(path=path, total=np.float64(acc[e]), end=np.array(e, np.int32),
                acc=acc[path[:, 0], path[:, 1]].copy(), weights=np.array(w[::-1], dtype=np.int64))


def from_oracle(ref, live, c, mrc, variant, cost_kind, mode="insert"):
    """Run the CPU oracle over ``live`` (12, T) in ``mode`` ('insert' | 'set_live') and apply the definition.
    -> (backward(...) dict with the oracle's matrices under 'acc_matrix' / 'cost_matrix', the oracle)."""
    import oracle
    o = oracle.OtwOracle(ref, c, mrc, variant, cost_kind, keep_cost=True)
    T = live.shape[1]
    if T == 0:
        rows = 0
    elif mode == "set_live":
        o.set_live(live)
        rows = T
    else:
        rows = o.run(live)
    acc, cost = o.acc_cost(), o.cost()
    st = o.state
    m = backward(acc, cost, st["t"], st["j"], c, rows)
    m["acc_matrix"], m["cost_matrix"] = acc, cost
    return m, o


def forward_sum(cost, path, weights):
    """The sequential forward-order sum of w * cost along ``path`` (what ``total`` must equal bit for bit)."""
    s = np.float64(0.0)
    for k, (x, y) in enumerate(path):
        s = cost[x, y] if k == 0 else s + weights[k] * cost[x, y]
    return s
