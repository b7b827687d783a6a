"""Serial restatement of the contract of rts_dtw_subseq_paths (include/rtsync.h) for one pair: subsequence DTW of an
excerpt `a` (rows, matched entirely) against a piece `b` (columns, free at both ends), with the path.

    D[0][j] = c(0, j)
    D[i][0] = D[i-1][0] + c(i, 0)
    D[i][j] = first minimum of (D[i][j-1] + c, D[i-1][j] + c, D[i-1][j-1] + 2c)       (left, up, diag)
    end   = first j minimising D[M-1][j]
    total = D[M-1][end]
    path  = from (M-1, end) the chosen predecessor of every cell until a cell of row 0, in forward order;
            start = the column of that row-0 cell

The cell costs are the oracle's own cost matrix (oracle.binding.dtw(a, b)[0]: 1 - <a_i, b_j> as one fma chain in k
order); Python floats are IEEE doubles, so every sum below is the float64 sum and there is one right answer."""
import numpy as np

LEFT, UP, DIAG = 0, 1, 2


def dot_cost(a, b):
    """[M][N] cost matrix of a (12, M) against b (12, N), feature-major float64."""
    import oracle.binding as ob
    return ob.dtw(a, b)[0]


def subseq_from_cost(C):
    """-> (path int32 (P, 2), total, start, end, D[M-1][:] float64 (N,)) for the cost matrix C [M][N], M, N >= 1."""
    C = [[float(v) for v in r] for r in np.asarray(C, dtype=np.float64)]
    M, N = len(C), len(C[0])
    D = list(C[0])
    back = [None]                       # row 0 has no predecessors
    for i in range(1, M):
        Ci = C[i]
        nD, nb = [D[0] + Ci[0]], [UP]
        for j in range(1, N):
            c = Ci[j]
            best, s = nD[j - 1] + c, LEFT
            o1 = D[j] + c
            if o1 < best:
                best, s = o1, UP
            o2 = D[j - 1] + 2 * c
            if o2 < best:
                best, s = o2, DIAG
            nD.append(best)
            nb.append(s)
        D = nD
        back.append(nb)
    end = 0
    for j in range(1, N):
        if D[j] < D[end]:
            end = j
    i, j = M - 1, end
    rev = [(i, j)]
    while i > 0:
        s = back[i][j]
        if s != LEFT:
            i -= 1
        if s != UP:
            j -= 1
        rev.append((i, j))
    path = np.array(rev[::-1], dtype=np.int32).reshape(-1, 2)
    return path, D[end], int(path[0, 1]), end, np.array(D, dtype=np.float64)


def subseq(a, b):
    """The model for feature-major a (12, M), b (12, N)."""
    return subseq_from_cost(dot_cost(a, b))


def path_cost(C, path):
    """Re-accumulates the cell costs along `path` in order, doubled on diagonal steps: the float64 sums the DP made."""
    C = np.asarray(C, dtype=np.float64)
    i0, j0 = int(path[0][0]), int(path[0][1])
    acc = float(C[i0, j0])
    for (pi, pj), (i, j) in zip(path[:-1], path[1:]):
        c = float(C[int(i), int(j)])
        acc = acc + (2 * c if (i - pi == 1 and j - pj == 1) else c)
    return acc


def planted(N, A, L, seed, noise=0.03, stretch=False):
    """A synthetic piece of N frames and, as the excerpt, its frames [A, A + L) with small noise (renormalised, float32
    values) -- with `stretch`, every third frame of the excerpt repeated.  -> (excerpt (12, M), piece (12, N))."""
    from real_time_audio_sync_amd import synth
    piece = synth.synth_ref(N, seed=seed)
    cols = np.arange(A, A + L)
    if stretch:
        cols = np.repeat(cols, np.where(np.arange(L) % 3 == 2, 2, 1))
    rs = np.random.RandomState(seed + 1)
    q = piece[:, cols] + noise * rs.rand(12, len(cols))
    q = (q / np.sqrt((q * q).sum(axis=0, keepdims=True))).astype(np.float32).astype(np.float64)
    return q, piece
