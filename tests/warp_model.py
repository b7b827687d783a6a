"""The renderer's definition in numpy (include/rtsync.h, rts_warp_run and rts_warp_anchors): WSOLA along
a piecewise-linear integer time map, to the bit.  Python integers carry the map (exact at any size), float64 numpy the
sums, in the operation order the header states."""
import numpy as np

MIN_N, MAX_N, MAX_DELTA = 64, 4096, 1024
SEG_LIMIT, POS_LIMIT = 1 << 31, 1 << 62
(PATH_EMPTY, PATH_START, PATH_BACKWARD, PATH_SHORT_OUT, PATH_SHORT_IN, PATH_TOO_MANY, NO_MAP, BAD_MAP,
 BAD_STATE) = (1 << i for i in range(9))


def hann(n):
    """The periodic Hann window (filters.hann_window_periodic, bit for bit)."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(int(n), dtype=np.float64) / int(n))


def n_ok(N):
    return MIN_N <= N <= MAX_N and N % 16 == 0


def blocks(n_out, N):
    if not n_ok(N):
        return -1
    return 0 if n_out <= 0 else -(-int(n_out) // (N // 2))


def as_f32(x):
    """Samples as the kernels see them: float32, or PCM16 scaled by 1/32768 (exact)."""
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(np.float32) * np.float32(1.0 / 32768.0)
    assert x.dtype == np.float32
    return x


def fetch(x, lo, n):
    """x[lo .. lo + n) with zeros outside the signal."""
    out = np.zeros(n, np.float32)
    a, b = max(lo, 0), min(lo + n, len(x))
    if b > a:
        out[a - lo:b - lo] = x[a:b]
    return out


def seg_ok(o0, i0, o1, i1, reach):
    """One segment of a map (csrc/warp_plan.h, warp_segment_ok); reach: one past the largest output position asked of it."""
    if not (0 <= o0 < POS_LIMIT and o1 < POS_LIMIT and reach < POS_LIMIT and -POS_LIMIT < i0 < POS_LIMIT and i1 < POS_LIMIT):
        return False
    if o1 <= o0 or i1 < i0 or reach < o1:
        return False
    return o1 - o0 < SEG_LIMIT and i1 - i0 < SEG_LIMIT and reach - o0 <= SEG_LIMIT


def map_ok(op, ip, n_out):
    """The rules of a time map (the run kernel's RTS_WARP_BAD_MAP)."""
    A = len(op)
    if A < 2 or op[0] != 0:
        return False
    return all(seg_ok(int(op[s]), int(ip[s]), int(op[s + 1]), int(ip[s + 1]),
                      max(int(op[s + 1]), int(n_out)) if s == A - 2 else int(op[s + 1])) for s in range(A - 1))


def amap(k, H, op, ip):
    """a_k: the map at output position k H, exact integers."""
    t = k * H
    s = 0
    for j in range(len(op)):
        if int(op[j]) <= t:
            s = j
    s = min(s, len(op) - 2)
    o0, i0, o1, i1 = int(op[s]), int(ip[s]), int(op[s + 1]), int(ip[s + 1])
    return i0 + ((t - o0) * (i1 - i0)) // (o1 - o0)


def corr(win, tgt, N):
    """c(delta) for every window offset: eight interleaved partial sums, q ascending, then the fixed tree."""
    cand = np.lib.stride_tricks.sliding_window_view(win, N)            # (2 D + 1, N)
    C = cand.shape[0]
    t = tgt.astype(np.float64).reshape(N // 8, 8)
    s = np.zeros((C, 8))
    for q in range(N // 8):
        s = s + cand[:, 8 * q:8 * q + 8].astype(np.float64) * t[q][None, :]   # exact products, one rounding per add
    return ((s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])) + ((s[:, 4] + s[:, 5]) + (s[:, 6] + s[:, 7]))


def pick(c, D):
    """Window offset of the first maximum in the order delta = 0, -D, .., D (strictly greater replaces)."""
    best, bv = D, c[D]
    for d in range(2 * D + 1):
        if c[d] > bv:
            bv, best = c[d], d
    return best


def warp(x, op, ip, n_out, N=1024, D=256, w=None, state=(0, 0), k_count=None):
    """Blocks state[0] .. min(state[0] + k_count, K) - 1.  Returns (y, state, info): y float32, the blocks laid end to end
    from the first one rendered, cut at n_out; the new (k, p_prev); info = {"p": positions, "ties": blocks in which the
    maximum was reached by at least two distinct candidates}."""
    x = as_f32(x)
    H = N // 2
    w = hann(N) if w is None else np.asarray(w, dtype=np.float64)
    K = blocks(n_out, N)
    k0, prev = int(state[0]), int(state[1])
    k1 = K if k_count is None else min(K, k0 + int(k_count))
    y = np.zeros(max(k1 - k0, 0) * H, np.float32)
    ps, ties = [], 0
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(k0, k1):
            a = amap(k, H, op, ip)
            if k == 0 or D == 0:
                p = a
            else:
                c = corr(fetch(x, a - D, N + 2 * D), fetch(x, prev + H, N), N)
                p = a + pick(c, D) - D
                if not np.all(np.isnan(c)) and int(np.sum(c == np.nanmax(c))) >= 2:
                    ties += 1
            f = w[:H] * fetch(x, p, H).astype(np.float64)
            if k > 0:
                e = w[H:] * fetch(x, prev + H, H).astype(np.float64)
                blk = e + f
            else:
                blk = f
            y[(k - k0) * H:(k - k0 + 1) * H] = blk.astype(np.float32)
            prev = p
            ps.append(p)
    keep = max(0, min(len(y), int(n_out) - k0 * H))
    return y[:keep], (max(k0, k1), prev), {"p": ps, "ties": ties}


def anchors(path, onto, hop, n_out, n_in, A_max):
    """The anchors rule.  path: (P, 2) integers (an empty path: P = 0).  Returns (out_pos, in_pos, status); the lists are
    empty when the status is non-zero."""
    path = np.asarray(path, dtype=np.int64).reshape(-1, 2)
    if len(path) < 1:
        return [], [], PATH_EMPTY
    u, v = path[:, onto], path[:, 1 - onto]
    st = 0
    if u[0] != 0:
        st |= PATH_START
    if v[0] < 0 or np.any(np.diff(u) < 0) or np.any(np.diff(v) < 0):
        st |= PATH_BACKWARD
    if n_out <= int(u[-1]) * hop:
        st |= PATH_SHORT_OUT
    if n_in < int(v[-1]) * hop:
        st |= PATH_SHORT_IN
    keep = [t for t in range(len(path)) if t == 0 or u[t] != u[t - 1]]
    if len(keep) + 1 > A_max:
        st |= PATH_TOO_MANY
    if st:
        return [], [], st
    return [int(u[t]) * hop for t in keep] + [int(n_out)], [int(v[t]) * hop for t in keep] + [int(n_in)], 0
