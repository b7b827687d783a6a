"""The ensemble definitions of include/rtsync.h (rts_ensemble_create) restated in plain Python, for
tests/test_ensemble_cpu.py (which holds them to closed forms and to the golden tables) and tests/test_ensemble_gpu.py
(which holds the kernels to them).  Python floats are float64 and every expression below is written in the operation order
of the definition, so `==` on its results is a bit-for-bit comparison.  Nothing here imports the package."""
import bisect
import math
import struct

import annot_model as am

NAN = struct.unpack("<d", struct.pack("<Q", 0x7ff8000000000000))[0]
INT32_MAX = 2 ** 31 - 1


def invertible(beats):
    return len(beats) >= 1 and all(beats[i] > beats[i - 1] for i in range(1, len(beats)))


def invert(x, times, beats, frame_seconds):
    """Beat x -> frame of the piece with rows (times[i], beats[i]), -1: none."""
    if x != x or not invertible(beats):
        return -1
    i = bisect.bisect_left([float(b) for b in beats], x)          # the first row with x <= beats[i]
    if i >= len(beats):
        return -1
    if x < float(beats[i]) - 1.0:
        return -1
    end = times[i]
    start = 0.0 if i == 0 else times[i - 1]
    time = end - (float(beats[i]) - x) * (end - start)
    q = time / frame_seconds + 0.5
    if q != q or q == math.inf:
        return -1
    if q < 0.0:
        return 0
    f = math.floor(q)
    return -1 if f > INT32_MAX else f


def member_beat(y_last, times, beats, frame_seconds, frame0=0):
    """The beat of a member whose last stored path point has reference index y_last (None: no path point); NaN: none.
    `times` None: the stream has no piece."""
    if y_last is None or y_last < 0 or times is None:
        return NAN
    beat = am.lookup(y_last, times, beats, frame_seconds, frame0)[0]
    return NAN if beat is None else beat


def fuse_step(betas, strikes, out, max_dev, patience):
    """One fusion step of a group.  `betas`: the members' beats in member order (NaN: none); `strikes` / `out`: lists,
    updated in place.  -> (consensus, spread, n_in, n_valid, devs)."""
    m = len(betas)
    valid = [b == b for b in betas]
    inset = [valid[i] and not out[i] for i in range(m)]
    if not any(inset):
        inset = list(valid)
    n_valid, n_in = sum(valid), sum(inset)
    if n_in == 0:
        return NAN, NAN, 0, n_valid, [NAN] * m
    v = [betas[i] for i in range(m) if inset[i]]                  # member order: a stable sort breaks ties by index
    v = sorted(v, key=_Less)
    n = len(v)
    consensus = v[(n - 1) // 2] if n % 2 else (v[n // 2 - 1] + v[n // 2]) * 0.5
    spread = v[n - 1] - v[0]
    consensus = consensus if consensus == consensus else NAN
    spread = spread if spread == spread else NAN
    devs = []
    for i in range(m):
        if not valid[i]:
            devs.append(NAN)
            continue
        d = betas[i] - consensus
        devs.append(d if d == d else NAN)
        if abs(d) > max_dev:
            strikes[i] = min(strikes[i] + 1, patience)
        else:
            strikes[i] = 0
        out[i] = 1 if strikes[i] >= patience else 0
    return consensus, spread, n_in, n_valid, devs


class _Less(object):
    """Sort key that compares with `<` on the floats alone: -0.0 and 0.0 tie, and sorted() is stable."""
    __slots__ = ("v",)

    def __init__(self, v):
        self.v = v

    def __lt__(self, other):
        return self.v < other.v


def curve(paths, groups, tables, pieces, frame0, T, frame_seconds, max_dev, patience):
    """The offline curve.  `paths`: per stream a list of (x, y) with non-decreasing x; `groups[b]` in [-1, n_groups);
    `tables[p]` = (times, beats); `pieces[b]` (outside the tables: no piece), `frame0[b]`.
    -> (consensus [G][T], spread [G][T], n_in [G][T], out [B][T])."""
    B = len(paths)
    G = max(groups) + 1
    members = [[b for b in range(B) if groups[b] == g] for g in range(G)]
    cons = [[NAN] * T for _ in range(G)]
    spread = [[NAN] * T for _ in range(G)]
    n_in = [[0] * T for _ in range(G)]
    outs = [[0] * T for _ in range(B)]
    cur = [-1] * B
    strikes, out = [0] * B, [0] * B
    cache = {}
    for t in range(T):
        for b in range(B):
            p = paths[b]
            while cur[b] + 1 < len(p) and p[cur[b] + 1][0] <= t:
                cur[b] += 1
        for g, mem in enumerate(members):
            betas = []
            for b in mem:
                y = paths[b][cur[b]][1] if cur[b] >= 0 else None
                key = (b, y)
                if key not in cache:
                    tab = tables[pieces[b]] if 0 <= pieces[b] < len(tables) else (None, None)
                    cache[key] = member_beat(y, tab[0], tab[1], frame_seconds, frame0[b])
                betas.append(cache[key])
            s, o = [strikes[b] for b in mem], [out[b] for b in mem]
            c, sp, ni, _, _ = fuse_step(betas, s, o, max_dev, patience)
            for k, b in enumerate(mem):
                strikes[b], out[b] = s[k], o[k]
                outs[b][t] = o[k]
            cons[g][t], spread[g][t], n_in[g][t] = c, sp, ni
    return cons, spread, n_in, outs
