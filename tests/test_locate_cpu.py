"""rts_locate (subsequence DTW, csrc/locate.hip) without a GPU: the entry point exists with the header's signature, its
argument checks answer before the first HIP call, and the SERIAL RESTATEMENT of its contract -- ``locate_ref`` below,
which tests/test_locate_gpu.py compares the kernel with bit for bit -- is itself pinned to the DTW oracle: the cost it
reports for a piece equals acc_cost[-1][-1] of plain DTW (oracle.binding.dtw, the restatement of the reference's dtw.py)
of the query against exactly the range it reports."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (M query frames, N piece frames): one row, one column short of it, N < M, both sides of the 64-row strip boundary,
# three strips against a piece that is no multiple of anything
SHAPES = [(1, 5), (5, 3), (17, 40), (63, 64), (64, 129), (65, 300), (130, 257)]


def dot_cost(q, ref):
    """1 - <q_i, ref_j> as one fma chain in k order, [M][N]: the oracle's own cost matrix (dtw.py:11).
    q (12, M), ref (12, N) feature-major."""
    import oracle.binding as ob
    return ob.dtw(q, ref)[0]


def euclid_cost(q, ref):
    """||q_i - ref_j||_2 cell by cell through oracle.binding's orc_euclid, [M][N]."""
    import oracle.binding as ob
    fn = ob.lib().orc_euclid
    a, b = np.ascontiguousarray(np.asarray(q, dtype=np.float64).T), np.ascontiguousarray(np.asarray(ref, dtype=np.float64).T)
    pa, pb, M, N = a.ctypes.data, b.ctypes.data, a.shape[0], b.shape[0]
    out = np.empty((M, N))
    for i in range(M):
        out[i] = [fn(pa + 96 * i, pb + 96 * j, 12) for j in range(N)]
    return out


def locate_ref(C):
    """The contract of rts_locate for one query and one piece, from their cost matrix C [M][N]:
        D[0][j] = c(0, j), S[0][j] = j;   D[i][0] = D[i-1][0] + c(i, 0), S[i][0] = S[i-1][0];
        otherwise the first minimum of (D[i][j-1] + c, D[i-1][j] + c, D[i-1][j-1] + 2c), S of the chosen predecessor;
        end = first j minimising D[M-1][j], cost = D[M-1][end], start = S[M-1][end].
    Python floats are IEEE doubles, so every sum is the float64 sum.  -> (cost, end, start, D[M-1][:], S[M-1][:])."""
    C = [[float(v) for v in r] for r in np.asarray(C, dtype=np.float64)]
    M, N = len(C), len(C[0])
    D, S = list(C[0]), list(range(N))
    for i in range(1, M):
        Ci = C[i]
        nD, nS = [D[0] + Ci[0]], [S[0]]
        for j in range(1, N):
            c = Ci[j]
            best, s = nD[j - 1] + c, nS[j - 1]
            o1 = D[j] + c
            if o1 < best:
                best, s = o1, S[j]
            o2 = D[j - 1] + 2 * c
            if o2 < best:
                best, s = o2, S[j - 1]
            nD.append(best)
            nS.append(s)
        D, S = nD, nS
    end = 0
    for j in range(1, N):
        if D[j] < D[end]:
            end = j
    return D[end], end, S[end], np.array(D), np.array(S, dtype=np.int32)


def excerpt_case():
    """The end-to-end case of the GPU file: three synthetic pieces and, as the query, frames [A, A + 64) of piece 1 with
    small noise (renormalised, float32 values).  -> (pieces, query (12, 64), A)."""
    from real_time_audio_sync_amd import synth
    pieces = [synth.synth_ref(n, seed=700 + k) for k, n in enumerate((260, 340, 300))]
    A = 117
    rs = np.random.RandomState(7)
    q = pieces[1][:, A:A + 64] + 0.03 * rs.rand(12, 64)
    q = (q / np.sqrt((q * q).sum(axis=0, keepdims=True))).astype(np.float32).astype(np.float64)
    return pieces, q, A


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as ge
    ge.build()
    from real_time_audio_sync_amd import _native
    return _native


ARGS = ["const void *queries_dev", "int q_dtype", "int M_max", "const int32_t *q_len_dev", "int B", "const void *pool_dev",
        "int pool_dtype", "int F", "long long n_pool_frames", "const long long *piece_first_dev",
        "const int32_t *piece_len_dev", "int P", "int cost_kind", "double *cost_dev", "int32_t *end_dev",
        "int32_t *start_dev", "double *row_dev", "int32_t *rowstart_dev", "void *stream"]


def test_header_declares_exports_and_binding(nat):
    txt = open(os.path.join(ROOT, "include", "rtsync.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+rts_locate\s*\(([^)]*)\)\s*;", txt)
    assert m, "include/rtsync.h does not declare rts_locate"
    assert [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")] == ARGS
    assert hasattr(ctypes.CDLL(nat.SO_PATH), "rts_locate")
    fn = nat.EXPORTS["rts_locate"]
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(ARGS)
    import real_time_audio_sync_amd as pkg
    from real_time_audio_sync_amd import _handle, locate
    assert pkg.locate_batch is locate.locate_batch and callable(_handle._BatchedHandle.locate)


def test_argument_errors_come_before_any_hip_call(nat):
    p = ctypes.c_void_p(4096)   # never dereferenced: every call below is refused on the host
    good = dict(queries_dev=p, q_dtype=nat.F32, M_max=64, q_len_dev=None, B=2, pool_dev=p, pool_dtype=nat.F32, F=12,
                n_pool_frames=100, piece_first_dev=p, piece_len_dev=p, P=3, cost_kind=nat.COST_DOT, cost_dev=p, end_dev=p,
                start_dev=p, row_dev=None, rowstart_dev=None, stream=None)
    names = [a.split()[-1].lstrip("*") for a in ARGS]
    assert names == list(good)

    def call(**kw):
        nat.lib.rts_otw_set_waves(None, 4)    # leaves another message behind
        a = dict(good, **kw)
        rc = nat.lib.rts_locate(*[a[n] for n in names])
        return rc, nat.lib.rts_last_error()

    for ptr in ("queries_dev", "pool_dev", "piece_first_dev", "piece_len_dev", "cost_dev", "end_dev", "start_dev"):
        rc, msg = call(**{ptr: None})
        assert rc == -1 and ptr.encode() in msg, (ptr, rc, msg)
    rc, msg = call(M_max=0)
    assert rc == -1 and b"M_max" in msg, (rc, msg)
    rc, msg = call(M_max=257)
    assert rc == -2 and b"M_max" in msg, (rc, msg)
    rc, msg = call(F=13)
    assert rc == -2 and b"12" in msg and b"F " in msg, (rc, msg)
    for arg, bad in (("q_dtype", 2), ("pool_dtype", 7), ("cost_kind", 2), ("P", 0), ("P", 65536), ("B", 0), ("B", 65536),
                     ("n_pool_frames", 0)):
        rc, msg = call(**{arg: bad})
        assert rc == -1 and arg.encode() in msg, (arg, rc, msg)


def test_product_does_not_import_the_oracle():
    for fn in ("locate.py", "_handle.py", "csrc/locate.hip", "csrc/cost.h", "csrc/otw_device.h", "csrc/otw_stamps.h",
               "csrc/otw_host.h"):
        src = open(os.path.join(ROOT, "real_time_audio_sync_amd", fn)).read()
        assert "import oracle" not in src and "from oracle" not in src and "liboracle" not in src, fn


def _pair(M, N, seed):
    from real_time_audio_sync_amd import synth
    ref = synth.synth_ref(N, seed=seed)
    q = synth.synth_live(synth.synth_ref(M + 8, seed=seed + 1), seed=seed + 2)[:, :M]
    assert q.shape[1] == M
    return q, ref


@pytest.mark.parametrize("M,N", SHAPES)
def test_restatement_cost_is_plain_dtw_of_the_reported_range(M, N):
    """Rounding is monotone, so the free-start DP minimises the float64 path value over the same paths plain DTW of the
    query against ref[:, start:end+1] minimises it over: the two costs are the same double."""
    import oracle.binding as ob
    q, ref = _pair(M, N, 1000 + 7 * M + N)
    cost, end, start, D, S = locate_ref(dot_cost(q, ref))
    assert 0 <= start <= end < N
    assert cost == ob.dtw(q, ref[:, start:end + 1])[1][-1, -1]
    assert cost == D.min() and end == int(np.argmin(D)) and start == S[end]
    if M == 1:
        assert start == end
    # the Euclidean cost: the same identity with the restatement run on the range's own cost matrix
    ce = euclid_cost(q, ref)
    cost, end, start, _, _ = locate_ref(ce)
    sub = ce[:, start:end + 1]
    acc = np.empty_like(sub)
    for i in range(M):
        for j in range(sub.shape[1]):
            if i == 0 and j == 0:
                acc[i, j] = sub[i, j]
            elif i == 0:
                acc[i, j] = acc[i, j - 1] + sub[i, j]
            elif j == 0:
                acc[i, j] = acc[i - 1, j] + sub[i, j]
            else:
                acc[i, j] = min(acc[i, j - 1] + sub[i, j], acc[i - 1, j] + sub[i, j], acc[i - 1, j - 1] + 2 * sub[i, j])
    assert cost == acc[-1, -1]


def test_planted_excerpt_is_found_where_it_was_planted():
    """The input of the GPU file's end-to-end test: by the restatement alone piece 1 is the cheapest and the reported
    start lies within 8 frames of where the excerpt was cut out, for both cost kinds."""
    pieces, q, A = excerpt_case()
    for cost_fn in (dot_cost, euclid_cost):
        res = [locate_ref(cost_fn(q, p))[:3] for p in pieces]
        assert min(range(3), key=lambda k: (res[k][0], k)) == 1, res
        cost, end, start = res[1]
        assert abs(start - A) <= 8 and abs(end - (A + 63)) <= 8, (start, end)
