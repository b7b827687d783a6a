// rts_otw_backward: the backward path of on-line time warping -- from a stream's current best point back
// to (0, 0) over the accumulated-cost cells the tracker has evaluated.
//
// Two device parts:
//   1. trace replay: the plain 8-wave otw_advance_kernel in its kMirrorTrace instantiation, run on the handle's scratch
//      state like the dense replay.  Where the dense flavour mirrors a cell into [2N][N], this one appends it to a log
//      with one slot per row strip (keyed by its row) and one per column strip (keyed by its column): a header
//      (first index, cells) and at most c + 1 accumulated costs, 8 bytes per evaluated cell and nothing per cell that
//      was never evaluated;
//   2. otw_backtrace_kernel, one workgroup per stream: the end cell (best_point at the clamped end position) and the
//      walk.  A cell's predecessor is the first of left, up, diagonal whose acc (+ d, + d, + 2 d) reproduces the cell's
//      own acc; d is recomputed with the tracker's cost code (otw_live_frame / otw_ref_frame / cell_cost, as
//      otw_path_cost_kernel does).  The walk is a dependent chain, so it never touches global memory: the workgroup stages
//      a (K + 1) x (K + 1) tile of the log behind the current cell in LDS together with the tile's K x K costs, one thread
//      walks until it leaves the tile (at least K steps), and the next tile is staged behind the cell it stopped at.
#pragma once
#include "otw_device.h"  // the tracker's cost code: otw_live_frame, otw_ref_frame, cell_cost
#include "otw_host.h"    // the handle, replay_source() and launch()

namespace rts {

constexpr int kBtK = 32;         // tile edge: 33 x 33 accumulated costs, 32 x 32 costs, 2 x 32 frames = 24 KB of LDS
constexpr int kBtThreads = 256;  // four waves stage a tile; thread 0 walks it

struct BacktraceArgs {
    const int32_t *state;  // [B][RTS_STATE_LEN]: the replay's final state
    const int2 *hdr;       // the log (OtwArgs::trace_hdr / trace_cells)
    const double *cells;
    int2 *tmp;             // [B][cap]: the path in walking order
    const void *ref, *live;
    const long long *ref_first;
    const int32_t *ref_len;
    long long live_stride;
    int live_f64, ref_f64, euclid, variant;
    int N, c, rows, cap;   // rows = 2 N_max, cap = 3 N_max + 8
    int32_t *path, *path_len, *end;
    double *total, *acc;   // acc: optional
};

// One stream's log.  acc[x][y] of the reference's dense matrix: the logged value where the cell was evaluated -- it then
// sits in row x's slot or in column y's -- and the matrix's initial value elsewhere.
struct BtLog {
    const int2 *hdr;
    const double *cells;
    int rows, c1;
    double sentinel;
};
__device__ __forceinline__ double bt_acc(const BtLog &g, int x, int y) {
    int2 h = g.hdr[x];
    int n = h.y < 0 ? 0 : (h.y > g.c1 ? g.c1 : h.y);
    unsigned o = (unsigned)(y - h.x);
    if (o < (unsigned)n) return g.cells[(size_t)x * g.c1 + o];
    h = g.hdr[g.rows + y];
    n = h.y < 0 ? 0 : (h.y > g.c1 ? g.c1 : h.y);
    o = (unsigned)(x - h.x);
    if (o < (unsigned)n) return g.cells[(size_t)(g.rows + y) * g.c1 + o];
    return g.sentinel;
}

// np.argmin (first minimum) of n values spread over the workgroup: thread `tid` brings the first minimum (v, i) of the
// indices it looked at (i = 0x7fffffff: none).  Result in every thread.
__device__ __forceinline__ int bt_first_argmin(double v, int i, double *red_v, int *red_i, int tid) {
    __syncthreads();
    red_v[tid] = v;
    red_i[tid] = i;
    __syncthreads();
    for (int s = kBtThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const double v2 = red_v[tid + s];
            const int i2 = red_i[tid + s];
            const bool take = i2 != 0x7fffffff && (red_i[tid] == 0x7fffffff || v2 < red_v[tid] || (v2 == red_v[tid] && i2 < red_i[tid]));
            if (take) {
                red_v[tid] = v2;
                red_i[tid] = i2;
            }
        }
        __syncthreads();
    }
    return red_i[0];
}

__global__ void __launch_bounds__(kBtThreads) otw_backtrace_kernel(BacktraceArgs a) {
    constexpr int K = kBtK;
    __shared__ double A[K + 1][K + 2];  // acc at (x0 + i, y0 + j): the tile and, at i = 0 / j = 0, the cells it leaves through
    __shared__ double Dt[K][K + 1];     // cost at (x0 + 1 + i, y0 + 1 + j)
    __shared__ double lfs[K][kF], rfs[K][kF];
    __shared__ double red_v[kBtThreads];
    __shared__ int red_i[kBtThreads];
    __shared__ int s_x, s_y, s_n, s_done;
    const int b = blockIdx.x, tid = threadIdx.x;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    const int32_t *st = a.state + (size_t)b * RTS_STATE_LEN;
    const int Nb = a.ref_len ? a.ref_len[b] : a.N;
    int2 *tmp = a.tmp + (size_t)b * a.cap;
    if (st[RTS_ST_FIRST_INSERT] || st[RTS_ST_CONSUMED] < 1) {  // no frame consumed
        if (tid == 0) {
            a.path_len[b] = 0;
            a.total[b] = qnan;
            a.end[2 * b] = -1;
            a.end[2 * b + 1] = -1;
        }
        return;
    }
    BtLog g;
    g.hdr = a.hdr + (size_t)b * 3 * (a.rows / 2);
    g.cells = a.cells + (size_t)b * 3 * (a.rows / 2) * (size_t)(a.c + 1);
    g.rows = a.rows;
    g.c1 = a.c + 1;
    g.sentinel = (a.variant == RTS_VARIANT_OTW) ? 1e10 : (double)INFINITY;
    OtwEnv e;
    e.live = a.live;
    e.live_f64 = a.live_f64;
    e.live_base = (long long)b * a.live_stride * kF;
    e.ref_f64 = a.ref_f64;
    e.ref = a.ref_first ? static_cast<const char *>(a.ref) + a.ref_first[b] * (long long)kF * (a.ref_f64 ? 8 : 4) : a.ref;

    // end position: a stop or an overflow leaves one index one past the end (and t keeps counting on overflow)
    int rows_used = st[RTS_ST_CONSUMED];
    if (rows_used > 2 * Nb) rows_used = 2 * Nb;
    if ((long long)rows_used > a.live_stride) rows_used = (int)a.live_stride;
    int te = st[RTS_ST_T], je = st[RTS_ST_J];
    te = te > rows_used - 1 ? rows_used - 1 : te;
    je = je > Nb - 1 ? Nb - 1 : je;
    te = te < 0 ? 0 : te;
    je = je < 0 ? 0 : je;
    // best_point (otw_eran.py:192-211) on the log: row te over columns [j1, je], column je over rows [t1, te]
    const int c = a.c;
    const int j1 = (je - c + 1 > 0) ? je - c + 1 : 0, t1 = (te - c + 1 > 0) ? te - c + 1 : 0;
    double bv = 0.0;
    int bi = 0x7fffffff;
    for (int i = tid; i <= je - j1; i += kBtThreads) {
        const double v = bt_acc(g, te, j1 + i);
        if (bi == 0x7fffffff || v < bv) bv = v, bi = i;
    }
    const int ridx = bt_first_argmin(bv, bi, red_v, red_i, tid);
    const double rmin = red_v[0];
    bi = 0x7fffffff;
    for (int i = tid; i <= te - t1; i += kBtThreads) {
        const double v = bt_acc(g, t1 + i, je);
        if (bi == 0x7fffffff || v < bv) bv = v, bi = i;
    }
    const int cidx = bt_first_argmin(bv, bi, red_v, red_i, tid);
    const double cmin = red_v[0];
    const int ex = (rmin < cmin) ? te : t1 + cidx, ey = (rmin < cmin) ? j1 + ridx : je;
    if (tid == 0) {
        s_x = ex;
        s_y = ey;
        s_n = 0;
        s_done = 0;
    }
    for (;;) {
        __syncthreads();
        if (s_done) break;
        const int x0 = s_x - K, y0 = s_y - K;
        if (tid < K) {
            const int gx = x0 + 1 + tid;
            if (gx >= 0) {
                double f[kF];
                otw_live_frame(e, gx, f);
#pragma unroll
                for (int q = 0; q < kF; q++) lfs[tid][q] = f[q];
            }
        } else if (tid < 2 * K) {
            const int gy = y0 + 1 + (tid - K);
            if (gy >= 0) {
                double f[kF];
                otw_ref_frame(e, gy, f);
#pragma unroll
                for (int q = 0; q < kF; q++) rfs[tid - K][q] = f[q];
            }
        }
        for (int idx = tid; idx < (K + 1) * (K + 1); idx += kBtThreads) {
            const int i = idx / (K + 1), j = idx % (K + 1);
            const int gx = x0 + i, gy = y0 + j;
            A[i][j] = (gx < 0 || gy < 0) ? qnan : bt_acc(g, gx, gy);  // outside the matrix: matches nothing
        }
        __syncthreads();
        for (int idx = tid; idx < K * K; idx += kBtThreads) {
            const int i = idx / K, j = idx % K;
            if (x0 + 1 + i >= 0 && y0 + 1 + j >= 0) {
                double lf[kF], rf[kF];
#pragma unroll
                for (int q = 0; q < kF; q++) {
                    lf[q] = lfs[i][q];
                    rf[q] = rfs[j][q];
                }
                Dt[i][j] = cell_cost(lf, rf, a.euclid);
            }
        }
        __syncthreads();
        if (tid == 0) {
            int i = K, j = K, n = s_n, done = 0;
            for (;;) {
                const int gx = x0 + i, gy = y0 + j;
                if (n >= a.cap) {  // cannot happen (a path has at most 3 N_b - 1 points); keeps a broken log in bounds
                    done = 1;
                    break;
                }
                tmp[n] = make_int2(gx, gy);
                n += 1;
                if (gx == 0 && gy == 0) {
                    done = 1;
                    break;
                }
                const double acc = A[i][j], d = Dt[i - 1][j - 1];
                const bool hl = gy > 0, hu = gx > 0;
                int mv;  // 0 left, 1 up, 2 diagonal: the candidate order of eval_path_cost (otw_eran.py:228-234)
                if (hl && A[i][j - 1] + d == acc) mv = 0;
                else if (hu && A[i - 1][j] + d == acc) mv = 1;
                else if (hl && hu && A[i - 1][j - 1] + 2 * d == acc) mv = 2;
                else mv = (hl && hu) ? 2 : (hl ? 0 : 1);  // NaN features only: any step towards (0, 0)
                i -= (mv != 0);
                j -= (mv != 1);
                if (i == 0 || j == 0) break;  // left the tile: the next one is staged behind this cell
            }
            s_x = x0 + i;
            s_y = y0 + j;
            s_n = n;
            s_done = done;
        }
    }
    const int n = s_n;
    for (int k = tid; k < n; k += kBtThreads) {  // forward order
        const int2 p = tmp[n - 1 - k];
        reinterpret_cast<int2 *>(a.path)[(size_t)b * a.cap + k] = p;
        if (a.acc) a.acc[(size_t)b * a.cap + k] = bt_acc(g, p.x, p.y);
    }
    if (tid == 0) {
        a.path_len[b] = n;
        a.total[b] = bt_acc(g, ex, ey);
        a.end[2 * b] = ex;
        a.end[2 * b + 1] = ey;
    }
}

// Workspace layout: [64-byte header, unused][headers: B * 3 N_max int2][cells: B * 3 N_max * (c + 1) double]
// [walk order: B * (3 N_max + 8) int2], every part 16-byte aligned.  Linear in N_max.
struct BackwardLayout {
    size_t hdr_off, hdr_bytes, cells_off, tmp_off, total;
};
static bool backward_layout(int N_max, int c, int B, BackwardLayout *l) {
    size_t slots, cells, tmp;
    if (__builtin_mul_overflow((size_t)B, (size_t)3 * (size_t)N_max, &slots)) return false;
    if (__builtin_mul_overflow(slots, (size_t)8 * ((size_t)c + 1), &cells)) return false;
    if (__builtin_mul_overflow((size_t)B, ((size_t)3 * (size_t)N_max + 8) * 8, &tmp)) return false;
    if (slots > ((size_t)1 << 59)) return false;
    l->hdr_off = 64;
    l->hdr_bytes = (slots * 8 + 15) & ~(size_t)15;
    l->cells_off = l->hdr_off + l->hdr_bytes;
    size_t end;
    if (__builtin_add_overflow(l->cells_off, (cells + 15) & ~(size_t)15, &end)) return false;
    l->tmp_off = end;
    if (__builtin_add_overflow(end, (tmp + 15) & ~(size_t)15, &end)) return false;
    l->total = end;
    return true;
}

}  // namespace rts

extern "C" {

int rts_otw_backward_workspace_bytes(int N_max, int c, int B, size_t *bytes) {
    using namespace rts;
    if (!bytes) return set_error(RTS_ERR_INVALID, "bytes is NULL");
    if (N_max < 1) return set_error(RTS_ERR_INVALID, "N_max must be >= 1 (got %d)", N_max);
    if (c < 1) return set_error(RTS_ERR_INVALID, "c must be >= 1 (got %d)", c);
    if (B < 1) return set_error(RTS_ERR_INVALID, "B must be >= 1 (got %d)", B);
    if ((long long)N_max * 3 + 8 > 0x3fffffffLL) return set_error(RTS_ERR_INVALID, "N_max too large");
    BackwardLayout l;
    if (!backward_layout(N_max, c, B, &l)) return set_error(RTS_ERR_INVALID, "N_max * c * B overflows size_t");
    *bytes = l.total;
    return RTS_OK;
}

int rts_otw_backward(rts_otw *h, const void *live_dev, int live_dtype, int T_max, const int32_t *live_len_dev,
                     int32_t *path_dev, int32_t *path_len_dev, double *total_dev, int32_t *end_dev, double *acc_dev,
                     void *ws_dev, size_t ws_bytes, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!path_dev) return set_error(RTS_ERR_INVALID, "path_dev is NULL");
    if (!path_len_dev) return set_error(RTS_ERR_INVALID, "path_len_dev is NULL");
    if (!total_dev) return set_error(RTS_ERR_INVALID, "total_dev is NULL");
    if (!end_dev) return set_error(RTS_ERR_INVALID, "end_dev is NULL");
    if (!ws_dev) return set_error(RTS_ERR_INVALID, "ws_dev is NULL");
    if ((uintptr_t)ws_dev & 15) return set_error(RTS_ERR_INVALID, "ws_dev must be 16-byte aligned");
    if ((uintptr_t)path_dev & 7) return set_error(RTS_ERR_INVALID, "path_dev must be 8-byte aligned");
    BackwardLayout l;
    if (!backward_layout(h->N, h->c, h->B, &l)) return set_error(RTS_ERR_INVALID, "N_max * c * B overflows size_t");
    if (ws_bytes < l.total)
        return set_error(RTS_ERR_INVALID, "ws_bytes = %zu is less than rts_otw_backward_workspace_bytes = %zu", ws_bytes, l.total);
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    OtwArgs a;
    if (int rc = replay_source(h, live_dev, live_dtype, T_max, live_len_dev, s, &a); rc != RTS_OK) return rc;
    if (!h->bw_ev[0]) {
        for (int i = 0; i < 3; i++) RTS_HIP(hipEventCreate(&h->bw_ev[i]));
    }
    char *ws = static_cast<char *>(ws_dev);
    RTS_HIP(hipEventRecord(h->bw_ev[0], s));  // (behind the reset of the scratch state: B threads)
    RTS_HIP(hipMemsetAsync(ws + l.hdr_off, 0, l.hdr_bytes, s));  // every slot: no cells
    a.trace_hdr = reinterpret_cast<int2 *>(ws + l.hdr_off);
    a.trace_cells = reinterpret_cast<double *>(ws + l.cells_off);
    a.trace_rows = 2 * h->N;
    if (h->src_kind != 0) {  // (a fresh handle has consumed nothing: the scratch state says so to the kernel below)
        if (int rc = launch(h, a, s, 0); rc != RTS_OK) return rc;
    }
    RTS_HIP(hipEventRecord(h->bw_ev[1], s));
    BacktraceArgs g;
    g.state = h->rp_state;
    g.hdr = a.trace_hdr;
    g.cells = a.trace_cells;
    g.tmp = reinterpret_cast<int2 *>(ws + l.tmp_off);
    g.ref = h->ref;
    g.live = a.live;
    g.ref_first = h->refs.first;
    g.ref_len = h->refs.len;
    g.live_stride = a.live_stride;
    g.live_f64 = a.live_f64;
    g.ref_f64 = a.ref_f64;
    g.euclid = h->cost_kind == RTS_COST_EUCLID;
    g.variant = h->variant;
    g.N = h->N;
    g.c = h->c;
    g.rows = 2 * h->N;
    g.cap = h->path_cap;
    g.path = path_dev;
    g.path_len = path_len_dev;
    g.end = end_dev;
    g.total = total_dev;
    g.acc = acc_dev;
    hipLaunchKernelGGL(otw_backtrace_kernel, dim3(h->B), dim3(kBtThreads), 0, s, g);
    RTS_HIP(hipGetLastError());
    RTS_HIP(hipEventRecord(h->bw_ev[2], s));
    return RTS_OK;
}

int rts_otw_backward_times(rts_otw *h, float *replay_ms, float *backtrace_ms) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!replay_ms || !backtrace_ms) return set_error(RTS_ERR_INVALID, "replay_ms / backtrace_ms is NULL");
    if (!h->bw_ev[0]) return set_error(RTS_ERR_INVALID, "rts_otw_backward has not been called on this handle");
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    RTS_HIP(hipEventSynchronize(h->bw_ev[2]));
    RTS_HIP(hipEventElapsedTime(replay_ms, h->bw_ev[0], h->bw_ev[1]));
    RTS_HIP(hipEventElapsedTime(backtrace_ms, h->bw_ev[1], h->bw_ev[2]));
    return RTS_OK;
}

}  // extern "C"
