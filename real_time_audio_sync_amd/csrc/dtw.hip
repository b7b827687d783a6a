// Offline DTW for gfx950: dtw.DTW(seq_a, seq_b) -> (cost, acc_cost, path)   (/root/reference/dtw.py:5-53)
//
//   dtw_cost_kernel       cost[i][j] = 1 - <a_i, b_j>  (K = 12: far too thin for MFMA to matter; one fma
//                         chain per element in dgemm's k-order, coalesced stores), whole chip.
//   dtw_sdp_kernel        the accumulated-cost recurrence as a strip DP (sdp.h): a wave owns 64 rows, its
//                         lanes are skewed in time and exchange predecessors by DPP; the waves of a
//                         workgroup and the workgroups of a launch form one pipeline down the matrix, so a
//                         single long pair spreads over many CUs and a batch of short pairs fills the chip.
//                         Every cell does the reference's three float64 adds and first-minimum argmin
//                         (dtw.py:35-40): acc_cost is bit-identical to the serial double loop.
//   dtw_hops_kernel /     dtw.py:43-52 over the packed step codes: the columns at which the path crosses the strip
//   dtw_segment_kernel    boundaries (one dependent load per strip), then every strip's segment walked by its own wave.
//   dtw_back_decode_kernel optional: the reference's `back` matrix as int8 [M][N].
//
// rts_dtw_paths is the same pipeline without the dense outputs: no dtw_cost_kernel, the strip DP without staging
// (nothing but step codes, boundary rows and entry columns leaves the chip), and every pair with lengths of its own
// (pair_dims) inside a workspace slice sized by the call's maxima.
//
// rts_dtw_subseq_paths is rts_dtw_paths with both ends of b free (sdp::DtwSubseqPolicy): dtw_subseq_sdp_kernel frees the
// first row and parks the last one in the workspace, the backtrack (the FREE instantiations of dtw_hops_kernel / dtw_segment_kernel, or of
// dtw_tail_kernel) starts at that row's first minimum and stops on row 0.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "common.h"
#include "sdp.h"

namespace rts {

constexpr int kDtwF = 12;

struct DtwArgs {
    const void *a;  // [B][M][F] (a_stride frames between pairs; 0 = shared)
    const void *b;  // [B][N][F]
    double *cost;   // [B][M][N]
    double *acc;    // [B][M][N]
    int8_t *back;   // [B][M][N] or NULL
    int32_t *path;  // [B][M+N][2]
    int32_t *path_len;  // [B]
    long long a_stride, b_stride;
    int M, N, a_f64, b_f64;
    uint32_t *codes;           // [B][codes_words]
    unsigned long long *bnd;   // [B][n_strips][N]
    int32_t *entb;             // [B][n_strips][N]
    int32_t *cross, *lens;     // [B][n_strips]
    int32_t *pscr;             // [B][scratch_pairs(M, N)][2] path segments as walked (sdp::path_segment)
    double *yrec;              // [B][N][14] prepared column records
    int32_t *err;
    int32_t *ticket;           // [B] next row group of each pair (sdp::for_each_rowgroup)
    int n_rg, n_strips_wg;
    // rts_dtw_paths only (NULL in rts_dtw): M and N above are then the maxima that size every pair's slices
    const int32_t *a_len, *b_len;  // [B] the pairs' own lengths (NULL = the maximum)
    double *total;                 // [B] acc_cost[M_k-1][N_k-1]
    // rts_dtw_subseq_paths only: total is D[M_k-1][end]
    int32_t *start, *end;          // [B] columns of the path's first and last point
    double *row;                   // [B][N] D[M_k-1][:] or NULL
};

// The pair's own M and N: the maximum without a length table, and never more than it.  Everything a pair keeps in the
// workspace is indexed with its own N inside its slice (the DP and the backtrack both get it from here).
__device__ __forceinline__ void pair_dims(const DtwArgs &g, int pair, int &M, int &N) {
    M = g.M;
    N = g.N;
    if (g.a_len) M = min(g.a_len[pair], g.M);
    if (g.b_len) N = min(g.b_len[pair], g.N);
}

// What path_len / total say beyond the path itself: the fault contract, and a pair without cells.  One thread, after
// the pair's backtrack.
__device__ __forceinline__ void dtw_report(const DtwArgs &g, int pair, bool has_cells) {
    if (*g.err != 0) {
        g.path_len[pair] = -1;
        if (g.total) g.total[pair] = __longlong_as_double(0x7ff8000000000000LL);  // NaN
    } else if (!has_cells) {
        g.path_len[pair] = 0;
        if (g.total) g.total[pair] = __longlong_as_double(0x7ff0000000000000LL);  // +inf
    }
}

// The same for rts_dtw_subseq_paths, which also reports start and end.
__device__ __forceinline__ void dtw_subseq_report(const DtwArgs &g, int pair, bool has_cells) {
    dtw_report(g, pair, has_cells);
    if (*g.err != 0 || !has_cells) {
        g.start[pair] = -1;
        g.end[pair] = -1;
    }
}

// Where pair `pair` (M x N, its own lengths) keeps its last row and where its free-ended backtrack reports.
__device__ __forceinline__ sdp::FreeEnds dtw_free_ends(const DtwArgs &g, int pair, int M, int N) {
    const int last_rg = (sdp::n_strips(M) + g.n_strips_wg - 1) / g.n_strips_wg - 1;
    sdp::FreeEnds fe;
    fe.row = g.bnd + (size_t)pair * sdp::n_strips(g.M) * g.N + (size_t)last_rg * N;
    fe.total = g.total + pair;
    fe.start = g.start + pair;
    fe.end = g.end + pair;
    fe.row_out = g.row ? g.row + (size_t)pair * g.N : nullptr;
    return fe;
}

// One thread per column j and kCostRows consecutive rows: b_j stays in registers, the a rows are wave-uniform
// (broadcast) loads, every store instruction writes 512 contiguous bytes of one row.
constexpr int kCostRows = 32;

template <bool A64, bool B64>
__global__ void __launch_bounds__(256) dtw_cost_kernel(DtwArgs g) {
    const int pair = blockIdx.z;
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i0 = blockIdx.y * kCostRows;
    if (j >= g.N) return;
    double b[kDtwF];
    sdp::load_frame(g.b, B64, (long long)pair * g.b_stride + j, b);
    double *out = g.cost + ((size_t)pair * g.M + i0) * g.N + j;
    const int rows = (g.M - i0 < kCostRows) ? g.M - i0 : kCostRows;
    for (int r = 0; r < rows; r++) {
        double a[kDtwF];
        sdp::load_frame(g.a, A64, (long long)pair * g.a_stride + i0 + r, a);
        double s = 0.0;
#pragma unroll
        for (int f = 0; f < kDtwF; f++) s = fma(a[f], b[f], s);
        out[(size_t)r * g.N] = 1.0 - s;
    }
}

__global__ void __launch_bounds__(256) dtw_prep_kernel(DtwArgs g) {
    const int pair = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    int M, N;
    pair_dims(g, pair, M, N);
    if (j >= N || M < 1) return;
    const void *b = g.b_f64 ? (const void *)(reinterpret_cast<const double *>(g.b) + (long long)pair * g.b_stride * kDtwF)
                            : (const void *)(reinterpret_cast<const float *>(g.b) + (long long)pair * g.b_stride * kDtwF);
    sdp::prep_column<sdp::DtwPolicy>(b, g.b_f64, j, g.yrec + (size_t)pair * g.N * sdp::kYRec);
}

// H helper waves per strip.  <2>: two strips per workgroup (6 waves); <3>: one strip per workgroup (4 waves, the DP wave
// has a SIMD to itself) -- see sdp::pick_config.  STAGE: acc_cost goes to HBM (rts_dtw); without it (rts_dtw_paths) the
// pair has its own lengths and row-group count, and its final cost goes to total[pair].
template <int H, bool STAGE>
__global__ void __launch_bounds__(H == 2 ? 384 : 256) dtw_sdp_kernel(DtwArgs g) {
    extern __shared__ __align__(16) unsigned char dtw_smem[];
    const int pair = blockIdx.y;
    // rts_dtw: every pair is M x N.  rts_dtw_paths: the pair's own lengths and, from them, its own row-group count
    // -- the grid is sized for the longest pair, and the workgroups beyond a shorter one's row groups leave at their
    // first ticket.
    int M = g.M, N = g.N, n_rg = g.n_rg;
    if constexpr (!STAGE) {
        pair_dims(g, pair, M, N);
        if (M < 1 || N < 1) return;  // the whole workgroup: nothing of such a pair is read
        n_rg = (sdp::n_strips(M) + g.n_strips_wg - 1) / g.n_strips_wg;
    }
    sdp::Problem pb;
    pb.x = g.a_f64 ? (const void *)(reinterpret_cast<const double *>(g.a) + (long long)pair * g.a_stride * kDtwF)
                   : (const void *)(reinterpret_cast<const float *>(g.a) + (long long)pair * g.a_stride * kDtwF);
    pb.x_f64 = g.a_f64;
    pb.yrec = g.yrec + (size_t)pair * g.N * sdp::kYRec;
    pb.M = M;
    pb.N = N;
    pb.D = STAGE ? g.acc + (size_t)pair * g.M * g.N : nullptr;
    pb.ldD = g.N;
    pb.codes = g.codes + (size_t)pair * sdp::codes_words(g.M, g.N);
    pb.bnd = g.bnd + (size_t)pair * sdp::n_strips(g.M) * g.N;
    pb.entb = g.entb + (size_t)pair * sdp::n_strips(g.M) * g.N;
    pb.err = g.err;
    pb.last = STAGE ? nullptr : g.total + pair;
    sdp::for_each_rowgroup(g.ticket + pair, n_rg, g.n_strips_wg, dtw_smem, [&](int rg) {
        sdp::run_rowgroup<sdp::DtwPolicy, STAGE, H>(pb, rg, n_rg, g.n_strips_wg, dtw_smem);
    });
}

// The strip DP of rts_dtw_subseq_paths: dtw_sdp_kernel<H, false> with the first row freed and the last row kept
// (sdp::DtwSubseqPolicy) instead of the last cell.  A kernel of its own, so that the instantiations above stay the code
// they were.
template <int H>
__global__ void __launch_bounds__(H == 2 ? 384 : 256) dtw_subseq_sdp_kernel(DtwArgs g) {
    extern __shared__ __align__(16) unsigned char dtw_smem[];
    const int pair = blockIdx.y;
    int M, N;
    pair_dims(g, pair, M, N);
    if (M < 1 || N < 1) return;  // the whole workgroup: nothing of such a pair is read
    const int n_rg = (sdp::n_strips(M) + g.n_strips_wg - 1) / g.n_strips_wg;
    sdp::Problem pb;
    pb.x = g.a_f64 ? (const void *)(reinterpret_cast<const double *>(g.a) + (long long)pair * g.a_stride * kDtwF)
                   : (const void *)(reinterpret_cast<const float *>(g.a) + (long long)pair * g.a_stride * kDtwF);
    pb.x_f64 = g.a_f64;
    pb.yrec = g.yrec + (size_t)pair * g.N * sdp::kYRec;
    pb.M = M;
    pb.N = N;
    pb.D = nullptr;
    pb.ldD = g.N;
    pb.codes = g.codes + (size_t)pair * sdp::codes_words(g.M, g.N);
    pb.bnd = g.bnd + (size_t)pair * sdp::n_strips(g.M) * g.N;  // slot n_rg - 1 receives the last row (dtw_free_ends)
    pb.entb = g.entb + (size_t)pair * sdp::n_strips(g.M) * g.N;
    pb.err = g.err;
    pb.last = nullptr;
    sdp::for_each_rowgroup(g.ticket + pair, n_rg, g.n_strips_wg, dtw_smem, [&](int rg) {
        sdp::run_rowgroup<sdp::DtwSubseqPolicy, false, H>(pb, rg, n_rg, g.n_strips_wg, dtw_smem);
    });
}

// The backtrack kernels.  FREE: the ends of b are free (rts_dtw_subseq_paths, sdp::FreeEnds): the hops begin at the
// first minimum of the last row, strip 0's walk stops on row 0, and start / end are reported too.
template <bool FREE>
__global__ void __launch_bounds__(64) dtw_hops_kernel(DtwArgs g) {
    __shared__ uint32_t win[2 * sdp::kBtChunks * 64];
    const int pair = blockIdx.x, S = sdp::n_strips(g.M);
    int M, N;
    pair_dims(g, pair, M, N);
    if (M < 1 || N < 1) return;
    sdp::FreeEnds fe;
    if constexpr (FREE) fe = dtw_free_ends(g, pair, M, N);
    sdp::path_hops<FREE>(g.codes + (size_t)pair * sdp::codes_words(g.M, g.N), g.entb + (size_t)pair * S * g.N, M, N,
                         g.cross + (size_t)pair * S, win, FREE ? &fe : nullptr);
}

template <int PASS, bool FREE>
__global__ void __launch_bounds__(64) dtw_segment_kernel(DtwArgs g) {
    __shared__ uint32_t win[2 * sdp::kBtChunks * 64];
    const int pair = blockIdx.y, s = blockIdx.x, S = sdp::n_strips(g.M);
    int32_t *path = g.path + (size_t)pair * (g.M + g.N) * 2;
    int M, N;
    pair_dims(g, pair, M, N);
    const bool has_cells = (M >= 1 && N >= 1);
    // the grid has a workgroup per strip of the longest pair: the ones beyond this pair's strips touch nothing
    if (has_cells && s < sdp::n_strips(M)) {
        sdp::FreeEnds fe;
        if constexpr (FREE) fe = dtw_free_ends(g, pair, M, N);
        sdp::path_segment<FREE>(g.codes + (size_t)pair * sdp::codes_words(g.M, g.N), M, N, s, g.cross + (size_t)pair * S,
                                g.lens + (size_t)pair * S, PASS, path, g.path_len + pair, win,
                                g.pscr + (size_t)pair * 2 * sdp::scratch_pairs(g.M, g.N), FREE ? &fe : nullptr);
    }
    if (PASS == 1 && s == 0 && threadIdx.x == 0) {
        if constexpr (FREE)
            dtw_subseq_report(g, pair, has_cells);
        else
            dtw_report(g, pair, has_cells);
    }
}

// hops + both segment passes of a short pair in one launch (at most sdp::kTailStrips strips: one wave each)
template <bool FREE>
__global__ void __launch_bounds__(64 * sdp::kTailStrips) dtw_tail_kernel(DtwArgs g) {
    extern __shared__ __align__(16) unsigned char dtw_smem[];
    const int pair = blockIdx.x, S = sdp::n_strips(g.M);
    int M, N;
    pair_dims(g, pair, M, N);
    const bool has_cells = (M >= 1 && N >= 1);  // uniform over the workgroup
    // one wave per strip of the longest pair: the waves beyond this pair's strips go through path_tail's barriers and
    // write nothing
    if (has_cells) {
        sdp::FreeEnds fe;
        if constexpr (FREE) fe = dtw_free_ends(g, pair, M, N);
        sdp::path_tail<FREE>(g.codes + (size_t)pair * sdp::codes_words(g.M, g.N), g.entb + (size_t)pair * S * g.N, M, N,
                             g.cross + (size_t)pair * S, g.lens + (size_t)pair * S,
                             g.path + (size_t)pair * (g.M + g.N) * 2, g.path_len + pair,
                             reinterpret_cast<uint32_t *>(dtw_smem),
                             g.pscr + (size_t)pair * 2 * sdp::scratch_pairs(g.M, g.N), FREE ? &fe : nullptr);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if constexpr (FREE)
            dtw_subseq_report(g, pair, has_cells);
        else
            dtw_report(g, pair, has_cells);
    }
}

__global__ void __launch_bounds__(256) dtw_back_decode_kernel(DtwArgs g) {
    const int pair = blockIdx.z, i = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= g.N) return;
    const uint32_t *codes = g.codes + (size_t)pair * sdp::codes_words(g.M, g.N);
    const int l = i & 63, t = j + l;
    const uint32_t w = codes[((size_t)(i >> 6) * sdp::n_chunks(g.N) + (t >> 4)) * 64 + l];
    g.back[((size_t)pair * g.M + i) * g.N + j] = (int8_t)((w >> (2 * (t & 15))) & 3);
}

// The one size function behind rts_dtw_workspace_bytes, rts_dtw_paths_workspace_bytes and
// rts_dtw_subseq_paths_workspace_bytes: the sections are sdp_plan.h's table, which dtw_enqueue carves.
static int dtw_workspace(int M, int N, int B, size_t *bytes, const char *m_name, const char *n_name) {
    if (!bytes) return set_error(RTS_ERR_INVALID, "bytes is NULL");
    if (M < 1 || N < 1 || B < 1) return set_error(RTS_ERR_INVALID, "%s, %s, B must be >= 1", m_name, n_name);
    *bytes = sdp::workspace_bytes(M, N, B);
    return RTS_OK;
}

// The argument checks the three calls share (M, N: the call's maxima), workspace and the alignment of path_dev
// included: `ws_fn` is the name of the caller's own rts_*_workspace_bytes, for the message.
static int dtw_check(int a_dtype, int b_dtype, int F, int M, int N, int B, const void *path_dev, const void *ws_dev,
                     size_t ws_bytes, const char *m_name, const char *n_name, const char *ws_fn) {
    if (F != kDtwF) return set_error(RTS_ERR_UNSUPPORTED, "F must be 12 chroma bins (got %d)", F);
    if (M < 1 || N < 1 || B < 1)
        return set_error(RTS_ERR_INVALID, "%s, %s, B must be >= 1 (got %d %d %d)", m_name, n_name, M, N, B);
    if (!dtype_ok(a_dtype) || !dtype_ok(b_dtype)) return set_error(RTS_ERR_INVALID, "bad dtype");
    if ((long long)M * N > 0x7fffffffLL * 4) return set_error(RTS_ERR_INVALID, "%s*%s too large", m_name, n_name);
    if (B > 65535) return set_error(RTS_ERR_INVALID, "at most 65535 pairs per call");
    const size_t need = sdp::workspace_bytes(M, N, B);
    if (ws_bytes < need)
        return set_error(RTS_ERR_INVALID, "workspace of %zu bytes is smaller than %s = %zu", ws_bytes, ws_fn, need);
    if (((uintptr_t)ws_dev & 15) != 0) return set_error(RTS_ERR_INVALID, "workspace must be 16-byte aligned");
    // sdp::path_segment copies a segment to its place as (i, j) pairs, one 8-byte store each
    if (((uintptr_t)path_dev & 7) != 0) return set_error(RTS_ERR_INVALID, "path_dev must be 8-byte aligned");
    return RTS_OK;
}

// The caller's buffers, sizes and dtypes as the kernels get them (the workspace fields: dtw_enqueue).  rts_dtw has no
// length tables and no total / start / end / row; the path-only calls have no cost / acc / back.
static DtwArgs dtw_args(const void *a_dev, int a_dtype, long long a_stride, const int32_t *a_len_dev, const void *b_dev,
                        int b_dtype, long long b_stride, const int32_t *b_len_dev, int M, int N, double *cost_dev,
                        double *acc_dev, int8_t *back_dev, int32_t *path_dev, int32_t *path_len_dev, double *total_dev,
                        int32_t *start_dev, int32_t *end_dev, double *row_dev) {
    DtwArgs g;
    g.a = a_dev;
    g.b = b_dev;
    g.cost = cost_dev;
    g.acc = acc_dev;
    g.back = back_dev;
    g.path = path_dev;
    g.path_len = path_len_dev;
    g.a_stride = a_stride;
    g.b_stride = b_stride;
    g.M = M;
    g.N = N;
    g.a_f64 = a_dtype == RTS_F64;
    g.b_f64 = b_dtype == RTS_F64;
    g.a_len = a_len_dev;
    g.b_len = b_len_dev;
    g.total = total_dev;
    g.start = start_dev;
    g.end = end_dev;
    g.row = row_dev;
    return g;
}

// Carves the workspace and enqueues the pipeline; `g` arrives with the caller's buffers, sizes and dtypes filled in.
// DENSE: rts_dtw (cost and acc_cost are written); otherwise rts_dtw_paths or, with SUBSEQ, rts_dtw_subseq_paths.
template <bool DENSE, bool SUBSEQ = false>
static int dtw_enqueue(DtwArgs g, int B, void *ws_dev, hipStream_t s) {
    static_assert(!(DENSE && SUBSEQ), "the subsequence form has no dense outputs");
    // one strip per workgroup / two (sdp::pick_config); their residency is asked once per device and LDS padding
    void (*const k_sdp1)(DtwArgs) = SUBSEQ ? &dtw_subseq_sdp_kernel<3> : &dtw_sdp_kernel<3, DENSE>;
    void (*const k_sdp2)(DtwArgs) = SUBSEQ ? &dtw_subseq_sdp_kernel<2> : &dtw_sdp_kernel<2, DENSE>;
    static int residency[sdp::kResidencyDevices][3];
    const int M = g.M, N = g.N, strips = sdp::n_strips(M);
    sdp::Plan plan;
    void (*k_sdp)(DtwArgs);
    if (int rc = sdp::launch_plan(k_sdp1, k_sdp2, strips, B, residency, &plan, &k_sdp); rc != RTS_OK) return rc;
    const sdp::WorkspaceLayout ws = sdp::workspace_carve(ws_dev, M, N, B, &g, &g.pscr);
    g.n_rg = plan.n_rg;
    g.n_strips_wg = plan.NS;
    RTS_HIP(hipMemsetAsync(g.err, 0, 16, s));
    RTS_HIP(hipMemsetAsync(g.ticket, 0, sizeof(int32_t) * (size_t)B, s));
    // (n_rg is the longest pair's: with per-pair lengths, whenever any pair can have more than one row group)
    if (plan.n_rg > 1) RTS_HIP(hipMemsetD32Async((hipDeviceptr_t)g.bnd, (int)sdp::kSentinel32, ws.len[sdp::kBnd] / 4, s));
    if (DENSE) {
        const dim3 grid((N + 255) / 256, (M + kCostRows - 1) / kCostRows, B);
        if (g.a_f64 && g.b_f64)
            hipLaunchKernelGGL((dtw_cost_kernel<true, true>), grid, dim3(256), 0, s, g);
        else if (g.a_f64)
            hipLaunchKernelGGL((dtw_cost_kernel<true, false>), grid, dim3(256), 0, s, g);
        else if (g.b_f64)
            hipLaunchKernelGGL((dtw_cost_kernel<false, true>), grid, dim3(256), 0, s, g);
        else
            hipLaunchKernelGGL((dtw_cost_kernel<false, false>), grid, dim3(256), 0, s, g);
        RTS_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(dtw_prep_kernel, dim3((N + 255) / 256, B), dim3(256), 0, s, g);
    hipLaunchKernelGGL(k_sdp, dim3(plan.grid, B), dim3(plan.block), plan.smem, s, g);
    RTS_HIP(hipGetLastError());
    if (strips <= sdp::kTailStrips) {
        hipLaunchKernelGGL(dtw_tail_kernel<SUBSEQ>, dim3(B), dim3(64 * strips), sdp::tail_lds_bytes(strips), s, g);
    } else {
        hipLaunchKernelGGL(dtw_hops_kernel<SUBSEQ>, dim3(B), dim3(64), 0, s, g);
        hipLaunchKernelGGL((dtw_segment_kernel<0, SUBSEQ>), dim3(strips, B), dim3(64), 0, s, g);
        hipLaunchKernelGGL((dtw_segment_kernel<1, SUBSEQ>), dim3(strips, B), dim3(64), 0, s, g);
    }
    RTS_HIP(hipGetLastError());
    if (g.back) {
        hipLaunchKernelGGL(dtw_back_decode_kernel, dim3((N + 255) / 256, M, B), dim3(256), 0, s, g);
        RTS_HIP(hipGetLastError());
    }
    return RTS_OK;
}

// rts_dtw_paths (SUBSEQ = false: start_dev, end_dev and row_dev are absent) and rts_dtw_subseq_paths.
template <bool SUBSEQ>
static int dtw_paths_call(const void *a_dev, int a_dtype, long long a_stride, const int32_t *a_len_dev, const void *b_dev,
                          int b_dtype, long long b_stride, const int32_t *b_len_dev, int F, int M_max, int N_max, int B,
                          int32_t *path_dev, int32_t *path_len_dev, double *total_dev, int32_t *start_dev, int32_t *end_dev,
                          double *row_dev, void *ws_dev, size_t ws_bytes, void *stream) {
    if (!a_dev) return set_error(RTS_ERR_INVALID, "a_dev is NULL");
    if (!b_dev) return set_error(RTS_ERR_INVALID, "b_dev is NULL");
    if (!path_dev) return set_error(RTS_ERR_INVALID, "path_dev is NULL");
    if (!path_len_dev) return set_error(RTS_ERR_INVALID, "path_len_dev is NULL");
    if (!total_dev) return set_error(RTS_ERR_INVALID, "total_dev is NULL");
    if (SUBSEQ && !start_dev) return set_error(RTS_ERR_INVALID, "start_dev is NULL");
    if (SUBSEQ && !end_dev) return set_error(RTS_ERR_INVALID, "end_dev is NULL");
    if (!ws_dev) return set_error(RTS_ERR_INVALID, "ws_dev is NULL");
    if (int rc = dtw_check(a_dtype, b_dtype, F, M_max, N_max, B, path_dev, ws_dev, ws_bytes, "M_max", "N_max",
                           SUBSEQ ? "rts_dtw_subseq_paths_workspace_bytes" : "rts_dtw_paths_workspace_bytes");
        rc != RTS_OK)
        return rc;
    if (a_stride != 0 && a_stride < M_max)
        return set_error(RTS_ERR_INVALID, "a_stride must be 0 (shared) or >= M_max (got %lld)", a_stride);
    if (b_stride != 0 && b_stride < N_max)
        return set_error(RTS_ERR_INVALID, "b_stride must be 0 (shared) or >= N_max (got %lld)", b_stride);
    const DtwArgs g = dtw_args(a_dev, a_dtype, a_stride, a_len_dev, b_dev, b_dtype, b_stride, b_len_dev, M_max, N_max, nullptr,
                               nullptr, nullptr, path_dev, path_len_dev, total_dev, start_dev, end_dev, row_dev);
    return dtw_enqueue<false, SUBSEQ>(g, B, ws_dev, (hipStream_t)stream);
}

}  // namespace rts

extern "C" {

int rts_dtw_workspace_bytes(int M, int N, int B, size_t *bytes) {
    return rts::dtw_workspace(M, N, B, bytes, "M", "N");
}

int rts_dtw(const void *a_dev, int a_dtype, long long a_stride, const void *b_dev, int b_dtype,
            long long b_stride, int F, int M, int N, int B, double *cost_dev, double *acc_dev,
            int8_t *back_dev, int32_t *path_dev, int32_t *path_len_dev, void *ws_dev, size_t ws_bytes,
            void *stream) {
    using namespace rts;
    if (!a_dev || !b_dev || !cost_dev || !acc_dev || !path_dev || !path_len_dev || !ws_dev)
        return set_error(RTS_ERR_INVALID, "NULL device buffer");
    if (int rc = dtw_check(a_dtype, b_dtype, F, M, N, B, path_dev, ws_dev, ws_bytes, "M", "N", "rts_dtw_workspace_bytes");
        rc != RTS_OK)
        return rc;
    const DtwArgs g = dtw_args(a_dev, a_dtype, a_stride, nullptr, b_dev, b_dtype, b_stride, nullptr, M, N, cost_dev, acc_dev,
                               back_dev, path_dev, path_len_dev, nullptr, nullptr, nullptr, nullptr);
    return dtw_enqueue<true>(g, B, ws_dev, (hipStream_t)stream);
}

// The layout is rts_dtw's, sized by the maxima: a pair's slices hold its own, smaller arrays from their start.
int rts_dtw_paths_workspace_bytes(int M_max, int N_max, int B, size_t *bytes) {
    return rts::dtw_workspace(M_max, N_max, B, bytes, "M_max", "N_max");
}

int rts_dtw_paths(const void *a_dev, int a_dtype, long long a_stride, const int32_t *a_len_dev, const void *b_dev,
                  int b_dtype, long long b_stride, const int32_t *b_len_dev, int F, int M_max, int N_max, int B,
                  int32_t *path_dev, int32_t *path_len_dev, double *total_dev, void *ws_dev, size_t ws_bytes,
                  void *stream) {
    return rts::dtw_paths_call<false>(a_dev, a_dtype, a_stride, a_len_dev, b_dev, b_dtype, b_stride, b_len_dev, F, M_max,
                                      N_max, B, path_dev, path_len_dev, total_dev, nullptr, nullptr, nullptr, ws_dev,
                                      ws_bytes, stream);
}

// The workspace is rts_dtw_paths': the last row lives in the boundary slot of a pair's last row group, which that call
// leaves unused.
int rts_dtw_subseq_paths_workspace_bytes(int M_max, int N_max, int B, size_t *bytes) {
    return rts::dtw_workspace(M_max, N_max, B, bytes, "M_max", "N_max");
}

int rts_dtw_subseq_paths(const void *a_dev, int a_dtype, long long a_stride, const int32_t *a_len_dev, const void *b_dev,
                         int b_dtype, long long b_stride, const int32_t *b_len_dev, int F, int M_max, int N_max, int B,
                         int32_t *path_dev, int32_t *path_len_dev, double *total_dev, int32_t *start_dev,
                         int32_t *end_dev, double *row_dev, void *ws_dev, size_t ws_bytes, void *stream) {
    return rts::dtw_paths_call<true>(a_dev, a_dtype, a_stride, a_len_dev, b_dev, b_dtype, b_stride, b_len_dev, F, M_max,
                                     N_max, B, path_dev, path_len_dev, total_dev, start_dev, end_dev, row_dev, ws_dev,
                                     ws_bytes, stream);
}

}  // extern "C"
