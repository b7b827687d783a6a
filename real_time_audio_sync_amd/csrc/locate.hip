// Locate: subsequence DTW of B live excerpts (M <= 256 frames each) against P pieces of a reference pool, for gfx950.
//
// The recurrence is dtw.py:32-40 (cost c, options left + c, up + c, diag + 2c in this order, first minimum) with the
// first row freed: D[0][j] = c(0, j), and every cell carries along the column S at which its best path left row 0.  The
// answer per (stream, piece) is the first minimum of the last row, its column (end) and its S (start): no dense matrix,
// no back-pointers, no backtrack pass.
//
// Mapping (sdp.h in small).  One workgroup per (piece, stream), one wave per STRIP of 64 query rows, lane = row, lanes
// skewed in time: at strip step s lane l evaluates column j = s - l, so (i, j-1) is the lane's own previous value and
// (i-1, j), (i-1, j-1) arrive by wave_shr:1 DPP (value and start index).  Strip w + 1 runs kLag chunks of 16 steps behind
// strip w in the same workgroup and takes strip w's bottom row from a 64-column LDS ring; all waves advance in lockstep,
// one LDS-only barrier per chunk.  Nothing is handed through HBM and nothing spins.
//
// Costs.  Every lane keeps its query row in registers (float64).  Wave 0 stages the piece's frames through LDS, one chunk
// of 16 columns ahead, in the pool's own element type: a ring of 5 S + 1 chunks covers the columns all S strips are
// working on.  The 16 costs of a chunk do not depend on the recurrence; a lane computes them from its 16 skewed column
// records before it enters the dependent chain.  Reading the records skewed (every lane another column) instead of
// sweeping whole columns into a cost ring costs LDS bandwidth (48 or 96 bytes per cell) but needs 9 / 4.6 KB of LDS per
// strip instead of sdp.h's 48 KB ring, so a CU holds sixteen 64-row problems at once: this kernel is fed B x P
// independent problems and is built for residency, not for the latency of one.
//
// The lane that owns row M - 1 keeps the running first minimum.  The optional last row (D and S) leaves through a
// 16-entry LDS tile per chunk, so that HBM sees one 128-byte / 64-byte segment per chunk instead of a store per step.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <type_traits>

#include "common.h"
#include "cost.h"
#include "sdp.h"

namespace rts {

constexpr int kLocF = 12;
constexpr int kLocMaxM = 256;
constexpr int kLocChunk = 16;  // steps between two workgroup barriers
constexpr int kLocLag = 5;     // chunks strip w + 1 runs behind strip w: lane 63 finishes column 16m + 15 at step 16m + 78

struct LocArgs {
    const void *q;           // [B][M_max][12]
    const int32_t *q_len;    // [B] or NULL
    const void *pool;        // [n_pool][12]
    const long long *first;  // [P]
    const int32_t *len;      // [P]
    double *cost;            // [B][P]
    int32_t *end, *start;    // [B][P]
    double *row;             // optional [B][n_pool]
    int32_t *rowstart;       // optional [B][n_pool]
    long long n_pool;
    int M_max, P, q_f64;
};

__host__ __device__ inline int loc_ring_chunks(int S) { return kLocLag * S + 1; }
// frame ring, bottom rows of strips 0 .. S-2 (value, start), the last-row tile of the current chunk (value, start)
__host__ __device__ inline size_t loc_lds_bytes(int S, bool y64) {
    return (size_t)loc_ring_chunks(S) * kLocChunk * kLocF * (y64 ? 8 : 4) + (size_t)(S - 1) * 64 * 12 + kLocChunk * 12;
}

template <bool Y64, bool EUCLID>
__global__ void __launch_bounds__(kLocMaxM) locate_kernel(LocArgs g) {
    using yel = typename std::conditional<Y64, double, float>::type;
    extern __shared__ __align__(16) unsigned char loc_smem[];
    const int p = blockIdx.x, b = blockIdx.y;
    const int S = (int)(blockDim.x >> 6);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const size_t out = (size_t)b * g.P + p;

    int M = g.q_len ? g.q_len[b] : g.M_max;
    M = M < g.M_max ? M : g.M_max;
    const long long first = g.first[p];
    const int N = g.len[p];
    if (M < 1 || N < 1 || first < 0 || first > g.n_pool - N) {  // nothing to match: the whole workgroup leaves
        if (threadIdx.x == 0) {
            g.cost[out] = INFINITY;
            g.end[out] = -1;
            g.start[out] = -1;
        }
        return;
    }

    const int RC = loc_ring_chunks(S), R = RC * kLocChunk;  // ring size in chunks / columns
    yel *ring = reinterpret_cast<yel *>(loc_smem);           // [R][12]
    double *brD = reinterpret_cast<double *>(loc_smem + (size_t)R * kLocF * sizeof(yel));  // [S-1][64]
    double *obD = brD + (size_t)(S - 1) * 64;                                                // [16]
    int32_t *brS = reinterpret_cast<int32_t *>(obD + kLocChunk);                             // [S-1][64]
    int32_t *obS = brS + (size_t)(S - 1) * 64;                                               // [16]

    const int nact = sdp::n_strips(M);  // strips that hold rows of this stream's query (waves beyond only keep the barriers)
    const int nch = (N + 63 + kLocChunk - 1) / kLocChunk;
    const int K = nch + kLocLag * (nact - 1);
    const int i = wave * 64 + lane;
    const int own_wave = (M - 1) >> 6, own_lane = (M - 1) & 63;
    const bool own = (wave == own_wave) && (lane == own_lane);
    const bool want_rows = (g.row != nullptr) || (g.rowstart != nullptr);

    double x[kLocF];
    {
        const long long fr = (long long)b * g.M_max + (i < M ? i : M - 1);
        sdp::load_frame(g.q, g.q_f64, fr, x);
    }

    // wave 0: the 192 elements of column chunk cc, three per lane (columns past the piece repeat its last one: their
    // costs feed cells outside the matrix only)
    const yel *ypool = reinterpret_cast<const yel *>(g.pool);
    yel pf[3];
    auto fetch = [&](int cc) {
#pragma unroll
        for (int e = 0; e < 3; e++) {
            const int v = lane + 64 * e;
            int col = kLocChunk * cc + v / kLocF;
            col = col < N ? col : N - 1;
            pf[e] = ypool[(first + col) * kLocF + v % kLocF];
        }
    };
    auto commit = [&](int cc) {
        yel *dst = ring + (size_t)(cc % RC) * kLocChunk * kLocF;
#pragma unroll
        for (int e = 0; e < 3; e++) dst[lane + 64 * e] = pf[e];
    };
    if (wave == 0) {
        fetch(0);
        commit(0);
    }
    lds_barrier();

    double prev = 0.0, upprev = 0.0, minv = INFINITY;
    int sprev = 0, supprev = 0, mine = -1, mins = -1;
    int ridx = lane == 0 ? 0 : R - lane;  // ring slot of my current column (-lane at step 0)

    for (int k = 0; k < K; k++) {
        // Slot (k + 1) % RC holds chunk k - 5 S, which no strip reads any more: strip S - 1 is at columns >= 16 (k - 5 S + 1) + 1.
        const bool pre = (wave == 0) && (k + 1 < nch);
        if (pre) fetch(k + 1);
        const int m = k - kLocLag * wave;  // my strip's chunk
        if (wave < nact && m >= 0 && m < nch) {
            // ---- the row above, columns [16m, 16m + 16): lane q holds column 16m + q
            double upD = 0.0;
            int upS = 0;
            if (wave > 0 && lane < kLocChunk) {
                const int c = (kLocChunk * m + lane) & 63;
                upD = brD[(wave - 1) * 64 + c];
                upS = brS[(wave - 1) * 64 + c];
            }
            const int jneg = lane - kLocChunk * m;  // column of step q is q - jneg
            // ---- the chunk's 16 costs, ahead of the dependent chain
            double cst[kLocChunk];
#pragma unroll
            for (int q = 0; q < kLocChunk; q++) {
                double y[kLocF];
                if constexpr (Y64) {
                    const double2 *rec = reinterpret_cast<const double2 *>(ring + (size_t)ridx * kLocF);
#pragma unroll
                    for (int f = 0; f < kLocF / 2; f++) {
                        const double2 t = rec[f];
                        y[2 * f] = t.x;
                        y[2 * f + 1] = t.y;
                    }
                } else {
                    const float4 *rec = reinterpret_cast<const float4 *>(ring + (size_t)ridx * kLocF);
#pragma unroll
                    for (int f = 0; f < kLocF / 4; f++) {
                        const float4 t = rec[f];
                        y[4 * f] = (double)t.x;
                        y[4 * f + 1] = (double)t.y;
                        y[4 * f + 2] = (double)t.z;
                        y[4 * f + 3] = (double)t.w;
                    }
                }
                if constexpr (EUCLID) {
                    cst[q] = euclid12(x, y);
                } else {  // sdp::DtwPolicy::cost: one fma chain in k order
                    double s = 0.0;
#pragma unroll
                    for (int f = 0; f < kLocF; f++) s = fma(x[f], y[f], s);
                    cst[q] = 1.0 - s;
                }
                ridx = (ridx + 1 == R) ? 0 : ridx + 1;
            }
            // ---- 16 steps of the recurrence.  FIRST: this strip holds query row 0 (lane 0); COL0: some lane is at column 0.
            auto steps = [&](auto first_c, auto col0_c) {
                constexpr bool FIRST = decltype(first_c)::value;
                constexpr bool COL0 = decltype(col0_c)::value;
                const bool first_row = FIRST && lane == 0;
                sdp::static_for<0, kLocChunk>([&](auto qc) {
                    constexpr int q = decltype(qc)::value;
                    const double c = cst[q];
                    const int j = q - jneg;
                    const double up = sdp::shr1(prev, sdp::readlane_d(upD, q));
                    const int sup = sdp::shr1_i(sprev, __builtin_amdgcn_readlane(upS, q));
                    // the value by two v_min_f64, the start index of the first minimum by compares off that chain
                    const double o0 = prev + c, o1 = up + c, o2 = upprev + 2 * c;
                    const double m01 = sdp::vmin(o0, o1);
                    double best = sdp::vmin(m01, o2);
                    int ss = (o1 < o0) ? sup : sprev;
                    ss = (o2 < m01) ? supprev : ss;
                    if (COL0 && q == jneg) {  // column 0: only (i-1, 0)
                        best = o1;
                        ss = sup;
                    }
                    if (first_row) {  // free start: D[0][j] = c, S[0][j] = j
                        best = c;
                        ss = j;
                    }
                    upprev = up;
                    supprev = sup;
                    prev = best;
                    sprev = ss;
                    if (wave + 1 < nact && lane == 63) {  // bottom row, for the strip below
                        brD[wave * 64 + (j & 63)] = best;
                        brS[wave * 64 + (j & 63)] = ss;
                    }
                    const bool upd = own && j >= 0 && j < N && best < minv;  // strict: the first minimum stays
                    minv = upd ? best : minv;
                    mine = upd ? j : mine;
                    mins = upd ? ss : mins;
                    if (want_rows && own) {
                        obD[q] = best;
                        obS[q] = ss;
                    }
                });
            };
            const bool col0 = (kLocChunk * m < 64);
            if (wave == 0) {
                if (col0)
                    steps(sdp::BoolC<true>(), sdp::BoolC<true>());
                else
                    steps(sdp::BoolC<true>(), sdp::BoolC<false>());
            } else {
                if (col0)
                    steps(sdp::BoolC<false>(), sdp::BoolC<true>());
                else
                    steps(sdp::BoolC<false>(), sdp::BoolC<false>());
            }
            // ---- the last row's 16 cells of this chunk: columns 16m - own_lane + [0, 16), lane q stores step q's
            if (want_rows && wave == own_wave) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const int col = kLocChunk * m - own_lane + lane;
                if (lane < kLocChunk && col >= 0 && col < N) {
                    const size_t at = (size_t)b * (size_t)g.n_pool + (size_t)(first + col);
                    if (g.row) g.row[at] = obD[lane];
                    if (g.rowstart) g.rowstart[at] = obS[lane];
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
        if (pre) commit(k + 1);
        lds_barrier();
    }
    if (own) {
        g.cost[out] = minv;
        g.end[out] = mine;
        g.start[out] = mins;
    }
}

}  // namespace rts

namespace rts {

constexpr int kLocMaxK = 32;            // ranks per (stream, piece) of rts_locate_matches
constexpr int kLocMatchThreads = 256;   // locate_matches_kernel: four waves scan one row
constexpr int kLocOverlapThreads = 1024;

struct LocMatchArgs {
    const int32_t *q_len;      // [B] or NULL
    const long long *first;    // [P]
    const int32_t *len;        // [P]
    const double *row;         // [B][n_pool]: D[M-1][:] of every valid piece at its pool position
    const int32_t *rowstart;   // [B][n_pool]: S[M-1][:]
    double *cost;              // [B][P][K]
    int32_t *end, *start;      // [B][P][K]
    int32_t *n;                // [B][P]
    long long n_pool;
    double max_cost;
    int M_max, P, K;
};

__device__ __forceinline__ bool loc_piece_valid(long long first, int N, long long n_pool) {
    return N >= 1 && first >= 0 && first <= n_pool - N;
}

// One workgroup, behind locate_kernel and in front of locate_matches_kernel.
// 1. n[b][p] = -1 for a valid piece whose pool range intersects that of another valid piece (its cells of the row hold
//    "the value of one of them"), 0 otherwise: every thread tests its pieces against the whole table.
// 2. locate_kernel left its own (cost, end, start) packed [B][P] at the front of the [B][P][K] outputs; those of the
//    flagged pieces move to their slot 0, at K (b P + p).  Index i moves up to K i >= i, so chunks of the packed
//    array are taken from the top down, each read into registers before any of it is written: a store can only land
//    on packed entries of this chunk or of one already moved.  Entries of pieces without a flag are not moved at
//    all: locate_matches_kernel finds rank 0 again in the row, bit for bit.
__global__ void __launch_bounds__(kLocOverlapThreads) locate_overlap_kernel(LocMatchArgs g, int B) {
    for (int p = threadIdx.x; p < g.P; p += kLocOverlapThreads) {
        const long long f = g.first[p];
        const int N = g.len[p];
        int flag = 0;
        if (loc_piece_valid(f, N, g.n_pool)) {
            for (int q = 0; q < g.P; q++) {
                const long long fq = g.first[q];
                const int Nq = g.len[q];
                if (q != p && loc_piece_valid(fq, Nq, g.n_pool) && fq < f + N && f < fq + Nq) flag = -1;
            }
        }
        for (int b = 0; b < B; b++) g.n[(size_t)b * g.P + p] = flag;
    }
    __syncthreads();
    if (g.K == 1) return;  // slot 0 is the packed entry itself
    const long long total = (long long)B * g.P;
    for (long long c0 = (total - 1) / kLocOverlapThreads * kLocOverlapThreads; c0 >= 0; c0 -= kLocOverlapThreads) {
        const long long i = c0 + threadIdx.x;
        const bool mv = i < total && g.n[i] < 0;
        double c = 0.0;
        int e = 0, s = 0;
        if (mv) {
            c = g.cost[i];
            e = g.end[i];
            s = g.start[i];
        }
        __syncthreads();
        if (mv) {
            g.cost[i * g.K] = c;
            g.end[i * g.K] = e;
            g.start[i * g.K] = s;
        }
    }
}

// Ranked non-overlapping matches of one (piece, stream) from its last row: K rounds of a first-minimum reduction.  A
// round: every lane scans columns tid, tid + 256, ... (coalesced; the row stays in L2 between
// rounds) and keeps its first minimum among the finite columns whose own range [S[j], j] meets no range taken so far --
// the interval test against the <= K ranges in LDS, run (with the load of S[j]) only for a column that would improve the
// lane's minimum; the (value, column) pairs are combined over their total order by a butterfly in the wave and through
// LDS across the four waves; thread 0 appends the winner.  Nothing is written but the outputs.
__global__ void __launch_bounds__(kLocMatchThreads) locate_matches_kernel(LocMatchArgs g) {
    constexpr int kWaves = kLocMatchThreads / 64;
    __shared__ double wv[kWaves];
    __shared__ int wc[kWaves];
    __shared__ int rs[kLocMaxK], re[kLocMaxK];  // ranges taken: start, end
    __shared__ int more;
    const int p = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const size_t out = (size_t)b * g.P + p;
    const int K = g.K;

    int M = g.q_len ? g.q_len[b] : g.M_max;
    M = M < g.M_max ? M : g.M_max;
    const long long first = g.first[p];
    const int N = g.len[p];
    const bool nothing = M < 1 || !loc_piece_valid(first, N, g.n_pool);  // locate_kernel's own test
    if (nothing || g.n[out] < 0) {  // uniform: the whole workgroup leaves before its first barrier
        // nothing to match: n = 0, every slot empty.  Overlapping piece: n = -1 and slot 0 are already in place.
        for (int k = tid + (nothing ? 0 : 1); k < K; k += kLocMatchThreads) {
            g.cost[out * K + k] = INFINITY;
            g.end[out * K + k] = -1;
            g.start[out * K + k] = -1;
        }
        if (nothing && tid == 0) g.n[out] = 0;
        return;
    }

    const double *D = g.row + (size_t)b * (size_t)g.n_pool + (size_t)first;
    const int32_t *S = g.rowstart + (size_t)b * (size_t)g.n_pool + (size_t)first;
    int n = 0;
    for (int r = 0; r < K; r++) {
        double v = INFINITY;  // a lane without a column never wins
        int c = 0x7fffffff;
        for (int j = tid; j < N; j += kLocMatchThreads) {
            const double d = D[j];
            if (d < v && d > -INFINITY) {  // strict: the lane's first minimum stays; NaN and +-inf never enter
                const int s = S[j];
                bool taken = false;
                for (int q = 0; q < r; q++) taken |= (s <= re[q]) & (j >= rs[q]);
                if (!taken) {
                    v = d;
                    c = j;
                }
            }
        }
        for (int d = 32; d >= 1; d >>= 1) {
            const double ov = __shfl_xor(v, d);
            const int oc = __shfl_xor(c, d);
            if (ov < v || (ov == v && oc < c)) {
                v = ov;
                c = oc;
            }
        }
        if (lane == 0) {
            wv[wave] = v;
            wc[wave] = c;
        }
        lds_barrier();
        if (tid == 0) {
#pragma unroll
            for (int w = 1; w < kWaves; w++) {
                if (wv[w] < v || (wv[w] == v && wc[w] < c)) {
                    v = wv[w];
                    c = wc[w];
                }
            }
            const bool hit = c < N && !(v > g.max_cost);
            if (hit) {
                const int s = S[c];
                rs[r] = s;
                re[r] = c;
                g.cost[out * K + r] = v;
                g.end[out * K + r] = c;
                g.start[out * K + r] = s;
            }
            more = hit;
        }
        lds_barrier();
        if (!more) break;  // uniform
        n = r + 1;
    }
    for (int k = n + tid; k < K; k += kLocMatchThreads) {
        g.cost[out * K + k] = INFINITY;
        g.end[out * K + k] = -1;
        g.start[out * K + k] = -1;
    }
    if (tid == 0) g.n[out] = n;
}

// The argument checks rts_locate and rts_locate_matches share (all of them before the first HIP call).
static int loc_check(const void *queries_dev, int q_dtype, int M_max, int B, const void *pool_dev, int pool_dtype, int F,
                     long long n_pool_frames, const long long *piece_first_dev, const int32_t *piece_len_dev, int P,
                     int cost_kind, const double *cost_dev, const int32_t *end_dev, const int32_t *start_dev) {
    if (!queries_dev) return set_error(RTS_ERR_INVALID, "queries_dev is NULL");
    if (!pool_dev) return set_error(RTS_ERR_INVALID, "pool_dev is NULL");
    if (!piece_first_dev) return set_error(RTS_ERR_INVALID, "piece_first_dev is NULL");
    if (!piece_len_dev) return set_error(RTS_ERR_INVALID, "piece_len_dev is NULL");
    if (!cost_dev) return set_error(RTS_ERR_INVALID, "cost_dev is NULL");
    if (!end_dev) return set_error(RTS_ERR_INVALID, "end_dev is NULL");
    if (!start_dev) return set_error(RTS_ERR_INVALID, "start_dev is NULL");
    if (F != kLocF) return set_error(RTS_ERR_UNSUPPORTED, "F must be 12 chroma bins (got %d)", F);
    if (M_max < 1) return set_error(RTS_ERR_INVALID, "M_max must be >= 1 (got %d)", M_max);
    if (M_max > kLocMaxM)
        return set_error(RTS_ERR_UNSUPPORTED, "M_max must be <= %d query frames (got %d)", kLocMaxM, M_max);
    if (B < 1 || B > 65535) return set_error(RTS_ERR_INVALID, "B must be in [1, 65535] (got %d)", B);
    if (P < 1 || P > 65535) return set_error(RTS_ERR_INVALID, "P must be in [1, 65535] (got %d)", P);
    if (n_pool_frames < 1) return set_error(RTS_ERR_INVALID, "n_pool_frames must be >= 1 (got %lld)", n_pool_frames);
    if (!dtype_ok(q_dtype)) return set_error(RTS_ERR_INVALID, "bad q_dtype %d", q_dtype);
    if (!dtype_ok(pool_dtype)) return set_error(RTS_ERR_INVALID, "bad pool_dtype %d", pool_dtype);
    if (cost_kind != RTS_COST_DOT && cost_kind != RTS_COST_EUCLID)
        return set_error(RTS_ERR_INVALID, "bad cost_kind %d", cost_kind);
    return RTS_OK;
}

static void loc_launch(const LocArgs &g, int B, int pool_dtype, int cost_kind, hipStream_t s) {
    const int S = sdp::n_strips(g.M_max);
    const bool y64 = pool_dtype == RTS_F64, euclid = cost_kind == RTS_COST_EUCLID;
    const dim3 grid(g.P, B), block(64 * S);
    const size_t smem = loc_lds_bytes(S, y64);
    if (y64 && euclid)
        hipLaunchKernelGGL((locate_kernel<true, true>), grid, block, smem, s, g);
    else if (y64)
        hipLaunchKernelGGL((locate_kernel<true, false>), grid, block, smem, s, g);
    else if (euclid)
        hipLaunchKernelGGL((locate_kernel<false, true>), grid, block, smem, s, g);
    else
        hipLaunchKernelGGL((locate_kernel<false, false>), grid, block, smem, s, g);
}

constexpr size_t kLocWsAlign = 256;
inline size_t loc_ws_round(size_t n) { return (n + kLocWsAlign - 1) / kLocWsAlign * kLocWsAlign; }
// ws_dev rounded up to 256 | rows double [B][n_pool], rounded up to 256 | starts int32 [B][n_pool], rounded up to 256
inline size_t loc_ws_bytes(int B, long long n_pool) {
    const size_t cells = (size_t)B * (size_t)n_pool;
    return kLocWsAlign + loc_ws_round(cells * sizeof(double)) + loc_ws_round(cells * sizeof(int32_t));
}
constexpr long long kLocMaxPool = 1LL << 40;  // keeps B * n_pool_frames * 12 far inside size_t

}  // namespace rts

extern "C" {

int rts_locate(const void *queries_dev, int q_dtype, int M_max, const int32_t *q_len_dev, int B, const void *pool_dev,
               int pool_dtype, int F, long long n_pool_frames, const long long *piece_first_dev,
               const int32_t *piece_len_dev, int P, int cost_kind, double *cost_dev, int32_t *end_dev,
               int32_t *start_dev, double *row_dev, int32_t *rowstart_dev, void *stream) {
    using namespace rts;
    const int rc = loc_check(queries_dev, q_dtype, M_max, B, pool_dev, pool_dtype, F, n_pool_frames, piece_first_dev,
                             piece_len_dev, P, cost_kind, cost_dev, end_dev, start_dev);
    if (rc != RTS_OK) return rc;
    LocArgs g;
    g.q = queries_dev;
    g.q_len = q_len_dev;
    g.pool = pool_dev;
    g.first = piece_first_dev;
    g.len = piece_len_dev;
    g.cost = cost_dev;
    g.end = end_dev;
    g.start = start_dev;
    g.row = row_dev;
    g.rowstart = rowstart_dev;
    g.n_pool = n_pool_frames;
    g.M_max = M_max;
    g.P = P;
    g.q_f64 = q_dtype == RTS_F64;
    loc_launch(g, B, pool_dtype, cost_kind, (hipStream_t)stream);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

int rts_locate_matches_workspace_bytes(int B, long long n_pool_frames, size_t *bytes) {
    using namespace rts;
    if (!bytes) return set_error(RTS_ERR_INVALID, "bytes is NULL");
    if (B < 1 || B > 65535) return set_error(RTS_ERR_INVALID, "B must be in [1, 65535] (got %d)", B);
    if (n_pool_frames < 1 || n_pool_frames > kLocMaxPool)
        return set_error(RTS_ERR_INVALID, "n_pool_frames must be in [1, 2^40] (got %lld)", n_pool_frames);
    *bytes = loc_ws_bytes(B, n_pool_frames);
    return RTS_OK;
}

int rts_locate_matches(const void *queries_dev, int q_dtype, int M_max, const int32_t *q_len_dev, int B,
                       const void *pool_dev, int pool_dtype, int F, long long n_pool_frames,
                       const long long *piece_first_dev, const int32_t *piece_len_dev, int P, int cost_kind, int K,
                       double max_cost, double *cost_dev, int32_t *end_dev, int32_t *start_dev, int32_t *n_dev,
                       void *ws_dev, size_t ws_bytes, void *stream) {
    using namespace rts;
    const int rc = loc_check(queries_dev, q_dtype, M_max, B, pool_dev, pool_dtype, F, n_pool_frames, piece_first_dev,
                             piece_len_dev, P, cost_kind, cost_dev, end_dev, start_dev);
    if (rc != RTS_OK) return rc;
    if (!n_dev) return set_error(RTS_ERR_INVALID, "n_dev is NULL");
    if (!ws_dev) return set_error(RTS_ERR_INVALID, "ws_dev is NULL");
    if (K < 1) return set_error(RTS_ERR_INVALID, "K must be >= 1 (got %d)", K);
    if (K > kLocMaxK) return set_error(RTS_ERR_UNSUPPORTED, "K must be <= %d ranks (got %d)", kLocMaxK, K);
    if (max_cost != max_cost) return set_error(RTS_ERR_INVALID, "max_cost is NaN");
    if (n_pool_frames > kLocMaxPool)
        return set_error(RTS_ERR_INVALID, "n_pool_frames must be <= 2^40 (got %lld)", n_pool_frames);
    const size_t need = loc_ws_bytes(B, n_pool_frames);
    if (ws_bytes < need) return set_error(RTS_ERR_INVALID, "ws_bytes is %zu, %zu are needed", ws_bytes, need);
    const size_t cells = (size_t)B * (size_t)n_pool_frames;
    unsigned char *base = reinterpret_cast<unsigned char *>(loc_ws_round(reinterpret_cast<uintptr_t>(ws_dev)));
    double *row = reinterpret_cast<double *>(base);
    int32_t *rowstart = reinterpret_cast<int32_t *>(base + loc_ws_round(cells * sizeof(double)));
    hipStream_t s = (hipStream_t)stream;
    // 1. the locate kernel as it is: rows into the workspace, its own answers packed [B][P] at the front of the outputs
    LocArgs g;
    g.q = queries_dev;
    g.q_len = q_len_dev;
    g.pool = pool_dev;
    g.first = piece_first_dev;
    g.len = piece_len_dev;
    g.cost = cost_dev;
    g.end = end_dev;
    g.start = start_dev;
    g.row = row;
    g.rowstart = rowstart;
    g.n_pool = n_pool_frames;
    g.M_max = M_max;
    g.P = P;
    g.q_f64 = q_dtype == RTS_F64;
    loc_launch(g, B, pool_dtype, cost_kind, s);
    RTS_HIP(hipGetLastError());
    // 2. overlap flags (and slot 0 of the flagged pieces), 3. the ranks
    LocMatchArgs m;
    m.q_len = q_len_dev;
    m.first = piece_first_dev;
    m.len = piece_len_dev;
    m.row = row;
    m.rowstart = rowstart;
    m.cost = cost_dev;
    m.end = end_dev;
    m.start = start_dev;
    m.n = n_dev;
    m.n_pool = n_pool_frames;
    m.max_cost = max_cost;
    m.M_max = M_max;
    m.P = P;
    m.K = K;
    hipLaunchKernelGGL(locate_overlap_kernel, dim3(1), dim3(kLocOverlapThreads), 0, s, m, B);
    RTS_HIP(hipGetLastError());
    hipLaunchKernelGGL(locate_matches_kernel, dim3(P, B), dim3(kLocMatchThreads), 0, s, m);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

}  // extern "C"
