// Windowed time warping for gfx950: the chroma-level half of wtw.WTW.insert (the reference's wtw.py:92-128) with
// get_cost_matrix (:162-171), run_dtw (:173-217) and find_path (:219-240), batched over B independent live streams, each
// against one reference chroma or against its own slice of a pool of references.
//
// Whenever a stream has a full window of W live frames, the window is the W x W normalised-cosine cost in the reference's
// dot orders (sdp::WtwPolicy: norms as an fma chain = x.dot(x) on a contiguous copy, cross term in OpenBLAS's strided ddot
// order), the unit-weight DP over it (candidates (i-1,j), (i,j-1), (i-1,j-1), strict '<' in that order), the walk back
// from its last cell, and the hand-over rule of wtw.py:107-128 (append the sub-path points with l <= dtw_hop / hop, move
// (live_ptr, ref_ptr) to the last appended point).  D, the paths and the pointers are bit-identical to the serial loops.
// Two paths do this; wtw_select() picks one per handle, at create:
//
// Windows of at most kWinW = 128 frames (tests.py:174's W = 20, wtw_live.py's W = 100): wtw_win_kernel, one workgroup per
// stream, every window of a push in ONE launch, the cost matrix and the step codes in LDS (described at the kernel).
//
// Longer windows (up to BASELINE configs[4]'s W = 10 000, where one window is 1e8 cells; from 65 frames with
// RTS_WTW_WIN=0) run as a strip DP (sdp.h) spread over many workgroups: per window one launch of wtw_big_dp_kernel (a
// pipeline of row groups down the W x W matrix, step codes packed 2 bits per cell in HBM), the backtrack kernels
// (wtw_big_hops_kernel, wtw_big_segment_kernel: every strip's path segment by its own wave; one wtw_big_tail_ctl_kernel
// for windows of few strips) and wtw_big_ctl_kernel (hand-over, then the column bookkeeping of wtw.py:92-100 up to the
// next window).  The host enqueues as many such rounds as the pushed columns can possibly complete windows; rounds with
// nothing pending return at once.  Everything stays asynchronous.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "sdp.h"
#include "snapshot.h"  // rts_wtw_export / rts_wtw_import: the record kernels both trackers share

namespace rts {

constexpr int kWF = 12;
constexpr int kWtwMaxW = 16384;

struct WtwArgs {
    const double *ref;    // [M][F]; with per-stream references [n_ref_frames][F], stream b at ref_first[b]
    double *live;         // [B][live_stride][F]  (live_stride = 2M, 2 M_max with per-stream references)
    int32_t *appended;    // [B] columns written to `live` so far
    int32_t *state;       // [B][8]: chroma_ptr, live_ptr, ref_ptr, status, n_path, n_windows, cells_lo, cells_hi
    int32_t *path;        // [B][path_cap][2]
    int32_t *appended_next;  // [B] the other count array: the next append writes it, then the host swaps the two
    double *dlast;        // [B][W][W] last window's D (optional, NULL = not stored)
    // the strip DP only (NULL on a handle that runs wtw_win_kernel):
    int32_t *ws_sub;           // [B][4W] ints: the window's sub-path, reversed
    int32_t *ws_scr;           // [B][scratch_pairs(W, W)][2]: its segments as walked (sdp::path_segment)
    int32_t *ctl;              // [B][8]: pending, live_ptr, ref_ptr, n, m of the window being computed
    uint32_t *codes;           // [B][codes_words(W, W)] packed step codes
    unsigned long long *bnd;   // [B][n_strips(W)][W] rows handed between row groups
    int32_t *entb;             // [B][n_strips(W)][W] entry columns of the strips' bottom rows (sdp.h)
    int32_t *cross, *lens;     // [B][n_strips(W)] strip-boundary crossings / segment lengths of the window's path
    double *yrec;              // [B][W][14] prepared records of the window's reference columns
    int32_t *err;
    int32_t *ticket;           // [B] next row group of the pending window (sdp::for_each_rowgroup); zeroed by the control step
    int n_rg, n_strips_wg;
    int M, live_stride, W, hopf, path_cap;
    int fill_separate;         // long windows: the hand-over's fill and column records by wtw_big_fill_kernel
    // per-stream references (rts_wtw_create_refs), NULL for a single-reference handle: stream b follows frames
    // [ref_first[b], ref_first[b] + ref_len[b]) of `ref`.  The kernels take every reference quantity from wtw_ref().
    const long long *ref_first;
    const int32_t *ref_len;
};

// Stream b's reference: its frames, its length M and its live capacity N = 2M (wtw.py:52).  Plain loads of a uniform
// address; every kernel resolves this once, at its start.
struct WtwRef {
    const double *ref;
    int M, N;
};
__device__ __forceinline__ WtwRef wtw_ref(const WtwArgs &g, int b) {
    WtwRef r;
    if (g.ref_first) {
        r.ref = g.ref + g.ref_first[b] * kWF;
        r.M = g.ref_len[b];
    } else {
        r.ref = g.ref;
        r.M = g.M;
    }
    r.N = 2 * r.M;
    return r;
}

// ---- windows of at most kWinW frames: every window of a push in ONE launch, one workgroup per stream -------------
//
// wtw_live.py runs W = 100 / hop = 50, tests.py:174 W = 20 / hop = 10: thousands of small windows per stream, each one
// depending on the hand-over of the one before.  wtw_win_kernel<R, STAGE> keeps a stream's whole window loop on the device.
// Per window k, between workgroup barriers:
//   A. waves 1.. : the n x m cost matrix (1 - x.y / (|x| |y|), wtw.py:169, the reference's dot orders) into LDS -- lanes
//      own columns (reference frame and norm in registers), the waves share the rows (each stages its own rows' live
//      frames and their norms in a wave-private slice of LDS: no barrier inside the phase);
//      wave 0, at the same time: find_path + hand-over of window k - 1 (below).
//   B. row 0 and column 0 of D are running sums (wtw.py:187-198): two lanes accumulate them in the reference's order.
//   C. the interior on R waves, one matrix row per lane, lanes skewed in time (lane l of wave r owns row 1 + 64 r + l and
//      handles column 1 + t - l at step t): the three predecessors of a cell are registers -- the lane's own previous
//      value, the previous value of the lane above (DPP wave_shr:1; lane 0 receives row 0, or wave 0's bottom row, from
//      LDS) and what that move delivered one step earlier.  Same float64 operations and candidate order as
//      wtw.py:201-215 (sdp::WtwPolicy::cell), so D and the path are bit-identical.  The block's 16 costs are fetched
//      into registers before its 16 dependent steps.  With R = 2 (65 < W <= 128) wave 1 runs 5 blocks behind wave 0; one
//      LDS barrier per 16 steps.  Step codes: 2 bits per cell, 16 steps of a lane per dword.
//      Beside the values the lanes propagate, for every cell below row h = dtw_hop / hop, the column at which the cell's
//      best path leaves row h (the same recurrence driven by the step codes; row h + 1 seeds it).  At the last cell that
//      is the column r* of the last point the hand-over will append (wtw.py:113: l <= h), hence the next window's
//      pointers (live_ptr + h, ref_ptr + r*; wtw.py:118-124) are known the moment the DP ends -- without the path.
//   wave 0 in phase A of the next iteration walks the path back from (h, r*) -- only the part that is handed over; from
//      (n-1, m-1) when the window is no taller than the hop -- with the position in SGPRs and the row's code word one
//      v_readlane away (find_path, wtw.py:219-240), and appends it (wtw.py:107-117).
// The column bookkeeping up to the next window is in closed form (the same rules as wtw_ctl_body below).
constexpr int kWinW = 128;       // the largest window of this kernel: two DP waves of 64 rows (wtw_select)
constexpr int kWinKW = 12;       // code words per lane: 64 + 127 - 1 steps at most
constexpr int kWinPadFront = 64;  // doubles in front of / behind the cost matrix: lanes that are not on a valid cell read
constexpr int kWinPadBack = 208;  // (and ignore) whatever their row pointer + step lands on

// wave 0's bottom row (bot / botx): 64 slots in front and 32 behind for the steps at which lane 63 is not on a valid cell,
// and 80 more where every other lane's share of the same unconditional store lands
constexpr int kWinBotFront = 64, kWinBotBack = 32, kWinBotDummy = 80;
constexpr int kWinBotPad = kWinBotFront + kWinBotBack + kWinBotDummy;

// Windows of at most kWinPrefW frames (tests.py:174: 20): while the DP of window k runs, the idle cost waves fetch what the
// cost phase of window k + 1 will need -- its live rows (live_ptr + hop is known) into xs / nx, and the 128 reference frames
// from ref_ptr on (the next window starts at ref_ptr + r*, r* < W, so its columns are among them) into ypre / nypre -- so
// that phase A reads LDS instead of waiting for L2 (3 k of the 5 k cycles of a 20-frame window's cost phase).
constexpr int kWinPrefW = 64;   // (the one-wave kernel's whole range)
constexpr int kWinPrefN = 128;  // reference frames fetched: two per lane of the fetching waves

__host__ __device__ inline int win_ldc(int W) { return (W | 1) + 1; }  // even > W: lanes a row apart hit different LDS banks
__host__ __device__ inline size_t win_lds_bytes(int W) {
    const size_t feat = sizeof(double) * ((size_t)W * kWF + (size_t)W);                    // xs, nx
    const size_t walk = sizeof(uint32_t) * 2 * kWinKW * 64 + sizeof(double) * (3 * (size_t)W + 32 + kWinBotPad) +  // codes; row 0, column 0 (padded), bottom row of wave 0 (padded)
                        sizeof(int32_t) * ((size_t)W + kWinBotPad) + sizeof(int32_t) * 4 * (size_t)W;  // its crossing columns (padded); sub-path
    const size_t pref = (W <= kWinPrefW) ? sizeof(int32_t) * (W & 1) + sizeof(double) * (kWinPrefN * kWF + kWinPrefN) : 0;  // (alignment) ypre, nypre
    return sizeof(double) * ((size_t)W * win_ldc(W) + kWinPadFront + kWinPadBack) + feat + walk + pref + 128;
}

#ifdef RTS_WIN_STAMPS
// diagnostic build only, stream 0: [0] phase A as wave 0 sees it (walk + hand-over + wait for the cost waves), [1] running
// sums, [2] DP, [3] wave 0's own walk + hand-over, [4] wave 1's own cost phase, [5] windows
__device__ long long g_win_stamps[8];
#define RTS_WIN_STAMP(slot)                                                       \
    do {                                                                          \
        const long long now_ = (long long)__builtin_amdgcn_s_memtime();           \
        if (b == 0 && tid == 0) g_win_stamps[slot] += now_ - stamp_t;             \
        stamp_t = now_;                                                           \
    } while (0)
#else
#define RTS_WIN_STAMP(slot) \
    do {                    \
    } while (0)
#endif

// One block of 16 DP steps of wtw_win_kernel, as a macro so that each DP wave gets its own straight-line copy (W1: this is the
// second wave; NSTEP: 16, or 8 for a short last block -- it fetches the crossing columns of wave 0's bottom row for its lane 0 and has no row to hand on; the first
// wave does the opposite).  Not a lambda: inside a generic lambda the compiler lowers the step's selects to exec-mask branch
// ladders (135 branches per block), and a branch inside the block costs the overlap between consecutive steps.  The block's
// 16 costs and 16 values of the row above lane 0 are fetched first (one LDS round trip per block instead of one per step);
// every lane stores every step -- lane 63 to bot[column] (column = t - 62 is hit exactly once per window; steps at which the
// lane is not on a valid cell land in the padding), the others to a scratch strip -- because a conditional store would be a
// branch again (228 cycles per step with it, 139 in the one-wave kernel that has none).
#define RTS_WIN_DP_BLOCK(W1, NSTEP)                                                                                \
    {                                                                                                              \
                double cbuf[16], ubuf[16]; \
                int uxbuf[16]; \
_Pragma("unroll") \
                for (int q = 0; q < (NSTEP); q++) { \
                    const int t = 16 * kb + q; \
                    cbuf[q] = crow[t]; \
                    ubuf[q] = upin[(t + 1 < m) ? t + 1 : 0]; \
                    uxbuf[q] = (W1) ? botx[(t + 1 < m) ? t + 1 : 0] : 0; \
                } \
                double *bw = (lane == 63) ? bot + (16 * kb - 62) : bot_dummy + lane; \
                int32_t *bxw = (lane == 63) ? botx + (16 * kb - 62) : botx_dummy + lane; \
                word = 0; \
_Pragma("unroll") \
                for (int q = 0; q < (NSTEP); q++) { \
                    const int t = 16 * kb + q; \
                    const unsigned jj = (unsigned)(t - lane); \
                    const bool incol = jj < (unsigned)mint; \
                    const bool valid = incol && lane < rows; \
                    const double du = sdp::shr1(dlast_v, ubuf[q]); \
                    const int xu = sdp::shr1_i(xl, uxbuf[q]); \
                    double dv; \
                    int code; \
                    sdp::WtwPolicy::cell(false, false, du, dlast_v, du_prev, cbuf[q], dv, code); \
                    int xn = (code == sdp::kUp) ? xu : ((code == sdp::kDiag) ? xu_prev : xl); \
                    const int xh = (code == sdp::kUp) ? (int)jj + 1 : ((code == sdp::kDiag) ? (int)jj : xl); \
                    xn = is_h1 ? xh : xn; \
                    du_prev = du; \
                    xu_prev = xu; \
                    word |= (uint32_t)code << (2 * q); \
                    if (incol) { \
                        dlast_v = dv; \
                        xl = xn; \
                    } \
                    if constexpr (R > 1 && !(W1)) { /* only the first DP wave has a row to hand on */ \
                        bw[q] = dv; \
                        bxw[q] = xn; \
                    } \
                    if (STAGE && valid) dout[jj + 1] = dv; \
                } \
    }

template <int R, bool STAGE>
__global__ void __launch_bounds__(R == 1 ? 256 : 512) wtw_win_kernel(WtwArgs g) {
    constexpr int NT = (R == 1) ? 256 : 512;  // two waves per SIMD for the wide windows: their cost phase is fp64-bound
    constexpr int NCW = NT / 64 - 1;          // cost waves: 1 .. NCW (wave 0 walks the previous window's path meanwhile)
    extern __shared__ __align__(16) unsigned char wtw_smem[];
    const int W = g.W, ldc = win_ldc(W);
    const int b = blockIdx.x, tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    int32_t *sh = reinterpret_cast<int32_t *>(wtw_smem);                          // [32] control words
    double *C = reinterpret_cast<double *>(wtw_smem + 128) + kWinPadFront;        // [W][ldc]
    double *xs = C + (size_t)W * ldc + kWinPadBack;                               // [W][F] live window (row i staged by wave 1 + i % NCW)
    double *nx = xs + (size_t)W * kWF;                                            // [W]
    uint32_t *codes = reinterpret_cast<uint32_t *>(nx + W);                       // [2][kWinKW][64]
    double *row0 = reinterpret_cast<double *>(codes + 2 * kWinKW * 64);           // [W + 16] D[0][:]
    double *col0 = row0 + W + 16;                                                 // [W + 16] D[:][0]
    double *bot = col0 + W + 16 + kWinBotFront;                                   // [W] D[64][:] (wave 0's last row), padded
    double *bot_dummy = bot + W + kWinBotBack;                                    // [80]
    int32_t *botx = reinterpret_cast<int32_t *>(bot_dummy + kWinBotDummy) + kWinBotFront;  // [W] ... and its crossing columns, padded
    int32_t *botx_dummy = botx + W + kWinBotBack;                                 // [80]
    int32_t *sub = botx_dummy + kWinBotDummy;                                     // [2W][2], reversed
    // the int32 run botx .. sub in front of ypre is 5 W + kWinBotPad words: one more for odd W keeps the doubles on 8 bytes
    static_assert(kWinBotPad % 2 == 0, "wtw_win_kernel: the constant part of the int32 run in front of ypre must be an even count");
    double *ypre = reinterpret_cast<double *>(sub + 4 * (size_t)W + (W & 1));    // [kWinPrefN][F] reference frames pref_rp .. (W <= kWinPrefW)
    double *nypre = ypre + kWinPrefN * kWF;                                       // [kWinPrefN] their norms

    int32_t *st = g.state + (size_t)b * 8;
    const double *live = g.live + (size_t)b * g.live_stride * kWF;
    int32_t *path = g.path + (size_t)b * g.path_cap * 2;
    const WtwRef sr = wtw_ref(g, b);
    const int appended_raw = g.appended[b];
    const int appended = appended_raw < sr.N ? appended_raw : sr.N;
    // state in registers (uniform: every thread computes the same values; n_path is kept by wave 0 only)
    int chroma_ptr = st[0], live_ptr = st[1], ref_ptr = st[2], status = st[3], n_path = st[4], n_windows = st[5];
    long long cells = ((long long)(uint32_t)st[7] << 32) | (uint32_t)st[6];
    // the window whose path wave 0 still has to walk: its pointers and where the walk starts
    int have_prev = 0, plp = 0, prp = 0, pwi = 0, pwj = 0;
    int have_pref = 0, pref_lp = 0, pref_rp = 0;  // what the cost waves fetched during the last DP phase
    const int h = g.hopf;

    for (;;) {
        // ---- wtw.py:92-100 in closed form up to the next window (see wtw_ctl_body)
        int pending = 0, m = 0;
        const int n = W;
        if (status == RTS_RUNNING && chroma_ptr < appended) {
            if (ref_ptr >= (sr.M - 1 - W) || live_ptr >= (sr.N - 1 - W)) {
                chroma_ptr += 1;
                status = RTS_STOP_REF_END;
            } else if (live_ptr + W <= appended) {
                chroma_ptr = live_ptr + W;
                m = W;
                if (ref_ptr + m > sr.M) m = sr.M - ref_ptr;
                pending = m > 0 ? 1 : 0;
                if (!pending) chroma_ptr = appended;
            } else {
                chroma_ptr = appended;
            }
        }
        if (!pending && !have_prev) break;
        const int lp = live_ptr, rp = ref_ptr;
#ifdef RTS_WIN_STAMPS
        long long stamp_t = (long long)__builtin_amdgcn_s_memtime();
#endif
        // ---- A. wave 0: path + hand-over of the previous window; waves 1..: this window's cost matrix
        if (wave == 0) {
            if (have_prev) {
#ifdef RTS_WIN_STAMPS
                const long long w0_ = (long long)__builtin_amdgcn_s_memtime();
#endif
                // find_path (wtw.py:219-240) from the last point that is handed over back to (0, 0); sub[] holds it reversed
                int i = pwi, j = pwj, len = 1;
                if (lane == 0) {
                    sub[0] = i;
                    sub[1] = j;
                }
                int cur = -1;
                uint32_t cw = 0;
                while (i > 0 && j > 0) {  // interior cells: the code of (i, j) is bit pair t & 15 of word t >> 4 of lane (i-1) & 63
                    const int l = (i - 1) & 63;
                    const int t = l + j - 1;
                    const int key = ((i - 1) >> 6) * kWinKW + (t >> 4);
                    if (key != cur) {  // uniform
                        cw = codes[(size_t)key * 64 + lane];
                        cur = key;
                    }
                    const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)cw, l);
                    const int code = (int)((w >> (2 * (t & 15))) & 3u);
                    i -= (code != sdp::kLeft) ? 1 : 0;   // kUp, kDiag
                    j -= (code != sdp::kUp) ? 1 : 0;     // kLeft, kDiag
                    if (lane == 0) {
                        sub[2 * len] = i;
                        sub[2 * len + 1] = j;
                    }
                    len++;
                }
                // on row 0 the path runs left, on column 0 up (wtw.py:187-198): the rest is a straight line to (0, 0)
                const int rest = i + j;  // one of them is 0
                for (int q = lane; q < rest; q += 64) {
                    sub[2 * (len + q)] = i > 0 ? i - 1 - q : 0;
                    sub[2 * (len + q) + 1] = j > 0 ? j - 1 - q : 0;
                }
                len += rest;
                // hand-over (wtw.py:107-117): every walked point has l <= dtw_hop / hop; forwards
                for (int f = lane; f < len; f += 64) {
                    if (n_path + f < g.path_cap) {
                        path[2 * (size_t)(n_path + f)] = sub[2 * (len - 1 - f)] + plp;
                        path[2 * (size_t)(n_path + f) + 1] = sub[2 * (len - 1 - f) + 1] + prp;
                    }
                }
                n_path += len;
#ifdef RTS_WIN_STAMPS
                if (b == 0 && lane == 0) g_win_stamps[3] += (long long)__builtin_amdgcn_s_memtime() - w0_;
#endif
            }
        } else if (pending) {
#ifdef RTS_WIN_STAMPS
            const long long c0_ = (long long)__builtin_amdgcn_s_memtime();
#endif
            const int cwv = wave - 1;
            double y0[kWF], y1[kWF];
            double ny0;
            const int nrows = (n - cwv + NCW - 1) / NCW;
            // (uniform) everything this window needs was fetched during the previous window's DP phase
            const bool pref = (R == 1) && W <= kWinPrefW && have_pref && lp == pref_lp && rp >= pref_rp && rp - pref_rp + m <= kWinPrefN;
            if (pref) {
                const int off = rp - pref_rp + (lane < m ? lane : m - 1);
#pragma unroll
                for (int f = 0; f < kWF; f++) y0[f] = ypre[off * kWF + f];
                ny0 = nypre[off];
            } else {
                // my columns' reference frames first (their latency hides behind the staging of the rows)
                sdp::load_frame(sr.ref, 1, (long long)rp + (lane < m ? lane : m - 1), y0);
                if (m > 64) sdp::load_frame(sr.ref, 1, (long long)rp + (64 + lane < m ? 64 + lane : m - 1), y1);
                // my rows (cwv, cwv + NCW, ...) into my slice of xs / nx: wave-private, no barrier
                for (int q = lane; q < nrows * kWF; q += 64) {
                    const int row = cwv + NCW * (q / kWF);
                    xs[row * kWF + q % kWF] = live[(size_t)(lp + row) * kWF + q % kWF];
                }
                for (int q = lane; q < nrows; q += 64) {
                    const int row = cwv + NCW * q;
                    double x[kWF];
#pragma unroll
                    for (int f = 0; f < kWF; f++) x[f] = xs[row * kWF + f];
                    nx[row] = sdp::WtwPolicy::norm(x);
                }
                ny0 = sdp::WtwPolicy::norm(y0);
            }
            const double ny1 = (m > 64) ? sdp::WtwPolicy::norm(y1) : 1.0;
            for (int i = cwv; i < n; i += NCW) {
                double x[kWF];
#pragma unroll
                for (int f = 0; f < kWF; f++) x[f] = xs[i * kWF + f];  // wave-uniform: a broadcast
                const double nxi = nx[i];
                const double c0 = sdp::WtwPolicy::cost(x, nxi, y0, ny0);  // wtw.py:169
                if (lane < m) C[(size_t)i * ldc + lane] = c0;
                if (m > 64) {
                    const double c1 = sdp::WtwPolicy::cost(x, nxi, y1, ny1);
                    if (64 + lane < m) C[(size_t)i * ldc + 64 + lane] = c1;
                }
            }
#ifdef RTS_WIN_STAMPS
            if (b == 0 && tid == 64) g_win_stamps[4] += (long long)__builtin_amdgcn_s_memtime() - c0_;
#endif
        }
        __syncthreads();
        RTS_WIN_STAMP(0);
        if (!pending) {  // that was the last window's path
            have_prev = 0;
            continue;
        }
        // ---- B. row 0 (lane 0) and column 0 (lane 1) of D: running sums in the reference's order (wtw.py:183-198).  16
        // costs per LDS round trip, then 16 dependent adds; the stores run up to 15 elements past the end (the arrays
        // are padded for it), so nothing in the loop depends on the element count
        if (wave == 0 && lane < 2) {
            const int cnt = lane == 0 ? m : n;
            const double *src = C;
            const int stride = lane == 0 ? 1 : ldc;
            double *out = lane == 0 ? row0 : col0;
            double acc = 0.0;
            for (int q0 = 0; q0 < cnt; q0 += 16) {
                double v[16];
#pragma unroll
                // (past the end: row 0 into the padding behind C; column 0 up to 15 rows -- 15 ldc doubles -- past C,
                // into xs / nx / codes, all inside this workgroup's LDS: read and never used)
                for (int q = 0; q < 16; q++) v[q] = src[q * stride];
                src += 16 * stride;
                if (q0 == 0) {
                    acc = v[0];
                    out[0] = acc;
#pragma unroll
                    for (int q = 1; q < 16; q++) {
                        acc = acc + v[q];
                        out[q] = acc;
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < 16; q++) {
                        acc = acc + v[q];
                        out[q] = acc;
                    }
                }
                out += 16;
            }
        }
        __syncthreads();
        if (STAGE) {
            double *dl = g.dlast + (size_t)b * W * W;
            for (int q = tid; q < m; q += NT) dl[q] = row0[q];
            for (int q = tid; q < n; q += NT) dl[(size_t)q * W] = col0[q];
        }
        RTS_WIN_STAMP(1);
        // ---- C. interior DP: lane l of wave r owns row 1 + 64 r + l, column 1 + t - l at local step t
        const bool has_cross = h + 1 <= n - 1;  // the path goes below row h: wtw.py:118-124's "change"
        if (R == 1 && W <= kWinPrefW && wave >= 1) {  // the idle cost waves: what the next window's cost phase will read (see kWinPrefW)
            const int cwv = wave - 1, nlp = lp + h;
            const int nrows = (n - cwv + NCW - 1) / NCW;
            for (int q = lane; q < nrows * kWF; q += 64) {
                const int row = cwv + NCW * (q / kWF);
                const int fr = (nlp + row < sr.N) ? nlp + row : sr.N - 1;
                xs[row * kWF + q % kWF] = live[(size_t)fr * kWF + q % kWF];
            }
            for (int q = lane; q < nrows; q += 64) {
                const int row = cwv + NCW * q;
                double x[kWF];
#pragma unroll
                for (int f = 0; f < kWF; f++) x[f] = xs[row * kWF + f];
                nx[row] = sdp::WtwPolicy::norm(x);
            }
            if (wave <= 2) {  // waves 1 and 2: 64 reference frames each
                const int slot = 64 * (wave - 1) + lane;
                double yv[kWF];
                sdp::load_frame(sr.ref, 1, (long long)((rp + slot < sr.M) ? rp + slot : sr.M - 1), yv);
#pragma unroll
                for (int f = 0; f < kWF; f++) ypre[slot * kWF + f] = yv[f];
                nypre[slot] = sdp::WtwPolicy::norm(yv);
            }
        }
        {
            const int r = wave;
            const int nint = n - 1, mint = m - 1;                       // interior rows / columns
            const int rows = (r < R) ? ((nint - 64 * r) < 64 ? (nint - 64 * r) : 64) : 0;
            const int T = (rows > 0 && mint > 0) ? rows + mint - 1 : 0;
            const int blocks = (T + 15) >> 4;
            const int T0 = (nint > 0 && mint > 0) ? (nint < 64 ? nint : 64) + mint - 1 : 0;
            const int T1 = (nint > 64 && mint > 0) ? (nint - 64) + mint - 1 : 0;
            const int rounds0 = (T0 + 15) >> 4, rounds1 = T1 > 0 ? 5 + ((T1 + 15) >> 4) : 0;
            const int rounds_all = (R == 1 || rounds0 > rounds1) ? rounds0 : rounds1;
            const int i = 1 + 64 * r + lane;
            const int ic = i < n ? i : n - 1;
            // D[i][0] and D[i-1][0]: what the first interior step of this lane sees as `left` and `diag`
            double dlast_v = col0[ic], du_prev = col0[ic - 1 >= 0 ? ic - 1 : 0];
            // crossing columns: column 0 is left through (h, 0)
            int xl = 0, xu_prev = 0;
            const bool is_h1 = (i == h + 1);
            const double *upin = (r == 0) ? row0 : bot;                  // the row above this wave's lane 0
            double *dout = STAGE ? g.dlast + ((size_t)b * W + ic) * W : nullptr;
            const double *crow = C + (size_t)ic * ldc + 1 - lane;         // crow[t] = C[i][1 + t - lane]
            const bool short_tail = (R == 1) && blocks > 0 && (T - 16 * (blocks - 1) <= 8);  // wave-uniform
            const int loop_rounds = short_tail ? rounds_all - 1 : rounds_all;
            for (int k = 0; k < loop_rounds; k++) {
                if (R > 1) lds_barrier();  // wave 1 reads bottom-row values wave 0 wrote at least one round ago
                const int kb = k - 5 * r;
                if (kb < 0 || kb >= blocks) continue;  // wave-uniform
#ifdef RTS_WIN_STAMPS
                const long long blk_t0_ = (long long)__builtin_amdgcn_s_memtime();
#endif
                uint32_t word = 0;
                if (R > 1 && r > 0) RTS_WIN_DP_BLOCK(true, 16) else RTS_WIN_DP_BLOCK(false, 16)
                codes[((size_t)r * kWinKW + kb) * 64 + lane] = word;
#ifdef RTS_WIN_STAMPS
                if (b == 0 && lane == 0 && r < 2) g_win_stamps[6 + r] += (long long)__builtin_amdgcn_s_memtime() - blk_t0_;  // a DP wave's own block time
#endif
            }
            if (short_tail) {  // one DP wave: a last block of at most 8 steps runs as 8 (tests.py:174's 20-frame windows sweep 37 steps)
                const int kb = blocks - 1;
                uint32_t word = 0;
                RTS_WIN_DP_BLOCK(false, 8)
                codes[((size_t)r * kWinKW + kb) * 64 + lane] = word;
            }
            if (r < R && lane < rows && i == n - 1) sh[2] = xl;  // the last cell's crossing column
        }
        __syncthreads();
        RTS_WIN_STAMP(2);
        // ---- the next window's pointers (wtw.py:118-128), and what wave 0 walks during the next phase A
        const int xstar = (has_cross && m > 1) ? sh[2] : 0;  // (m == 1: the path is column 0)
        have_pref = (R == 1 && W <= kWinPrefW) ? 1 : 0;
        pref_lp = lp + h;
        pref_rp = rp;
        plp = lp;
        prp = rp;
        pwi = has_cross ? h : n - 1;
        pwj = has_cross ? xstar : m - 1;
        have_prev = 1;
        live_ptr = lp + h;
        ref_ptr = rp + (has_cross ? xstar : h);
        n_windows += 1;
        cells += (long long)n * m;
#ifdef RTS_WIN_STAMPS
        if (b == 0 && tid == 0) g_win_stamps[5] += 1;
#endif
    }
    if (status == RTS_RUNNING && chroma_ptr >= sr.N && appended_raw > sr.N) status = RTS_LIVE_OVERFLOW;
    if (tid == 0) {
        st[0] = chroma_ptr;
        st[1] = live_ptr;
        st[2] = ref_ptr;
        st[3] = status;
        st[4] = n_path;
        st[5] = n_windows;
        st[6] = (int32_t)(uint32_t)(cells & 0xffffffffLL);
        st[7] = (int32_t)(uint32_t)((unsigned long long)cells >> 32);
    }
}

// ---- windows of more than kWinW frames (from 65 with RTS_WTW_WIN=0): strip DP over many workgroups (sdp.h) ---------

// H helper waves per strip: <.., 2> two strips per workgroup, <.., 3> one strip per workgroup (sdp::pick_config).
template <bool STAGE, int H>
__global__ void __launch_bounds__(H == 2 ? 384 : 256) wtw_big_dp_kernel(WtwArgs g) {
    extern __shared__ __align__(16) unsigned char wtw_smem[];
    const int b = blockIdx.y;
    const int32_t *ctl = g.ctl + (size_t)b * 8;
    if (ctl[0] == 0) return;  // no window pending for this stream
    const int lp = ctl[1];
    sdp::Problem pb;
    pb.x = g.live + ((size_t)b * g.live_stride + lp) * kWF;  // rows: the live window (wtw.py:101)
    pb.x_f64 = 1;
    pb.yrec = g.yrec + (size_t)b * g.W * sdp::kYRec;  // columns: the reference window (wtw.py:102), prepared by ctl
    pb.M = ctl[3];
    pb.N = ctl[4];
    pb.D = STAGE ? g.dlast + (size_t)b * g.W * g.W : nullptr;
    pb.ldD = g.W;
    pb.codes = g.codes + (size_t)b * sdp::codes_words(g.W, g.W);
    pb.bnd = g.bnd + (size_t)b * sdp::n_strips(g.W) * g.W;
    pb.entb = g.entb + (size_t)b * sdp::n_strips(g.W) * g.W;
    pb.err = g.err;
    sdp::for_each_rowgroup(g.ticket + b, g.n_rg, g.n_strips_wg, wtw_smem, [&](int rg) {
        sdp::run_rowgroup<sdp::WtwPolicy, STAGE, H>(pb, rg, g.n_rg, g.n_strips_wg, wtw_smem);
    });
}

// find_path (wtw.py:219-240) for the pending window of each stream, over the packed step codes (sdp.h): the
// strip-boundary crossings, then every strip's segment by its own wave -- count, then write -- into ws_sub,
// forward-ordered; ctl[5] receives the sub-path's length.
__global__ void __launch_bounds__(64) wtw_big_hops_kernel(WtwArgs g) {
    __shared__ uint32_t win[2 * sdp::kBtChunks * 64];
    const int b = blockIdx.x, S = sdp::n_strips(g.W);
    const int32_t *ctl = g.ctl + (size_t)b * 8;
    if (ctl[0] == 0) return;
    sdp::path_hops(g.codes + (size_t)b * sdp::codes_words(g.W, g.W), g.entb + (size_t)b * S * g.W, ctl[3], ctl[4],
                   g.cross + (size_t)b * S, win);
}

template <int PASS>
__global__ void __launch_bounds__(64) wtw_big_segment_kernel(WtwArgs g) {
    __shared__ uint32_t win[2 * sdp::kBtChunks * 64];
    const int b = blockIdx.y, s = blockIdx.x, S = sdp::n_strips(g.W);
    int32_t *ctl = g.ctl + (size_t)b * 8;
    if (ctl[0] == 0 || s >= sdp::n_strips(ctl[3])) return;
    sdp::path_segment(g.codes + (size_t)b * sdp::codes_words(g.W, g.W), ctl[3], ctl[4], s, g.cross + (size_t)b * S,
                      g.lens + (size_t)b * S, PASS, g.ws_sub + (size_t)b * 4 * g.W, ctl + 5, win,
                      g.ws_scr + (size_t)b * 2 * sdp::scratch_pairs(g.W, g.W));
}

// Hands a window to the DP launch that follows: its boundary words start as "not written", and its reference columns
// become float64 records with their norms.  `tid` of `nt` threads share the work.
__device__ __forceinline__ void wtw_window_handover(const WtwArgs &g, int b, int ref_ptr, int nm, size_t tid, size_t nt) {
    const int W = g.W;
    const WtwRef sr = wtw_ref(g, b);
    unsigned long long *bnd = g.bnd + (size_t)b * sdp::n_strips(W) * W;
    const size_t words = (size_t)(g.n_rg > 1 ? g.n_rg - 1 : 0) * nm;
    for (size_t k = tid; k < words; k += nt) bnd[k] = sdp::kSentinel;
    for (size_t col = tid; col < (size_t)nm; col += nt)
        sdp::prep_column<sdp::WtwPolicy>(sr.ref, 1, (long long)ref_ptr + (long long)col,
                                         g.yrec + (size_t)b * W * sdp::kYRec - (size_t)ref_ptr * sdp::kYRec);
}

// Long windows (W = 10 000: 12.5 MB of boundary words): the hand-over by many workgroups instead of the control
// kernel's one -- after it, reading the window it has just announced in ctl[].
__global__ void __launch_bounds__(256) wtw_big_fill_kernel(WtwArgs g) {
    const int b = blockIdx.y;
    const int32_t *ctl = g.ctl + (size_t)b * 8;
    if (ctl[0] == 0) return;
    wtw_window_handover(g, b, ctl[2], ctl[4], (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}

// One workgroup per stream.  If a window is pending (its sub-path was just written by the kernels above): the
// hand-over (wtw.py:107-128).  Then the column bookkeeping of wtw.py:92-100 in closed
// form up to the next event: between two windows the stop test (wtw.py:96) sees constant pointers, and a window
// fires exactly when chroma_ptr reaches live_ptr + W.
__device__ __forceinline__ void wtw_ctl_body(const WtwArgs &g) {
    __shared__ int s_cnt;
    const int b = blockIdx.x, tid = threadIdx.x, NT = blockDim.x;
    const int W = g.W;
    int32_t *st = g.state + (size_t)b * 8;
    int32_t *ctl = g.ctl + (size_t)b * 8;
    int32_t *sub = g.ws_sub + (size_t)b * 4 * W;
    int32_t *path = g.path + (size_t)b * g.path_cap * 2;
    const int pending = ctl[0];
    int lp = ctl[1], rp = ctl[2];
    const int n = ctl[3], m = ctl[4];
    int live_ptr = st[1], ref_ptr = st[2], n_path = st[4];
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    if (pending) {
        // sub[] holds the path from (0, 0) to (n-1, m-1); l is non-decreasing along it, so the points handed over
        // (l <= dtw_hop / hop, wtw.py:113) are a prefix of it
        // (written by another wave of this workgroup when the backtrack ran in the same launch: not through L1)
        int len = __hip_atomic_load(ctl + 5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        len = len < 1 ? 1 : (len > 2 * W ? 2 * W : len);
        int local = 0;
        for (int q = tid; q < len; q += NT) local += (sub[2 * q] <= g.hopf) ? 1 : 0;
        if (local) atomicAdd(&s_cnt, local);
        __syncthreads();
        const int cnt = s_cnt;
        for (int f = tid; f < cnt; f += NT) {
            if (n_path + f < g.path_cap) {
                path[2 * (size_t)(n_path + f)] = sub[2 * f] + lp;
                path[2 * (size_t)(n_path + f) + 1] = sub[2 * f + 1] + rp;
            }
        }
        if (cnt < len && cnt >= 1) {  // "change": the path went past the hop (wtw.py:118-124)
            live_ptr = lp + sub[2 * (cnt - 1)];  // the last appended point
            ref_ptr = rp + sub[2 * (cnt - 1) + 1];
        } else {
            live_ptr = lp + g.hopf;
            ref_ptr = rp + g.hopf;
        }
        n_path += cnt;
    }
    __syncthreads();
    // ---- bookkeeping up to the next event (uniform across the workgroup: everything below depends on state only)
    const WtwRef sr = wtw_ref(g, b);
    const int appended_raw = g.appended[b];
    const int appended = appended_raw < sr.N ? appended_raw : sr.N;
    int chroma_ptr = st[0], status = st[3], n_windows = st[5];
    long long cells = ((long long)(uint32_t)st[7] << 32) | (uint32_t)st[6];
    if (pending) {
        n_windows += 1;
        cells += (long long)n * m;
    }
    int next_pending = 0, nn = 0, nm = 0;
    if (status == RTS_RUNNING && chroma_ptr < appended) {
        if (ref_ptr >= (sr.M - 1 - W) || live_ptr >= (sr.N - 1 - W)) {
            chroma_ptr += 1;  // wtw.py:92-97: the next column trips the boundary check
            status = RTS_STOP_REF_END;
        } else if (live_ptr + W <= appended) {
            chroma_ptr = live_ptr + W;  // the column that completes the window (wtw.py:100)
            nn = W;
            nm = W;
            if (ref_ptr + nm > sr.M) nm = sr.M - ref_ptr;  // numpy slice truncation of chroma_ref[:, rp:rp+W]
            next_pending = nm > 0 ? 1 : 0;
            if (!next_pending) chroma_ptr = appended;  // unreachable (wtw.py:96 stops first); never stall
        } else {
            chroma_ptr = appended;
        }
    }
    if (!next_pending && status == RTS_RUNNING && chroma_ptr >= sr.N && appended_raw > sr.N) status = RTS_LIVE_OVERFLOW;
    if (next_pending && !g.fill_separate) wtw_window_handover(g, b, ref_ptr, nm, tid, NT);
    __syncthreads();
    if (tid == 0) {
        st[0] = chroma_ptr;
        st[1] = live_ptr;
        st[2] = ref_ptr;
        st[3] = (*g.err != 0 && status == RTS_RUNNING) ? RTS_DEVICE_FAULT : status;
        st[4] = n_path;
        st[5] = n_windows;
        st[6] = (int32_t)(uint32_t)(cells & 0xffffffffLL);
        st[7] = (int32_t)(uint32_t)((unsigned long long)cells >> 32);
        g.ticket[b] = 0;  // the DP launch that follows hands its row groups out from 0 again
        ctl[0] = next_pending;
        ctl[1] = live_ptr;
        ctl[2] = ref_ptr;
        ctl[3] = nn;
        ctl[4] = nm;
    }
}

__global__ void __launch_bounds__(1024) wtw_big_ctl_kernel(WtwArgs g) { wtw_ctl_body(g); }

// Backtrack (if a window is pending) and control step in one launch, for windows of at most sdp::kTailStrips strips.
__global__ void __launch_bounds__(64 * sdp::kTailStrips) wtw_big_tail_ctl_kernel(WtwArgs g) {
    extern __shared__ __align__(16) unsigned char wtw_smem[];
    const int b = blockIdx.x, S = sdp::n_strips(g.W);
    int32_t *ctl = g.ctl + (size_t)b * 8;
    if (ctl[0] != 0)  // uniform over the workgroup
        sdp::path_tail(g.codes + (size_t)b * sdp::codes_words(g.W, g.W), g.entb + (size_t)b * S * g.W, ctl[3], ctl[4],
                       g.cross + (size_t)b * S, g.lens + (size_t)b * S, g.ws_sub + (size_t)b * 4 * g.W, ctl + 5,
                       reinterpret_cast<uint32_t *>(wtw_smem), g.ws_scr + (size_t)b * 2 * sdp::scratch_pairs(g.W, g.W));
    __syncthreads();
    wtw_ctl_body(g);
}

// wtw.py:76-77: the check made at the top of insert(), before any column is processed.
__global__ void wtw_precheck_kernel(int32_t *state, int B, int M, const int32_t *ref_len) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int Mb = ref_len ? ref_len[b] : M, Nb = 2 * Mb;  // this stream's M and N = 2M (wtw.py:52)
    int32_t *st = state + (size_t)b * 8;
    if (st[3] == RTS_RUNNING && (st[2] >= Mb - 1 || st[1] >= Nb - 1)) st[3] = RTS_STOP_REF_END;
}

// Append n_new[b] columns from cols [B][n_max][F] to the live history; columns beyond the 2M capacity
// are dropped (the reference would raise IndexError at that column) and reported as status
// LIVE_OVERFLOW by the window / control kernel once it has walked the columns that did fit.
// grid (B, slices): a push of a whole recording is 200 KB per stream, so several workgroups share a stream's copy.  Every
// slice reads the old count from `appended`; slice 0 writes the new one to `appended_next`, and the host swaps the two
// arrays after the launch (the kernels that follow read the new one).  N is the history stride: with per-stream references
// 2 M_max, and the kernels that walk the columns apply a stream's own capacity 2 M_b.
constexpr int kWtwAppendSlices = 8;
__global__ void wtw_append_kernel(double *live, int32_t *appended, int32_t *appended_next, int32_t *state, const void *cols,
                                  int cols_f64, const int32_t *n_new, int n_uniform, int n_max, int B, int N) {
    const int b = blockIdx.x;
    if (b >= B) return;
    int nn = n_new ? n_new[b] : n_uniform;
    nn = nn < 0 ? 0 : (nn > n_max ? n_max : nn);  // never read a neighbouring stream's columns
    const int base_raw = appended[b];
    const int base = base_raw < N ? base_raw : N;
    const int running = state[(size_t)b * 8 + 3] == RTS_RUNNING;
    int take = nn;
    if (base + take > N) take = N - base > 0 ? N - base : 0;
    if (blockIdx.y == 0 && threadIdx.x == 0)
        appended_next[b] = (!running || nn <= 0) ? base_raw : ((take < nn) ? N + 1 : base + take);  // N+1: a column was dropped
    if (!running) return;  // sticky stop: later columns are ignored
    const int total = take * kWF;
    const int per = (total + gridDim.y - 1) / gridDim.y;
    const int lo = blockIdx.y * per, hi = (lo + per < total) ? lo + per : total;
    for (int idx = lo + threadIdx.x; idx < hi; idx += blockDim.x) {
        const size_t src = ((size_t)b * n_max) * kWF + idx;
        const double v = cols_f64 ? reinterpret_cast<const double *>(cols)[src]
                                  : (double)reinterpret_cast<const float *>(cols)[src];
        live[((size_t)b * N + base) * kWF + idx] = v;
    }
}

// rts_wtw_restart: what rts_wtw_reset does, for the selected streams only; grid (slices, sel.n).  The state words, the
// appended count (the array the next push reads; that push writes every entry of the other one), the stream's slice of
// the live history (zeros again, wtw.py:55), its control and ticket words of the strip-DP pipeline and, when the stream
// moves to another piece, its row of the reference tables.  Everything else a window needs (column records, boundary
// words, step codes) is rebuilt by the hand-over of every window.  Other streams' words are not written.
__global__ void __launch_bounds__(256) wtw_restart_kernel(RestartSel sel, int32_t *state, int32_t *appended, double *live,
                                                          long long live_per_stream, int32_t *ctl, int32_t *ticket,
                                                          long long *ref_first, int32_t *ref_len) {
    if ((int)blockIdx.y >= sel.n) return;
    const int b = sel.idx[blockIdx.y];
    double *lv = live + (long long)b * live_per_stream;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < live_per_stream; i += stride) lv[i] = 0.0;
    if (blockIdx.x == 0 && threadIdx.x < 8) {
        state[(size_t)b * 8 + threadIdx.x] = 0;
        if (ctl) ctl[(size_t)b * 8 + threadIdx.x] = 0;
        if (threadIdx.x == 0) {
            appended[b] = 0;
            if (ticket) ticket[b] = 0;
            if (sel.set_ref) {
                ref_first[b] = sel.first[blockIdx.y];
                ref_len[b] = sel.len[blockIdx.y];
            }
        }
    }
}

// rts_wtw_recent: the last min(M_max, n) columns of stream b's live chroma history into out[b], zeros behind them; one
// workgroup per stream.  n is the appended count capped at the stream's own capacity 2 M_b (the count reads past the
// history stride when a column was dropped).  Nothing the tracker owns is written.
__global__ void __launch_bounds__(256) wtw_recent_kernel(const double *live, const int32_t *appended, int live_stride, int M,
                                                         const int32_t *ref_len, int M_max, double *out, int32_t *len_out,
                                                         const uint8_t *mask) {
    const int b = blockIdx.x;
    const int cap = 2 * (ref_len ? ref_len[b] : M);
    int n = appended[b];
    n = n < 0 ? 0 : n;
    n = n > cap ? cap : n;
    n = n > live_stride ? live_stride : n;
    const int len = (mask && !mask[b]) ? 0 : (n < M_max ? n : M_max);
    const long long src0 = ((long long)b * live_stride + (n - len)) * kWF;
    double *dst = out + (size_t)b * M_max * kWF;
    for (int idx = threadIdx.x; idx < M_max * kWF; idx += blockDim.x) dst[idx] = idx < len * kWF ? live[src0 + idx] : 0.0;
    if (threadIdx.x == 0) len_out[b] = len;
}

}  // namespace rts

// One launch signature for every kernel that takes the handle's arguments.
typedef void (*rts_wtw_kernel)(rts::WtwArgs);

struct rts_wtw {
    rts::WtwArgs args;   // every buffer and size of the handle: what the kernels are launched with
    rts::RefTable refs;  // per-stream references (rts_wtw_create_refs): owns args.ref_first / args.ref_len
    int B;
    int device;  // the HIP device the handle's buffers live on
    // decided at create (wtw_select): the strip DP (dp != NULL) or the window kernel (win != NULL)
    rts_wtw_kernel dp;    // wtw_big_dp_kernel<STAGE, H> for this handle's keep_last_d and helper count
    rts_wtw_kernel win;   // wtw_win_kernel<R, STAGE> for its DP waves and keep_last_d
    rts::sdp::Plan plan;  // of `dp` (plan.grid x B workgroups; args.n_rg / n_strips_wg repeat it) or `win` (B workgroups)
    void *sdp_ws;         // the strip DP's workspace, one allocation: what args.err .. args.ticket point into (sdp_plan.h)
};

namespace rts {

// Which kernels serve windows of W frames: wtw_win_kernel up to kWinW (128) frames, the strip DP above.  (Measured on 64
// streams, hop = W / 2: the window kernel is on a par with the strip DP's launch-per-window rounds at W = 100 and ahead
// of them below.)  The knobs (tests and A/B runs; results do not depend on them): RTS_WTW_WIN=0 sends windows of 65 to
// kWinW frames to the strip DP, which keeps its one- and two-strip forms covered -- windows of at most kWinOnlyW frames
// run on the window kernel whatever is set; RTS_WIN_FORCE_R2, two DP waves in the window kernel at any W.
constexpr int kWinOnlyW = 64;
// Returns the DP waves of wtw_win_kernel (interior rows 1 .. W-1: one wave up to 65 frames), 0 for the strip DP.
static int wtw_select(int W) {
    const char *win_e = getenv("RTS_WTW_WIN"), *r2_e = getenv("RTS_WIN_FORCE_R2");
    if (W > kWinW || (W > kWinOnlyW && win_e && atoi(win_e) == 0)) return 0;
    return (W <= 65 && !r2_e) ? 1 : 2;
}

// The instantiations, [STAGE][...]: all of them ask for more dynamic LDS than the default limit (raised at create).
static const rts_wtw_kernel kWtwDpKernels[2][2] = {{wtw_big_dp_kernel<false, 3>, wtw_big_dp_kernel<false, 2>},  // [helpers == 2]
                                                   {wtw_big_dp_kernel<true, 3>, wtw_big_dp_kernel<true, 2>}};
static const rts_wtw_kernel kWtwWinKernels[2][2] = {{wtw_win_kernel<1, false>, wtw_win_kernel<2, false>},  // [DP waves - 1]
                                                    {wtw_win_kernel<1, true>, wtw_win_kernel<2, true>}};

// The constructor behind rts_wtw_create (first_host == NULL: one reference of M frames) and rts_wtw_create_refs (M =
// M_max, per-stream tables of B entries, already checked).  Every argument is checked before the first HIP call.
static int wtw_create(const double *chroma_ref_dev, int F, int M, int B, int win_frames, int hop_frames, int keep_last_d,
                      const long long *first_host, const int32_t *len_host, rts_wtw **out) {
    if (F < 1) return set_error(RTS_ERR_INVALID, "F must be >= 1 (got %d)", F);
    if (F != kWF) return set_error(RTS_ERR_UNSUPPORTED, "F must be 12 chroma bins (got %d)", F);
    if (M < 1 || B < 1) return set_error(RTS_ERR_INVALID, "M and B must be >= 1");
    if (win_frames < 1) return set_error(RTS_ERR_INVALID, "dtw_win_size / hop_size must be >= 1 frame");
    if (hop_frames < 1)
        return set_error(RTS_ERR_INVALID, "dtw_hop_size / hop_size must be >= 1 frame (the reference loops forever at 0)");
    if (win_frames > kWtwMaxW)
        return set_error(RTS_ERR_UNSUPPORTED, "window of %d frames exceeds the supported %d", win_frames, kWtwMaxW);
    rts_wtw *h = (rts_wtw *)calloc(1, sizeof(rts_wtw));
    if (!h) return set_error(RTS_ERR_INVALID, "out of host memory");
    WtwArgs &g = h->args;
    g.ref = chroma_ref_dev;
    if (hipError_t ed = hipGetDevice(&h->device); ed != hipSuccess) {
        free(h);
        return set_error(RTS_ERR_HIP, "hipGetDevice failed: %s", hipGetErrorString(ed));
    }
    g.M = M;
    g.live_stride = 2 * M;  // wtw.py:52
    h->B = B;
    g.W = win_frames;
    g.hopf = hop_frames;
    g.path_cap = (g.live_stride / hop_frames + 2) * (win_frames + hop_frames + 2);
    const int W = win_frames;
    const int win_waves = wtw_select(W);
    const bool big = win_waves == 0, stage = keep_last_d != 0;
    hipError_t e = hipSuccess;
    if (big) {
        // once per handle, so without sdp::launch_plan's residency cache: the occupancy queries are made at every create
        const int rc = sdp::launch_plan(kWtwDpKernels[stage][0], kWtwDpKernels[stage][1], sdp::n_strips(W), B, nullptr, &h->plan, &h->dp);
        if (rc != RTS_OK) {
            free(h);
            return rc;
        }
        g.n_strips_wg = h->plan.NS;
        g.n_rg = h->plan.n_rg;
        g.fill_separate = ((size_t)(g.n_rg > 1 ? g.n_rg - 1 : 0) * W > (1u << 16)) ? 1 : 0;  // more than 0.5 MB of boundary words
    } else {
        h->win = kWtwWinKernels[stage][win_waves - 1];
        h->plan.grid = B;
        h->plan.block = win_waves == 1 ? 256 : 512;
        h->plan.smem = win_lds_bytes(W);
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(h->win), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    }
    if (e != hipSuccess) {
        free(h);
        return set_error(RTS_ERR_HIP, "WTW allocation failed: %s", hipGetErrorString(e));
    }
    const size_t nB = (size_t)B;
    const struct {
        bool wanted;
        void **buf;
        size_t bytes;
    } allocs[] = {
        {true, (void **)&g.live, sizeof(double) * kWF * (size_t)g.live_stride * nB},
        {true, (void **)&g.appended, sizeof(int32_t) * nB},
        {true, (void **)&g.appended_next, sizeof(int32_t) * nB},
        {true, (void **)&g.state, sizeof(int32_t) * 8 * nB},
        {true, (void **)&g.path, sizeof(int32_t) * 2 * (size_t)g.path_cap * nB},
        {stage, (void **)&g.dlast, sizeof(double) * nB * W * W},
        {big, (void **)&g.ws_sub, sizeof(int32_t) * 4 * (size_t)W * nB},
        {big, (void **)&g.ctl, sizeof(int32_t) * 8 * nB},
        {big, &h->sdp_ws, big ? sdp::workspace_bytes(W, W, B) : 0},  // every window is at most W x W
    };
    for (const auto &a : allocs)
        if (e == hipSuccess && a.wanted) e = hipMalloc(a.buf, a.bytes);
    if (e == hipSuccess && big) sdp::workspace_carve(h->sdp_ws, W, W, B, &g, &g.ws_scr);
    if (e == hipSuccess && first_host) e = ref_table_upload(&h->refs, first_host, len_host, B);
    if (e != hipSuccess) {
        rts_wtw_destroy(h);
        return set_error(RTS_ERR_HIP, "WTW allocation failed: %s", hipGetErrorString(e));
    }
    g.ref_first = h->refs.first;
    g.ref_len = h->refs.len;
    int rc = rts_wtw_reset(h, nullptr);
    if (rc != RTS_OK) {
        rts_wtw_destroy(h);
        return rc;
    }
    if (hipError_t es = hipStreamSynchronize(nullptr); es != hipSuccess) {
        rts_wtw_destroy(h);
        return set_error(RTS_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(es));
    }
    *out = h;
    return RTS_OK;
}

int wtw_batch(const rts_wtw *h) { return h->B; }
int wtw_history(const rts_wtw *h) { return h->args.live_stride; }
int wtw_tempo_view(const rts_wtw *h, TempoTail *t) {
    t->state = h->args.state;
    t->state_len = RTS_WTW_STATE_LEN;
    t->st_n_path = RTS_WTW_ST_N_PATH;
    t->path = h->args.path;
    t->path_cap = h->args.path_cap;
    t->ref_len = h->args.ref_len;
    t->N = h->args.M;
    t->B = h->B;
    return h->args.M;
}

}  // namespace rts

extern "C" {

int rts_wtw_create(const double *chroma_ref_dev, int F, int M, int B, int win_frames, int hop_frames, int keep_last_d,
                   rts_wtw **out) {
    using namespace rts;
    if (!out) return set_error(RTS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!chroma_ref_dev) return set_error(RTS_ERR_INVALID, "chroma_ref_dev is NULL");
    return wtw_create(chroma_ref_dev, F, M, B, win_frames, hop_frames, keep_last_d, nullptr, nullptr, out);
}

int rts_wtw_create_refs(const double *chroma_refs_dev, int F, long long n_ref_frames, const long long *first_host,
                        const int32_t *len_host, int B, int win_frames, int hop_frames, int keep_last_d, rts_wtw **out) {
    using namespace rts;
    if (!out) return set_error(RTS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!chroma_refs_dev) return set_error(RTS_ERR_INVALID, "chroma_refs_dev is NULL");
    if (!first_host || !len_host) return set_error(RTS_ERR_INVALID, "first_host / len_host is NULL");
    if (B < 1) return set_error(RTS_ERR_INVALID, "B must be >= 1 (got %d)", B);
    const int m_max = ref_ranges_check(B, nullptr, first_host, len_host, n_ref_frames, 0, nullptr);
    if (m_max < 0) return m_max;
    const int rc = wtw_create(chroma_refs_dev, F, m_max, B, win_frames, hop_frames, keep_last_d, first_host, len_host, out);
    if (rc == RTS_OK) (*out)->refs.n_frames = n_ref_frames;
    return rc;
}

int rts_wtw_destroy(rts_wtw *h) {
    if (!h) return RTS_OK;
    rts::ref_table_free(&h->refs);
    const rts::WtwArgs &g = h->args;
    void *const bufs[] = {g.live, g.appended, g.appended_next, g.state, g.path, g.dlast, g.ws_sub, g.ctl, h->sdp_ws};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    free(h);
    return RTS_OK;
}

int rts_wtw_reset(rts_wtw *h, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    const WtwArgs &g = h->args;
    if (g.state) {  // (rts_wtw_create resets before the handle is complete; the device is current there by construction)
        if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    }
    hipStream_t s = (hipStream_t)stream;
    RTS_HIP(hipMemsetAsync(g.appended, 0, sizeof(int32_t) * (size_t)h->B, s));
    RTS_HIP(hipMemsetAsync(g.state, 0, sizeof(int32_t) * 8 * (size_t)h->B, s));
    // wtw.py:55: chroma_live starts as zeros
    RTS_HIP(hipMemsetAsync(g.live, 0, sizeof(double) * kWF * (size_t)g.live_stride * h->B, s));
    if (g.ctl) RTS_HIP(hipMemsetAsync(g.ctl, 0, sizeof(int32_t) * 8 * (size_t)h->B, s));
    if (g.err) RTS_HIP(hipMemsetAsync(g.err, 0, 16, s));
    if (g.ticket) RTS_HIP(hipMemsetAsync(g.ticket, 0, sizeof(int32_t) * (size_t)h->B, s));
    return RTS_OK;
}

int rts_wtw_restart(rts_wtw *h, const uint8_t *mask_host, const long long *first_host, const int32_t *len_host,
                    void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!mask_host) return set_error(RTS_ERR_INVALID, "mask_host is NULL");
    if (int rc = restart_check(h->B, mask_host, first_host, len_host, h->refs.first ? h->refs.n_frames : -1, h->args.M, "M_max");
        rc != RTS_OK)
        return rc;
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const WtwArgs &g = h->args;
    RestartSel sel;
    for (int pos = 0; restart_next_chunk(h->B, mask_host, first_host, len_host, &pos, &sel) > 0;) {
        hipLaunchKernelGGL(wtw_restart_kernel, dim3(16, sel.n), dim3(256), 0, s, sel, g.state, g.appended, g.live,
                           (long long)g.live_stride * kWF, g.ctl, g.ticket, h->refs.first, h->refs.len);
        RTS_HIP(hipGetLastError());
    }
    return RTS_OK;
}

int rts_wtw_recent(rts_wtw *h, int M_max, double *out_dev, int32_t *len_dev, const uint8_t *mask_dev, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!out_dev) return set_error(RTS_ERR_INVALID, "out_dev is NULL");
    if (!len_dev) return set_error(RTS_ERR_INVALID, "len_dev is NULL");
    if (M_max < 1) return set_error(RTS_ERR_INVALID, "M_max must be >= 1 (got %d)", M_max);
    if (M_max > 256) return set_error(RTS_ERR_UNSUPPORTED, "M_max = %d exceeds the 256 frames rts_locate takes", M_max);
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    hipLaunchKernelGGL(wtw_recent_kernel, dim3(h->B), dim3(256), 0, (hipStream_t)stream, h->args.live, h->args.appended,
                       h->args.live_stride, h->args.M, h->args.ref_len, M_max, out_dev, len_dev, mask_dev);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

int rts_wtw_tempo(rts_wtw *h, int K, double ahead, double *slope_dev, double *pos_dev, int32_t *n_dev, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!slope_dev) return set_error(RTS_ERR_INVALID, "slope_dev is NULL");
    if (!n_dev) return set_error(RTS_ERR_INVALID, "n_dev is NULL");
    if (int rc = tempo_tail_check(K, ahead, h->args.M); rc != RTS_OK) return rc;
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    TempoTail t = {};
    wtw_tempo_view(h, &t);
    t.K = K;
    t.ahead = ahead;
    t.slope = slope_dev;
    t.pos = pos_dev;
    t.n_out = n_dev;
    return tempo_tail_enqueue(t, nullptr, (hipStream_t)stream);
}

int rts_wtw_push(rts_wtw *h, const void *cols_dev, int cols_dtype, int n_max, const int32_t *n_new_dev, int precheck,
                 void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (n_max < 0) return set_error(RTS_ERR_INVALID, "n_max < 0");
    if (n_max > 0 && !cols_dev) return set_error(RTS_ERR_INVALID, "cols_dev is NULL");
    if (!dtype_ok(cols_dtype)) return set_error(RTS_ERR_INVALID, "bad cols_dtype %d", cols_dtype);
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    WtwArgs &g = h->args;
    const int B = h->B;
    if (precheck) {
        hipLaunchKernelGGL(wtw_precheck_kernel, dim3((B + 63) / 64), dim3(64), 0, s, g.state, B, g.M, g.ref_len);
        RTS_HIP(hipGetLastError());
    }
    if (n_max == 0) return RTS_OK;
    hipLaunchKernelGGL(wtw_append_kernel, dim3(B, n_max >= 64 ? kWtwAppendSlices : 1), dim3(256), 0, s, g.live, g.appended,
                       g.appended_next, g.state, cols_dev, cols_dtype == RTS_F64, n_new_dev, n_max, n_max, B, g.live_stride);
    {
        int32_t *t = g.appended;
        g.appended = g.appended_next;
        g.appended_next = t;
    }
    RTS_HIP(hipGetLastError());
    if (h->win) {
        hipLaunchKernelGGL(h->win, dim3(h->plan.grid), dim3(h->plan.block), h->plan.smem, s, g);
    } else {
        // one (dp, ctl) round per window the new columns can complete: the first needs at least one column, every
        // further one dtw_hop / hop more (the live pointer advances by exactly that per window, wtw.py:118-128)
        const int rounds = n_max / g.hopf + 1, S = sdp::n_strips(g.W);
        hipLaunchKernelGGL(wtw_big_ctl_kernel, dim3(B), dim3(1024), 0, s, g);
        if (g.fill_separate) hipLaunchKernelGGL(wtw_big_fill_kernel, dim3(128, B), dim3(256), 0, s, g);
        for (int r = 0; r < rounds; r++) {
            hipLaunchKernelGGL(h->dp, dim3(h->plan.grid, B), dim3(h->plan.block), h->plan.smem, s, g);
            if (S <= sdp::kTailStrips) {
                hipLaunchKernelGGL(wtw_big_tail_ctl_kernel, dim3(B), dim3(64 * S), sdp::tail_lds_bytes(S), s, g);
            } else {
                hipLaunchKernelGGL(wtw_big_hops_kernel, dim3(B), dim3(64), 0, s, g);
                hipLaunchKernelGGL((wtw_big_segment_kernel<0>), dim3(S, B), dim3(64), 0, s, g);
                hipLaunchKernelGGL((wtw_big_segment_kernel<1>), dim3(S, B), dim3(64), 0, s, g);
                hipLaunchKernelGGL(wtw_big_ctl_kernel, dim3(B), dim3(1024), 0, s, g);
            }
            if (g.fill_separate) hipLaunchKernelGGL(wtw_big_fill_kernel, dim3(128, B), dim3(256), 0, s, g);
        }
    }
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

int rts_wtw_read_states(rts_wtw *h, int32_t *states, void *stream) {
    using namespace rts;
    if (!h || !states) return set_error(RTS_ERR_INVALID, "NULL argument");
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    RTS_HIP(hipMemcpyAsync(states, h->args.state, sizeof(int32_t) * 8 * (size_t)h->B, hipMemcpyDeviceToHost, s));
    RTS_HIP(hipStreamSynchronize(s));
    return RTS_OK;
}

int rts_wtw_read_path(rts_wtw *h, int b, int32_t *pairs, int cap_pairs, int *n, void *stream) {
    using namespace rts;
    if (!h || !n) return set_error(RTS_ERR_INVALID, "NULL argument");
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    return read_path(h->args.state, 8, 4, h->args.path, h->args.path_cap, b, h->B, pairs, cap_pairs, n, (hipStream_t)stream);
}

int rts_wtw_read_last_d(rts_wtw *h, int b, double *d_host, void *stream) {
    using namespace rts;
    if (!h || !d_host) return set_error(RTS_ERR_INVALID, "NULL argument");
    if (b < 0 || b >= h->B) return set_error(RTS_ERR_INVALID, "stream index %d out of range [0, %d)", b, h->B);
    const int W = h->args.W;
    if (!h->args.dlast) return set_error(RTS_ERR_INVALID, "handle was created with keep_last_d = 0");
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    RTS_HIP(hipMemcpyAsync(d_host, h->args.dlast + (size_t)b * W * W, sizeof(double) * (size_t)W * W, hipMemcpyDeviceToHost, s));
    RTS_HIP(hipStreamSynchronize(s));
    return RTS_OK;
}

#ifdef RTS_WIN_STAMPS
/* Diagnostic build only: reads and clears the per-phase cycle sums of wtw_win_kernel (stream 0, wave 0). */
int rts_wtw_read_win_stamps(long long *out) {
    static const long long zero[8] = {0};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(rts::g_win_stamps), sizeof(long long) * 8) != hipSuccess) return -3;
    return hipMemcpyToSymbol(HIP_SYMBOL(rts::g_win_stamps), zero, sizeof(zero)) == hipSuccess ? 0 : -3;
}
#endif

int rts_wtw_state_view(rts_wtw *h, int32_t **state_dev) {
    using namespace rts;
    if (!h || !state_dev) return set_error(RTS_ERR_INVALID, "NULL argument");
    *state_dev = h->args.state;
    return RTS_OK;
}

int rts_wtw_device_views(rts_wtw *h, double **live_chroma_dev, int *live_capacity, double **last_d_dev) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (live_chroma_dev) *live_chroma_dev = h->args.live;
    if (live_capacity) *live_capacity = h->args.live_stride;
    if (last_d_dev) *last_d_dev = h->args.dlast;
    return RTS_OK;
}

// ---- snapshots (include/rtsync.h; csrc/snapshot.h has the kernels) ----------------------------------------------------
// The handle as the record kernels see it: what wtw_restart_kernel resets, and D where the handle keeps it.  `appended`
// is the count array the host has current at this call; an import writes the other one too.
static rts::SnapView wtw_snap_view(const rts_wtw *h, const void *blob, long long rec_stride, int32_t *status) {
    const rts::WtwArgs &g = h->args;
    rts::SnapView v;
    memset(&v, 0, sizeof(v));
    v.kind = RTS_SNAPSHOT_WTW;
    v.state = g.state;
    v.state_words = RTS_WTW_STATE_LEN;
    v.st_n_path = RTS_WTW_ST_N_PATH;
    v.mid = reinterpret_cast<unsigned long long *>(g.dlast);
    v.mid_stride = (long long)g.W * g.W;
    v.param = g.dlast ? g.W : 0;
    v.mid_gate = 5;  // n_windows: D is whatever hipMalloc left there until the first window has run
    v.path = g.path;
    v.path_cap = g.path_cap;
    v.hist = g.live;
    v.hist_stride = g.live_stride;
    v.count = g.appended;
    v.count2 = g.appended_next;
    v.ref_first = h->refs.first;
    v.ref_len = h->refs.len;
    v.len_default = g.M;
    v.ctl = g.ctl;
    v.ticket = g.ticket;
    v.zero_hist = 1;
    v.blob = static_cast<unsigned char *>(const_cast<void *>(blob));
    v.rec_stride = rec_stride;
    v.status = status;
    return v;
}

static void wtw_snap_desc(const rts_wtw *h, int n, long long rec_stride, rts_snapshot_desc *d) {
    memset(d, 0, sizeof(*d));
    d->kind = RTS_SNAPSHOT_WTW;
    d->version = RTS_SNAPSHOT_VERSION;
    d->n = n;
    d->ref_dtype = RTS_F64;
    d->rec_stride = rec_stride;
    d->F = rts::kWF;
    d->window = h->args.W;
    d->hop = h->args.hopf;
    d->keep_last_d = h->args.dlast != nullptr;
}

static long long wtw_snap_need(const rts_wtw *h) {
    return rts::snap::wtw_rec_stride(h->args.M, h->args.W, h->args.dlast != nullptr, h->args.path_cap);
}

int rts_wtw_snapshot_bytes(const rts_wtw *h, size_t *bytes) {
    using namespace rts;
    if (!h || !bytes) return set_error(RTS_ERR_INVALID, "NULL argument");
    if (int rc = snap_stride_check(wtw_snap_need(h), -1, "M_max", h->args.M); rc != RTS_OK) return rc;
    *bytes = (size_t)wtw_snap_need(h);
    return RTS_OK;
}

int rts_wtw_export(rts_wtw *h, const int32_t *idx_host, int n, void *blob_dev, long long rec_stride,
                   rts_snapshot_desc *desc_out, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!desc_out) return set_error(RTS_ERR_INVALID, "desc_out is NULL");
    if (int rc = snap_check_sel(h->B, idx_host, n, "idx_host", blob_dev, rec_stride); rc != RTS_OK) return rc;
    if (int rc = snap_stride_check(wtw_snap_need(h), rec_stride, "M_max", h->args.M); rc != RTS_OK) return rc;
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    wtw_snap_desc(h, n, rec_stride, desc_out);
    return snap_enqueue(false, wtw_snap_view(h, blob_dev, rec_stride, nullptr), idx_host, n, nullptr, nullptr, (hipStream_t)stream);
}

int rts_wtw_import(rts_wtw *h, const int32_t *slot_host, int n, const void *blob_dev, long long rec_stride,
                   const rts_snapshot_desc *desc, const long long *first_host, const int32_t *len_host,
                   int32_t *status_dev, void *stream) {
    return rts::wtw_import_records(h, slot_host, n, blob_dev, rec_stride, desc, first_host, len_host, status_dev, stream, 0);
}

}  // extern "C"

namespace rts {

int wtw_import_records(rts_wtw *h, const int32_t *slot_host, int n, const void *blob_dev, long long rec_stride,
                       const rts_snapshot_desc *desc, const long long *first_host, const int32_t *len_host,
                       int32_t *status_dev, void *stream, int dry) {
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!desc) return set_error(RTS_ERR_INVALID, "desc is NULL");
    if (!status_dev) return set_error(RTS_ERR_INVALID, "status_dev is NULL");
    if (int rc = snap_check_sel(h->B, slot_host, n, "slot_host", blob_dev, rec_stride); rc != RTS_OK) return rc;
    rts_snapshot_desc mine;
    wtw_snap_desc(h, n, rec_stride, &mine);
    if (int rc = snap_check_import(*desc, mine, slot_host, first_host, len_host, h->refs, h->args.M, "M_max"); rc != RTS_OK) return rc;
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    SnapView v = wtw_snap_view(h, blob_dev, rec_stride, status_dev);
    v.dry = dry;
    return snap_enqueue(true, v, slot_host, n, first_host, len_host, (hipStream_t)stream);
}

}  // namespace rts
