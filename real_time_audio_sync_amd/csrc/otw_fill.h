// Band fill of a fresh OTW stream as one dense anti-diagonal wavefront ("band fill").
//
// While the band fills (t < c) otw_decide returns Both unconditionally, so the first c-1 steps of a fresh stream are
// fixed in advance: t = j = s, both strips start at 0, no decision feeds back into the arithmetic.  The cells they
// evaluate are the dense DTW matrix of the square [0, c-1] x [0, c-1]; the two band argmins of step s are the first
// minima of row s over columns [0, s] and of column s over rows [0, s].  The step loop runs that as c-1 dependent Both
// steps of full 512-cell chains; here it is D = c + c/2 - 1 stages of two cells per thread.
//
//   * thread p owns rows 2p and 2p+1 (their live frames in registers); at stage d it evaluates column d - p of both,
//     the upper row first: the lower row's `up` is the value just computed, its `diag` the upper row's previous one;
//   * the reference frames 0..c-1 sit in LDS, feature-major, as float64 (a float32 reference widens exactly);
//   * `left` is the row's own previous value; the upper row's `up` comes from lane p-1 (its lower row) by a DPP wave
//     shift and its `diag` is that `up` of the stage before; lane 0 of wave w takes them from what lane 63 of wave
//     w-1 held after the stage before (the schedule below).  One reference frame read from LDS and one shift serve two
//     cells;
//   * the column argmin (first minimum of column j over the rows so far) travels down the column with `up`; the row
//     argmin stays in the owning thread.  Both compare with a strict <, rows and columns in ascending order, from
//     (inf, 0x7fffffff): what strip_chain's reduction followed by decide()'s "corner wins only if strictly smaller"
//     gives, a NaN never winning.  On the diagonal (j == i) the owner of row i holds both and takes step i's path point;
//   * column c-1 (the column band) stays in the owning thread until the sweep is over; row c-1 (the row band) is a
//     thread of the last wave, which stores it chunk by chunk.
//
// Schedule: chunks of K = kFillChunk stages, the waves skewed by a chunk.  Wave w runs its stages K w behind wave 0: in
// global chunk g it executes stages [(g - w) K, (g - w + 1) K) back to back, without a barrier, then joins the one
// LDS-only barrier of the chunk; a wave with no stage in a chunk (before 64 w, which opens a chunk because K divides 64,
// or after its last) only joins the barrier, so every wave executes the same ceil(D / K) + nw - 1 barriers and nothing
// polls.  (One barrier per stage, every wave in the same phase, took 1 570 cycles per stage at c = 500; this takes about
// 840 -- profiles/otw_fill_chunked_summary.md, with the forms tried: K = 8 / 16 / 32, one row per thread.)
//   * hand-over ring: lane 63 of wave w < nw - 1 leaves its stage-d values (value, column argmin and its index) in slot
//     d % kFillRing of its own ring, all K of a chunk in one store after the chunk's last stage (during the chunk they
//     collect in pub_*, shifted a lane per stage).  Wave w + 1 fetches what its chunk needs in one read before its first
//     stage, lane l taking stage d0 - 1 + l, and shifts the register down a lane per stage, so lane 0's chain never waits
//     for LDS.  Invariant: in one global chunk wave w + 1 reads stages (g-w-1) K - 1 .. (g-w) K - 2, published at least a
//     barrier earlier, while wave w writes stages (g-w) K .. (g-w+1) K - 1; together 2K + 1 consecutive stages from
//     (g-w-1) K - 1 to (g-w+1) K - 1, which a ring of 2K slots would fold onto each other at the two ends.  kFillRing =
//     2K + 1 keeps them apart, and the barrier keeps the chunks apart;
//   * a full chunk is an unrolled block of K stages without a branch or a store, the next stage's costs computed beside
//     the current stage's chain (a scheduling fence per stage keeps the compiler from hoisting all K stages' frame reads:
//     that form needed 400 registers).  Two forms: the interior one (no thread of the wave left of column 0, on the
//     diagonal or in column c-1 during the chunk) and the general one, which does that work with selects.  The last,
//     partial chunk of a wave runs the general stage in a loop.
//
// The stream is left as the step loop leaves it after consuming exactly its first c frames (t = j = c-1, decision taken):
// all 16 state words, both bands in the layout the prologue reloads under !first, the path points.  otw_advance_kernel,
// launched right behind, resumes from there as after any rts_otw_insert.
//
// The cell value is the chain's expression min(min(up + d, diag + 2d), left + d) with v_min_f64.  The chains take `up`
// for row strips and `left` for column strips as the first operand; v_min_f64 returns the smaller number, or the one
// that is a number, whatever the order, so the value does not depend on it.  Missing predecessors of the cells of row 0
// and column 0 are +inf for every variant, as in the chains while their strips start at 0 (x_in = inf, prevb[0] = inf).
#pragma once
#include "otw_device.h"  // OtwArgs, cell_cost, vmin, the wave shifts, otw_load_feat, otw_live_frame: the step kernel's own

namespace rts {

constexpr int kFillMaxC = 500;  // the handles with W <= 512 (two matrix rows per thread, 256 threads, four waves)

// Eligibility of stream b, uniform for its workgroup (every thread reads the same words).
__device__ __forceinline__ bool otw_fill_eligible(const OtwArgs &a, int b, int nthreads, int &live_len_out, int &N_out) {
    const int32_t *st = a.state + (size_t)b * RTS_STATE_LEN;
    int live_len = a.live_len[b];
    if (a.clamp_len && live_len > (int)a.live_stride) live_len = (int)a.live_stride;
    const int N = a.ref_first ? a.ref_len[b] : a.N;
    live_len_out = live_len;
    N_out = N;
    const int c = a.c;
    // set_live that ends exactly at the hand-over leaves t one past the last frame (otw_make_plan): the step loop keeps it
    const int need = c + ((a.mode == RTS_MODE_SET_LIVE) ? 1 : 0);
    return st[RTS_ST_FIRST_INSERT] == 1 && st[RTS_ST_STATUS] == RTS_RUNNING && st[RTS_ST_CONSUMED] == 0 &&
           st[RTS_ST_N_PATH] == 0 && c >= 2 && c <= kFillMaxC && c <= nthreads && live_len >= need && N >= c &&
           a.path_cap >= c && a.dense_acc == nullptr;
}

// Staged reference frames: feature-major doubles, frame y at column y + kFillPad.  The pad on either side lets the
// threads of a wave that are not inside the square yet (column < 0) or no more (column > c-1) read without a clamp; what
// they read (zeros) feeds cells nobody uses.  A wave's last stage is at column c + 62 at most and reads one ahead.
constexpr int kFillPad = 64, kFillCols = kFillPad + kFillMaxC + kFillPad;
constexpr int kFillRows = 2;    // matrix rows per thread
constexpr int kFillChunk = 16;  // stages a wave runs between two barriers (divides 64)
constexpr int kFillRing = 2 * kFillChunk + 1;  // hand-over slots per producing wave (the invariant in the header)
constexpr int kFillMaxWaves = (kFillMaxC / kFillRows + 63) / 64;
static_assert(64 % kFillChunk == 0, "a wave's first stage, 64 w, must open a chunk");

struct FillHand {  // slot d % kFillRing of row w: what lane 63 of wave w held after stage d
    double v[kFillMaxWaves - 1][kFillRing], cv[kFillMaxWaves - 1][kFillRing];
    int ci[kFillMaxWaves - 1][kFillRing];
};

__host__ __device__ constexpr int otw_fill_threads(int c) { return 64 * (((c + kFillRows - 1) / kFillRows + 63) / 64); }

// lane i receives lane i+1's value; lane 63 receives `lane63` (DPP wave_shl:1; lanes without a source keep `old`).
__device__ __forceinline__ int wave_shift_down(int v, int lane63) {
    return __builtin_amdgcn_update_dpp(lane63, v, 0x130, 0xf, 0xf, false);
}
__device__ __forceinline__ double wave_shift_down(double v, double lane63) {
    const int lo = wave_shift_down(__double2loint(v), __double2loint(lane63));
    const int hi = wave_shift_down(__double2hiint(v), __double2hiint(lane63));
    return __hiloint2double(hi, lo);
}

// The costs of the thread's R cells of column jb + KK.
#define RTS_FILL_COST(DST, KK)                                                                                        \
    {                                                                                                                 \
        double rf[kF];                                                                                                \
        _Pragma("unroll") for (int f = 0; f < kF; f++) rf[f] = rp0[f * kFillCols + (KK)];                             \
        _Pragma("unroll") for (int r = 0; r < R; r++) DST[r] = cell_cost(lf[r], rf, EUCLID);                          \
    }
// One stage of a wave: column jb + KK of the thread's R rows.  GEN = 0 is the interior form: no thread of the wave is
// left of column 0, on the diagonal or in column c-1 anywhere in the chunk.  No branch and no store: the hand-over comes
// out of pf_* (lane 0 holds this stage's, the registers shift down a lane per stage) and goes into pub_* (lane 63's value
// shifted in from the top; in the last wave, which publishes nothing, row c-1's value takes that place), column c-1's
// into colv.
#define RTS_FILL_STAGE(KK, GEN)                                                                                       \
    {                                                                                                                 \
        const int j = jb + (KK);                                                                                      \
        double dn[R];                                                                                                 \
        RTS_FILL_COST(dn, (KK) + 1) /* the next stage's costs: independent work beside this stage's chain */          \
        const double up0 = wave_shift_up(val[R - 1], pf_v); /* (R p - 1, j): the thread above, a stage ago */         \
        double cvr = wave_shift_up(cv, pf_cv);                                                                        \
        int cir = __builtin_amdgcn_update_dpp(pf_ci, ci, 0x138, 0xf, 0xf, false);                                     \
        pf_v = wave_shift_down(pf_v, pf_v);                                                                           \
        pf_cv = wave_shift_down(pf_cv, pf_cv);                                                                        \
        pf_ci = wave_shift_down(pf_ci, pf_ci);                                                                        \
        double up = up0, dg = dgp;                                                                                    \
        _Pragma("unroll") for (int r = 0; r < R; r++) {                                                               \
            const int i = R * p + r;                                                                                  \
            double nv = vmin(vmin(up + dc[r], dg + 2 * dc[r]), val[r] + dc[r]);                                       \
            if (GEN) {                                                                                                \
                nv = (j < 0) ? inf : nv; /* a row enters the square at column 0 with left = diag = +inf */            \
                if (r == 0) {                                                                                         \
                    const bool origin = (j == 0) & (p == 0);                                                          \
                    nv = origin ? dc[0] : nv; /* acc[0][0] = d(0, 0) */                                               \
                    d00 = origin ? dc[0] : d00;                                                                       \
                }                                                                                                     \
            }                                                                                                         \
            /* first minima, ascending, strict <: min(old, new) is the new value exactly when new < old */           \
            const bool rless = nv < rmin[r];                                                                          \
            rmin[r] = vmin(rmin[r], nv);                                                                              \
            ridx[r] = rless ? j : ridx[r];                                                                            \
            const bool cless = nv < cvr;                                                                              \
            cvr = vmin(cvr, nv);                                                                                      \
            cir = cless ? i : cir;                                                                                    \
            if (GEN) {                                                                                                \
                const bool od = j == i; /* step i's best_point: row i over [0, i] against column i over [0, i] */     \
                const bool rw = rmin[r] < cvr;                                                                        \
                px[r] = od ? (rw ? i : cir) : px[r];                                                                  \
                py[r] = od ? (rw ? ridx[r] : i) : py[r];                                                              \
                colv[r] = (j == c - 1) ? nv : colv[r]; /* the column band */                                          \
            }                                                                                                         \
            dg = val[r]; /* (i, j-1) is the diagonal neighbour of the row below */                                    \
            up = nv;                                                                                                  \
            val[r] = nv;                                                                                              \
        }                                                                                                             \
        dgp = up0;                                                                                                    \
        cv = cvr;                                                                                                     \
        ci = cir;                                                                                                     \
        double rv = val[0];                                                                                           \
        _Pragma("unroll") for (int r = 1; r < R; r++) rv = (row_r == r) ? val[r] : rv;                                \
        const double rvb = wave_bcast(rv, row_lane);                                                                  \
        pub_v = wave_shift_down(pub_v, last_wave ? rvb : val[R - 1]);                                                 \
        pub_cv = wave_shift_down(pub_cv, cv);                                                                         \
        pub_ci = wave_shift_down(pub_ci, ci);                                                                         \
        _Pragma("unroll") for (int r = 0; r < R; r++) dc[r] = dn[r];                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                            \
    }

template <bool EUCLID>
__device__ __forceinline__ void otw_bandfill_body(const OtwArgs &a, int32_t *took, double (*refs)[kFillCols], FillHand &hand) {
    constexpr int R = kFillRows, K = kFillChunk;
    int2 *pts = reinterpret_cast<int2 *>(&refs[0][0]);  // the filtered variant's points, once the sweep is over

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nw = (int)blockDim.x >> 6;
    const int b = blockIdx.x, c = a.c, p = tid;
    int live_len, N;
    const bool ok = otw_fill_eligible(a, b, R * (int)blockDim.x, live_len, N);
    if (tid == 0) took[b] = ok ? 1 : 0;
    if (!ok) return;

    const double inf = INFINITY;
    const bool set_live = a.mode == RTS_MODE_SET_LIVE;
    OtwEnv e;
    e.b = b;
    e.lane = lane;
    e.live = a.live;
    e.live_f64 = a.live_f64;
    e.live_base = (long long)b * a.live_stride * kF;
    const void *ref = a.ref_first ? static_cast<const void *>(static_cast<const char *>(a.ref) +
                                                              a.ref_first[b] * (long long)kF * (a.ref_f64 ? 8 : 4))
                                  : a.ref;
    double lf[R][kF];  // this thread's rows R p .. R p + R-1 (rows past c-1 repeat the last one and are never used)
#pragma unroll
    for (int r = 0; r < R; r++) otw_live_frame(e, (R * p + r < c) ? R * p + r : c - 1, lf[r]);
    for (int idx = tid; idx < kF * kFillCols; idx += (int)blockDim.x) (&refs[0][0])[idx] = 0.0;
    __syncthreads();
    for (int idx = tid; idx < c * kF; idx += (int)blockDim.x) {
        const int fr = idx / kF, f = idx % kF;
        refs[f][kFillPad + fr] = otw_load_feat(ref, a.ref_f64, (long long)fr * kF + f);
    }
    __syncthreads();

    double *bb = a.bands + (size_t)b * 2 * (c + 1);
    // A row enters the square at column 0 with left = diag = +inf; until then (warm-up stages of its wave) its value is
    // forced to +inf, which is also what its running minimum starts from.
    double val[R], rmin[R], colv[R], dgp = inf, cv = inf, d00 = 0.0;
    int ridx[R], px[R], py[R], ci = 0x7fffffff;
#pragma unroll
    for (int r = 0; r < R; r++) {
        val[r] = inf;
        rmin[r] = inf;
        colv[r] = inf;
        ridx[r] = 0x7fffffff;
        px[r] = py[r] = 0;
    }
    const int P = (c + R - 1) / R;  // threads that own a row of the square
    const int D = P + c - 1;        // stages of the sweep
    // stages at which a thread of this wave is inside the square
    const int d_lo = 64 * wave, d_end = (d_lo + 63 + c - 1 < D - 1) ? d_lo + 63 + c - 1 : D - 1;
    const int row_p = (c - 1) / R, row_r = (c - 1) % R, row_lane = row_p & 63;  // row c-1: a thread of the last wave
    const bool last_wave = wave == nw - 1;
    const int G = (D + K - 1) / K + nw - 1;
    for (int g = 0; g < G; g++) {
        const int d0 = (g - wave) * K;  // this wave runs K w stages behind wave 0
        if (d0 >= d_lo && d0 <= d_end) {
            const int n = (d_end + 1 - d0 < K) ? d_end + 1 - d0 : K;
            const int jb = d0 - p;
            const double *rp0 = &refs[0][kFillPad + jb];  // column d0 - p of the staged frames
            // what lane 63 of the wave above left after stages d0-1 .. d0+K-2, all published before the last barrier:
            // lane l takes stage d0-1+l (row 0 has nothing above it)
            double pf_v = inf, pf_cv = inf;
            int pf_ci = 0x7fffffff;
            if (wave > 0) {
                                const int s = (d0 - 1 + lane) % kFillRing;
                pf_v = hand.v[wave - 1][s];
                pf_cv = hand.cv[wave - 1][s];
                pf_ci = hand.ci[wave - 1][s];
            }
            double pub_v = 0.0, pub_cv = 0.0;
            int pub_ci = 0;
            const bool warm = d0 < d_lo + 63, last_col = d0 + K - 1 >= d_lo + c - 1;
            const bool on_diag = d0 + K - 1 >= (R + 1) * d_lo && d0 <= (R + 1) * (d_lo + 63) + R - 1;
            double dc[R];
            RTS_FILL_COST(dc, 0)
            if (n < K) {
                for (int k = 0; k < n; k++) RTS_FILL_STAGE(k, 1)
            } else if (warm || on_diag || last_col) {
#pragma unroll
                for (int k = 0; k < K; k++) RTS_FILL_STAGE(k, 1)
            } else {
#pragma unroll
                for (int k = 0; k < K; k++) RTS_FILL_STAGE(k, 0)
            }
            // stage d0 + k of the chunk sits in lane 64 - n + k of pub_*
            if (lane >= 64 - n) {
                const int d = d0 + lane - (64 - n);
                if (!last_wave) {
                    const int s = d % kFillRing;
                    hand.v[wave][s] = pub_v;
                    hand.cv[wave][s] = pub_cv;
                    hand.ci[wave][s] = pub_ci;
                } else if (d >= row_p && d < row_p + c) {  // the row band at the hand-over
                    bb[1 + d - row_p] = pub_v;
                }
            }
        }
        lds_barrier();
    }
#pragma unroll
    for (int r = 0; r < R; r++)
        if (R * p + r < c) bb[(c + 1) + 1 + R * p + r] = colv[r];

    // ---- path and control tail: the bottom half of otw_decide, step by step
    const bool filt = a.variant == RTS_VARIANT_LIVENOTE_V2;
    int2 *path = reinterpret_cast<int2 *>(a.path) + (size_t)b * a.path_cap;
    const int sl = set_live ? 1 : 0;  // set_live decides at (0, 0) too: one point in front
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int i = R * p + r;
        if (!filt) {
            if (i >= 1 && i < c) path[i - 1 + sl] = make_int2(px[r], py[r]);
        } else if (i < c) {
            pts[i] = make_int2(px[r], py[r]);  // (every wave is past its last read of the frames: the sweep's last barrier)
        }
    }
    __syncthreads();
    if (tid == 0) {
        int32_t *st = a.state + (size_t)b * RTS_STATE_LEN;
        const bool deferred = set_live && a.variant != RTS_VARIANT_OTW;
        int run_count = st[RTS_ST_RUN_COUNT], prev = st[RTS_ST_PREVIOUS], pend = -2, n_path = 0, last_x = -1, last_y = -1;
        for (int t = set_live ? 0 : 1; t < c; t++) {
            if (t > 0 && deferred && pend != -2) {  // livenote_v2.py:149-155, at the top of the step
                run_count = (pend == prev) ? run_count + 1 : 1;
                if (pend != RTS_DIR_BOTH) prev = pend;
                pend = -2;
            }
            int x = 0, y = 0;
            if (t == 0) {
                x = (d00 != d00) ? 0x7fffffff : 0;  // band_argmin over the one cell (0, 0); rmin < cmin is false
                if (!filt) path[0] = make_int2(x, y);
            } else if (filt) {
                x = pts[t].x;
                y = pts[t].y;
            }
            if (filt && (n_path == 0 || (x > last_x && y >= last_y))) {  // livenote_v2.py:198
                path[n_path] = make_int2(x, y);
                n_path += 1;
                last_x = x;
                last_y = y;
            } else if (!filt) {
                n_path += 1;
            }
            const int nd = RTS_DIR_BOTH;  // tt < c
            if (deferred) {
                pend = nd;
            } else {
                run_count = (nd == prev) ? run_count + 1 : 1;
                if (nd != RTS_DIR_BOTH) prev = nd;
            }
        }
        const double qnan = __longlong_as_double(0x7ff8000000000000LL);
        bb[0] = qnan;  // column -1 / row -1 of the (c+1)-word bands
        bb[c + 1] = qnan;
        st[RTS_ST_T] = c - 1;
        st[RTS_ST_J] = c - 1;
        st[RTS_ST_DIRECTION] = RTS_DIR_BOTH;
        st[RTS_ST_PREVIOUS] = prev;
        st[RTS_ST_RUN_COUNT] = run_count;
        st[RTS_ST_STATUS] = RTS_RUNNING;
        st[RTS_ST_FIRST_INSERT] = 0;
        st[RTS_ST_N_PATH] = n_path;
        st[RTS_ST_CONSUMED] = c;
        st[RTS_ST_ROW_STRIPS] = c - 1;
        st[RTS_ST_COL_STRIPS] = c - 1;
        st[RTS_ST_CELLS_LO] = c * c;
        st[RTS_ST_CELLS_HI] = 0;
        st[RTS_ST_PATH_TRUNCATED] = 0;
        st[14] = pend;
        st[RTS_ST_BAND_RECOMPUTES] = 0;
    }
}
#undef RTS_FILL_STAGE
#undef RTS_FILL_COST

__global__ void __launch_bounds__(64 * kFillMaxWaves) __attribute__((amdgpu_waves_per_eu(2, 2)))
otw_bandfill_kernel(OtwArgs a, int32_t *took) {
    __shared__ double refs[kF][kFillCols];
    __shared__ FillHand hand;
    if (a.cost_kind == RTS_COST_EUCLID)
        otw_bandfill_body<true>(a, took, refs, hand);
    else
        otw_bandfill_body<false>(a, took, refs, hand);
}

}  // namespace rts
