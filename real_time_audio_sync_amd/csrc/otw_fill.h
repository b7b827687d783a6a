// Band fill of a fresh OTW stream as one dense anti-diagonal wavefront ("band fill").
//
// Included by otw.hip behind otw_advance_kernel: it uses that file's cell_cost, otw_load_feat, otw_live_frame, vmin,
// wave_shift_up and OtwArgs, so the bit patterns cannot drift.
//
// While the band fills (t < c) otw_decide returns Both unconditionally, so the first c-1 steps of a fresh stream are
// fixed in advance: t = j = s, both strips start at 0, no decision feeds back into the arithmetic.  The cells they
// evaluate are the dense DTW matrix of the square [0, c-1] x [0, c-1]; the two band argmins of step s are the first
// minima of row s over columns [0, s] and of column s over rows [0, s].  The step loop runs that as c-1 dependent Both
// steps of full 512-cell chains; here it is c + c/2 - 1 stages of two cells per thread.
//
//   * thread p owns rows 2p and 2p+1 (their live frames in registers); at stage d it evaluates column d - p of both,
//     the upper row first: the lower row's `up` is the value just computed, its `diag` the upper row's previous one;
//   * the reference frames 0..c-1 sit in LDS, feature-major, as float64 (a float32 reference widens exactly);
//   * `left` is the row's own previous value; the upper row's `up` comes from lane p-1 (its lower row) by a DPP wave
//     shift and its `diag` is that `up` of the stage before; lane 0 of wave w takes them from an LDS slot lane 63 of
//     wave w-1 published a stage earlier (two slots, by stage parity; one LDS-only barrier per stage).  One reference
//     frame read from LDS, one shift and one barrier serve two cells: with one row per thread (eight waves, 2c-1
//     stages) the sweep took 0.52 ms at c = 500, with two 0.49 ms (profiles/otw_fill_summary.md);
//   * the column argmin (first minimum of column j over the rows so far) travels down the column with `up`; the row
//     argmin stays in the owning thread.  Both compare with a strict <, rows and columns in ascending order, from
//     (inf, 0x7fffffff): what strip_chain's reduction followed by decide()'s "corner wins only if strictly smaller"
//     gives, a NaN never winning.  On the diagonal (j == i) the owner of row i holds both and takes step i's path point;
//   * a wave none of whose rows is inside the square at a stage only joins the barrier.
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

namespace rts {

constexpr int kFillMaxC = 500;  // the handles with W <= 512 (two matrix rows per thread, 256 threads)

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
// they read (zeros) feeds cells nobody uses.
constexpr int kFillPad = 64, kFillCols = kFillPad + 512 + kFillPad;
constexpr int kFillRows = 2;  // matrix rows per thread

__host__ __device__ constexpr int otw_fill_threads(int c) { return 64 * (((c + kFillRows - 1) / kFillRows + 63) / 64); }

__global__ void __launch_bounds__(64 * ((kFillMaxC / kFillRows + 63) / 64)) otw_bandfill_kernel(OtwArgs a, int32_t *took) {
    constexpr int R = kFillRows;
    __shared__ double refs[kF][kFillCols];
    __shared__ double hand_v[2][8], hand_cv[2][8];
    __shared__ int hand_ci[2][8];
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
    const int euclid = a.cost_kind == RTS_COST_EUCLID;
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
    double val[R], rmin[R], dgp = inf, cv = inf, d00 = 0.0;
    int ridx[R], px[R], py[R], ci = 0x7fffffff;
#pragma unroll
    for (int r = 0; r < R; r++) {
        val[r] = inf;
        rmin[r] = inf;
        ridx[r] = 0x7fffffff;
        px[r] = py[r] = 0;
    }
    const int P = (c + R - 1) / R;  // threads that own a row of the square
    const int d_lo = 64 * wave, d_hi = 64 * wave + 63 + c - 1;  // stages at which a thread of this wave is inside the square
    const double *rp = &refs[0][kFillPad + d_lo - p];           // column d - p of the staged frames, at stage d_lo
    for (int d = 0; d <= P + c - 2; d++) {
        if (d >= d_lo && d <= d_hi) {
            const int j = d - p;
            // what lane 63 of the wave above left a stage ago (row 0 has nothing above it)
            double hin_v = inf, hin_cv = inf;
            int hin_ci = 0x7fffffff;
            if (wave > 0) {
                const int s = (d - 1) & 1;
                hin_v = hand_v[s][wave - 1];
                hin_cv = hand_cv[s][wave - 1];
                hin_ci = hand_ci[s][wave - 1];
            }
            double rf[kF];
#pragma unroll
            for (int f = 0; f < kF; f++) rf[f] = rp[f * kFillCols];
            rp += 1;
            double dc[R];
#pragma unroll
            for (int r = 0; r < R; r++) dc[r] = cell_cost(lf[r], rf, euclid);
            const double up0 = wave_shift_up(val[R - 1], hin_v);  // (R p - 1, j): the thread above, a stage ago
            double cvr = wave_shift_up(cv, hin_cv);
            int cir = __builtin_amdgcn_update_dpp(hin_ci, ci, 0x138, 0xf, 0xf, false);
            const bool warm = d < d_lo + 63, outside = j < 0;
            const bool on_diag = d >= (R + 1) * d_lo && d <= (R + 1) * (d_lo + 63) + R - 1;
            const bool last_col = d >= d_lo + c - 1;
            double up = up0, dg = dgp;
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int i = R * p + r;
                double nv = vmin(vmin(up + dc[r], dg + 2 * dc[r]), val[r] + dc[r]);
                if (warm) nv = outside ? inf : nv;
                if (r == 0 && d == 0) {
                    if (p == 0) {
                        nv = dc[0];  // acc[0][0] = d(0, 0)
                        d00 = nv;
                    }
                }
                // first minima, ascending, strict <: min(old, new) is the new value exactly when new < old (old is never NaN)
                const bool rless = nv < rmin[r];
                rmin[r] = vmin(rmin[r], nv);
                ridx[r] = rless ? j : ridx[r];
                const bool cless = nv < cvr;
                cvr = vmin(cvr, nv);
                cir = cless ? i : cir;
                if (on_diag) {  // the stages at which a row of this wave is on the diagonal
                    if (j == i) {  // step i's best_point: row i over [0, i] against column i over [0, i]
                        const bool rw = rmin[r] < cvr;
                        px[r] = rw ? i : cir;
                        py[r] = rw ? ridx[r] : i;
                    }
                }
                if (wave == nw - 1) {  // row c-1: the row band at the hand-over
                    if (i == c - 1 && j >= 0 && j < c) bb[1 + j] = nv;
                }
                if (last_col) {  // the stages at which a thread of this wave reaches column c-1: the column band
                    if (j == c - 1 && i < c) bb[(c + 1) + 1 + i] = nv;
                }
                dg = val[r];  // (i, j-1) is the diagonal neighbour of the row below
                up = nv;
                val[r] = nv;
            }
            dgp = up0;
            cv = cvr;
            ci = cir;
            if (wave < nw - 1) {
                if (lane == 63) {
                    hand_v[d & 1][wave] = val[R - 1];
                    hand_cv[d & 1][wave] = cv;
                    hand_ci[d & 1][wave] = ci;
                }
            }
        }
        lds_barrier();
    }

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

}  // namespace rts
