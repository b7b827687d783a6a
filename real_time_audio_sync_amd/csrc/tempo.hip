// Tempo: the slope of an alignment path over a trailing window of K points, and the position its regression line gives.
//   livenote_live.py:203-206   after every insert the live loop prints the wall-clock frame next to ln.path[-1], and the
//                              operator compares the two columns                            -> tempo_tail_kernel (rts_otw_tempo,
//                                                                                             rts_wtw_tempo, one launch per feed
//                                                                                             of a live handle)
//   the tempo curve of an offline alignment (rts_dtw_paths, backward paths, stored paths)   -> tempo_curve_kernel (rts_path_tempo)
//   slope in beats per minute through the annotation tables                                 -> rts_annot_bpm
// The definition is include/rtsync.h's (rts_path_tempo); limits, the overflow rule and the launch geometry are
// csrc/tempo_plan.h's.
//
// Arithmetic.  The per-point terms x, y, x^2, xy are summed as unsigned 64-bit integers that may wrap: den = n Sxx - Sx^2
// and num = n Sxy - Sx Sy formed from them are the true integers modulo 2^64, hence the true integers whenever those fit
// in int64, which tempo_overflows() guarantees for windows without a bad point.  A bad point (outside the limits) only
// counts: its window is NaN whatever its terms wrapped to.  The float64 part is tempo_fit, one rounding per operation (the
// build compiles with -ffp-contract=off).
//
// Every kernel bounds what it reads: path points inside min(len, P_max) / min(stored, path_cap), rows inside the piece's
// own range, the LDS ring inside its kTempoChunk + K entries.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "annot_device.h"
#include "common.h"
#include "tempo_device.h"
#include "tempo_plan.h"

namespace rts {

// One workgroup per path, kTempoChunk points per turn, one per lane.  Per turn: the lanes' terms are scanned inside each
// wave by shuffles, the waves' totals meet in LDS, and with the carry of the turns before every lane holds the running sums
// up to its own point, which it leaves in the ring; its window's sums are those minus the ring's entry K points back.
// Dynamic LDS: the ring, tempo_curve_lds_bytes(K).
__global__ void __launch_bounds__(kTempoThreads)
tempo_curve_kernel(const int32_t *path, int P_max, const int32_t *len_dev, int K, double ahead, long long x_limit,
                   long long y_limit, double *slope_out, double *pos_out) {
    extern __shared__ uint64_t tempo_ring[];
    __shared__ uint64_t wave_tot[kTempoWaves][kTempoSums];
    __shared__ uint32_t wave_bad[kTempoWaves];
    const int R = tempo_ring_entries(K);
    uint64_t *r_x = tempo_ring, *r_y = tempo_ring + R, *r_xx = tempo_ring + 2 * (size_t)R, *r_xy = tempo_ring + 3 * (size_t)R;
    uint32_t *r_bad = reinterpret_cast<uint32_t *>(tempo_ring + 4 * (size_t)R);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int n = len_dev[b];
    if (n > P_max) n = P_max;
    const int2 *pts = reinterpret_cast<const int2 *>(path) + (size_t)b * P_max;
    TempoSums carry = {0, 0, 0, 0, 0};
    int s0 = 0;  // the ring slot of point `base`
    for (int base = 0; base < n; base += kTempoChunk) {
        const int i = base + tid;
        const bool have = i < n;
        int2 p = make_int2(0, 0);
        TempoSums v = {0, 0, 0, 0, 0};
        if (have) {
            p = pts[i];
            v = tempo_point(p.x, p.y, x_limit, y_limit);
        }
        for (int d = 1; d < 64; d <<= 1) {
            const TempoSums up = tempo_shfl_up(v, d);
            if (lane >= d) tempo_add(v, up);
        }
        if (lane == 63) {
            wave_tot[w][0] = v.x;
            wave_tot[w][1] = v.y;
            wave_tot[w][2] = v.xx;
            wave_tot[w][3] = v.xy;
            wave_bad[w] = v.bad;
        }
        __syncthreads();
        tempo_add(v, carry);
        for (int q = 0; q < kTempoWaves; q++) {
            const TempoSums tq = {wave_tot[q][0], wave_tot[q][1], wave_tot[q][2], wave_tot[q][3], wave_bad[q]};
            if (q < w) tempo_add(v, tq);
            tempo_add(carry, tq);
        }
        const int slot = tempo_ring_wrap(s0 + tid, R);
        r_x[slot] = v.x;
        r_y[slot] = v.y;
        r_xx[slot] = v.xx;
        r_xy[slot] = v.xy;
        r_bad[slot] = v.bad;
        __syncthreads();
        if (have) {
            int nw = i + 1;
            if (i >= K) {  // the sums up to point i - K leave the window
                nw = K;
                const int back = tempo_ring_back(slot, K, R);
                const TempoSums old = {r_x[back], r_y[back], r_xx[back], r_xy[back], r_bad[back]};
                tempo_sub(v, old);
            }
            double sl, ps;
            tempo_fit(nw, v, p.x, p.y, ahead, &sl, &ps);
            const size_t e = (size_t)b * P_max + i;
            slope_out[e] = sl;
            if (pos_out) pos_out[e] = ps;
        }
        s0 = tempo_ring_wrap(s0 + kTempoChunk, R);
        // the next turn writes wave_tot before its first barrier (read above, before this turn's second one) and the
        // ring behind it (slots this turn's lanes read above): both are ordered by the barriers as they stand
    }
}

// Beats per minute of `slope` at frame `frame` of `piece`: one beat per table segment, like get_beat.
__device__ __forceinline__ double tempo_bpm(const AnnotTables &t, int piece, long long frame, double slope) {
    const AnnotPiece p = annot_piece(t, piece);
    if (p.n < 1 || frame < 0 || slope != slope) return annot_nan();
    const double time = (double)frame * t.frame_seconds;
    const int i = annot_row(p, time);
    if (i >= p.n) return annot_nan();
    const double end = p.times[i];
    if (i == 0 && end == 0.0) return annot_nan();
    const double start = i == 0 ? 0.0 : p.times[i - 1];
    if (end == start) return annot_nan();
    const double bpm = (slope * 60.0) / (end - start);
    return bpm == bpm ? bpm : annot_nan();
}

// One wave per stream: lane l adds the terms of points l, l + 64, ... of the stream's last n = min(K, stored) points, a
// butterfly of shuffles adds the lanes, lane 0 fits and stores.  No LDS, no barrier.
__global__ void __launch_bounds__(kTempoTailThreads) tempo_tail_kernel(TempoTail t, AnnotTables a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int Nb = t.ref_len ? t.ref_len[b] : t.N;
    const long long y_limit = Nb, x_limit = 2 * (long long)Nb;
    int points = t.state[(size_t)b * t.state_len + t.st_n_path];  // counts on past path_cap once the path is truncated
    points = points > t.path_cap ? t.path_cap : (points < 0 ? 0 : points);
    const int n = points < t.K ? points : t.K;
    const int2 *pts = reinterpret_cast<const int2 *>(t.path) + (size_t)b * t.path_cap + (points - n);
    TempoSums v = {0, 0, 0, 0, 0};
    for (int k = lane; k < n; k += kTempoTailThreads) {
        const int2 p = pts[k];
        tempo_add(v, tempo_point(p.x, p.y, x_limit, y_limit));
    }
    for (int m = 32; m >= 1; m >>= 1) {
        const TempoSums o = tempo_shfl_xor(v, m);
        tempo_add(v, o);
    }
    if (lane != 0) return;
    double sl = annot_nan(), ps = annot_nan(), bpm = annot_nan();
    if (n > 0) {
        const int2 last = pts[n - 1];
        tempo_fit(n, v, last.x, last.y, t.ahead, &sl, &ps);
        if (t.bpm && t.piece && t.frame0) {
            const long long frame = last.y < 0 ? -1 : (long long)last.y + t.frame0[b];
            bpm = tempo_bpm(a, t.piece[b], frame, sl);
        }
    }
    t.slope[b] = sl;
    if (t.pos) t.pos[b] = ps;
    if (t.bpm) t.bpm[b] = bpm;
    t.n_out[b] = n;
    __threadfence_system();
}

// grid (ceil(n_max / 256), B): one lane per entry, like annot_beats_kernel.
__global__ void __launch_bounds__(kTempoBpmThreads)
tempo_bpm_kernel(AnnotTables t, const int32_t *frames, const double *slope, int n_max, const int32_t *n_dev,
                 const int32_t *piece_dev, const int32_t *frame0_dev, double *bpm_out) {
    const int b = blockIdx.y;
    const int k = blockIdx.x * kTempoBpmThreads + threadIdx.x;
    int n = n_dev ? n_dev[b] : n_max;
    if (n > n_max) n = n_max;
    if (k >= n) return;
    const size_t e = (size_t)b * n_max + k;
    const int32_t f = frames[e];
    const long long frame = f < 0 ? -1 : (long long)f + (frame0_dev ? frame0_dev[b] : 0);
    bpm_out[e] = tempo_bpm(t, piece_dev[b], frame, slope[e]);
}

int tempo_tail_check(int K, double ahead, int N_max) {
    if (!tempo_k_ok(K)) return set_error(RTS_ERR_INVALID, "K must be in [%d, %d] (got %d)", kTempoMinK, kTempoMaxK, K);
    if (!isfinite(ahead)) return set_error(RTS_ERR_INVALID, "ahead must be finite");
    if (tempo_overflows(K, 2 * (long long)N_max, N_max))
        return set_error(RTS_ERR_UNSUPPORTED, "K^2 * x_limit * y_limit = %d^2 * %lld * %d reaches 2^63: the window's sums may "
                                              "leave int64", K, 2 * (long long)N_max, N_max);
    return RTS_OK;
}

int tempo_tail_enqueue(const TempoTail &t, const rts_annot *annot, hipStream_t s) {
    AnnotTables none = {};  // P == 0: no piece has a table
    hipLaunchKernelGGL(tempo_tail_kernel, dim3(t.B), dim3(kTempoTailThreads), 0, s, t, annot ? *annot_tables(annot) : none);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

}  // namespace rts

extern "C" {

int rts_path_tempo(const int32_t *path_dev, int P_max, const int32_t *len_dev, int B, int K, double ahead, long long x_limit,
                   long long y_limit, double *slope_dev, double *pos_dev, void *stream) {
    using namespace rts;
    if (!len_dev) return set_error(RTS_ERR_INVALID, "len_dev is NULL");
    if (!slope_dev) return set_error(RTS_ERR_INVALID, "slope_dev is NULL");
    if (B < 1) return set_error(RTS_ERR_INVALID, "B must be >= 1 (got %d)", B);
    if (P_max < 0 || (P_max > 0 && !path_dev)) return set_error(RTS_ERR_INVALID, "path_dev is NULL or P_max < 0");
    if (!tempo_k_ok(K)) return set_error(RTS_ERR_INVALID, "K must be in [%d, %d] (got %d)", kTempoMinK, kTempoMaxK, K);
    if (!isfinite(ahead)) return set_error(RTS_ERR_INVALID, "ahead must be finite");
    if (x_limit < 1 || y_limit < 1)
        return set_error(RTS_ERR_INVALID, "x_limit and y_limit must be >= 1 (got %lld, %lld)", x_limit, y_limit);
    if (tempo_overflows(K, x_limit, y_limit))
        return set_error(RTS_ERR_UNSUPPORTED, "K^2 * x_limit * y_limit = %d^2 * %lld * %lld reaches 2^63: the window's sums may "
                                              "leave int64", K, x_limit, y_limit);
    if (P_max == 0) return RTS_OK;
    static_assert(tempo_curve_lds_bytes(kTempoMaxK) <= kTempoLdsLimit, "the ring fits the default dynamic LDS limit");
    hipLaunchKernelGGL(tempo_curve_kernel, dim3(B), dim3(kTempoThreads), tempo_curve_lds_bytes(K), (hipStream_t)stream, path_dev,
                       P_max, len_dev, K, ahead, x_limit, y_limit, slope_dev, pos_dev);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

int rts_annot_bpm(rts_annot *h, const int32_t *frames_dev, const double *slope_dev, int n_max, const int32_t *n_dev,
                  const int32_t *piece_dev, const int32_t *frame0_dev, int B, double *bpm_dev, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!frames_dev || !slope_dev || !piece_dev || !bpm_dev)
        return set_error(RTS_ERR_INVALID, "frames_dev, slope_dev, piece_dev and bpm_dev must be given");
    if (B < 1 || B > 65535) return set_error(RTS_ERR_INVALID, "B must be in [1, 65535] (got %d)", B);
    if (n_max < 0) return set_error(RTS_ERR_INVALID, "n_max must be >= 0");
    if (int rc = check_device(annot_device(h), "handle"); rc != RTS_OK) return rc;
    if (n_max == 0) return RTS_OK;
    const TempoGrid g = tempo_bpm_grid(B, n_max);
    hipLaunchKernelGGL(tempo_bpm_kernel, dim3(g.x, g.y), dim3(kTempoBpmThreads), 0, (hipStream_t)stream, *annot_tables(h),
                       frames_dev, slope_dev, n_max, n_dev, piece_dev, frame0_dev, bpm_dev);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

}  // extern "C"
