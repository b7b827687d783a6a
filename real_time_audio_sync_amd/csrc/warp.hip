// Renderer: one recording on another's time axis, along an alignment path.  Time-scale modification by waveform-similarity
// overlap-add (WSOLA) along a piecewise-linear integer time map, defined by this project to the bit (include/rtsync.h,
// rts_warp_run; tests/warp_model.py is the definition in numpy).  The reference has no renderer.
//
//   frames of N samples, hop H = N / 2, window w[0 .. N) (host doubles), x[n] = 0 outside the signal
//   a_k  = the map at output position k H                                         (exact 64-bit integers)
//   p_0  = a_0;  p_k = a_k + the delta in [-D, D] whose frame x[a_k + delta ..] correlates best with the natural
//          continuation x[p_{k-1} + H ..] of the frame before (first maximum in the order 0, -D, -D + 1, .., D)
//   y[k H + m] = float32( w[m + H] * (double)x[p_{k-1} + H + m] + w[m] * (double)x[p_k + m] ),  m = 0 .. H-1
//
// Layout.  The chain p_{k-1} -> p_k is serial, so one workgroup walks the blocks of one stream in order.  Per block it
// stages the target frame (N floats) and the candidate window x[a_k - D .. a_k + D + N) in LDS.  Lanes own candidates:
// lane l of a turn reads window[j + i], consecutive lanes consecutive addresses (ds_read_b32, conflict-free), against
// target[i], the same address in every lane (a broadcast, read 16 bytes at a time).  The eight partial sums of the
// definition are eight independent add chains per lane.  The 2 D candidates other than delta = 0 divide evenly among the
// lanes when D is a multiple of 256; delta = 0 would leave one lane a whole turn of its own, so eight lanes of wave 0 take
// its eight partial sums instead, one chain of N / 8 terms each, and a shuffle tree adds them in the defined order.  The
// argmax over (value, scan order) goes down each wave by shuffles and across the waves through LDS.  The block's two
// frames are then both in LDS and the workgroup writes it with 16-byte stores.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>

#include "common.h"
#include "warp_plan.h"

// The two products of an output sample are not exact in float64 (the window is a double), so the bit contract forbids
// contracting them with the add into a fused multiply-add: one multiply each, one add, one rounding to float32.  This
// pragma switches contraction off for everything below under the build's -ffp-contract=off and under hipcc's own default
// alike (csrc/resample.hip has the long form); -ffp-contract=fast ignores it, and this file must never be built with
// it.  The correlation sums do use fma(), explicitly: the product of two float32 values is exact in float64, only the
// add rounds, and fma(a, b, s) gives the bits of s + a * b.
#pragma clang fp contract(off)

namespace rts {

struct WarpGeom {
    const double *w;  // [N] on the device
    int N, H, delta;
};

__device__ __forceinline__ float warp_sample(const void *src, int kind, long long i, long long n_in) {
    if (i < 0 || i >= n_in) return 0.0f;
    return kind == RTS_F32 ? reinterpret_cast<const float *>(src)[i]
                           : (float)reinterpret_cast<const int16_t *>(src)[i] * (1.0f / 32768.0f);  // exact
}

// (value, rank) `a` beats `b`: greater, or equal and earlier in the scan.  A NaN value beats nothing.
__device__ __forceinline__ bool warp_beats(double av, int ar, double bv, int br) { return av > bv || (av == bv && ar < br); }

// One workgroup per stream: blocks k .. min(k + k_count, K) - 1 of the stream, k and p_{k-1} from state[b].
__global__ void __launch_bounds__(kWarpThreads)
    warp_run_kernel(WarpGeom g, const void *samples, int kind, long long sample_stride, const long long *n_in_dev,
                    const long long *anchors, const int32_t *n_anchor_dev, int A_max, const long long *n_out_dev,
                    long long *state, long long k_count, float *out, long long out_stride, int32_t *status_dev) {
    extern __shared__ __attribute__((aligned(16))) float warp_lds[];
    __shared__ double red_v[kWarpWaves];
    __shared__ int red_r[kWarpWaves];
    __shared__ double c0_s;
    __shared__ int bad_s;
    const int N = g.N, H = g.H, D = g.delta;
    float *tgt = warp_lds;      // x[p_{k-1} + H + i], i < N
    float *win = warp_lds + N;  // x[a_k - D + i],     i < N + 2 D
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    const int A = n_anchor_dev[b];
    long long n_in = n_in_dev[b];
    const long long n_out = n_out_dev[b];
    const long long k_start = state[2 * b];
    long long p_prev = state[2 * b + 1];
    if (A < 2 || A > A_max) {  // no map: rts_warp_anchors refused the path
        if (tid == 0) status_dev[b] = RTS_WARP_NO_MAP;
        return;
    }
    if (n_out < 0 || n_out >= kWarpPosLimit || k_start < 0 || p_prev <= -kWarpPosLimit || p_prev >= kWarpPosLimit) {
        if (tid == 0) status_dev[b] = RTS_WARP_BAD_STATE;
        return;
    }
    if (n_in < 0) n_in = 0;
    const long long *an = anchors + (size_t)b * (size_t)A_max * 2;

    // every segment of the map, before any position is computed from it
    if (tid == 0) bad_s = an[0] != 0;
    __syncthreads();
    for (int s = tid; s < A - 1; s += kWarpThreads) {
        const long long o1 = an[2 * s + 2];
        const long long reach = (s == A - 2 && n_out > o1) ? n_out : o1;
        if (!warp_segment_ok(an[2 * s], an[2 * s + 1], o1, an[2 * s + 3], reach)) bad_s = 1;
    }
    __syncthreads();
    if (bad_s) {
        if (tid == 0) status_dev[b] = RTS_WARP_BAD_MAP;
        return;
    }

    const long long K = n_out / H + (n_out % H != 0);
    if (k_start > K) {
        if (tid == 0) status_dev[b] = RTS_WARP_BAD_STATE;
        return;
    }
    const long long k_end = K - k_start < k_count ? K : k_start + k_count;
    const size_t esz = kind == RTS_F32 ? sizeof(float) : sizeof(int16_t);
    const void *src = reinterpret_cast<const unsigned char *>(samples) + (size_t)b * (size_t)sample_stride * esz;
    float *row = out + (size_t)b * (size_t)out_stride;
    const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;  // H % 8 == 0: every block of the row is aligned alike

    // the cursor: the last anchor at or before k_start H by bisection, forward only from there
    int s = 0;
    if (k_start < k_end) {
        const long long t0 = k_start * H;
        int lo = 0, hi = A - 2;  // an[2 lo] <= t0 holds: an[0] = 0
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (an[2 * mid] <= t0) lo = mid; else hi = mid - 1;
        }
        s = lo;
    }
    long long o0 = an[2 * s], i0 = an[2 * s + 1], o1 = an[2 * s + 2], i1 = an[2 * s + 3];

    for (long long k = k_start; k < k_end; k++) {
        const long long t = k * H;
        while (s < A - 2 && o1 <= t) {
            s++;
            o0 = o1, i0 = i1, o1 = an[2 * s + 2], i1 = an[2 * s + 3];
        }
        const long long a = warp_map_pos(t, o0, i0, o1, i1);
        if (k > 0)
            for (int i = tid; i < N; i += kWarpThreads) tgt[i] = warp_sample(src, kind, p_prev + H + i, n_in);
        for (int i = tid; i < N + 2 * D; i += kWarpThreads) win[i] = warp_sample(src, kind, a - D + i, n_in);
        __syncthreads();

        int best_j = D;  // delta = 0
        if (k > 0 && D > 0) {
            double bv = -__builtin_inf();
            int br = INT_MAX;
            for (int c = tid; c < 2 * D; c += kWarpThreads) {
                const int j = c < D ? c : c + 1;  // window offset of delta = j - D; delta = 0 is wave 0's, below
                const float *cp = win + j;
                double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0, s6 = 0.0, s7 = 0.0;
                // the reads of step q + 8 are issued before the sums of step q, so that a wave waits for LDS once per step
                // and not once per pair of reads
                float c0 = cp[0], c1 = cp[1], c2 = cp[2], c3 = cp[3], c4 = cp[4], c5 = cp[5], c6 = cp[6], c7 = cp[7];
                float4 ta = *reinterpret_cast<const float4 *>(tgt), tb = *reinterpret_cast<const float4 *>(tgt + 4);
#define RTS_WARP_SUMS()                                   \
    s0 = __builtin_fma((double)c0, (double)ta.x, s0);     \
    s1 = __builtin_fma((double)c1, (double)ta.y, s1);     \
    s2 = __builtin_fma((double)c2, (double)ta.z, s2);     \
    s3 = __builtin_fma((double)c3, (double)ta.w, s3);     \
    s4 = __builtin_fma((double)c4, (double)tb.x, s4);     \
    s5 = __builtin_fma((double)c5, (double)tb.y, s5);     \
    s6 = __builtin_fma((double)c6, (double)tb.z, s6);     \
    s7 = __builtin_fma((double)c7, (double)tb.w, s7)
                for (int q = 8; q < N; q += 8) {
                    const float n0 = cp[q + 0], n1 = cp[q + 1], n2 = cp[q + 2], n3 = cp[q + 3];
                    const float n4 = cp[q + 4], n5 = cp[q + 5], n6 = cp[q + 6], n7 = cp[q + 7];
                    const float4 na = *reinterpret_cast<const float4 *>(tgt + q);
                    const float4 nb = *reinterpret_cast<const float4 *>(tgt + q + 4);
                    RTS_WARP_SUMS();
                    c0 = n0, c1 = n1, c2 = n2, c3 = n3, c4 = n4, c5 = n5, c6 = n6, c7 = n7;
                    ta = na, tb = nb;
                }
                RTS_WARP_SUMS();
#undef RTS_WARP_SUMS
                const double cv = ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7));
                if (warp_beats(cv, j + 1, bv, br)) bv = cv, br = j + 1;
            }
            if (wave == 0) {
                // delta = 0, rank 0: lane r < 8 runs the chain s_r, lane 0 adds the eight in the defined order
                double sr = 0.0;
                if (lane < 8)
                    for (int q = lane; q < N; q += 8) sr = __builtin_fma((double)win[D + q], (double)tgt[q], sr);
                const double e0 = __shfl(sr, 0), e1 = __shfl(sr, 1), e2 = __shfl(sr, 2), e3 = __shfl(sr, 3);
                const double e4 = __shfl(sr, 4), e5 = __shfl(sr, 5), e6 = __shfl(sr, 6), e7 = __shfl(sr, 7);
                const double c0 = ((e0 + e1) + (e2 + e3)) + ((e4 + e5) + (e6 + e7));
                if (lane == 0) {
                    c0_s = c0;
                    if (warp_beats(c0, 0, bv, br)) bv = c0, br = 0;
                }
            }
            for (int off = 32; off >= 1; off >>= 1) {
                const double ov = __shfl_down(bv, off);
                const int orr = __shfl_down(br, off);
                if (warp_beats(ov, orr, bv, br)) bv = ov, br = orr;
            }
            if (lane == 0) red_v[wave] = bv, red_r[wave] = br;
            __syncthreads();
            bv = red_v[0], br = red_r[0];
#pragma unroll
            for (int v = 1; v < kWarpWaves; v++)
                if (warp_beats(red_v[v], red_r[v], bv, br)) bv = red_v[v], br = red_r[v];
            const double c0 = c0_s;
            // a NaN at delta = 0 is never replaced (nothing is greater than it); no winner at all: every value was NaN
            best_j = (br == INT_MAX || br == 0 || c0 != c0) ? D : br - 1;
        }
        const long long p = a + (best_j - D);

        // the block: both frames are in LDS
        const float *cur = win + best_j;  // x[p_k + m]
        const long long left = n_out - t;
        const int lim = left < H ? (int)left : H;
        float *dst = row + (size_t)(k - k_start) * (size_t)H;
        for (int m = 4 * tid; m < H; m += 4 * kWarpThreads) {
            float y[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const double f = g.w[m + i] * (double)cur[m + i];
                if (k > 0) {
                    const double e = g.w[m + i + H] * (double)tgt[m + i];
                    y[i] = (float)(e + f);  // the earlier frame's product first; contraction is off (top of the file)
                } else {
                    y[i] = (float)f;
                }
            }
            if (vec && m + 4 <= lim) {
                *reinterpret_cast<float4 *>(dst + m) = make_float4(y[0], y[1], y[2], y[3]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (m + i < lim) dst[m + i] = y[i];
            }
        }
        p_prev = p;
        __syncthreads();  // target and window are restaged by the next block
    }
    if (tid == 0) {
        state[2 * b] = k_end;
        state[2 * b + 1] = p_prev;
        status_dev[b] = 0;
    }
}

// One workgroup per path: the points where u = path[t][onto] changes become anchors (u hop_f, v hop_f), v = path[t][1 -
// onto], and (n_out, n_in) closes the map.  Flags, a workgroup prefix sum (ballots within a wave, wave totals through LDS),
// a scatter; the count so far is carried from turn to turn in a register every lane holds alike.
__global__ void __launch_bounds__(kWarpAnchorThreads)
    warp_anchors_kernel(const int32_t *path, int P_max, const int32_t *path_len_dev, int onto, int hop_f,
                        const long long *n_out_dev, const long long *n_in_dev, long long *anchors, int A_max,
                        int32_t *n_anchor_dev, int32_t *status_dev) {
    __shared__ int wave_cnt[kWarpAnchorWaves];
    __shared__ int st_s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int len = path_len_dev[b];
    if (len > P_max) len = P_max;
    const int32_t *pt = path + (size_t)b * (size_t)P_max * 2;
    long long *an = anchors + (size_t)b * (size_t)A_max * 2;
    if (tid == 0) st_s = len < 1 ? RTS_WARP_PATH_EMPTY : 0;
    __syncthreads();
    int base = 0;
    const int turns = warp_anchor_turns(len, P_max);
    for (int turn = 0; turn < turns; turn++) {
        const int t = turn * kWarpAnchorThreads + tid;
        bool flag = false;
        long long u = 0, v = 0;
        int st = 0;
        if (t < len) {
            u = pt[2 * t + onto], v = pt[2 * t + 1 - onto];
            if (t == 0) {
                flag = true;
                if (u != 0) st |= RTS_WARP_PATH_START;
                if (v < 0) st |= RTS_WARP_PATH_BACKWARD;
            } else {
                const long long up = pt[2 * t - 2 + onto], vp = pt[2 * t - 1 - onto];
                flag = u != up;
                if (u < up || v < vp) st |= RTS_WARP_PATH_BACKWARD;
            }
        }
        if (st) atomicOr(&st_s, st);
        const unsigned long long m = __ballot(flag);
        if (lane == 0) wave_cnt[wave] = __popcll(m);
        __syncthreads();
        int idx = base + __popcll(m & ((1ull << lane) - 1));
        int total = 0;
#pragma unroll
        for (int w = 0; w < kWarpAnchorWaves; w++) {
            if (w < wave) idx += wave_cnt[w];
            total += wave_cnt[w];
        }
        if (flag && idx < A_max) {  // (the closing anchor needs a slot as well: counted below)
            an[2 * idx] = u * hop_f;
            an[2 * idx + 1] = v * hop_f;
        }
        base += total;
        __syncthreads();  // wave_cnt is rewritten by the next turn
    }
    if (tid == 0) {
        int st = st_s;
        const long long n_out = n_out_dev[b], n_in = n_in_dev[b];
        if (len >= 1) {
            const long long ul = pt[2 * (len - 1) + onto], vl = pt[2 * (len - 1) + 1 - onto];
            if (n_out <= ul * hop_f) st |= RTS_WARP_PATH_SHORT_OUT;
            if (n_in < vl * hop_f) st |= RTS_WARP_PATH_SHORT_IN;
        }
        if (base + 1 > A_max) st |= RTS_WARP_PATH_TOO_MANY;
        if (st == 0) {
            an[2 * base] = n_out;
            an[2 * base + 1] = n_in;
        }
        n_anchor_dev[b] = st ? 0 : base + 1;
        status_dev[b] = st;
    }
}

}  // namespace rts

struct rts_warp {
    rts::WarpGeom g;
    int device;
};

extern "C" {

long long rts_warp_blocks(long long n_out, int N) { return rts::warp_blocks(n_out, N); }

int rts_warp_destroy(rts_warp *p) {
    if (!p) return RTS_OK;
    if (p->g.w) (void)hipFree(const_cast<double *>(p->g.w));
    free(p);
    return RTS_OK;
}

int rts_warp_create(int N, int delta, const double *window_host, rts_warp **out) {
    using namespace rts;
    if (!out) return set_error(RTS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (N < 2 || N % 2 != 0) return set_error(RTS_ERR_INVALID, "N must be even and >= 2 (got %d)", N);
    if (delta < 0) return set_error(RTS_ERR_INVALID, "delta must be >= 0 (got %d)", delta);
    if (!window_host) return set_error(RTS_ERR_INVALID, "window_host is NULL");
    if (!warp_n_ok(N))
        return set_error(RTS_ERR_UNSUPPORTED, "N = %d: supported frame lengths are the multiples of 16 in [%d, %d]", N, kWarpMinN, kWarpMaxN);
    if (!warp_delta_ok(delta)) return set_error(RTS_ERR_UNSUPPORTED, "delta = %d exceeds the supported %d", delta, kWarpMaxDelta);
    rts_warp *p = (rts_warp *)calloc(1, sizeof(rts_warp));
    if (!p) return set_error(RTS_ERR_INVALID, "out of host memory");
    double *dev = nullptr;
    hipError_t e = hipGetDevice(&p->device);
    if (e == hipSuccess) e = hipMalloc((void **)&dev, sizeof(double) * (size_t)N);
    if (e == hipSuccess) e = hipMemcpy(dev, window_host, sizeof(double) * (size_t)N, hipMemcpyHostToDevice);
    p->g.w = dev;
    if (e != hipSuccess) {
        rts_warp_destroy(p);
        return set_error(RTS_ERR_HIP, "rts_warp_create: %s", hipGetErrorString(e));
    }
    p->g.N = N;
    p->g.H = N / 2;
    p->g.delta = delta;
    *out = p;
    return RTS_OK;
}

int rts_warp_anchors(const int32_t *path_dev, int P_max, const int32_t *path_len_dev, int onto, int hop_f,
                     const long long *n_out_dev, const long long *n_in_dev, int B, long long *anchors_dev, int A_max,
                     int32_t *n_anchor_dev, int32_t *status_dev, void *stream) {
    using namespace rts;
    if (P_max < 0) return set_error(RTS_ERR_INVALID, "P_max must be >= 0 (got %d)", P_max);
    if (!path_dev && P_max > 0) return set_error(RTS_ERR_INVALID, "path_dev is NULL");
    if (!path_len_dev) return set_error(RTS_ERR_INVALID, "path_len_dev is NULL");
    if (onto != 0 && onto != 1) return set_error(RTS_ERR_INVALID, "onto must be 0 or 1 (got %d)", onto);
    if (hop_f < 1) return set_error(RTS_ERR_INVALID, "hop_f must be >= 1 (got %d)", hop_f);
    if (!n_out_dev) return set_error(RTS_ERR_INVALID, "n_out_dev is NULL");
    if (!n_in_dev) return set_error(RTS_ERR_INVALID, "n_in_dev is NULL");
    if (B < 1 || B > kWarpMaxBatch) return set_error(RTS_ERR_INVALID, "B must be in [1, %d] (got %d)", kWarpMaxBatch, B);
    if (A_max < 2) return set_error(RTS_ERR_INVALID, "A_max must be >= 2 (got %d)", A_max);
    if (!anchors_dev) return set_error(RTS_ERR_INVALID, "anchors_dev is NULL");
    if (!n_anchor_dev) return set_error(RTS_ERR_INVALID, "n_anchor_dev is NULL");
    if (!status_dev) return set_error(RTS_ERR_INVALID, "status_dev is NULL");
    hipLaunchKernelGGL(warp_anchors_kernel, dim3(B), dim3(kWarpAnchorThreads), 0, (hipStream_t)stream, path_dev, P_max,
                       path_len_dev, onto, hop_f, n_out_dev, n_in_dev, anchors_dev, A_max, n_anchor_dev, status_dev);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

int rts_warp_run(rts_warp *plan, const void *samples_dev, int sample_dtype, long long sample_stride,
                 const long long *n_in_dev, const long long *anchors_dev, const int32_t *n_anchor_dev, int A_max,
                 const long long *n_out_dev, long long *state_dev, long long k_count, float *out_dev, long long out_stride,
                 int32_t *status_dev, int B, void *stream) {
    using namespace rts;
    if (!plan) return set_error(RTS_ERR_INVALID, "plan is NULL");
    if (!samples_dev) return set_error(RTS_ERR_INVALID, "samples_dev is NULL");
    if (sample_dtype != RTS_F32 && sample_dtype != RTS_I16) return set_error(RTS_ERR_INVALID, "sample_dtype must be RTS_F32 or RTS_I16");
    if (sample_stride < 0) return set_error(RTS_ERR_INVALID, "sample_stride must be >= 0");
    if (!n_in_dev) return set_error(RTS_ERR_INVALID, "n_in_dev is NULL");
    if (!anchors_dev) return set_error(RTS_ERR_INVALID, "anchors_dev is NULL");
    if (!n_anchor_dev) return set_error(RTS_ERR_INVALID, "n_anchor_dev is NULL");
    if (A_max < 2) return set_error(RTS_ERR_INVALID, "A_max must be >= 2 (got %d)", A_max);
    if (!n_out_dev) return set_error(RTS_ERR_INVALID, "n_out_dev is NULL");
    if (!state_dev) return set_error(RTS_ERR_INVALID, "state_dev is NULL");
    if (k_count < 0) return set_error(RTS_ERR_INVALID, "k_count must be >= 0 (got %lld)", k_count);
    if (out_stride < 0) return set_error(RTS_ERR_INVALID, "out_stride must be >= 0");
    if (!out_dev && k_count > 0) return set_error(RTS_ERR_INVALID, "out_dev is NULL");
    if (!status_dev) return set_error(RTS_ERR_INVALID, "status_dev is NULL");
    if (B < 1 || B > kWarpMaxBatch) return set_error(RTS_ERR_INVALID, "B must be in [1, %d] (got %d)", kWarpMaxBatch, B);
    if (int rc = check_device(plan->device, "plan"); rc != RTS_OK) return rc;
    hipLaunchKernelGGL(warp_run_kernel, dim3(B), dim3(kWarpThreads), warp_lds_bytes(plan->g.N, plan->g.delta),
                       (hipStream_t)stream, plan->g, samples_dev, sample_dtype, sample_stride, n_in_dev, anchors_dev,
                       n_anchor_dev, A_max, n_out_dev, state_dev, k_count, out_dev, out_stride, status_dev);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

}  // extern "C"
