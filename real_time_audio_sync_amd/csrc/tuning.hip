// Tuning: how far a source lies from A4 = 440 Hz, found on the device from the STFT rts_chroma_frames writes.
//   chroma.py:24   "# TODO: check additions (tuning, normalization, etc.)": the reference's front end is built for 440 Hz
//                  and nothing else                                          -> tuning_hist_kernel (rts_tuning_accumulate)
//                                                                               tuning_pick_kernel (rts_tuning_pick)
// The definition is include/rtsync.h's (rts_tuning_accumulate); the rules create and pick check, the LDS layout, the edge
// search and the pick's arithmetic are csrc/tuning_plan.h's.
//
// Arithmetic.  Every float64 operation is rounded on its own, in the order the header gives (contraction is off for this
// file as for the whole build); sqrt and / are the correctly rounded ones.  Peak frequencies are placed by a binary search
// in a table of edges the host built, so no logarithm is taken here, and the counts are integers: the histogram is the
// same whatever the order of the adds.
//
// Every kernel bounds what it reads and writes: bins inside [0, n_bins) of frames inside [0, n_frames), edges inside
// [0, n_edges), histogram rows inside [0, S) (a frame whose segment lies outside is dropped), bins inside [0, R).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "common.h"
#include "tuning_plan.h"

#pragma clang fp contract(off)

namespace rts {

struct TuningGeom {
    int n_bins, k_lo, k_hi, R, n_edges;
    double bin_hz, thr_pow;
    const double *edges;  // device, [n_edges]
    TuningLds lds;
};

// The workgroup's counters into row `seg` of the caller's histogram, and back to zero.  The caller has a barrier between
// the last LDS add and this, and one between this and the next.
__device__ __forceinline__ void tuning_flush(uint32_t *h, int R, unsigned long long *hist, int seg) {
    for (int i = threadIdx.x; i < R; i += kTuningThreads) {
        const uint32_t v = h[i];
        if (v) {
            atomicAdd(&hist[(size_t)seg * R + i], (unsigned long long)v);
            h[i] = 0;
        }
    }
}

// One persistent workgroup per contiguous range of frames.  Per frame: the lanes' registers, loaded one frame ahead with
// 16-byte loads, become P in LDS and a lane maximum; the wave maxima meet in LDS; after the barrier the next frame's loads
// are issued and every lane tests its bins of [k_lo, k_hi] in LDS, the few dozen peaks doing the interpolation, the edge
// search and one LDS add each.  The counters go to the caller's histogram when the segment changes and at the end.
__global__ void __launch_bounds__(kTuningThreads)
tuning_hist_kernel(TuningGeom g, const double2 *stft, long long n_frames, const int32_t *seg_dev, int S,
                   unsigned long long *hist) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tuning_lds_raw[];
    double *P = reinterpret_cast<double *>(tuning_lds_raw);
    double *E_lds = reinterpret_cast<double *>(tuning_lds_raw + g.lds.edges_off);
    double *wmax = reinterpret_cast<double *>(tuning_lds_raw + g.lds.wmax_off);
    uint32_t *h = reinterpret_cast<uint32_t *>(tuning_lds_raw + g.lds.hist_off);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int G = gridDim.x;
    const long long m0 = tuning_first_frame(n_frames, G, blockIdx.x), m1 = tuning_first_frame(n_frames, G, blockIdx.x + 1);
    if (m0 >= m1) return;

    for (int i = tid; i < g.R; i += kTuningThreads) h[i] = 0;
    if (g.lds.edges_staged)
        for (int i = tid; i < g.n_edges; i += kTuningThreads) E_lds[i] = g.edges[i];

    double2 v[kTuningPerLane];
    const double2 *src = stft + (size_t)m0 * g.n_bins;
#pragma unroll
    for (int q = 0; q < kTuningPerLane; q++) {
        const int k = tid + q * kTuningThreads;
        v[q] = k < g.n_bins ? src[k] : make_double2(0.0, 0.0);
    }

    int cur = -1;  // the segment the counters belong to; -1: none yet, they are zero
    long long since = 0;
    for (long long m = m0; m < m1; m++) {
        int seg = seg_dev ? seg_dev[m] : 0;
        if (seg < 0 || seg >= S) seg = -1;  // the frame counts nowhere
        if (seg >= 0 && (seg != cur || since >= kTuningFlushFrames)) {
            if (cur >= 0) tuning_flush(h, g.R, hist, cur);  // behind the barrier that ended the frame before
            cur = seg;
            since = 0;
        }
        double mx = 0.0;  // P >= 0
#pragma unroll
        for (int q = 0; q < kTuningPerLane; q++) {
            const int k = tid + q * kTuningThreads;
            if (k < g.n_bins) {
                const double re2 = v[q].x * v[q].x, im2 = v[q].y * v[q].y;
                const double p = re2 + im2;
                P[k] = p;
                mx = p > mx ? p : mx;
            }
        }
        for (int s = 32; s >= 1; s >>= 1) {
            const double o = __shfl_xor(mx, s, 64);
            mx = o > mx ? o : mx;
        }
        if (lane == 0) wmax[w] = mx;
        __syncthreads();
        if (m + 1 < m1) {  // the next frame's loads fly while this one is searched
            src += g.n_bins;
#pragma unroll
            for (int q = 0; q < kTuningPerLane; q++) {
                const int k = tid + q * kTuningThreads;
                v[q] = k < g.n_bins ? src[k] : make_double2(0.0, 0.0);
            }
        }
        if (seg >= 0) {
            double pmax = wmax[0];
#pragma unroll
            for (int q = 1; q < kTuningWaves; q++) pmax = wmax[q] > pmax ? wmax[q] : pmax;
            const double lim = g.thr_pow * pmax;
            for (int k = g.k_lo + tid; k <= g.k_hi; k += kTuningThreads) {  // 1 <= k <= n_bins - 2
                const double pa = P[k - 1], pb = P[k], pc = P[k + 1];
                if (pb > pa && pb >= pc && pb >= lim) {
                    const double a = sqrt(pa), b = sqrt(pb), c = sqrt(pc);
                    const double avg = 0.5 * (c - a);
                    const double sh = (2.0 * b - c) - a;
                    const double d = sh > 0 ? avg / sh : 0.0;
                    const double f = ((double)k + d) * g.bin_hz;
                    const int n = g.lds.edges_staged ? tuning_edge_index(E_lds, g.n_edges, f)
                                                     : tuning_edge_index(g.edges, g.n_edges, f);
                    const int bin = tuning_hist_bin(n, g.n_edges, g.R);
                    if (bin >= 0) atomicAdd(&h[bin], 1u);
                }
            }
            since++;
        }
        __syncthreads();  // P, the wave maxima and the counters are this frame's up to here
    }
    if (cur >= 0) tuning_flush(h, g.R, hist, cur);
}

// One workgroup per histogram row: the row into LDS, its sum by a tree of adds (integers: any order), one score per lane
// and bin, and the first maximum by the order tuning_beats gives.
constexpr int kTuningPickThreads = 256;
__global__ void __launch_bounds__(kTuningPickThreads)
tuning_pick_kernel(const unsigned long long *hist, int R, int W, double *cents_out, long long *n_out) {
    __shared__ uint64_t row[kTuningMaxR];
    __shared__ uint64_t red_s[kTuningPickThreads];
    __shared__ int red_i[kTuningPickThreads];
    const int s = blockIdx.x, tid = threadIdx.x;
    uint64_t sum = 0;
    for (int i = tid; i < R; i += kTuningPickThreads) {
        row[i] = hist[(size_t)s * R + i];
        sum += row[i];
    }
    red_s[tid] = sum;
    __syncthreads();
    for (int step = kTuningPickThreads / 2; step >= 1; step >>= 1) {
        if (tid < step) red_s[tid] += red_s[tid + step];
        __syncthreads();
    }
    const uint64_t N = red_s[0];
    __syncthreads();
    uint64_t best = 0;
    int at = R;  // no bin yet: any bin beats it
    for (int i = tid; i < R; i += kTuningPickThreads) {
        const uint64_t sc = tuning_score(row, R, W, i);
        if (at == R || tuning_beats(sc, i, best, at)) {
            best = sc;
            at = i;
        }
    }
    red_s[tid] = best;
    red_i[tid] = at;
    __syncthreads();
    for (int step = kTuningPickThreads / 2; step >= 1; step >>= 1) {
        if (tid < step) {
            const uint64_t so = red_s[tid + step];
            const int io = red_i[tid + step];
            if (io < R && (red_i[tid] == R || tuning_beats(so, io, red_s[tid], red_i[tid]))) {
                red_s[tid] = so;
                red_i[tid] = io;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        cents_out[s] = N == 0 ? 0.0 : tuning_cents(red_i[0], R);
        n_out[s] = (long long)N;
    }
}

}  // namespace rts

struct rts_tuning {
    rts::TuningGeom g;
    int fft_len;
    int device;
};

extern "C" {

int rts_tuning_destroy(rts_tuning *p) {
    if (!p) return RTS_OK;
    if (p->g.edges) (void)hipFree(const_cast<double *>(p->g.edges));
    free(p);
    return RTS_OK;
}

int rts_tuning_create(int fft_len, int k_lo, int k_hi, int R, int n_edges, const double *edges_host, double bin_hz,
                      double thr_pow, rts_tuning **out) {
    using namespace rts;
    if (!out) return set_error(RTS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int bad = 0;
    const int why = tuning_create_refusal(fft_len, k_lo, k_hi, R, n_edges, edges_host, bin_hz, thr_pow, &bad);
    const int code = tuning_refusal_unsupported(why) ? RTS_ERR_UNSUPPORTED : RTS_ERR_INVALID;
    switch (why) {
    case kTuningOk: break;
    case kTuningBadFft:
        return set_error(code, "fft_len must be a power of two in [%d, %d] (got %d)", kTuningMinFft, kTuningMaxFft, fft_len);
    case kTuningBadBins:
        return set_error(code, "need 1 <= k_lo <= k_hi <= fft_len / 2 - 1 = %d (got k_lo %d, k_hi %d)", fft_len / 2 - 1, k_lo, k_hi);
    case kTuningBadR: return set_error(code, "R must be >= 1 (got %d)", R);
    case kTuningBigR: return set_error(code, "R = %d histogram bins exceed the supported %d", R, kTuningMaxR);
    case kTuningFewEdges: return set_error(code, "n_edges must be >= 2 (got %d)", n_edges);
    case kTuningNoEdges: return set_error(code, "edges_host is NULL");
    case kTuningBadEdges:
        return set_error(code, "edges_host[%d] is not finite, positive and above the edge before it", bad);
    case kTuningBadThr: return set_error(code, "thr_pow must be in [0, 1]");
    default: return set_error(code, "bin_hz must be finite and > 0");
    }
    rts_tuning *p = (rts_tuning *)calloc(1, sizeof(rts_tuning));
    if (!p) return set_error(RTS_ERR_INVALID, "out of host memory");
    double *dev = nullptr;
    hipError_t e = hipGetDevice(&p->device);
    if (e == hipSuccess) e = hipMalloc((void **)&dev, sizeof(double) * (size_t)n_edges);
    if (e == hipSuccess) e = hipMemcpy(dev, edges_host, sizeof(double) * (size_t)n_edges, hipMemcpyHostToDevice);
    p->g.edges = dev;
    if (e != hipSuccess) {
        rts_tuning_destroy(p);
        return set_error(RTS_ERR_HIP, "rts_tuning_create: %s", hipGetErrorString(e));
    }
    p->fft_len = fft_len;
    p->g.n_bins = fft_len / 2 + 1;
    p->g.k_lo = k_lo;
    p->g.k_hi = k_hi;
    p->g.R = R;
    p->g.n_edges = n_edges;
    p->g.bin_hz = bin_hz;
    p->g.thr_pow = thr_pow;
    p->g.lds = tuning_lds(fft_len, n_edges, R);
    static_assert(tuning_lds_bytes(kTuningMaxFft, 0, kTuningMaxR, false) <= kTuningLdsLimit, "P and the counters fit without the edges");
    *out = p;
    return RTS_OK;
}

int rts_tuning_accumulate(rts_tuning *p, const double *stft_dev, long long n_frames, const int32_t *seg_dev, int S,
                          unsigned long long *hist_dev, void *stream) {
    using namespace rts;
    if (!p) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (n_frames < 0) return set_error(RTS_ERR_INVALID, "n_frames must be >= 0 (got %lld)", n_frames);
    if (S < 1) return set_error(RTS_ERR_INVALID, "S must be >= 1 (got %d)", S);
    if (n_frames == 0) return RTS_OK;
    if (!stft_dev) return set_error(RTS_ERR_INVALID, "stft_dev is NULL");
    if (((uintptr_t)stft_dev & 15) != 0) return set_error(RTS_ERR_INVALID, "stft_dev must be 16-byte aligned");
    if (!hist_dev) return set_error(RTS_ERR_INVALID, "hist_dev is NULL");
    if (int rc = check_device(p->device, "handle"); rc != RTS_OK) return rc;
    hipLaunchKernelGGL(tuning_hist_kernel, dim3(tuning_groups(n_frames)), dim3(kTuningThreads), p->g.lds.bytes,
                       (hipStream_t)stream, p->g, reinterpret_cast<const double2 *>(stft_dev), n_frames, seg_dev, S, hist_dev);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

int rts_tuning_pick(rts_tuning *p, const unsigned long long *hist_dev, int S, int W, double *cents_dev, long long *n_dev,
                    void *stream) {
    using namespace rts;
    if (!p) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!hist_dev || !cents_dev || !n_dev) return set_error(RTS_ERR_INVALID, "hist_dev, cents_dev and n_dev must be given");
    if (S < 1) return set_error(RTS_ERR_INVALID, "S must be >= 1 (got %d)", S);
    if (tuning_pick_refusal(p->g.R, W) != kTuningOk)
        return set_error(RTS_ERR_INVALID, "W must be >= 0 with 2 W + 1 <= R = %d (got %d)", p->g.R, W);
    if (int rc = check_device(p->device, "handle"); rc != RTS_OK) return rc;
    hipLaunchKernelGGL(tuning_pick_kernel, dim3(S), dim3(kTuningPickThreads), 0, (hipStream_t)stream, hist_dev, p->g.R, W,
                       cents_dev, n_dev);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

}  // extern "C"
