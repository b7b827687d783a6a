// Rational-ratio polyphase resampler on the device: what the reference gets from librosa.load's silent resampling to
// 22 050 Hz (chroma.py:27, wtw.py:23), defined by this project to the bit (DESIGN.md "Resampler") instead of imitating an
// unpinned third-party resampler.
//
//   L / M = fs_out / fs_in (reduced), taps h[-half .. half] as host doubles (filters.resample_taps), and for output k
//     c    = k * M + half                                                     (64-bit)
//     y[k] = float32( sum over n = ceil((c - 2 half) / L) .. floor(c / L), ascending, of h[c - n L - half] * (double)x[n] )
//   each term one float64 multiply and one float64 add, no fused multiply-add, x[n] = 0 outside the signal.
//
// Layout.  With q = floor(c / L) and r = c mod L the taps of one output are h_arr[r + j L], j = 0 .. J_r - 1 (h_arr the
// table indexed from 0, J_r = floor((2 half - r) / L) + 1), against x[q - j].  The plan stores them PHASE-MAJOR and in
// the order of ascending n: row r of `taps` holds h_arr[r + (J_r - 1 - i) L] at column i, so the n loop of one output
// walks contiguous doubles from column 0, and its samples are the contiguous x[q - J_r + 1 .. q].  A workgroup owns a
// tile of consecutive outputs of one stream and stages the input window they cover in LDS once (neighbouring outputs
// share all but M / L of their ~2 half / L samples); every lane owns kOutPerLane outputs a workgroup-width apart, whose
// four independent add chains overlap.  The tap rows are read from global memory (the table is read-only and small
// enough to stay in L2: 82 KB for 147/320, 164 KB for 441/640).
//
// The same tile routine serves the one-shot call (rts_resample_run, grid = tiles x streams, samples from the caller's
// buffers) and the live handle's per-feed launch (one workgroup per stream, samples from the stream's carried tail
// followed by the staged feed; csrc/live.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "live_plan.h"

// The bit contract forbids contracting the multiply and the add of a term into a fused multiply-add.  This pragma
// switches contraction off for everything below under the build's -ffp-contract=off and under hipcc's own default
// (fast-honor-pragmas) alike; __dmul_rn / __dadd_rn would not.  -ffp-contract=fast ignores such pragmas by definition
// and fuses the terms into v_fmac_f64: this file must never be built with it.
#pragma clang fp contract(off)

namespace rts {

constexpr int kRsThreads = 256;
constexpr int kOutPerLane = 4;
constexpr int kRsTileOut = kRsThreads * kOutPerLane;  // most outputs of one tile
constexpr int kRsLiveTile = 512;                      // outputs per tile of the live launch: more workgroups per stream
constexpr int kRsWin = 12288;                         // floats of LDS for a tile's input window (48 KB)
constexpr int kRsMaxSpan = 4096;                      // largest ceil(2 half / L): samples under one output's taps
constexpr long long kRsMaxTaps = 1LL << 22;           // largest 2 half + 1 (32 MB of doubles)

struct RsGeom {
    const double *taps;  // [L][J] phase-major, ascending n
    int L, M, half, J;   // J = floor(2 half / L) + 1: row length, the most taps of one output
    int tile_out;        // outputs per tile, chosen so that a tile's window fits kRsWin
};

// Outputs [k0, k1) of one stream, k1 - k0 <= g.tile_out: stages samples lo .. hi through `fetch(n)` (absolute sample
// index -> float, zero outside the signal) and writes out[k - k0].  Every thread of the workgroup must call it.
template <typename Fetch>
__device__ __forceinline__ void resample_tile(const RsGeom &g, long long k0, long long k1, float *win, Fetch fetch,
                                              float *out) {
    const long long lo = (k0 * g.M + g.half) / g.L - (g.J - 1);
    const long long hi = ((k1 - 1) * g.M + g.half) / g.L;
    long long cnt = hi - lo + 1;
    if (cnt > kRsWin) cnt = 0;  // (the host sizes tile_out so that this never happens; nothing is read out of bounds)
    for (int i = threadIdx.x; i < cnt; i += kRsThreads) win[i] = fetch(lo + i);
    __syncthreads();
    const double *tp[kOutPerLane];
    const float *xp[kOutPerLane];
    int J[kOutPerLane];
    double s[kOutPerLane];
    int jmax = 0;
#pragma unroll
    for (int o = 0; o < kOutPerLane; o++) {
        const long long k = k0 + threadIdx.x + (long long)o * kRsThreads;
        const long long c = k * g.M + g.half;
        const long long q = c / g.L;
        const int r = (int)(c - q * g.L);
        const int j = (2 * g.half - r) / g.L + 1;
        J[o] = (k < k1 && cnt > 0) ? j : 0;
        tp[o] = g.taps + (size_t)r * g.J;
        xp[o] = win + (J[o] ? (int)(q - j + 1 - lo) : 0);
        s[o] = 0.0;
        if (J[o] > jmax) jmax = J[o];
    }
    for (int i = 0; i < jmax; i++) {
#pragma unroll
        for (int o = 0; o < kOutPerLane; o++)
            if (i < J[o]) s[o] = s[o] + tp[o][i] * (double)xp[o][i];  // one multiply, one add: contraction is off (top of the file)
    }
#pragma unroll
    for (int o = 0; o < kOutPerLane; o++)
        if (J[o]) out[threadIdx.x + o * kRsThreads] = (float)s[o];
    __syncthreads();  // the window is restaged by the next tile
}

__device__ __forceinline__ float rs_sample(const void *src, int kind, long long i) {
    return kind == RTS_F32 ? reinterpret_cast<const float *>(src)[i]
                           : (float)reinterpret_cast<const int16_t *>(src)[i] * (1.0f / 32768.0f);  // exact
}

// One-shot, grid (tiles, B): tile x of stream y.  n_out = min(ceil(n_in L / M), n_out_max).
__global__ void __launch_bounds__(kRsThreads) resample_run_kernel(RsGeom g, const void *samples, int kind,
                                                                  long long sample_stride, const int32_t *n_in_dev,
                                                                  int n_out_max, float *out, int32_t *n_out_dev) {
    __shared__ float win[kRsWin];
    const int b = blockIdx.y;
    long long n_in = n_in_dev[b];
    if (n_in < 0) n_in = 0;
    long long n_out = (n_in * g.L + g.M - 1) / g.M;
    if (n_out > n_out_max) n_out = n_out_max;
    if (blockIdx.x == 0 && threadIdx.x == 0) n_out_dev[b] = (int32_t)n_out;
    const long long k0 = (long long)blockIdx.x * g.tile_out;
    if (k0 >= n_out) return;
    const long long k1 = k0 + g.tile_out < n_out ? k0 + g.tile_out : n_out;
    const size_t esz = kind == RTS_F32 ? sizeof(float) : sizeof(int16_t);
    const void *src = reinterpret_cast<const unsigned char *>(samples) + (size_t)b * (size_t)sample_stride * esz;
    resample_tile(g, k0, k1, win, [&](long long n) { return (n >= 0 && n < n_in) ? rs_sample(src, kind, n) : 0.0f; },
                  out + (size_t)b * n_out_max + k0);
}

// Live feed, grid (B, tiles): the stream's signal so far ends with tail[0 .. T) (samples in_total - T .. in_total - 1,
// zeros before the signal began) followed by the n staged samples of this feed.  Outputs out_total .. avail(in_total +
// n) - 1 go to the stream's region of the second staging buffer (offset b * cap, so that no prefix sum over streams is
// needed), tiles of kRsLiveTile outputs dealt round-robin to the stream's workgroups.  Tail and totals are kept twice:
// every workgroup reads this feed's copy, which nothing writes during the launch, and workgroup y = 0 of the stream
// writes the next feed's (the host alternates the two), so the workgroups of a stream need no ordering among them.
__global__ void __launch_bounds__(kRsThreads) resample_live_kernel(RsGeom g, int T, const unsigned char *stage,
                                                                   size_t samples_off, int kind, int B, int cap,
                                                                   unsigned char *out_stage, const float *tail_all,
                                                                   const long long *tot_all, float *tail_next,
                                                                   long long *tot_next) {
    __shared__ float win[kRsWin];
    const int b = blockIdx.x;
    const int32_t *counts = reinterpret_cast<const int32_t *>(stage);
    const int32_t *offs = counts + B;
    int32_t *out_counts = reinterpret_cast<int32_t *>(out_stage);
    int32_t *out_offs = out_counts + B;
    float *out = reinterpret_cast<float *>(out_stage + samples_off) + (size_t)b * cap;
    const float *tail = tail_all + (size_t)b * T;
    long long n = counts[b];
    if (n < 0) n = 0;
    const size_t esz = kind == RTS_F32 ? sizeof(float) : sizeof(int16_t);
    const void *src = stage + samples_off + (size_t)offs[b] * esz;
    const long long in_total = tot_all[2 * b], out_total = tot_all[2 * b + 1];
    const long long in_new = in_total + n;
    long long out_new = in_new * g.L - g.half;
    out_new = out_new > 0 ? (out_new + g.M - 1) / g.M : 0;
    if (out_new - out_total > cap) out_new = out_total + cap;  // (the host refuses such a feed before it gets here)
    const long long base = in_total - T;  // absolute index of tail[0]
    auto fetch = [&](long long a) {
        const long long w = a - base;
        if (w < 0 || w >= T + n) return 0.0f;
        return w < T ? tail[w] : rs_sample(src, kind, w - T);
    };
    const int tile = g.tile_out < kRsLiveTile ? g.tile_out : kRsLiveTile;
    for (long long k0 = out_total + (long long)blockIdx.y * tile; k0 < out_new; k0 += (long long)gridDim.y * tile)
        resample_tile(g, k0, k0 + tile < out_new ? k0 + tile : out_new, win, fetch, out + (k0 - out_total));
    if (blockIdx.y != 0) return;
    // the next feed's tail is the last T samples of (tail, feed)
    for (int i = threadIdx.x; i < T; i += kRsThreads) tail_next[(size_t)b * T + i] = fetch(in_new - T + i);
    if (threadIdx.x == 0) {
        out_counts[b] = (int32_t)(out_new - out_total);
        out_offs[b] = b * cap;
        tot_next[2 * b] = in_new;
        tot_next[2 * b + 1] = out_new;
    }
}

// rts_live_restart on a resampling handle: the selected streams' new run starts on silence.
// tail_all [2][B][T] and tot_all [2][B][2]: both copies.
__global__ void resample_live_restart_kernel(RestartSel sel, int T, int B, float *tail_all, long long *tot_all) {
    const int b = sel.idx[blockIdx.x];
    for (int w = 0; w < 2; w++) {
        for (int i = threadIdx.x; i < T; i += blockDim.x) tail_all[((size_t)w * B + b) * T + i] = 0.0f;
        if (threadIdx.x == 0) tot_all[2 * ((size_t)w * B + b)] = tot_all[2 * ((size_t)w * B + b) + 1] = 0;
    }
}

}  // namespace rts

struct rts_resample {
    rts::RsGeom g;
    int T;  // ceil(2 half / L): the input samples a live stream carries from feed to feed
    int device;
};

namespace rts {

static long long gcd_ll(long long a, long long b) {
    while (b) {
        const long long t = a % b;
        a = b;
        b = t;
    }
    return a;
}

int resample_info(const rts_resample *p, int *L, int *M, int *half, int *T, int *device) {
    if (!p) return set_error(RTS_ERR_INVALID, "resample_plan is NULL");
    if (L) *L = p->g.L;
    if (M) *M = p->g.M;
    if (half) *half = p->g.half;
    if (T) *T = p->T;
    if (device) *device = p->device;
    return RTS_OK;
}

int resample_live_enqueue(const rts_resample *p, const unsigned char *stage, size_t samples_off, int sample_kind, int B,
                          int cap, unsigned char *out_stage, const float *tail, const long long *tot, float *tail_next,
                          long long *tot_next, int n_out_max, hipStream_t s) {
    const int tile = p->g.tile_out < kRsLiveTile ? p->g.tile_out : kRsLiveTile;
    int tiles = (n_out_max + tile - 1) / tile;
    if (tiles < 1) tiles = 1;    // tail and totals move on in any case
    if (tiles > 64) tiles = 64;  // (the kernel deals the tiles round-robin)
    hipLaunchKernelGGL(resample_live_kernel, dim3(B, tiles), dim3(kRsThreads), 0, s, p->g, p->T, stage, samples_off,
                       sample_kind, B, cap, out_stage, tail, tot, tail_next, tot_next);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

int resample_live_restart_enqueue(const rts_resample *p, const RestartSel &sel, int B, float *tail, long long *tot,
                                  hipStream_t s) {
    hipLaunchKernelGGL(resample_live_restart_kernel, dim3(sel.n), dim3(64), 0, s, sel, p->T, B, tail, tot);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

}  // namespace rts

extern "C" {

long long rts_resample_out_len(long long n_in, int L, int M) {
    if (n_in <= 0 || L < 1 || M < 1) return 0;
    return (n_in * L + M - 1) / M;
}

long long rts_resample_avail(long long in_total, int L, int M, int half) { return rts::resample_avail(in_total, L, M, half); }

int rts_resample_destroy(rts_resample *p) {
    if (!p) return RTS_OK;
    if (p->g.taps) (void)hipFree(const_cast<double *>(p->g.taps));
    free(p);
    return RTS_OK;
}

int rts_resample_create(int L, int M, const double *taps_host, int half, rts_resample **out) {
    using namespace rts;
    if (!out) return set_error(RTS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (L < 1) return set_error(RTS_ERR_INVALID, "L must be >= 1 (got %d)", L);
    if (M < 1) return set_error(RTS_ERR_INVALID, "M must be >= 1 (got %d)", M);
    if (gcd_ll(L, M) != 1) return set_error(RTS_ERR_INVALID, "L / M = %d / %d is not reduced (divide both by %lld)", L, M, gcd_ll(L, M));
    if (half < 1) return set_error(RTS_ERR_INVALID, "half must be >= 1 (got %d)", half);
    if (!taps_host) return set_error(RTS_ERR_INVALID, "taps_host is NULL");
    if (2LL * half + 1 > kRsMaxTaps)
        return set_error(RTS_ERR_UNSUPPORTED, "a table of 2 * %d + 1 taps exceeds the supported %lld", half, kRsMaxTaps);
    const int J = (int)(2LL * half / L) + 1;
    const int T = (int)((2LL * half + L - 1) / L);
    if (T > kRsMaxSpan)
        return set_error(RTS_ERR_UNSUPPORTED, "ceil(2 half / L) = %d input samples under one output exceed the supported %d", T, kRsMaxSpan);
    // the most outputs whose window, ceil((n - 1) M / L) + J samples at the most, fits the LDS buffer
    long long tile_out = ((long long)(kRsWin - J) * L) / M;  // (n - 1) M <= (kRsWin - J) L - (L - 1) holds for n <= this
    if (tile_out > kRsTileOut) tile_out = kRsTileOut;
    if (tile_out < 64)
        return set_error(RTS_ERR_UNSUPPORTED, "M / L = %d / %d: one output per %.0f input samples leaves tiles of fewer than 64 "
                                              "outputs in %d samples of LDS", M, L, (double)M / L, kRsWin);
    rts_resample *p = (rts_resample *)calloc(1, sizeof(rts_resample));
    double *host = (double *)calloc((size_t)L * J, sizeof(double));
    if (!p || !host) {
        free(p);
        free(host);
        return set_error(RTS_ERR_INVALID, "out of host memory");
    }
    for (int r = 0; r < L; r++) {
        const int Jr = (int)((2LL * half - r) / L) + 1;
        for (int i = 0; i < Jr; i++) host[(size_t)r * J + i] = taps_host[r + (long long)(Jr - 1 - i) * L];
    }
    double *dev = nullptr;
    hipError_t e = hipGetDevice(&p->device);
    if (e == hipSuccess) e = hipMalloc((void **)&dev, sizeof(double) * (size_t)L * J);
    if (e == hipSuccess) e = hipMemcpy(dev, host, sizeof(double) * (size_t)L * J, hipMemcpyHostToDevice);
    free(host);
    p->g.taps = dev;
    if (e != hipSuccess) {
        rts_resample_destroy(p);
        return set_error(RTS_ERR_HIP, "rts_resample_create: %s", hipGetErrorString(e));
    }
    p->g.L = L;
    p->g.M = M;
    p->g.half = half;
    p->g.J = J;
    p->g.tile_out = (int)tile_out;
    p->T = T;
    *out = p;
    return RTS_OK;
}

int rts_resample_run(rts_resample *p, const void *samples_dev, int sample_dtype, long long sample_stride,
                     const int32_t *n_in_dev, int B, int n_out_max, float *out_dev, int32_t *n_out_dev, void *stream) {
    using namespace rts;
    if (!p) return set_error(RTS_ERR_INVALID, "plan is NULL");
    if (!samples_dev) return set_error(RTS_ERR_INVALID, "samples_dev is NULL");
    if (sample_dtype != RTS_F32 && sample_dtype != RTS_I16) return set_error(RTS_ERR_INVALID, "sample_dtype must be RTS_F32 or RTS_I16");
    if (sample_stride < 0) return set_error(RTS_ERR_INVALID, "sample_stride must be >= 0");
    if (!n_in_dev) return set_error(RTS_ERR_INVALID, "n_in_dev is NULL");
    if (B < 1 || B > 65535) return set_error(RTS_ERR_INVALID, "B must be in [1, 65535] (got %d)", B);
    if (n_out_max < 0) return set_error(RTS_ERR_INVALID, "n_out_max must be >= 0");
    if (!out_dev && n_out_max > 0) return set_error(RTS_ERR_INVALID, "out_dev is NULL");
    if (!n_out_dev) return set_error(RTS_ERR_INVALID, "n_out_dev is NULL");
    if (int rc = check_device(p->device, "plan"); rc != RTS_OK) return rc;
    int tiles = (n_out_max + p->g.tile_out - 1) / p->g.tile_out;
    if (tiles < 1) tiles = 1;  // n_out_dev is written in any case
    hipLaunchKernelGGL(resample_run_kernel, dim3(tiles, B), dim3(kRsThreads), 0, (hipStream_t)stream, p->g, samples_dev,
                       sample_dtype, sample_stride, n_in_dev, n_out_max, out_dev, n_out_dev);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

}  // extern "C"
