// The OTW tracker around its step kernel: the small service kernels (state reset and restart, dense-mirror fill, history
// append, recent frames, path cost), the handle with its kernel table, the launch and its argument builders, and the
// rts_otw_* ABI except rts_otw_backward (otw_backward.h) and the diagnostic entry points (otw_stamps.h).
#pragma once
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "otw_device.h"
#include "otw_fill.h"  // launch() enqueues otw_bandfill_kernel in front of the step kernel
#include "otw_plan.h"  // which instantiation a launch gets and whether the band fill runs: host-only, tested on the CPU
#include "snapshot.h"  // rts_otw_export / rts_otw_import: the record kernels both trackers share

namespace rts {

// What the kernel table takes from otw.hip, which defines them: the step kernel, the ring tags of its flavours and the
// dynamic LDS an instantiation needs.
struct LiveFromGlobal;
struct LiveFromGlobalLean;
template <int W, int DENSE, typename RT, bool SPEC, int NT>
__global__ void otw_advance_kernel(OtwArgs a);
template <int W, typename RT, bool SPEC>
constexpr size_t otw_lds_bytes();

// Fresh per-stream state (otw_eran.py:29-36 / livenote_v2.py:31-37).
__device__ __forceinline__ void otw_fresh_state(int32_t *st, int variant) {
    for (int i = 0; i < RTS_STATE_LEN; i++) st[i] = 0;
    st[RTS_ST_DIRECTION] = RTS_DIR_BOTH;
    st[RTS_ST_PREVIOUS] = RTS_DIR_NONE;
    st[RTS_ST_RUN_COUNT] = (variant == RTS_VARIANT_OTW) ? 1 : 0;
    st[RTS_ST_STATUS] = RTS_RUNNING;
    st[RTS_ST_FIRST_INSERT] = 1;
    st[14] = -2;
}

__global__ void otw_reset_kernel(int32_t *state, int B, int variant) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    otw_fresh_state(state + (size_t)b * RTS_STATE_LEN, variant);
}

// rts_otw_restart: the same for the selected streams only, one workgroup each, plus everything else a stream carries from
// one launch to the next: its history length, its persisted bands (NaN = never evaluated, as after create) and, when the
// stream moves to another piece, its row of the reference tables.  A stream whose state says first_insert takes
// nothing else from memory (otw_advance_kernel's prologue: bands are reloaded only when !first, the band minima and the
// pipelined kernel's shadow bands are rebuilt in every launch), so this is all "fresh" means.  Other streams' words are
// not written.
__global__ void __launch_bounds__(64) otw_restart_kernel(RestartSel sel, int32_t *state, int32_t *hist_len, double *bands,
                                                         int band_len, long long *ref_first, int32_t *ref_len, int variant) {
    if ((int)blockIdx.x >= sel.n) return;
    const int b = sel.idx[blockIdx.x];
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    for (int i = threadIdx.x; i < band_len; i += blockDim.x) bands[(size_t)b * band_len + i] = qnan;
    if (threadIdx.x == 0) {
        otw_fresh_state(state + (size_t)b * RTS_STATE_LEN, variant);
        hist_len[b] = 0;
        if (sel.set_ref) {
            ref_first[b] = sel.first[blockIdx.x];
            ref_len[b] = sel.len[blockIdx.x];
        }
    }
}

// Dense mirror: the [per_stream] slices of the selected streams back to `v`; grid (slices, sel.n).
__global__ void otw_fill_sel_kernel(RestartSel sel, double *p, long long per_stream, double v) {
    if ((int)blockIdx.y >= sel.n) return;
    double *q = p + (long long)sel.idx[blockIdx.y] * per_stream;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < per_stream; i += stride) q[i] = v;
}

__global__ void otw_fill_kernel(double *p, long long n, double v) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long q = i; q < n; q += stride) p[q] = v;
}

// Append one frame per (active) stream to the handle-owned history and bump its length.
__global__ void otw_append_kernel(double *hist, int32_t *hist_len, const void *frames, int frames_f64,
                                  const uint8_t *active, int B, int cap) {
    const int b = blockIdx.x;
    const int f = threadIdx.x;
    if (b >= B || f >= kF) return;
    if (active && !active[b]) return;
    const int n = hist_len[b];
    if (n < cap) {
        const double v = frames_f64 ? reinterpret_cast<const double *>(frames)[b * kF + f]
                                    : (double)reinterpret_cast<const float *>(frames)[b * kF + f];
        hist[((size_t)b * cap + n) * kF + f] = v;
    }
    __syncthreads();
    if (f == 0) hist_len[b] = n + 1;  // may exceed cap: the kernel reports LIVE_OVERFLOW at t >= 2N
}

// Append n_new[b] (or n_uniform) frames from frames [B][n_max][F] to the history of stream b.
__global__ void otw_append_many_kernel(double *hist, int32_t *hist_len, const void *frames, int frames_f64,
                                       const int32_t *n_new, int n_uniform, int n_max, int B, int cap) {
    const int b = blockIdx.x;
    if (b >= B) return;
    int nn = n_new ? n_new[b] : n_uniform;
    nn = nn < 0 ? 0 : (nn > n_max ? n_max : nn);  // never read a neighbouring stream's frames
    const int base = hist_len[b];
    __syncthreads();
    for (int idx = threadIdx.x; idx < nn * kF; idx += blockDim.x) {
        const int fr = base + idx / kF;
        if (fr < cap) {
            const size_t src = (size_t)b * n_max * kF + idx;
            hist[((size_t)b * cap + fr) * kF + idx % kF] =
                frames_f64 ? reinterpret_cast<const double *>(frames)[src]
                           : (double)reinterpret_cast<const float *>(frames)[src];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) hist_len[b] = base + (nn > 0 ? nn : 0);
}

// rts_otw_recent: the last min(M_max, n) frames of stream b's history into out[b], zeros behind them; one workgroup per
// stream.  n is what the stream has consumed, capped at its own capacity 2 N_b (hist_len runs past it on
// RTS_LIVE_OVERFLOW) and at the history stride.  `hist` is NULL until the first insert / push: every stream then reads
// as empty.  Nothing the tracker owns is written.
__global__ void __launch_bounds__(256) otw_recent_kernel(const double *hist, const int32_t *hist_len, int hist_stride, int N,
                                                         const int32_t *ref_len, int M_max, double *out, int32_t *len_out,
                                                         const uint8_t *mask) {
    const int b = blockIdx.x;
    const int cap = 2 * (ref_len ? ref_len[b] : N);
    int n = hist ? hist_len[b] : 0;
    n = n < 0 ? 0 : n;
    n = n > cap ? cap : n;
    n = n > hist_stride ? hist_stride : n;
    const int len = (mask && !mask[b]) ? 0 : (n < M_max ? n : M_max);
    const long long src0 = ((long long)b * hist_stride + (n - len)) * kF;
    double *dst = out + (size_t)b * M_max * kF;
    for (int idx = threadIdx.x; idx < M_max * kF; idx += blockDim.x) dst[idx] = idx < len * kF ? hist[src0 + idx] : 0.0;
    if (threadIdx.x == 0) len_out[b] = len;
}

// rts_otw_path_cost: the tracker's own cell cost at the last n = min(K, stored points) path points of every stream.
// One workgroup of 64 * ceil(K / 64) threads per stream; lane k owns point (stored - n + k): one int2 pair, the history
// frame t and the frame j of the stream's current reference range through the tracker's own loaders (otw_live_frame /
// otw_ref_frame: the reference widened as the tracker widens it), one cell_cost.  The mean is the sequential float64 sum,
// oldest point first, so thread 0 walks the LDS array in order behind one barrier -- a tree would round differently.
// A point whose indices lie outside the history or the range (never recorded by the tracker) costs NaN instead of being
// read.  Reads the handle's state only; the stores end with a system-scope fence because rts_live_watch points mean / n_out
// at host-mapped memory.
struct PathCostArgs {
    const int32_t *state, *path, *hist_len;
    const double *hist;
    const void *ref;
    const long long *ref_first;
    const int32_t *ref_len;
    int N, path_cap, hist_stride, ref_f64, euclid, K;
    double *mean, *costs;
    int32_t *n_out;
};
__global__ void __launch_bounds__(256) otw_path_cost_kernel(PathCostArgs a) {
    __shared__ double cost_s[256];
    const int b = blockIdx.x, k = threadIdx.x;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    const int Nb = a.ref_len ? a.ref_len[b] : a.N;
    int points = a.state[(size_t)b * RTS_STATE_LEN + RTS_ST_N_PATH];  // counts past path_cap once RTS_ST_PATH_TRUNCATED
    points = points > a.path_cap ? a.path_cap : (points < 0 ? 0 : points);
    if (!a.hist) points = 0;  // no frame has come through insert / push yet
    const int n = points < a.K ? points : a.K;
    int frames = a.hist ? a.hist_len[b] : 0;
    frames = frames > a.hist_stride ? a.hist_stride : frames;
    if (k < a.K) {
        double cost = qnan;
        if (k < n) {
            const int2 p = reinterpret_cast<const int2 *>(a.path)[(size_t)b * a.path_cap + (points - n + k)];
            if (p.x >= 0 && p.x < frames && p.y >= 0 && p.y < Nb) {
                OtwEnv e;
                e.live = a.hist;
                e.live_f64 = 1;
                e.live_base = (long long)b * a.hist_stride * kF;
                e.ref_f64 = a.ref_f64;
                e.ref = a.ref_first ? static_cast<const char *>(a.ref) + a.ref_first[b] * (long long)kF * (a.ref_f64 ? 8 : 4)
                                    : a.ref;
                double lf[kF], rf[kF];
                otw_live_frame(e, p.x, lf);
                otw_ref_frame(e, p.y, rf);
                cost = cell_cost(lf, rf, a.euclid);
            }
        }
        cost_s[k] = cost;
        if (a.costs) a.costs[(size_t)b * a.K + k] = cost;
    }
    __syncthreads();
    if (k == 0) {
        double sum = 0.0;
        for (int i = 0; i < n; i++) sum = sum + cost_s[i];
        a.mean[b] = n > 0 ? sum / (double)n : qnan;
        a.n_out[b] = n;
        __threadfence_system();
    }
}

// One otw_advance_kernel instantiation as the handle launches it: eight waves -- wave 0: control (+ chains of steps that
// are not hits), waves 1/2: chains, 3..7: cost strips, ring refill -- per stream; the wide forms (otw_plan::threads) have
// 12 or 16, all the further ones cost strips.  fn == NULL: the handle has no kernel for that kind of launch, which is
// refused.
struct OtwKernel {
    const void *fn;
    size_t smem;  // dynamic LDS
    int pipelined, ring, threads;  // what the instantiation is (set_kernel, from its template arguments): rts_otw_read_kernel
};

static_assert(otw_plan::kRingFloat == RTS_OTW_RING_FLOAT && otw_plan::kRingDouble == RTS_OTW_RING_DOUBLE &&
                  otw_plan::kRingNone == RTS_OTW_RING_NONE && otw_plan::kRingNoneLean == RTS_OTW_RING_NONE_LEAN,
              "otw_plan.h numbers the ring kinds as include/rtsync.h does");
template <typename RT>
constexpr int ring_kind() {
    if constexpr (std::is_same<RT, float>::value) return otw_plan::kRingFloat;
    else if constexpr (std::is_same<RT, double>::value) return otw_plan::kRingDouble;
    else if constexpr (std::is_same<RT, LiveFromGlobal>::value) return otw_plan::kRingNone;
    else return otw_plan::kRingNoneLean;
}

}  // namespace rts

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct rts_otw {
    const void *ref;
    int ref_dtype, F, N, B, c, max_run_count, variant, cost_kind;
    int W, path_cap;
    int hist_stride;    // frames per stream in `hist`: 2N (2 N_max with per-stream references)
    int32_t *state;     // [B][16]
    int32_t *path;      // [B][path_cap][2]
    double *bands;      // [B][2][c+1]
    double *hist;       // [B][hist_stride][F], allocated on first insert
    rts::RefTable refs;  // per-stream references (rts_otw_create_refs): lengths N_b in the pool `ref` points to
    int32_t *hist_len;  // [B]
    long long *debug;   // diagnostic builds only
    double *dense_acc, *dense_cost;  // caller-owned, optional
    int spec;           // 1: pipelined kernel (no dense mirror); 0: plain kernel
    int device;         // the HIP device the handle's buffers live on (one handle = one device)
    int cus;            // its compute units
    int tp_from;        // batches of at least tp_from streams per CU take the residency-oriented kernel flavour
    int waves;          // RTS_OTW_WAVES: 0 = auto, or 8 / 12 / 16 waves per stream where the kernel has that form (otw_plan::threads)
    int fill;           // RTS_OTW_FILL: 1 = a launch that can bring c frames to a fresh stream runs otw_bandfill_kernel first
    int fill_last;      // the handle's last launch enqueued it (host-side: which kernels ran is decided per call)
    int32_t *fill_took; // [B]: 1 where the stream's band was filled by that kernel (written by it, for every stream)
    // the handle's kernels (resolve_kernels, at create): the dense mirror's, and the others by [live input is float64]
    rts::OtwKernel k_dense, k_plain[2];
    rts::OtwKernel k_trace;  // the trace replay of rts_otw_backward: the plain kernel at every band width, whatever RTS_OTW_SPEC
    // what the handle has consumed since the last reset, for rts_otw_replay_dense
    int src_kind;       // 0 nothing, 1 the buffers of the last rts_otw_run, 2 the handle-owned history, 3 mixed
    int run_dtype, run_T, run_mode;  // of the last rts_otw_run (the buffers themselves are the caller's and not remembered)
    int32_t *rp_state, *rp_path;     // scratch state of rts_otw_replay_dense / rts_otw_backward, allocated on first use
    double *rp_bands;
    hipEvent_t bw_ev[3];             // rts_otw_backward: before the replay, between its two parts, behind the backtrace
};

namespace rts {

// Resolves one entry of the handle's kernel table.  The dynamic-LDS limit is a per-device function attribute: raised
// here, at create, on the handle's device (a handle lives on one device).
template <int W, int DENSE, typename RT, bool SPEC, int NT = 512>
static int set_kernel(OtwKernel *k) {
    k->fn = reinterpret_cast<const void *>(&otw_advance_kernel<W, DENSE, RT, SPEC, NT>);
    k->smem = otw_lds_bytes<W, RT, SPEC>();
    k->pipelined = SPEC;
    k->ring = ring_kind<RT>();
    k->threads = NT;
    RTS_HIP(hipFuncSetAttribute(k->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k->smem));
    return RTS_OK;
}

// The instantiation of a table entry without mirror (otw_plan::entry).  The wide windows have one, the pipelined kernel
// without ring; an else branch, so that none of the ring kernels is instantiated for them.
template <int W>
static int set_entry(const otw_plan::Entry &e, int threads, OtwKernel *k) {
    if constexpr (W == 512) {  // the wide forms (otw_plan::threads): the pipelined ring kernels of this window alone
        if (threads != 512) {
            const bool f = e.ring == otw_plan::kRingFloat;
            if (threads == 768) return f ? set_kernel<W, 0, float, true, 768>(k) : set_kernel<W, 0, double, true, 768>(k);
            return f ? set_kernel<W, 0, float, true, 1024>(k) : set_kernel<W, 0, double, true, 1024>(k);
        }
    }
    if constexpr (W >= otw_plan::kWideWindow) {
        return set_kernel<W, 0, LiveFromGlobal, true>(k);
    } else {
        if (!e.pipelined) return e.ring == otw_plan::kRingFloat ? set_kernel<W, 0, float, false>(k) : set_kernel<W, 0, double, false>(k);
        switch (e.ring) {
            case otw_plan::kRingNoneLean: return set_kernel<W, 0, LiveFromGlobalLean, true>(k);
            case otw_plan::kRingFloat: return set_kernel<W, 0, float, true>(k);
            case otw_plan::kRingDouble: return set_kernel<W, 0, double, true>(k);
            default: return set_kernel<W, 0, LiveFromGlobal, true>(k);
        }
    }
}

// The handle's kernels, chosen once at create: everything the choice depends on is fixed then, except whether a launch
// writes a dense mirror and whether its live input is float64 (rts_otw_run's dtype; the history is always float64).
// The dense mirror (otw_eran.py:23,27) is a separate instantiation so that the default kernel carries none of its code;
// it runs the plain role-specialised kernel (otw_plan::mirror_entry).
template <int W>
static int resolve_kernels(rts_otw *h) {
    using MirrorRT = std::conditional_t<otw_plan::mirror_entry(W).ring == otw_plan::kRingNone, LiveFromGlobal, double>;
    static_assert(!otw_plan::mirror_entry(W).pipelined, "the pipelined kernel writes no dense mirror");
    if (int rc = set_kernel<W, kMirrorDense, MirrorRT, false>(&h->k_dense); rc != RTS_OK) return rc;
    if (int rc = set_kernel<W, kMirrorTrace, MirrorRT, false>(&h->k_trace); rc != RTS_OK) return rc;
    for (int live_f64 = 0; live_f64 < 2; live_f64++) {
        const otw_plan::Entry e = otw_plan::entry(W, h->spec, h->tp_from, h->cus, h->B, h->ref_dtype == RTS_F64, live_f64 != 0);
        if (!e.ok) continue;  // RTS_OTW_SPEC=0 at a wide window: no plain entry, launch() refuses
        const int threads = otw_plan::threads(W, e, h->B, h->cus, h->waves);  // (h->waves was checked at create)
        if (int rc = set_entry<W>(e, threads, &h->k_plain[live_f64]); rc != RTS_OK) return rc;
    }
    return RTS_OK;
}

static int resolve_kernels(rts_otw *h) {
    switch (h->W) {
        case 64: return resolve_kernels<64>(h);
        case 128: return resolve_kernels<128>(h);
        case 256: return resolve_kernels<256>(h);
        case 512: return resolve_kernels<512>(h);
        case 1024: return resolve_kernels<1024>(h);  // c up to 1012: one workgroup per CU
        case 2048: return resolve_kernels<2048>(h);  // c up to 2036: 32 cells per lane in the chains
    }
    return set_error(RTS_ERR_UNSUPPORTED, "no kernel for window %d", h->W);
}

static int no_kernel(const rts_otw *h) {
    return set_error(RTS_ERR_UNSUPPORTED, "band widths above 500 (c=%d) run only on the pipelined 8-wave kernel", h->c);
}

// max_new: the largest number of new frames the call can bring to any stream (a host-side hint).  Only a launch that can
// bring a fresh stream its first c frames pays for the band-fill kernel; which streams it fills is decided on the device
// (otw_fill_eligible), every other stream is left to the step loop untouched.
static int launch(rts_otw *h, const OtwArgs &args, hipStream_t s, int max_new) {
    if ((uintptr_t)args.live & 15) return set_error(RTS_ERR_INVALID, "live features must be 16-byte aligned");
    const bool fill = otw_plan::fill_gate(h->fill, max_new, h->c, h->W, args.dense_acc || args.trace_cells);
    if (args.state == h->state) h->fill_last = fill;  // (the dense and trace replays run on scratch state and never fill)
    if (fill) {
        const dim3 block(otw_fill_threads(h->c));
        hipLaunchKernelGGL(otw_bandfill_kernel, dim3(h->B), block, 0, s, args, h->fill_took);
        RTS_HIP(hipGetLastError());
    }
    const OtwKernel &k = args.trace_cells ? h->k_trace : args.dense_acc ? h->k_dense : h->k_plain[args.live_f64 != 0];
    if (!k.fn) return no_kernel(h);
    void *params[] = {const_cast<OtwArgs *>(&args)};
    RTS_HIP(hipLaunchKernel(k.fn, dim3(h->B), dim3(k.threads), params, k.smem, s));
    return RTS_OK;
}

static OtwArgs base_args(const rts_otw *h) {
    OtwArgs a;
    memset(&a, 0, sizeof(a));
    a.ref = h->ref;
    a.state = h->state;
    a.path = h->path;
    a.bands = h->bands;
    a.N = h->N;
    a.c = h->c;
    a.max_run_count = h->max_run_count;
    a.variant = h->variant;
    a.cost_kind = h->cost_kind;
    a.path_cap = h->path_cap;
    a.live_cap = 2 * h->N;  // per-stream references: the kernel takes 2 N_b from ref_len instead
    a.ref_first = h->refs.first;
    a.ref_len = h->refs.len;
    a.ref_f64 = h->ref_dtype == RTS_F64;
    a.debug = h->debug;
    a.spec = h->spec;
    a.dense_acc = h->dense_acc;
    a.dense_cost = h->dense_cost;
    return a;
}

// The same with the handle-owned history as the live input (rts_otw_insert, rts_otw_push and their replay).
static OtwArgs hist_args(const rts_otw *h) {
    OtwArgs a = base_args(h);
    a.live = h->hist;
    a.live_len = h->hist_len;
    a.live_stride = h->hist_stride;
    a.live_f64 = 1;
    a.mode = RTS_MODE_INSERT_LOOP;
    return a;
}

// rts_otw_insert / rts_otw_push: the history is allocated with the first frame, and the handle has now consumed
// frames of its own (src_kind 2, or 3 "mixed" behind an rts_otw_run).
static int begin_append(rts_otw *h) {
    if (!h->hist) {
        RTS_HIP(hipMalloc((void **)&h->hist, sizeof(double) * kF * (size_t)h->hist_stride * h->B));
    }
    h->src_kind = (h->src_kind == 0 || h->src_kind == 2) ? 2 : 3;
    return RTS_OK;
}

// Scratch state of the replays (rts_otw_replay_dense, rts_otw_backward), so that the handle itself is not disturbed:
// allocated on the first replay, kept with the handle.
static int replay_scratch(rts_otw *h) {
    if (h->rp_state) return RTS_OK;
    hipError_t e;
    if ((e = hipMalloc((void **)&h->rp_state, sizeof(int32_t) * RTS_STATE_LEN * (size_t)h->B)) != hipSuccess ||
        (e = hipMalloc((void **)&h->rp_path, sizeof(int32_t) * 2 * (size_t)h->path_cap * h->B)) != hipSuccess ||
        (e = hipMalloc((void **)&h->rp_bands, sizeof(double) * 2 * (size_t)(h->c + 1) * h->B)) != hipSuccess) {
        if (h->rp_state) (void)hipFree(h->rp_state);
        if (h->rp_path) (void)hipFree(h->rp_path);
        if (h->rp_bands) (void)hipFree(h->rp_bands);
        h->rp_state = h->rp_path = nullptr;
        h->rp_bands = nullptr;
        return set_error(RTS_ERR_HIP, "hipMalloc failed: %s", hipGetErrorString(e));
    }
    return RTS_OK;
}

// The live arguments of a launch over the caller's rts_otw_run buffers: that call's own, and a replay of it.
static void run_source(OtwArgs *a, const void *live_dev, int live_dtype, int T_max, const int32_t *live_len_dev, int mode) {
    a->live = live_dev;
    a->live_len = live_len_dev;
    a->live_stride = T_max;
    a->live_f64 = live_dtype == RTS_F64;
    a->mode = mode;
    a->clamp_len = 1;
}

// What a replay (rts_otw_replay_dense, rts_otw_backward) runs on.  The frames of an rts_otw_run are the caller's: the
// library does not keep a pointer to memory it does not own, the caller hands the buffers in again.  Frames that came
// through rts_otw_insert / rts_otw_push are in the handle's history.  Every refusal comes before anything is enqueued;
// then the scratch state is reset on `s`, and *a is the launch over the frames the handle has consumed since its last
// reset (none on a fresh handle) on that scratch state, with no dense mirror and no trace: the caller sets its own.
static int replay_source(rts_otw *h, const void *live_dev, int live_dtype, int T_max, const int32_t *live_len_dev,
                         hipStream_t s, OtwArgs *a) {
    if (h->src_kind == 3)
        return set_error(RTS_ERR_UNSUPPORTED, "rts_otw_insert / rts_otw_push after rts_otw_run without a reset: nothing to replay from");
    if (h->src_kind == 1) {
        if (!live_dev || !live_len_dev)
            return set_error(RTS_ERR_INVALID, "the handle's frames came from rts_otw_run: pass that call's live_dev / live_len_dev again");
        if (!dtype_ok(live_dtype)) return set_error(RTS_ERR_INVALID, "bad live_dtype %d", live_dtype);
        if (live_dtype != h->run_dtype || T_max != h->run_T)
            return set_error(RTS_ERR_INVALID, "live_dtype / T_max differ from the rts_otw_run being replayed (%d / %d then)", h->run_dtype, h->run_T);
        if ((uintptr_t)live_dev & 15) return set_error(RTS_ERR_INVALID, "live_dev must be 16-byte aligned");
    } else if (live_dev) {
        return set_error(RTS_ERR_INVALID, "the handle's frames came through rts_otw_insert / rts_otw_push (or it is fresh): live_dev must be NULL");
    }
    if (int rc = replay_scratch(h); rc != RTS_OK) return rc;  // first replay only
    hipLaunchKernelGGL(otw_reset_kernel, dim3((h->B + 63) / 64), dim3(64), 0, s, h->rp_state, h->B, h->variant);
    RTS_HIP(hipGetLastError());
    *a = h->src_kind == 1 ? base_args(h) : hist_args(h);
    if (h->src_kind == 1) run_source(a, live_dev, live_dtype, T_max, live_len_dev, h->run_mode);
    a->state = h->rp_state;
    a->path = h->rp_path;
    a->bands = h->rp_bands;
    a->dense_acc = a->dense_cost = nullptr;
    return RTS_OK;
}

// The dense mirror's "never evaluated" values (otw_eran.py:23,27 / livenote_v2.py:21-23) into acc / cost [B][2N][N]:
// every stream, or the streams of `sel` only.  The caller checks hipGetLastError.
static void fill_dense(const rts_otw *h, double *acc, double *cost, const RestartSel *sel, hipStream_t s) {
    const long long per = (long long)2 * h->N * h->N;
    const double sentinel = (h->variant == RTS_VARIANT_OTW) ? 1e10 : (double)INFINITY;
    if (sel) {
        hipLaunchKernelGGL(otw_fill_sel_kernel, dim3(64, sel->n), dim3(256), 0, s, *sel, acc, per, sentinel);
        hipLaunchKernelGGL(otw_fill_sel_kernel, dim3(64, sel->n), dim3(256), 0, s, *sel, cost, per, -1.0);
    } else {
        hipLaunchKernelGGL(otw_fill_kernel, dim3(2048), dim3(256), 0, s, acc, h->B * per, sentinel);
        hipLaunchKernelGGL(otw_fill_kernel, dim3(2048), dim3(256), 0, s, cost, h->B * per, -1.0);
    }
}

// The pipelined kernel (58 KB of LDS at c = 500 with float32 features: two workgroups per CU, like the plain kernel) is
// the faster one at every batch size measured; RTS_OTW_SPEC=0 selects the plain kernel (A/B runs, tests).  Batches of at
// least RTS_OTW_TP_FROM streams per CU take the residency-oriented flavour (tests: 0 selects it at any batch size).
// Results are identical.
// RTS_OTW_FILL=0 leaves the band fill of fresh streams to the step loop (otw_bandfill_kernel is never enqueued).
// RTS_OTW_WAVES=8 / 12 / 16 fixes the waves per stream of the kernels that have a wide form (otw_plan::threads; A/B runs,
// tests); unset or empty: chosen from the batch size.  Anything else is refused by rts_otw_create.
struct OtwKnobs {
    int spec, tp_from, fill, waves;
};
static OtwKnobs otw_knobs() {
    const char *sp = getenv("RTS_OTW_SPEC"), *tp = getenv("RTS_OTW_TP_FROM"), *fl = getenv("RTS_OTW_FILL");
    const char *wv = getenv("RTS_OTW_WAVES");
    int waves = 0;
    if (wv && *wv) {
        waves = atoi(wv);
        if (waves == 0) waves = -1;  // "0", "auto", "x": not a wave count
    }
    return {sp ? (atoi(sp) != 0) : 1, tp ? atoi(tp) : 2, fl ? (atoi(fl) != 0) : 1, waves};
}

// The constructor behind rts_otw_create (first_host == NULL: one reference of N frames) and rts_otw_create_refs (N =
// N_max, per-stream tables of B entries, already checked).  Every argument is checked before the first HIP call.
static int otw_create(const void *ref_dev, int ref_dtype, int F, int N, int B, int c, int max_run_count, int variant,
                      int cost_kind, const long long *first_host, const int32_t *len_host, rts_otw **out) {
    if (F < 1) return set_error(RTS_ERR_INVALID, "F must be >= 1 (got %d)", F);
    if (F != kF) return set_error(RTS_ERR_UNSUPPORTED, "F must be 12 chroma bins (got %d)", F);
    if (N < 1 || B < 1) return set_error(RTS_ERR_INVALID, "N and B must be >= 1 (got N=%d B=%d)", N, B);
    if (!dtype_ok(ref_dtype)) return set_error(RTS_ERR_INVALID, "bad ref_dtype %d", ref_dtype);
    if (c < 1) return set_error(RTS_ERR_INVALID, "c must be >= 1 (got %d)", c);
    if (c > otw_plan::kMaxC)
        return set_error(RTS_ERR_UNSUPPORTED, "band width c=%d exceeds the 2036 cells the LDS-resident kernel holds", c);
    if (max_run_count < 1) return set_error(RTS_ERR_INVALID, "max_run_count must be >= 1");
    if (variant < RTS_VARIANT_OTW || variant > RTS_VARIANT_LIVENOTE_V2)
        return set_error(RTS_ERR_INVALID, "bad variant %d", variant);
    if (cost_kind != RTS_COST_DOT && cost_kind != RTS_COST_EUCLID)
        return set_error(RTS_ERR_INVALID, "bad cost_kind %d", cost_kind);
    if ((long long)N * 3 + 8 > 0x3fffffffLL) return set_error(RTS_ERR_INVALID, "N too large");

    const OtwKnobs knobs = otw_knobs();
    if (!otw_plan::waves_ok(knobs.waves))
        return set_error(RTS_ERR_INVALID, "RTS_OTW_WAVES must be 8, 12 or 16 (got \"%s\")", getenv("RTS_OTW_WAVES"));

    rts_otw *h = (rts_otw *)calloc(1, sizeof(rts_otw));
    if (!h) return set_error(RTS_ERR_INVALID, "out of host memory");
    h->ref = ref_dev;
    h->ref_dtype = ref_dtype;
    h->F = F;
    h->N = N;
    h->B = B;
    h->c = c;
    h->max_run_count = max_run_count;
    h->variant = variant;
    h->cost_kind = cost_kind;
    h->W = otw_plan::window(c);
    h->spec = knobs.spec;
    h->waves = knobs.waves;
    h->tp_from = knobs.tp_from;
    h->fill = knobs.fill;
    h->hist_stride = 2 * N;
    h->path_cap = 3 * N + 8;  // one point per decide(); decides <= row strips + column strips <= 2N + N
    hipError_t e;
    if ((e = hipGetDevice(&h->device)) != hipSuccess ||
        (e = hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, h->device)) != hipSuccess) {
        free(h);
        return set_error(RTS_ERR_HIP, "hipGetDevice failed: %s", hipGetErrorString(e));
    }
    if ((e = hipMalloc((void **)&h->state, sizeof(int32_t) * RTS_STATE_LEN * (size_t)B)) != hipSuccess ||
        (e = hipMalloc((void **)&h->path, sizeof(int32_t) * 2 * (size_t)h->path_cap * B)) != hipSuccess ||
        (e = hipMalloc((void **)&h->bands, sizeof(double) * 2 * (size_t)(c + 1) * B)) != hipSuccess ||
        (e = hipMalloc((void **)&h->hist_len, sizeof(int32_t) * (size_t)B)) != hipSuccess ||
        (e = hipMalloc((void **)&h->fill_took, sizeof(int32_t) * (size_t)B)) != hipSuccess ||
        (first_host && (e = ref_table_upload(&h->refs, first_host, len_host, B)) != hipSuccess)) {
        rts_otw_destroy(h);
        return set_error(RTS_ERR_HIP, "hipMalloc failed: %s", hipGetErrorString(e));
    }
    int rc = resolve_kernels(h);
    if (rc == RTS_OK) rc = rts_otw_reset(h, nullptr);
    if (rc != RTS_OK) {
        rts_otw_destroy(h);
        return rc;
    }
    // a stream that has not consumed a frame has no bands yet: they read NaN (rts_otw_restart puts a stream back there)
    hipLaunchKernelGGL(otw_fill_kernel, dim3(64), dim3(256), 0, nullptr, h->bands, (long long)2 * (c + 1) * B,
                       __builtin_nan(""));
    if ((e = hipGetLastError()) != hipSuccess) {
        rts_otw_destroy(h);
        return set_error(RTS_ERR_HIP, "launch of the band fill failed: %s", hipGetErrorString(e));
    }
    if ((e = hipStreamSynchronize(nullptr)) != hipSuccess) {
        rts_otw_destroy(h);
        return set_error(RTS_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
    }
    *out = h;
    return RTS_OK;
}

int otw_batch(const rts_otw *h) { return h->B; }
int otw_history(const rts_otw *h) { return h->hist_stride; }
int otw_tempo_view(const rts_otw *h, TempoTail *t) {
    t->state = h->state;
    t->state_len = RTS_STATE_LEN;
    t->st_n_path = RTS_ST_N_PATH;
    t->path = h->path;
    t->path_cap = h->path_cap;
    t->ref_len = h->refs.len;
    t->N = h->N;
    t->B = h->B;
    return h->N;
}

// ---- snapshots (include/rtsync.h; csrc/snapshot.h has the kernels) ----------------------------------------------------
// The handle as the record kernels see it: exactly what otw_restart_kernel resets.
static SnapView otw_snap_view(const rts_otw *h, const void *blob, long long rec_stride, int32_t *status) {
    SnapView v;
    memset(&v, 0, sizeof(v));
    v.kind = RTS_SNAPSHOT_OTW;
    v.state = h->state;
    v.state_words = RTS_STATE_LEN;
    v.st_n_path = RTS_ST_N_PATH;
    v.mid = reinterpret_cast<unsigned long long *>(h->bands);
    v.mid_stride = 2LL * (h->c + 1);
    v.param = h->c;
    v.mid_gate = -1;
    v.path = h->path;
    v.path_cap = h->path_cap;
    v.hist = h->hist;
    v.hist_stride = h->hist_stride;
    v.count = h->hist_len;
    v.ref_first = h->refs.first;
    v.ref_len = h->refs.len;
    v.len_default = h->N;
    v.blob = static_cast<unsigned char *>(const_cast<void *>(blob));
    v.rec_stride = rec_stride;
    v.status = status;
    return v;
}

static void otw_snap_desc(const rts_otw *h, int n, long long rec_stride, rts_snapshot_desc *d) {
    memset(d, 0, sizeof(*d));
    d->kind = RTS_SNAPSHOT_OTW;
    d->version = RTS_SNAPSHOT_VERSION;
    d->n = n;
    d->ref_dtype = h->ref_dtype;
    d->rec_stride = rec_stride;
    d->F = h->F;
    d->c = h->c;
    d->max_run_count = h->max_run_count;
    d->variant = h->variant;
    d->cost_kind = h->cost_kind;
}

int otw_import_records(rts_otw *h, const int32_t *slot_host, int n, const void *blob_dev, long long rec_stride,
                       const rts_snapshot_desc *desc, const long long *first_host, const int32_t *len_host,
                       int32_t *status_dev, void *stream, int dry) {
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!desc) return set_error(RTS_ERR_INVALID, "desc is NULL");
    if (!status_dev) return set_error(RTS_ERR_INVALID, "status_dev is NULL");
    if (int rc = snap_check_sel(h->B, slot_host, n, "slot_host", blob_dev, rec_stride); rc != RTS_OK) return rc;
    rts_snapshot_desc mine;
    otw_snap_desc(h, n, rec_stride, &mine);
    if (int rc = snap_check_import(*desc, mine, slot_host, first_host, len_host, h->refs, h->N, "N_max"); rc != RTS_OK) return rc;
    if (h->dense_acc) return set_error(RTS_ERR_UNSUPPORTED, "rts_otw_import: the dense mirror is attached, and a record does not carry it");
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    if (n == 0) return RTS_OK;
    if (!dry) {
        if (int rc = begin_append(h); rc != RTS_OK) return rc;  // the slots now hold frames of the handle's own history
    }
    SnapView v = otw_snap_view(h, blob_dev, rec_stride, status_dev);
    v.dry = dry;
    return snap_enqueue(true, v, slot_host, n, first_host, len_host, (hipStream_t)stream);
}

}  // namespace rts

extern "C" {

int rts_otw_create(const void *ref_dev, int ref_dtype, int F, int N, int B, int c, int max_run_count,
                   int variant, int cost_kind, rts_otw **out) {
    using namespace rts;
    if (!out) return set_error(RTS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!ref_dev) return set_error(RTS_ERR_INVALID, "ref_dev is NULL");
    return otw_create(ref_dev, ref_dtype, F, N, B, c, max_run_count, variant, cost_kind, nullptr, nullptr, out);
}

int rts_otw_create_refs(const void *refs_dev, int ref_dtype, int F, long long n_ref_frames,
                        const long long *first_host, const int32_t *len_host, int B, int c, int max_run_count,
                        int variant, int cost_kind, rts_otw **out) {
    using namespace rts;
    if (!out) return set_error(RTS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!refs_dev) return set_error(RTS_ERR_INVALID, "refs_dev is NULL");
    if (!first_host || !len_host) return set_error(RTS_ERR_INVALID, "first_host / len_host is NULL");
    if (B < 1) return set_error(RTS_ERR_INVALID, "B must be >= 1 (got %d)", B);
    const int n_max = ref_ranges_check(B, nullptr, first_host, len_host, n_ref_frames, 0, nullptr);
    if (n_max < 0) return n_max;
    const int rc = otw_create(refs_dev, ref_dtype, F, n_max, B, c, max_run_count, variant, cost_kind, first_host, len_host, out);
    if (rc == RTS_OK) (*out)->refs.n_frames = n_ref_frames;
    return rc;
}

int rts_otw_destroy(rts_otw *h) {
    if (!h) return RTS_OK;
    if (h->state) (void)hipFree(h->state);
    if (h->path) (void)hipFree(h->path);
    if (h->bands) (void)hipFree(h->bands);
    if (h->hist) (void)hipFree(h->hist);
    if (h->hist_len) (void)hipFree(h->hist_len);
    if (h->fill_took) (void)hipFree(h->fill_took);
    rts::ref_table_free(&h->refs);
    if (h->rp_state) (void)hipFree(h->rp_state);
    if (h->rp_path) (void)hipFree(h->rp_path);
    if (h->rp_bands) (void)hipFree(h->rp_bands);
    for (int i = 0; i < 3; i++)
        if (h->bw_ev[i]) (void)hipEventDestroy(h->bw_ev[i]);
    free(h);
    return RTS_OK;
}

int rts_otw_reset(rts_otw *h, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    h->src_kind = 0;
    hipLaunchKernelGGL(otw_reset_kernel, dim3((h->B + 63) / 64), dim3(64), 0, s, h->state, h->B, h->variant);
    RTS_HIP(hipGetLastError());
    RTS_HIP(hipMemsetAsync(h->hist_len, 0, sizeof(int32_t) * (size_t)h->B, s));
    if (h->dense_acc) {
        fill_dense(h, h->dense_acc, h->dense_cost, nullptr, s);
        RTS_HIP(hipGetLastError());
    }
    return RTS_OK;
}

int rts_otw_restart(rts_otw *h, const uint8_t *mask_host, const long long *first_host, const int32_t *len_host,
                    void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!mask_host) return set_error(RTS_ERR_INVALID, "mask_host is NULL");
    if (int rc = restart_check(h->B, mask_host, first_host, len_host, h->refs.first ? h->refs.n_frames : -1, h->N, "N_max");
        rc != RTS_OK)
        return rc;
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    // (src_kind stays: frames a restarted stream receives through insert / push after an rts_otw_run make the handle
    // "mixed" there, as for any stream)
    RestartSel sel;
    for (int pos = 0; restart_next_chunk(h->B, mask_host, first_host, len_host, &pos, &sel) > 0;) {
        hipLaunchKernelGGL(otw_restart_kernel, dim3(sel.n), dim3(64), 0, s, sel, h->state, h->hist_len, h->bands,
                           2 * (h->c + 1), h->refs.first, h->refs.len, h->variant);
        if (h->dense_acc) fill_dense(h, h->dense_acc, h->dense_cost, &sel, s);
        RTS_HIP(hipGetLastError());
    }
    return RTS_OK;
}

int rts_otw_set_dense(rts_otw *h, double *acc_dev, double *cost_dev, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (h->refs.first)
        return set_error(RTS_ERR_UNSUPPORTED, "the dense mirror is not available on a handle with per-stream references");
    if ((acc_dev == nullptr) != (cost_dev == nullptr))
        return set_error(RTS_ERR_INVALID, "acc_dev and cost_dev must both be given or both be NULL");
    h->dense_acc = acc_dev;
    h->dense_cost = cost_dev;
    return rts_otw_reset(h, stream);
}

int rts_otw_replay_dense(rts_otw *h, const void *live_dev, int live_dtype, int T_max, const int32_t *live_len_dev,
                         double *acc_dev, double *cost_dev, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (h->refs.first)
        return set_error(RTS_ERR_UNSUPPORTED, "the dense replay is not available on a handle with per-stream references");
    if (!acc_dev || !cost_dev) return set_error(RTS_ERR_INVALID, "acc_dev / cost_dev is NULL");
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    OtwArgs a;
    if (int rc = replay_source(h, live_dev, live_dtype, T_max, live_len_dev, s, &a); rc != RTS_OK) return rc;
    fill_dense(h, acc_dev, cost_dev, nullptr, s);
    RTS_HIP(hipGetLastError());
    if (h->src_kind == 0) return RTS_OK;  // freshly constructed: the matrices are all sentinel (otw_eran.py:23,27)
    a.dense_acc = acc_dev;
    a.dense_cost = cost_dev;
    int rc = launch(h, a, s, 0);  // the dense mirror: always the step loop
    if (rc != RTS_OK) return rc;
    RTS_HIP(hipStreamSynchronize(s));
    return RTS_OK;
}

int rts_otw_set_waves(rts_otw *h, int waves) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (waves == 1 || waves == 2 || waves == 4)
        return set_error(RTS_ERR_UNSUPPORTED, "wave counts below 8 were retired: every kernel runs 8 waves per stream (got %d)", waves);
    if (waves != 8) return set_error(RTS_ERR_INVALID, "waves must be 8 (got %d)", waves);
    return RTS_OK;
}

const char *rts_otw_kernel_name(const rts_otw *) { return "otw_advance_kernel"; }

int rts_otw_read_kernel(const rts_otw *h, int live_dtype, int32_t out[4]) {
    using namespace rts;
    if (!h || !out) return set_error(RTS_ERR_INVALID, "NULL argument");
    if (!dtype_ok(live_dtype)) return set_error(RTS_ERR_INVALID, "bad live_dtype %d", live_dtype);
    const OtwKernel &k = h->dense_acc ? h->k_dense : h->k_plain[live_dtype == RTS_F64];
    if (!k.fn) return no_kernel(h);
    out[0] = h->W;
    out[1] = k.ring;
    out[2] = k.pipelined;
    out[3] = otw_plan::fill_gate(h->fill, h->c, h->c, h->W, h->dense_acc != nullptr);
    return RTS_OK;
}

int rts_otw_read_kernel_waves(const rts_otw *h, int live_dtype, int32_t *waves) {
    using namespace rts;
    if (!h || !waves) return set_error(RTS_ERR_INVALID, "NULL argument");
    if (!dtype_ok(live_dtype)) return set_error(RTS_ERR_INVALID, "bad live_dtype %d", live_dtype);
    const OtwKernel &k = h->dense_acc ? h->k_dense : h->k_plain[live_dtype == RTS_F64];
    if (!k.fn) return no_kernel(h);
    *waves = k.threads / 64;
    return RTS_OK;
}

int rts_otw_run(rts_otw *h, const void *live_dev, int live_dtype, int T_max, const int32_t *live_len_dev,
                int mode, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!live_dev || !live_len_dev) return set_error(RTS_ERR_INVALID, "live_dev / live_len_dev is NULL");
    if (!dtype_ok(live_dtype)) return set_error(RTS_ERR_INVALID, "bad live_dtype %d", live_dtype);
    if (T_max < 0) return set_error(RTS_ERR_INVALID, "T_max < 0");
    if (mode != RTS_MODE_INSERT_LOOP && mode != RTS_MODE_SET_LIVE) return set_error(RTS_ERR_INVALID, "bad mode %d", mode);
    hipStream_t s = (hipStream_t)stream;
    int rc = rts_otw_reset(h, stream);
    if (rc != RTS_OK) return rc;
    OtwArgs a = base_args(h);
    run_source(&a, live_dev, live_dtype, T_max, live_len_dev, mode);
    h->src_kind = 1;
    h->run_dtype = live_dtype;
    h->run_T = T_max;
    h->run_mode = mode;
    return launch(h, a, s, T_max);
}

int rts_otw_insert(rts_otw *h, const void *frames_dev, int frames_dtype, const uint8_t *active_dev, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!frames_dev) return set_error(RTS_ERR_INVALID, "frames_dev is NULL");
    if (!dtype_ok(frames_dtype)) return set_error(RTS_ERR_INVALID, "bad frames_dtype %d", frames_dtype);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    if (int rc = begin_append(h); rc != RTS_OK) return rc;
    hipLaunchKernelGGL(otw_append_kernel, dim3(h->B), dim3(64), 0, s, h->hist, h->hist_len, frames_dev,
                       frames_dtype == RTS_F64, active_dev, h->B, h->hist_stride);
    RTS_HIP(hipGetLastError());
    return launch(h, hist_args(h), s, 1);
}

int rts_otw_push(rts_otw *h, const void *frames_dev, int frames_dtype, int n_max, const int32_t *n_new_dev,
                 void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (n_max < 0) return set_error(RTS_ERR_INVALID, "n_max < 0");
    if (n_max == 0) return RTS_OK;
    if (!frames_dev) return set_error(RTS_ERR_INVALID, "frames_dev is NULL");
    if (!dtype_ok(frames_dtype)) return set_error(RTS_ERR_INVALID, "bad frames_dtype %d", frames_dtype);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    if (int rc = begin_append(h); rc != RTS_OK) return rc;
    hipLaunchKernelGGL(otw_append_many_kernel, dim3(h->B), dim3(128), 0, s, h->hist, h->hist_len, frames_dev,
                       frames_dtype == RTS_F64, n_new_dev, n_max, n_max, h->B, h->hist_stride);
    RTS_HIP(hipGetLastError());
    // n_max: a restarted or late-joining stream may catch up from a long excerpt in one call
    return launch(h, hist_args(h), s, n_max);
}

// rts_otw_recent / rts_otw_path_cost read the handle-owned history: frames of an rts_otw_run are the caller's memory.
static int refuse_run_frames(const rts_otw *h, const char *what) {
    if (h->src_kind == 1 || h->src_kind == 3)
        return rts::set_error(RTS_ERR_UNSUPPORTED, "%s: the handle has consumed an rts_otw_run since its last reset, whose frames "
                                                   "are the caller's memory and not in the handle's history", what);
    return RTS_OK;
}

int rts_otw_recent(rts_otw *h, int M_max, double *out_dev, int32_t *len_dev, const uint8_t *mask_dev, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!out_dev) return set_error(RTS_ERR_INVALID, "out_dev is NULL");
    if (!len_dev) return set_error(RTS_ERR_INVALID, "len_dev is NULL");
    if (M_max < 1) return set_error(RTS_ERR_INVALID, "M_max must be >= 1 (got %d)", M_max);
    if (M_max > 256) return set_error(RTS_ERR_UNSUPPORTED, "M_max = %d exceeds the 256 frames rts_locate takes", M_max);
    if (int rc = refuse_run_frames(h, "rts_otw_recent"); rc != RTS_OK) return rc;
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    hipLaunchKernelGGL(otw_recent_kernel, dim3(h->B), dim3(256), 0, (hipStream_t)stream, h->hist, h->hist_len, h->hist_stride,
                       h->N, h->refs.len, M_max, out_dev, len_dev, mask_dev);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

int rts_otw_path_cost(rts_otw *h, int K, double *mean_dev, int32_t *n_dev, double *costs_dev, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!mean_dev) return set_error(RTS_ERR_INVALID, "mean_dev is NULL");
    if (!n_dev) return set_error(RTS_ERR_INVALID, "n_dev is NULL");
    if (K < 1 || K > 256) return set_error(RTS_ERR_INVALID, "K must be in [1, 256] (got %d)", K);
    if (int rc = refuse_run_frames(h, "rts_otw_path_cost"); rc != RTS_OK) return rc;
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    PathCostArgs a;
    a.state = h->state;
    a.path = h->path;
    a.hist_len = h->hist_len;
    a.hist = h->hist;
    a.ref = h->ref;
    a.ref_first = h->refs.first;
    a.ref_len = h->refs.len;
    a.N = h->N;
    a.path_cap = h->path_cap;
    a.hist_stride = h->hist_stride;
    a.ref_f64 = h->ref_dtype == RTS_F64;
    a.euclid = h->cost_kind == RTS_COST_EUCLID;
    a.K = K;
    a.mean = mean_dev;
    a.costs = costs_dev;
    a.n_out = n_dev;
    hipLaunchKernelGGL(otw_path_cost_kernel, dim3(h->B), dim3(64 * ((K + 63) / 64)), 0, (hipStream_t)stream, a);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

int rts_otw_tempo(rts_otw *h, int K, double ahead, double *slope_dev, double *pos_dev, int32_t *n_dev, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!slope_dev) return set_error(RTS_ERR_INVALID, "slope_dev is NULL");
    if (!n_dev) return set_error(RTS_ERR_INVALID, "n_dev is NULL");
    if (int rc = tempo_tail_check(K, ahead, h->N); rc != RTS_OK) return rc;
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    TempoTail t = {};
    otw_tempo_view(h, &t);
    t.K = K;
    t.ahead = ahead;
    t.slope = slope_dev;
    t.pos = pos_dev;
    t.n_out = n_dev;
    return tempo_tail_enqueue(t, nullptr, (hipStream_t)stream);
}

int rts_otw_snapshot_bytes(const rts_otw *h, size_t *bytes) {
    using namespace rts;
    if (!h || !bytes) return set_error(RTS_ERR_INVALID, "NULL argument");
    const long long need = snap::otw_rec_stride(h->N, h->c);
    if (int rc = snap_stride_check(need, -1, "N_max", h->N); rc != RTS_OK) return rc;
    *bytes = (size_t)need;
    return RTS_OK;
}

int rts_otw_export(rts_otw *h, const int32_t *idx_host, int n, void *blob_dev, long long rec_stride,
                   rts_snapshot_desc *desc_out, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!desc_out) return set_error(RTS_ERR_INVALID, "desc_out is NULL");
    if (int rc = snap_check_sel(h->B, idx_host, n, "idx_host", blob_dev, rec_stride); rc != RTS_OK) return rc;
    if (int rc = snap_stride_check(snap::otw_rec_stride(h->N, h->c), rec_stride, "N_max", h->N); rc != RTS_OK) return rc;
    if (int rc = refuse_run_frames(h, "rts_otw_export"); rc != RTS_OK) return rc;
    if (h->dense_acc) return set_error(RTS_ERR_UNSUPPORTED, "rts_otw_export: the dense mirror is attached, and a record does not carry it");
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    otw_snap_desc(h, n, rec_stride, desc_out);
    return snap_enqueue(false, otw_snap_view(h, blob_dev, rec_stride, nullptr), idx_host, n, nullptr, nullptr, (hipStream_t)stream);
}

int rts_otw_import(rts_otw *h, const int32_t *slot_host, int n, const void *blob_dev, long long rec_stride,
                   const rts_snapshot_desc *desc, const long long *first_host, const int32_t *len_host,
                   int32_t *status_dev, void *stream) {
    return rts::otw_import_records(h, slot_host, n, blob_dev, rec_stride, desc, first_host, len_host, status_dev, stream, 0);
}

int rts_otw_read_states(rts_otw *h, int32_t *states, void *stream) {
    using namespace rts;
    if (!h || !states) return set_error(RTS_ERR_INVALID, "NULL argument");
    hipStream_t s = (hipStream_t)stream;
    RTS_HIP(hipMemcpyAsync(states, h->state, sizeof(int32_t) * RTS_STATE_LEN * (size_t)h->B, hipMemcpyDeviceToHost, s));
    RTS_HIP(hipStreamSynchronize(s));
    for (int b = 0; b < h->B; b++) states[b * RTS_STATE_LEN + 14] = 0;  // slot 14 is kernel-private
    return RTS_OK;
}

int rts_otw_read_state(rts_otw *h, int b, int32_t *state, void *stream) {
    using namespace rts;
    if (!h || !state) return set_error(RTS_ERR_INVALID, "NULL argument");
    if (b < 0 || b >= h->B) return set_error(RTS_ERR_INVALID, "stream index %d out of range [0, %d)", b, h->B);
    hipStream_t s = (hipStream_t)stream;
    RTS_HIP(hipMemcpyAsync(state, h->state + (size_t)b * RTS_STATE_LEN, sizeof(int32_t) * RTS_STATE_LEN,
                           hipMemcpyDeviceToHost, s));
    RTS_HIP(hipStreamSynchronize(s));
    state[14] = 0;
    return RTS_OK;
}

int rts_otw_read_path(rts_otw *h, int b, int32_t *pairs, int cap_pairs, int *n, void *stream) {
    using namespace rts;
    if (!h || !n) return set_error(RTS_ERR_INVALID, "NULL argument");
    return read_path(h->state, RTS_STATE_LEN, RTS_ST_N_PATH, h->path, h->path_cap, b, h->B, pairs, cap_pairs, n,
                     (hipStream_t)stream);
}

int rts_otw_read_fill(rts_otw *h, int32_t *took, void *stream) {
    using namespace rts;
    if (!h || !took) return set_error(RTS_ERR_INVALID, "NULL argument");
    if (!h->fill_last) {  // the last launch ran the step loop alone
        memset(took, 0, sizeof(int32_t) * (size_t)h->B);
        return RTS_OK;
    }
    hipStream_t s = (hipStream_t)stream;
    RTS_HIP(hipMemcpyAsync(took, h->fill_took, sizeof(int32_t) * (size_t)h->B, hipMemcpyDeviceToHost, s));
    RTS_HIP(hipStreamSynchronize(s));
    return RTS_OK;
}

int rts_otw_read_bands(rts_otw *h, int b, double *row_band, double *col_band, void *stream) {
    using namespace rts;
    if (!h || !row_band || !col_band) return set_error(RTS_ERR_INVALID, "NULL argument");
    if (b < 0 || b >= h->B) return set_error(RTS_ERR_INVALID, "stream index %d out of range [0, %d)", b, h->B);
    hipStream_t s = (hipStream_t)stream;
    const double *bb = h->bands + (size_t)b * 2 * (h->c + 1);
    RTS_HIP(hipMemcpyAsync(row_band, bb, sizeof(double) * (h->c + 1), hipMemcpyDeviceToHost, s));
    RTS_HIP(hipMemcpyAsync(col_band, bb + (h->c + 1), sizeof(double) * (h->c + 1), hipMemcpyDeviceToHost, s));
    RTS_HIP(hipStreamSynchronize(s));
    return RTS_OK;
}

int rts_otw_device_views(rts_otw *h, int32_t **path_dev, int *path_cap, int32_t **state_dev) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (path_dev) *path_dev = h->path;
    if (path_cap) *path_cap = h->path_cap;
    if (state_dev) *state_dev = h->state;
    return RTS_OK;
}

}  // extern "C"
