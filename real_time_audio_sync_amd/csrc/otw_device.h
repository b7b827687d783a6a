// What the OTW kernels share: the kernel arguments, the cell cost and the wave primitives of the chains, and the frame
// loaders.  One copy for the step kernel (otw.hip), the band fill (otw_fill.h), the service kernels (otw_host.h) and the
// backtrace (otw_backward.h), so the bit patterns cannot drift between them.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "common.h"
#include "cost.h"

namespace rts {

constexpr int kF = 12;
constexpr int kFetch = 8;  // frames fetched per ring refill

struct OtwArgs {
    const void *ref;          // [N][F]; with per-stream references [n_ref_frames][F], stream b at ref_first[b]
    const void *live;         // [B][live_stride][F]
    const int32_t *live_len;  // [B]
    int32_t *state;           // [B][RTS_STATE_LEN]
    int32_t *path;            // [B][path_cap][2]
    double *bands;            // [B][2][c+1]
    long long live_stride;    // frames between consecutive streams in `live`
    int N, c, max_run_count, variant, cost_kind, mode;
    int path_cap, live_cap;   // live_cap = 2N (otw_eran.py:14); the history stride is live_stride
    int ref_f64, live_f64;
    int clamp_len;            // run mode: never read past live_stride frames
    long long *debug;         // diagnostic builds only (-DRTS_OTW_STAMPS): [B][16] cycle sums (level 2: [B][128])
    int spec;                 // 1: the pipelined kernel was selected (host-side choice; the kernel does not read it)
    double *dense_acc;        // optional [B][2N][N]: the reference's dense acc_cost (otw_eran.py:27), NULL = off
    double *dense_cost;       // optional [B][2N][N]: the reference's dense cost (otw_eran.py:23)
    // per-stream references (rts_otw_create_refs), NULL for a single-reference handle: stream b follows frames
    // [ref_first[b], ref_first[b] + ref_len[b]) of `ref`, and its N is ref_len[b].  The kernel reads every reference
    // quantity from OtwEnv (e.ref, e.N, e.live_cap), which the prologue fills from these or from ref / N / live_cap.
    const long long *ref_first;
    const int32_t *ref_len;
    // trace replay (rts_otw_backward, otw_backward.h): the compact per-strip log of accumulated costs, NULL = off.
    // Stream b owns slots [b * 3 N_max, (b + 1) * 3 N_max): row strip x in slot x, column strip y in slot trace_rows + y.
    int2 *trace_hdr;      // per slot: (first index, cells) -- first column of a row strip, first row of a column strip
    double *trace_cells;  // per slot: c + 1 doubles
    int trace_rows;       // 2 N_max
};

// What a kernel instantiation mirrors of the cells it evaluates (the DENSE template argument): nothing, the reference's
// dense matrices (rts_otw_set_dense / rts_otw_replay_dense), or the per-strip log of rts_otw_backward.
constexpr int kMirrorDense = 1, kMirrorTrace = 2;

// Trace replay: where the cells of stream b's slot go, and its header (one lane calls otw_trace_open).
__device__ __forceinline__ double *otw_trace_slot(const OtwArgs &a, int b, int slot) {
    return a.trace_cells + ((size_t)b * 3 * (a.trace_rows / 2) + slot) * (size_t)(a.c + 1);
}
__device__ __forceinline__ void otw_trace_open(const OtwArgs &a, int b, int slot, int first, int n) {
    a.trace_hdr[(size_t)b * 3 * (a.trace_rows / 2) + slot] = make_int2(first, n);
}

__device__ __forceinline__ double dmin(double a, double b) { return (b < a) ? b : a; }

// np.dot on two strided column views == OpenBLAS ddot with inc != 1 (oracle: orc_dot_strided).
__device__ __forceinline__ double dot_strided12(const double (&x)[kF], const double (&y)[kF]) {
    double t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int i = 0; i < kF; i += 4) {
        const double m3 = y[i + 2] * x[i + 2];
        const double m4 = y[i + 3] * x[i + 3];
        const double a = fma(y[i], x[i], m3);
        const double b = fma(y[i + 1], x[i + 1], m4);
        t1 = t1 + a;
        t2 = t2 + b;
    }
    return t1 + t2;
}

__device__ __forceinline__ double cell_cost(const double (&lf)[kF], const double (&rf)[kF], int euclid) {
    return euclid ? euclid12(lf, rf) : (1.0 - dot_strided12(lf, rf));
}

// v_min_f64 without the canonicalising v_max pair hipcc adds around fmin().  Operands are never NaN
// on this path (costs of finite chroma; the +inf sentinel is handled exactly by the instruction).
__device__ __forceinline__ double vmin(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// lane i receives lane i-1's value; lane 0 receives `lane0` (DPP wave_shr:1; lanes without a source keep `old`).
__device__ __forceinline__ double wave_shift_up(double v, double lane0) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(lane0), __double2loint(v), 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(lane0), __double2hiint(v), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double wave_bcast(double v, int src_lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
    return __hiloint2double(hi, lo);
}

// A value every lane holds identically (an LDS broadcast read) -> SGPRs, so the control logic that
// consumes it runs on the scalar unit.
__device__ __forceinline__ double rfl(double v) {
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
    const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

// Minimum over the 64 lanes, returned in every lane.  Six DPP steps (row_shr 1/2/4/8, then
// row_bcast 15 and 31) leave the total in lane 63; lanes without a DPP source keep their own value.
#define RTS_DPP_MIN_STEP(CTRL, ROWMASK)                                                                       \
    do {                                                                                                      \
        const int tlo = __builtin_amdgcn_update_dpp(__double2loint(x), __double2loint(x), CTRL, ROWMASK, 0xf, false); \
        const int thi = __builtin_amdgcn_update_dpp(__double2hiint(x), __double2hiint(x), CTRL, ROWMASK, 0xf, false); \
        x = vmin(x, __hiloint2double(thi, tlo));                                                              \
    } while (0)

__device__ __forceinline__ double wave_min(double x) {
    RTS_DPP_MIN_STEP(0x111, 0xf);  // row_shr:1
    RTS_DPP_MIN_STEP(0x112, 0xf);  // row_shr:2
    RTS_DPP_MIN_STEP(0x114, 0xf);  // row_shr:4
    RTS_DPP_MIN_STEP(0x118, 0xf);  // row_shr:8
    RTS_DPP_MIN_STEP(0x142, 0xa);  // row_bcast:15
    RTS_DPP_MIN_STEP(0x143, 0xc);  // row_bcast:31
    return wave_bcast(x, 63);
}

// Two such minima at once, their DPP steps interleaved: a wave issues a dependent VALU instruction every 8.25 cycles, the
// instructions of two independent chains every 6.2 (profiles/experiments/r03_chain_latency.jsonl).
__device__ __forceinline__ void wave_min2(double &x0, double &x1) {
#define RTS_DPP_MIN_STEP2(CTRL, ROWMASK) \
    do {                                 \
        {                                \
            double &x = x0;              \
            RTS_DPP_MIN_STEP(CTRL, ROWMASK); \
        }                                \
        {                                \
            double &x = x1;              \
            RTS_DPP_MIN_STEP(CTRL, ROWMASK); \
        }                                \
    } while (0)
    RTS_DPP_MIN_STEP2(0x111, 0xf);  // row_shr:1
    RTS_DPP_MIN_STEP2(0x112, 0xf);  // row_shr:2
    RTS_DPP_MIN_STEP2(0x114, 0xf);  // row_shr:4
    RTS_DPP_MIN_STEP2(0x118, 0xf);  // row_shr:8
    RTS_DPP_MIN_STEP2(0x142, 0xa);  // row_bcast:15
    RTS_DPP_MIN_STEP2(0x143, 0xc);  // row_bcast:31
#undef RTS_DPP_MIN_STEP2
    x0 = wave_bcast(x0, 63);
    x1 = wave_bcast(x1, 63);
}

struct OtwEnv {  // launch-invariant values every helper needs
    int b, lane, c, N, live_len, live_cap, euclid, variant, mode, max_run_count, path_cap, live_f64, ref_f64;
    long long live_base;
    const void *live, *ref;
    int32_t *path;
    bool deferred_update;
};

__device__ __forceinline__ double otw_load_feat(const void *base, int is_f64, long long idx) {
    return is_f64 ? reinterpret_cast<const double *>(base)[idx] : (double)reinterpret_cast<const float *>(base)[idx];
}

// The 12 features of reference frame q, from global memory (frame-major [N][12]: 48 or 96 contiguous bytes).
__device__ __forceinline__ void otw_ref_frame(const OtwEnv &e, int q, double (&rf)[kF]) {
    if (e.ref_f64) {
        const double2 *p = reinterpret_cast<const double2 *>(reinterpret_cast<const double *>(e.ref) + (size_t)q * kF);
#pragma unroll
        for (int i = 0; i < kF / 2; i++) {
            const double2 v = p[i];
            rf[2 * i] = v.x;
            rf[2 * i + 1] = v.y;
        }
    } else {
        const float4 *p = reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(e.ref) + (size_t)q * kF);
#pragma unroll
        for (int i = 0; i < kF / 4; i++) {
            const float4 v = p[i];
            rf[4 * i] = (double)v.x;
            rf[4 * i + 1] = (double)v.y;
            rf[4 * i + 2] = (double)v.z;
            rf[4 * i + 3] = (double)v.w;
        }
    }
}

// The 12 features of this stream's live frame r, from global memory (windows without a live ring).
__device__ __forceinline__ void otw_live_frame(const OtwEnv &e, int r, double (&lf)[kF]) {
    if (e.live_f64) {
        const double2 *p = reinterpret_cast<const double2 *>(reinterpret_cast<const double *>(e.live) + e.live_base +
                                                             (long long)r * kF);
#pragma unroll
        for (int i = 0; i < kF / 2; i++) {
            const double2 v = p[i];
            lf[2 * i] = v.x;
            lf[2 * i + 1] = v.y;
        }
    } else {
        const float4 *p = reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(e.live) + e.live_base +
                                                           (long long)r * kF);
#pragma unroll
        for (int i = 0; i < kF / 4; i++) {
            const float4 v = p[i];
            lf[4 * i] = (double)v.x;
            lf[4 * i + 1] = (double)v.y;
            lf[4 * i + 2] = (double)v.z;
            lf[4 * i + 3] = (double)v.w;
        }
    }
}

}  // namespace rts
