// The regression window's device pieces, shared by the tempo kernels (csrc/tempo.hip) and the steering kernel of the live
// accompaniment (csrc/accomp.hip): the wrapping integer sums of a window, their shuffles, and tempo_fit, the float64 part
// of include/rtsync.h's definition (rts_path_tempo), one rounding per operation -- every file that includes this is
// compiled without contraction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "annot_device.h"

namespace rts {

struct TempoSums {
    uint64_t x, y, xx, xy;
    uint32_t bad;
};

__device__ __forceinline__ TempoSums tempo_point(int32_t x, int32_t y, long long x_limit, long long y_limit) {
    const uint64_t ux = (uint64_t)(int64_t)x, uy = (uint64_t)(int64_t)y;
    TempoSums s;
    s.x = ux;
    s.y = uy;
    s.xx = ux * ux;
    s.xy = ux * uy;
    s.bad = (x < 0 || x >= x_limit || y < 0 || y >= y_limit) ? 1u : 0u;
    return s;
}

__device__ __forceinline__ void tempo_add(TempoSums &a, const TempoSums &b) {
    a.x += b.x;
    a.y += b.y;
    a.xx += b.xx;
    a.xy += b.xy;
    a.bad += b.bad;
}

__device__ __forceinline__ void tempo_sub(TempoSums &a, const TempoSums &b) {
    a.x -= b.x;
    a.y -= b.y;
    a.xx -= b.xx;
    a.xy -= b.xy;
    a.bad -= b.bad;
}

__device__ __forceinline__ TempoSums tempo_shfl_up(const TempoSums &v, int d) {
    TempoSums r;
    r.x = __shfl_up((unsigned long long)v.x, d, 64);
    r.y = __shfl_up((unsigned long long)v.y, d, 64);
    r.xx = __shfl_up((unsigned long long)v.xx, d, 64);
    r.xy = __shfl_up((unsigned long long)v.xy, d, 64);
    r.bad = __shfl_up(v.bad, d, 64);
    return r;
}

__device__ __forceinline__ TempoSums tempo_shfl_xor(const TempoSums &v, int m) {
    TempoSums r;
    r.x = __shfl_xor((unsigned long long)v.x, m, 64);
    r.y = __shfl_xor((unsigned long long)v.y, m, 64);
    r.xx = __shfl_xor((unsigned long long)v.xx, m, 64);
    r.xy = __shfl_xor((unsigned long long)v.xy, m, 64);
    r.bad = __shfl_xor(v.bad, m, 64);
    return r;
}

// Slope and position of a window of n points with sums s, its newest point (xi, yi): include/rtsync.h, operation by operation.
__device__ __forceinline__ void tempo_fit(int n, const TempoSums &s, int32_t xi, int32_t yi, double ahead, double *slope,
                                          double *pos) {
    const double qnan = annot_nan();
    *slope = qnan;
    *pos = qnan;
    if (s.bad != 0 || n < 1) return;
    const uint64_t un = (uint64_t)n;
    const int64_t den = (int64_t)(un * s.xx - s.x * s.x);
    const int64_t num = (int64_t)(un * s.xy - s.x * s.y);
    if (!(den > 0)) return;
    const double sl = (double)num / (double)den;
    const int64_t sxr = (int64_t)(s.x - un * (uint64_t)(int64_t)xi);  // relative to the newest point
    const int64_t syr = (int64_t)(s.y - un * (uint64_t)(int64_t)yi);
    const double at = (double)yi + ((double)syr - sl * (double)sxr) / (double)n;
    const double p = at + sl * ahead;
    *slope = sl;
    *pos = p == p ? p : qnan;
}

}  // namespace rts
