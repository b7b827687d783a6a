// The time map of a path as the kernels of csrc/pathmap.hip see it (include/rtsync.h, rts_path_map, has the definition):
// one pair's path with its side and offsets, the workgroup's verdict on it, and the image of one position.  Device code
// only; the map kernel and the table transfer share it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rtsync.h"
#include "pathmap_plan.h"

// y = m_i + ((x - k_i) * (m_{i+1} - m_i)) / dk rounds the product, the quotient and the sum each on its own; contraction
// is off for everything below under the build's -ffp-contract=off and under hipcc's own default alike (csrc/resample.hip
// has the long form).
#pragma clang fp contract(off)

namespace rts {

struct PathSide {
    const int32_t *pts;    // the pair's points, [P][2]
    int P;                 // clamped to [0, P_max]
    int from;              // u's column
    long long off_u, off_v;
};

__device__ __forceinline__ long long pathmap_u(const PathSide &s, int t) { return (long long)s.pts[2 * (size_t)t + s.from] + s.off_u; }
__device__ __forceinline__ long long pathmap_v(const PathSide &s, int t) { return (long long)s.pts[2 * (size_t)t + (1 - s.from)] + s.off_v; }

__device__ __forceinline__ PathSide pathmap_side(const int32_t *path, int P_max, const int32_t *len, const int32_t *off, int from,
                                                 int b) {
    PathSide s;
    s.pts = path + pathmap_path_offset(b, P_max);
    s.P = pathmap_points(len[b], P_max);
    s.from = from;
    s.off_u = off ? off[2 * (size_t)b + from] : 0;
    s.off_v = off ? off[2 * (size_t)b + (1 - from)] : 0;
    return s;
}

__device__ __forceinline__ double pathmap_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// The status word of the pair, known to every lane of the workgroup on return: each lane looks at points tid, tid + 256,
// .. and their predecessors, the lanes' words meet by a butterfly inside each wave and the waves' through `red`
// (kPathmapWaves words of LDS).  Called by all kPathmapThreads lanes.
__device__ __forceinline__ int pathmap_status(const PathSide &s, int32_t *red) {
    const int tid = threadIdx.x;
    int st = s.P < 1 ? RTS_PATHMAP_EMPTY : RTS_PATHMAP_OK;
    for (int t = tid; t < s.P; t += kPathmapThreads) {
        const long long u = pathmap_u(s, t), v = pathmap_v(s, t);
        if (u < 0 || v < 0) st |= RTS_PATHMAP_NEGATIVE;
        if (t > 0 && (u < pathmap_u(s, t - 1) || v < pathmap_v(s, t - 1))) st |= RTS_PATHMAP_BACKWARD;
    }
    for (int d = 32; d >= 1; d >>= 1) st |= __shfl_xor(st, d, 64);
    if ((tid & 63) == 0) red[tid >> 6] = st;
    __syncthreads();
    st = 0;
    for (int w = 0; w < kPathmapWaves; w++) st |= red[w];
    return st;
}

// The image of x on a usable path (status 0): at most three bisections of u, log2 P dependent loads each.
__device__ __forceinline__ double pathmap_at(const PathSide &s, double x) {
    const int last = s.P - 1;
    if (!(x >= (double)pathmap_u(s, 0) && x <= (double)pathmap_u(s, last))) return pathmap_nan();  // NaN, or outside the knots
    int lo = 0, hi = last;  // e: the last point with u <= x; u[0] <= x holds
    while (lo < hi) {
        const int mid = lo + ((hi - lo + 1) >> 1);
        if ((double)pathmap_u(s, mid) <= x) lo = mid;
        else hi = mid - 1;
    }
    const int e = lo;
    const long long k = pathmap_u(s, e);
    lo = 0, hi = e;  // the first point with u == k
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (pathmap_u(s, mid) >= k) hi = mid;
        else lo = mid + 1;
    }
    const double m = (double)(pathmap_v(s, lo) + pathmap_v(s, e)) * 0.5;
    if (x == (double)k) return m;
    // x < u[last], so the next knot exists: its run begins at e + 1
    const long long k1 = pathmap_u(s, e + 1);
    lo = e + 1, hi = last;  // the last point with u == k1
    while (lo < hi) {
        const int mid = lo + ((hi - lo + 1) >> 1);
        if (pathmap_u(s, mid) <= k1) lo = mid;
        else hi = mid - 1;
    }
    const double m1 = (double)(pathmap_v(s, e + 1) + pathmap_v(s, lo)) * 0.5;
    return m + ((x - (double)k) * (m1 - m)) / (double)(k1 - k);
}

}  // namespace rts
