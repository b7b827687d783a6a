// Host side of the renderer (csrc/warp.hip): the limits of a plan, block counts, the LDS a launch asks for, the grids, and
// the two pieces of integer arithmetic the kernel shares with the host -- the time map and the rule that keeps it inside
// 64 bits.  No HIP in it, so tests/sanitize/warp_plan_driver.cpp runs it stand-alone.
//
// A plan renders frames of N samples at a hop of H = N / 2 and looks for each frame within +-delta samples of where the
// map puts it (include/rtsync.h, rts_warp_run, has the definition).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RTS_WARP_HD __host__ __device__
#else
#define RTS_WARP_HD
#endif

namespace rts {

constexpr int kWarpMinN = 64;
constexpr int kWarpMaxN = 4096;
constexpr int kWarpMaxDelta = 1024;
constexpr long long kWarpSegLimit = 1LL << 31;  // a segment of the map is shorter than this on both axes
constexpr long long kWarpPosLimit = 1LL << 62;  // |every position| stays under this: p + N + delta cannot leave int64

inline bool warp_n_ok(int N) { return N >= kWarpMinN && N <= kWarpMaxN && N % 16 == 0; }
inline bool warp_delta_ok(int delta) { return delta >= 0 && delta <= kWarpMaxDelta; }

// Blocks of H = N / 2 samples that cover n_out output samples: ceil(n_out / H); 0 for n_out <= 0, -1 for an N no plan takes.
inline long long warp_blocks(long long n_out, int N) {
    if (!warp_n_ok(N)) return -1;
    if (n_out <= 0) return 0;
    const long long H = N / 2;
    return n_out / H + (n_out % H != 0);
}

// ---- launch geometry ------------------------------------------------------------------------------------------------
// Run kernel: one workgroup of kWarpThreads lanes per stream.  Its dynamic LDS holds the target frame (N floats) and
// behind it the candidate window (N + 2 delta floats): 40 KB at N = 4096, delta = 1024.  N % 16 == 0 keeps both 16-byte
// aligned for the broadcast reads of the target.
constexpr int kWarpThreads = 512;
constexpr int kWarpWaves = kWarpThreads / 64;
constexpr size_t kWarpLdsLimit = 64 * 1024;  // what a launch may ask for without raising the kernel's limit
constexpr size_t warp_lds_bytes(int N, int delta) { return sizeof(float) * ((size_t)N + (size_t)N + 2 * (size_t)delta); }
static_assert(warp_lds_bytes(kWarpMaxN, kWarpMaxDelta) == 40 * 1024, "the largest plan takes 40 KB");
static_assert(warp_lds_bytes(kWarpMaxN, kWarpMaxDelta) + 256 <= kWarpLdsLimit, "beside the kernel's static words");

// Anchors kernel: one workgroup per path, kWarpAnchorThreads points per turn.
constexpr int kWarpAnchorThreads = 256;
constexpr int kWarpAnchorWaves = kWarpAnchorThreads / 64;
constexpr int warp_anchor_turns(int len, int P_max) {
    return ((len > P_max ? P_max : (len < 0 ? 0 : len)) + kWarpAnchorThreads - 1) / kWarpAnchorThreads;
}
constexpr int kWarpMaxBatch = 65535;

// ---- the time map ---------------------------------------------------------------------------------------------------
// One segment (o0, i0) -> (o1, i1) is usable when it runs forward on the output axis, does not run backward on the input
// axis, is shorter than 2^31 on both and keeps every position under 2^62.  `reach` is the largest output position the
// segment is asked about plus one: o1 for an inner segment; for the last one max(o1, n_out), the map being continued
// along its last segment for blocks that begin behind the last anchor.  With that, (t - o0) (i1 - i0) < 2^62.
RTS_WARP_HD inline bool warp_segment_ok(long long o0, long long i0, long long o1, long long i1, long long reach) {
    if (o0 < 0 || o0 >= kWarpPosLimit || o1 >= kWarpPosLimit || reach >= kWarpPosLimit) return false;
    if (i0 <= -kWarpPosLimit || i0 >= kWarpPosLimit || i1 >= kWarpPosLimit) return false;
    if (o1 <= o0 || i1 < i0 || reach < o1) return false;
    if (o1 - o0 >= kWarpSegLimit || i1 - i0 >= kWarpSegLimit) return false;
    return reach - o0 <= kWarpSegLimit;  // t <= reach - 1
}

// in_pos at output position t >= o0 of a segment that passed warp_segment_ok: exact, floor = truncation (no negative term).
RTS_WARP_HD inline long long warp_map_pos(long long t, long long o0, long long i0, long long o1, long long i1) {
    return i0 + ((t - o0) * (i1 - i0)) / (o1 - o0);
}

}  // namespace rts
