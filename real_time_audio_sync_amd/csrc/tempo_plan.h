// Host side of the tempo kernels (csrc/tempo.hip): the limits of the regression window, the check that keeps its integer
// sums exact, and the launch geometry of the curve and tail kernels.  No HIP in it, so tests/sanitize/tempo_plan_driver.cpp
// runs it stand-alone.
//
// The window at path point i is the K points that end there (fewer at the start of a path).  Slope and position come from
// two integers, den = n Sxx - Sx^2 and num = n Sxy - Sx Sy (include/rtsync.h, rts_path_tempo); the kernels form them in
// wrapping unsigned 64-bit arithmetic, which gives the true integers whenever those fit in int64.  With every coordinate
// inside [0, x_limit) x [0, y_limit): |num| = n^2 |cov(x, y)| <= K^2 x_limit y_limit / 4 and den = n^2 var(x) <= K^2
// x_limit^2 / 4, so the one product K^2 x_limit y_limit < 2^63 bounds num, and den as well while x_limit <= 4 y_limit (the
// trackers' own limits are x_limit = 2 y_limit).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace rts {

constexpr int kTempoMinK = 2;     // one point has no slope
constexpr int kTempoMaxK = 1024;  // sizes the curve kernel's LDS and the tail kernel's points per lane

inline bool tempo_k_ok(int K) { return K >= kTempoMinK && K <= kTempoMaxK; }

// K^2 * x_limit * y_limit >= 2^63: the integer sums of a window may leave int64 (RTS_ERR_UNSUPPORTED).  Limits >= 1 and a K
// that passed tempo_k_ok; the product is formed in 128 bits.
inline bool tempo_overflows(int K, long long x_limit, long long y_limit) {
    const unsigned __int128 top = (unsigned __int128)1 << 63;
    const unsigned __int128 p = (unsigned __int128)((unsigned long long)K * (unsigned long long)K) * (unsigned long long)x_limit;
    if (p >= top) return true;  // y_limit >= 1; and below, p < 2^63 keeps p * y_limit under 2^126
    return p * (unsigned long long)y_limit >= top;
}

// ---- launch geometry ------------------------------------------------------------------------------------------------
// Curve kernel: one workgroup of kTempoThreads lanes per path, kTempoChunk = kTempoThreads points per turn (one per lane).
// Its LDS is a ring of the running sums of the last kTempoChunk + K points: four 64-bit words (x, y, x^2, xy) and a
// 32-bit count of bad points each, plus one row of wave totals per scan.  46.2 KB at K = 1024.
constexpr int kTempoThreads = 256;
constexpr int kTempoChunk = kTempoThreads;
constexpr int kTempoWaves = kTempoThreads / 64;
constexpr int kTempoSums = 4;  // 64-bit running sums per point

constexpr int tempo_ring_entries(int K) { return kTempoChunk + K; }
constexpr size_t tempo_curve_lds_bytes(int K) {
    return (size_t)tempo_ring_entries(K) * (kTempoSums * sizeof(uint64_t) + sizeof(uint32_t));
}
constexpr size_t kTempoLdsLimit = 64 * 1024;  // what a launch may ask for without raising the kernel's limit
// The ring's arithmetic, for the kernel and for the stand-alone driver alike.  Point base + t of a turn lies in slot
// tempo_ring_wrap(s0 + t, R), s0 being the slot of the turn's first point (0 for the first turn, then tempo_ring_wrap(s0 +
// kTempoChunk, R)); the point K before the one in `slot` lies in tempo_ring_back(slot, K, R).  A turn overwrites points
// kTempoChunk + K back and older, which no window of the turn reaches.  Arguments in [0, 2R) / [0, R); results in [0, R).
constexpr int tempo_ring_wrap(int slot, int R) { return slot >= R ? slot - R : slot; }
constexpr int tempo_ring_back(int slot, int K, int R) { return slot - K < 0 ? slot - K + R : slot - K; }
// Turns the workgroup of a path of `len` points takes (len clamped to [0, P_max] first).
constexpr int tempo_curve_turns(int len, int P_max) {
    return ((len > P_max ? P_max : (len < 0 ? 0 : len)) + kTempoChunk - 1) / kTempoChunk;
}

// Tail kernel: one wave per stream, lane l takes points l, l + 64, ... of the stream's last min(K, stored) points.
constexpr int kTempoTailThreads = 64;
constexpr int kTempoTailTurns = (kTempoMaxK + kTempoTailThreads - 1) / kTempoTailThreads;

// rts_annot_bpm: one lane per entry, streams along y, like rts_annot_beats.
constexpr int kTempoBpmThreads = 256;
struct TempoGrid {
    unsigned x, y;
};
inline TempoGrid tempo_bpm_grid(int B, int n_max) {
    const TempoGrid g = {(unsigned)((n_max + kTempoBpmThreads - 1) / kTempoBpmThreads), (unsigned)B};
    return g;
}

}  // namespace rts
