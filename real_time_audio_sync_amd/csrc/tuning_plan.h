// Host side of the tuning estimator (csrc/tuning.hip): the rules rts_tuning_create and rts_tuning_pick check, the LDS
// layout and launch geometry of the histogram kernel, the edge search, and the pick -- integer arithmetic and one
// float64 expression, the very functions the pick kernel calls.  No HIP in it, so tests/sanitize/tuning_plan_driver.cpp
// runs it stand-alone.  The definition is include/rtsync.h's (rts_tuning_accumulate, rts_tuning_pick).
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define RTS_TU_HD __host__ __device__
#else
#define RTS_TU_HD
#endif

namespace rts {

constexpr int kTuningMinFft = 64;
constexpr int kTuningMaxFft = 8192;  // the chroma plan's own limit: the largest frame rts_chroma_frames writes
constexpr int kTuningMaxR = 1024;    // sizes the LDS histogram and the pick kernel's score table

// ---- what create and pick refuse ------------------------------------------------------------------------------------
enum TuningRefusal {
    kTuningOk = 0,
    kTuningBadFft,     // not a power of two in [kTuningMinFft, kTuningMaxFft]      (RTS_ERR_UNSUPPORTED)
    kTuningBadBins,    // not 1 <= k_lo <= k_hi <= fft_len / 2 - 1
    kTuningBadR,       // R < 1
    kTuningBigR,       // R > kTuningMaxR                                             (RTS_ERR_UNSUPPORTED)
    kTuningFewEdges,   // n_edges < 2
    kTuningNoEdges,    // edges_host is NULL
    kTuningBadEdges,   // an edge that is not finite and positive, or not above the one before it
    kTuningBadThr,     // thr_pow outside [0, 1] (NaN included)
    kTuningBadBinHz,   // bin_hz not finite and positive
    kTuningBadW,       // W < 0 or 2 W + 1 > R
};

inline bool tuning_refusal_unsupported(int why) { return why == kTuningBadFft || why == kTuningBigR; }

// The first rule a create call breaks, in the order of the list above; *bad_edge: the offending edge's index.
inline int tuning_create_refusal(int fft_len, int k_lo, int k_hi, int R, int n_edges, const double *edges, double bin_hz,
                                 double thr_pow, int *bad_edge) {
    const double inf = __builtin_inf();
    if (fft_len < kTuningMinFft || fft_len > kTuningMaxFft || (fft_len & (fft_len - 1)) != 0) return kTuningBadFft;
    if (k_lo < 1 || k_hi < k_lo || k_hi > fft_len / 2 - 1) return kTuningBadBins;
    if (R < 1) return kTuningBadR;
    if (R > kTuningMaxR) return kTuningBigR;
    if (n_edges < 2) return kTuningFewEdges;
    if (!edges) return kTuningNoEdges;
    for (int n = 0; n < n_edges; n++) {
        const bool ok = edges[n] > 0.0 && edges[n] < inf && (n == 0 || edges[n] > edges[n - 1]);  // NaN fails every test
        if (!ok) {
            if (bad_edge) *bad_edge = n;
            return kTuningBadEdges;
        }
    }
    if (!(thr_pow >= 0.0 && thr_pow <= 1.0)) return kTuningBadThr;
    if (!(bin_hz > 0.0 && bin_hz < inf)) return kTuningBadBinHz;
    return kTuningOk;
}

inline int tuning_pick_refusal(int R, int W) { return (W < 0 || 2LL * W + 1 > R) ? kTuningBadW : kTuningOk; }

// ---- the histogram kernel's geometry --------------------------------------------------------------------------------
// Persistent workgroups of kTuningThreads lanes, each owning a contiguous range of frames; lane t holds bins t, t +
// kTuningThreads, ... of the frame in flight, kTuningPerLane of them at the largest frame.
constexpr int kTuningThreads = 512;
constexpr int kTuningWaves = kTuningThreads / 64;
constexpr int kTuningPerLane = (kTuningMaxFft / 2 + 1 + kTuningThreads - 1) / kTuningThreads;
constexpr int kTuningMaxGroups = 512;  // two workgroups of the default layout per CU (LDS) on 256 CUs
// A workgroup's LDS counters are 32 bits wide and a frame has fewer than 2^12 peaks: flushed at least this often they
// stay below 2^32.
constexpr long long kTuningFlushFrames = 1LL << 19;
constexpr size_t kTuningLdsLimit = 64 * 1024;  // what a launch may ask for without raising the kernel's limit

// Dynamic LDS, in this order: P[n_bins rounded up to even] doubles, the edge table (n_edges doubles, when staged),
// kTuningWaves doubles of wave maxima, R 32-bit counters.
struct TuningLds {
    int p_doubles;      // n_bins rounded up to even: what follows stays 16-byte aligned
    int edges_staged;   // 1: the edge table lies in LDS behind P
    size_t edges_off, wmax_off, hist_off, bytes;  // byte offsets from the base
};
constexpr size_t tuning_lds_bytes(int fft_len, int n_edges, int R, bool staged) {
    return sizeof(double) * ((size_t)((fft_len / 2 + 2) & ~1) + (staged ? (size_t)n_edges : 0) + kTuningWaves) +
           sizeof(uint32_t) * (size_t)R;
}
inline TuningLds tuning_lds(int fft_len, int n_edges, int R) {
    TuningLds l;
    l.p_doubles = (fft_len / 2 + 2) & ~1;
    l.edges_staged = tuning_lds_bytes(fft_len, n_edges, R, true) <= kTuningLdsLimit ? 1 : 0;
    l.edges_off = sizeof(double) * (size_t)l.p_doubles;
    l.wmax_off = l.edges_off + (l.edges_staged ? sizeof(double) * (size_t)n_edges : 0);
    l.hist_off = l.wmax_off + sizeof(double) * kTuningWaves;
    l.bytes = l.hist_off + sizeof(uint32_t) * (size_t)R;
    return l;
}

// A workgroup stages the edge table once, so it is given at least kTuningMinFrames frames to spread that over.  Measured
// (profiles/tuning.md): 8 frames on at most 256 workgroups, and the table left in L2, are both slower at 2048 frames.
constexpr int kTuningMinFrames = 4;
inline int tuning_groups(long long n_frames) {
    const long long g = (n_frames + kTuningMinFrames - 1) / kTuningMinFrames;
    return g < kTuningMaxGroups ? (int)g : kTuningMaxGroups;
}
// Workgroup g of G owns frames [tuning_first_frame(g), tuning_first_frame(g + 1)): contiguous, lengths within one of
// each other.  g in [0, G], G >= 1; the product stays below 2^63 for every n_frames < 2^53.
RTS_TU_HD inline long long tuning_first_frame(long long n_frames, int G, int g) {
    return (n_frames / G) * g + ((n_frames % G) * g) / G;
}

// ---- the edge search ------------------------------------------------------------------------------------------------
// The largest n with E[n] <= f, -1 when there is none (f below E[0], or NaN): np.searchsorted(E, f, 'right') - 1.
// Reads E[0 .. n_edges) only.
template <typename Table>
RTS_TU_HD inline int tuning_edge_index(const Table &E, int n_edges, double f) {
    int lo = 0, hi = n_edges;  // E[i] <= f for every i < lo, E[i] > f (or f is NaN) for every i >= hi
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (E[mid] <= f) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}
// The histogram bin of edge index n, or -1 for a peak that is dropped (outside the table).
RTS_TU_HD inline int tuning_hist_bin(int n, int n_edges, int R) { return (n < 0 || n >= n_edges - 1) ? -1 : n % R; }

// ---- the pick -------------------------------------------------------------------------------------------------------
// score[i] = sum over d in [-W, W] of (W + 1 - |d|) * hist[(i + d) mod R], in unsigned 64-bit arithmetic (it wraps only
// past 2^64 / (W + 1)^2 counts).  R >= 1, 0 <= 2 W + 1 <= R, 0 <= i < R.
RTS_TU_HD inline uint64_t tuning_score(const uint64_t *hist, int R, int W, int i) {
    uint64_t s = (uint64_t)(W + 1) * hist[i];
    int up = i, down = i;
    for (int d = 1; d <= W; d++) {
        up = up + 1 == R ? 0 : up + 1;
        down = down == 0 ? R - 1 : down - 1;
        s += (uint64_t)(W + 1 - d) * (hist[up] + hist[down]);
    }
    return s;
}
// Does (score b, index ib) come before (score a, index ia)?  The larger score, and among equal ones the smaller index.
RTS_TU_HD inline bool tuning_beats(uint64_t sb, int ib, uint64_t sa, int ia) { return sb > sa || (sb == sa && ib < ia); }
// The centre of histogram bin i in cents; every operation rounded on its own (the sources are built without contraction).
RTS_TU_HD inline double tuning_cents(int i, int R) { return ((double)i + 0.5) * 100.0 / (double)R - 50.0; }

// The whole pick of one histogram, serially: what the pick kernel computes with one lane per bin.
inline void tuning_pick(const uint64_t *hist, int R, int W, double *cents, long long *n) {
    uint64_t N = 0;
    for (int i = 0; i < R; i++) N += hist[i];
    *n = (long long)N;
    *cents = 0.0;
    if (N == 0) return;
    uint64_t best = tuning_score(hist, R, W, 0);
    int at = 0;
    for (int i = 1; i < R; i++) {
        const uint64_t s = tuning_score(hist, R, W, i);
        if (tuning_beats(s, i, best, at)) {
            best = s;
            at = i;
        }
    }
    *cents = tuning_cents(at, R);
}

}  // namespace rts
