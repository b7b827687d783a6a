// Host side of the live accompaniment (csrc/accomp.hip): the limits of its parameters, the rule that keeps every product
// of the steering law inside 64 bits, and the integer part of the law itself, which the steering kernel and the host share
// -- steps 3, 5, 7 (tail) and 8 of include/rtsync.h, rts_live_accompany.  No HIP in it, so
// tests/sanitize/accomp_plan_driver.cpp runs it stand-alone.
//
// All positions are int64 samples.  H is the warp plan's hop N / 2, `hop` the microphone samples per live frame, hop_track
// the track samples per reference frame.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RTS_ACC_HD __host__ __device__
#else
#define RTS_ACC_HD
#endif

namespace rts {

constexpr int kAccMaxHopTrack = 65536;
constexpr int kAccMinK = 2, kAccMaxK = 1024;      // the tempo kernels' range (csrc/tempo_plan.h)
constexpr int kAccMaxRatePm = 4000;
constexpr long long kAccLimit31 = 1LL << 31;      // glide, |lead|, a segment of the map on either axis
constexpr long long kAccTargetLimit = 1LL << 52;  // |floor(y1 * hop_track)| stays below: exact in float64 and in int64
constexpr long long kAccPosLimit = 1LL << 61;     // |origin| and the end of a track stay below: tgt + origin - i0 fits

// status bits of a stream (RTS_ACC_* of include/rtsync.h)
constexpr int kAccOn = 1, kAccWait = 2, kAccFree = 4, kAccLo = 8, kAccHi = 16, kAccEnd = 32, kAccFull = 64, kAccLate = 128;

struct AccompGeom {
    int H, hop, hop_track, K;
    long long glide, lead;
    int rate_min_pm, rate_max_pm, chunk_blocks, A_max;
};

enum AccompRefusal {
    kAccOk = 0,
    kAccBadHopTrack,
    kAccBadK,
    kAccBadGlide,
    kAccBadLead,
    kAccBadRates,
    kAccBadChunk,
    kAccBadAnchors,
    kAccOverflow,  // RTS_ERR_UNSUPPORTED: a chunk of chunk_blocks blocks whose segment could reach 2^31 on either axis
};

// The longest segment is one chunk, Ls = chunk_blocks H output samples, and at most hi = Ls hop_track rate_max_pm / (hop
// 1000) track samples: both stay below 2^31 (the renderer's segment rule), formed in 128 bits.  With that, Ls hop_track
// rate_pm < 2^31 2^16 2^12 = 2^59 and d Ls < 2^62 in the law below.
inline bool accomp_chunk_overflows(int chunk_blocks, int H, int hop_track, int hop, int rate_max_pm) {
    const unsigned __int128 Ls = (unsigned __int128)(unsigned)chunk_blocks * (unsigned)H;
    if (Ls >= (unsigned __int128)kAccLimit31) return true;
    const unsigned __int128 hi = Ls * (unsigned)hop_track * (unsigned)rate_max_pm / ((unsigned __int128)(unsigned)hop * 1000u);
    return hi >= (unsigned __int128)kAccLimit31;
}

// Every parameter limit of rts_live_accompany, in the order of its table; H >= 1 and hop >= 1 come from the two plans.
inline AccompRefusal accomp_params_check(const AccompGeom &p) {
    if (p.hop_track < 1 || p.hop_track > kAccMaxHopTrack) return kAccBadHopTrack;
    if (p.K < kAccMinK || p.K > kAccMaxK) return kAccBadK;
    if (p.glide < 0 || p.glide >= kAccLimit31) return kAccBadGlide;
    if (p.lead <= -kAccLimit31 || p.lead >= kAccLimit31) return kAccBadLead;
    if (p.rate_min_pm < 0 || p.rate_min_pm > p.rate_max_pm || p.rate_max_pm > kAccMaxRatePm || p.rate_max_pm < 1) return kAccBadRates;
    if (p.chunk_blocks < 1) return kAccBadChunk;
    if (p.A_max < 2) return kAccBadAnchors;
    if (accomp_chunk_overflows(p.chunk_blocks, p.H, p.hop_track, p.hop, p.rate_max_pm)) return kAccOverflow;
    return kAccOk;
}

// A track [first, first + len) of the pool and its origin, in pool samples.
inline bool accomp_track_ok(long long first, long long len, long long origin) {
    if (first < 0 || len < 0 || first >= kAccPosLimit || len >= kAccPosLimit || first + len >= kAccPosLimit) return false;
    if (origin <= -kAccPosLimit || origin >= kAccPosLimit) return false;
    const long long at = first + origin;
    return at > -kAccPosLimit && at < kAccPosLimit;
}

// ---- the law's integers ---------------------------------------------------------------------------------------------
// Step 3: the blocks due once `fed` samples have arrived, the output clock having started at `base`, capped at chunk_blocks
// past the k rendered so far; *late when the cap cut it.  fed >= base >= 0.
RTS_ACC_HD inline long long accomp_due(long long fed, long long base, int H, long long k, int chunk_blocks, int *late) {
    const long long due = (fed - base) / H, cap = k + chunk_blocks;
    *late = due > cap;
    return due > cap ? cap : due;
}

// Step 5: floor(Ls hop_track rate_pm / (hop 1000)); rate_pm = 1000 gives the nominal step.
RTS_ACC_HD inline long long accomp_rate_step(long long Ls, int hop_track, int hop, int rate_pm) {
    return (Ls * hop_track * rate_pm) / ((long long)hop * 1000);
}
RTS_ACC_HD inline long long accomp_nominal(long long Ls, int hop_track, int hop) { return (Ls * hop_track) / hop; }

// Step 7, behind the float64 part: the distance d from the last anchor to the target, clamped to [0, 2^31 - 1], and the
// share of it this segment takes, floor(d Ls / (Ls + G)).  |tgt| < 2^52.
RTS_ACC_HD inline long long accomp_step_raw(long long tgt, long long origin, long long i0, long long Ls, long long G) {
    long long d = tgt + origin - i0;
    d = d < 0 ? 0 : (d > kAccLimit31 - 1 ? kAccLimit31 - 1 : d);
    return (d * Ls) / (Ls + G);
}

// Step 8: the step inside [lo, hi] and the anchor inside the track; the status bits it sets are added to *status.
RTS_ACC_HD inline long long accomp_advance(long long i0, long long step_raw, long long lo, long long hi, long long track_end,
                                           int *status) {
    long long step = step_raw;
    if (step < lo) step = lo, *status |= kAccLo;
    if (step > hi) step = hi, *status |= kAccHi;
    const long long stop = i0 > track_end ? i0 : track_end;
    long long i1 = i0 + step;
    if (i1 > stop) i1 = stop, *status |= kAccEnd;
    return i1;
}

// The ring of chunks: feed f (counted from 1) renders into slot f % kAccSlots, rows of chunk_blocks H float32 samples.
constexpr int kAccSlots = 4;  // kLiveSlots of csrc/live.hip
constexpr int kAccThreads = 64;
// bytes of one slot's words for B streams: int64 out_total, in_pos; double rate; int32 blocks, status, warp_status, seq
constexpr size_t accomp_words_bytes(int B) { return (size_t)B * (3 * 8 + 4 * 4); }

}  // namespace rts
