// The host-mapped word blocks of a live session (csrc/live.hip): ONE table says where every word of every
// block lies and what an empty word holds, and sizes, typed pointers and clears are derived from it.  No HIP, so
// tests/sanitize/live_pub_driver.cpp runs it stand-alone; the kernels of live.hip call the same functions.
//
// A block is a handful of planes.  A plane holds one word per stream (or, in the consensus block, per group), float64 or
// int32, at byte offset `per_B * B + lane * (element size)` of the block and `stride` elements from one stream to the
// next: 1 for the planar [B] planes, kLiveWords / kGateWords for the interleaved words of the status and the gate block.
// The float64 planes come first in every block, so every float64 word is 8-byte aligned for every B (static_assert below).
// The kernels that fill the blocks (csrc/live.hip lists them) get plain pointers made by pub_ptr.
// What a new publisher adds besides its entry here: the head of live.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#if defined(__HIPCC__)
#define RTS_PUB_HD __host__ __device__
#define RTS_PUB_UNROLL _Pragma("unroll")  // the table folds into straight-line stores in a kernel
#else
#define RTS_PUB_HD
#define RTS_PUB_UNROLL
#endif

namespace rts {

enum PubBlock { kPubStatus = 0, kPubGate, kPubConf, kPubBeats, kPubTempo, kPubEns, kPubBlocks };

constexpr int kLiveWords = 4;  // per stream in the status block: status, live position, ref position, feed number
constexpr int kGateWords = 3;  // per stream in the gate block behind level[B]: open, seen, passed

// The planes of each block, in the order of the table.
enum { kStatusStatus, kStatusLive, kStatusRef, kStatusFeed };
enum { kGateLevel, kGateOpen, kGateSeen, kGatePassed };
enum { kConfMean, kConfN };
enum { kBeatsBeat, kBeatsLabel, kBeatsRef };
enum { kTempoSlope, kTempoPos, kTempoBpm, kTempoN };
enum { kEnsConsensus, kEnsSpread, kEnsDev, kEnsNIn, kEnsNValid, kEnsStrikes, kEnsOut };

constexpr int64_t kPubNaN = 0x7ff8000000000000LL;  // the quiet NaN every empty float64 word holds

struct PubPlane {
    bool f64;        // float64, else int32
    int per_B, lane, stride;
    int64_t empty;   // bit pattern of the empty value (an int32 plane takes the low word)
    bool per_group;  // a word per group: only allocation and rts_live_reset clear it, never a restart or an import
};

constexpr int kPubMaxPlanes = 7;
struct PubLayout {
    int n;
    PubPlane plane[kPubMaxPlanes];
};

constexpr bool kPubF64 = true, kPubI32 = false, kPubGroup = true;
constexpr PubLayout kPubLayout[kPubBlocks] = {
    // status, 16 B: int32 [B][kLiveWords].  A restart republishes the first three from the tracker and keeps the fourth.
    {4, {{kPubI32, 0, 0, kLiveWords, 0}, {kPubI32, 0, 1, kLiveWords, 0}, {kPubI32, 0, 2, kLiveWords, 0}, {kPubI32, 0, 3, kLiveWords, 0}}},
    // gate, 8 B + 12 B: level[B], then int32 [B][kGateWords]
    {4, {{kPubF64, 0, 0, 1, kPubNaN}, {kPubI32, 8, 0, kGateWords, 0}, {kPubI32, 8, 1, kGateWords, 0}, {kPubI32, 8, 2, kGateWords, 0}}},
    // confidence, 8 B + 4 B: mean[B], n[B]
    {2, {{kPubF64, 0, 0, 1, kPubNaN}, {kPubI32, 8, 0, 1, 0}}},
    // beats, 8 B + 2 * 4 B: beat[B], label[B], ref_frame[B]
    {3, {{kPubF64, 0, 0, 1, kPubNaN}, {kPubI32, 8, 0, 1, -1}, {kPubI32, 12, 0, 1, -1}}},
    // tempo, 3 * 8 B + 4 B: slope[B], pos[B], bpm[B], n[B]
    {4, {{kPubF64, 0, 0, 1, kPubNaN}, {kPubF64, 8, 0, 1, kPubNaN}, {kPubF64, 16, 0, 1, kPubNaN}, {kPubI32, 24, 0, 1, 0}}},
    // consensus, 3 * 8 B + 4 * 4 B, sized for B groups: consensus[B], spread[B], dev[B], n_in[B], n_valid[B], strikes[B], out[B]
    {7, {{kPubF64, 0, 0, 1, kPubNaN, kPubGroup}, {kPubF64, 8, 0, 1, kPubNaN, kPubGroup}, {kPubF64, 16, 0, 1, kPubNaN},
         {kPubI32, 24, 0, 1, 0, kPubGroup}, {kPubI32, 28, 0, 1, 0, kPubGroup}, {kPubI32, 32, 0, 1, 0}, {kPubI32, 36, 0, 1, 0}}},
};

// The blocks whose per-stream words a restart empties: all but the status block (republished from the fresh tracker).
constexpr unsigned kPubRestartBlocks = ((1u << kPubBlocks) - 1) & ~(1u << kPubStatus);

RTS_PUB_HD constexpr size_t pub_elem_bytes(const PubPlane &p) { return p.f64 ? 8 : 4; }
RTS_PUB_HD constexpr size_t pub_plane_offset(const PubPlane &p, int B) { return (size_t)p.per_B * B + p.lane * pub_elem_bytes(p); }

RTS_PUB_HD constexpr size_t pub_block_bytes(PubBlock k, int B) {
    size_t bytes = 0;
    for (int i = 0; i < kPubLayout[k].n; i++) {
        const PubPlane &p = kPubLayout[k].plane[i];
        const size_t end = pub_plane_offset(p, B) + ((size_t)(B - 1) * p.stride + 1) * pub_elem_bytes(p);
        if (end > bytes) bytes = end;
    }
    return bytes;
}

// float64 first, every offset a multiple of the element size for every B, no plane beyond the table
constexpr bool pub_layout_ok() {
    for (int k = 0; k < kPubBlocks; k++) {
        if (kPubLayout[k].n < 1 || kPubLayout[k].n > kPubMaxPlanes) return false;
        for (int i = 0; i < kPubLayout[k].n; i++) {
            const PubPlane &p = kPubLayout[k].plane[i];
            if (p.per_B % (int)pub_elem_bytes(p) != 0 || p.stride < 1 || p.lane < 0 || p.lane >= p.stride) return false;
            if (i > 0 && p.f64 && !kPubLayout[k].plane[i - 1].f64) return false;
        }
    }
    return true;
}
static_assert(pub_layout_ok(), "live_pub.h: float64 planes first and 8-byte aligned for every B");

// Stream b's word (default: the first) in plane P of block K, typed by the table; `base`: the block, host or device side.
template <PubBlock K, int P>
RTS_PUB_HD inline auto pub_ptr(void *base, int B, int b = 0) {
    static_assert(P >= 0 && P < kPubLayout[K].n, "no such plane");
    constexpr PubPlane p = kPubLayout[K].plane[P];
    using T = std::conditional_t<p.f64, double, int32_t>;
    return reinterpret_cast<T *>(static_cast<unsigned char *>(base) + pub_plane_offset(p, B)) + (size_t)b * p.stride;
}

// (plain stores: a kernel that clears ends with a system-scope fence, the host clears while the device is idle)
RTS_PUB_HD inline void pub_store_empty(const PubPlane &p, unsigned char *base, int B, int b) {
    unsigned char *at = base + pub_plane_offset(p, B) + (size_t)b * p.stride * pub_elem_bytes(p);
    if (p.f64) {
        double v;
        __builtin_memcpy(&v, &p.empty, sizeof v);
        *reinterpret_cast<double *>(at) = v;
    } else {
        *reinterpret_cast<int32_t *>(at) = (int32_t)p.empty;
    }
}

// Every word of the block empty, the group words included: allocation and rts_live_reset.
inline void pub_clear_all(PubBlock k, void *base, int B) {
    for (int i = 0; i < kPubLayout[k].n; i++)
        for (int b = 0; b < B; b++) pub_store_empty(kPubLayout[k].plane[i], static_cast<unsigned char *>(base), B, b);
}

// The per-stream words of stream b empty, nobody else's and no group word touched.
RTS_PUB_HD inline void pub_clear_stream(PubBlock k, void *base, int B, int b) {
    RTS_PUB_UNROLL
    for (int i = 0; i < kPubLayout[k].n; i++)
        if (!kPubLayout[k].plane[i].per_group) pub_store_empty(kPubLayout[k].plane[i], static_cast<unsigned char *>(base), B, b);
}

// The blocks as the device sees them; NULL: never allocated.
struct PubSet {
    unsigned char *dev[kPubBlocks];
};

}  // namespace rts
