// The level gate of the live chain (rts_live_gate): two launches between the chroma (and difference)
// step and the tracker push, which keep the columns of a microphone nobody plays into away from its tracker -- the
// batched form of the operator who presses `r` when the music starts (livenote_live.py:145-150, :162) with an eye on the
// microphone meter (livenote_live.py:170-177, wtw_live.py:192-197).  Included by live.hip behind LiveArgs.
//
//   live_level_kernel   lev[b][m] = mean square of the fft_len pending samples column m of stream b was framed from
//   live_gate_kernel    the decision recurrence over the stream's new columns, the kept ones packed to the front of a
//                       second column buffer, counts, ordinals, and the four meter words of rts_live_levels
//
// State per stream, carried on the device from feed to feed: q, the length of the current run of quiet columns (it
// saturates at hold + 1; a closed stream is one with q > hold); whether the previous chroma column passed; seen and
// passed, the chroma columns completed and the columns handed on since create, reset or the last restart.  A fresh
// stream is closed whatever `hold` is: its q is kGateClosed, hold + 1 of the largest hold there is, which the first
// quiet column brings down to min(q + 1, hold + 1) = hold + 1 like any other.  So switching the gate on writes nothing
// to the device, rts_live_reset fills q with one 32-bit pattern, and live_restart_kernel stores it for its streams.
#pragma once

namespace rts {

constexpr int kGateMaxHold = 65535;
constexpr int kGateClosed = kGateMaxHold + 1;
constexpr int kGateBlock = 1024;  // columns decided, then copied, between two barriers of live_gate_kernel

struct GateArgs {
    double min_level;    // a column is loud iff level >= min_level (a NaN level is quiet)
    int hold, diff;
    double *lev;         // [B][cols_stride] levels of this feed's chroma columns
    double *gcols;       // [B][cols_stride][12] the columns handed to the tracker, packed to the front
    int32_t *n_gated;    // [B] their counts
    int32_t *q, *prev, *seen, *passed;  // [B]
    int32_t *ord;        // [B][ord_len] ordinal (among the stream's chroma columns) of every column handed on
    int ord_len;         // the bound tracker's history length
    double *pub_level;   // host-mapped [B]                (the gate block of csrc/live_pub.h: plane kGateLevel and,
    int32_t *pub_words;  // host-mapped [B][kGateWords]     interleaved from kGateOpen on, the three meter words)
};

// grid (n_max, B), one workgroup per column.  level = (sum_i (double)x[i] * (double)x[i]) / L over the L = fft_len
// samples at offset m * hop of the stream's pending buffer -- after PCM scaling and resampling, where the chroma kernel
// has just framed column m.  Every product is exact in float64; the order of the sum is a function of the index i alone:
// lane l owns the groups of four indices 4 (l + 256 k) .. + 3 and adds them in rising order, the up to three indices
// behind the last whole group go one each to lanes 0 .. 2, then the lanes of a wave fold by halves (32, 16, .. 1) and
// the four wave sums are added in wave order.  A group is one 16-byte load when the frame starts on a 16-byte boundary
// (hops and max_pending are arbitrary, so it may start on any sample) and four 4-byte loads otherwise: same values, same
// order, so a frame's level depends neither on where it lies in the buffer nor on how the audio was cut into feeds.
__global__ void __launch_bounds__(256) live_level_kernel(LiveArgs g, GateArgs t) {
    __shared__ double wave_sum[4];
    const int m = blockIdx.x, b = blockIdx.y;
    if (m >= g.n_frames[b]) return;
    const long long start = (long long)m * g.hop;
    if (start + g.L > g.cap) return;  // (n_frames comes from pending <= cap, so the frame lies inside the buffer)
    const float *x = g.buf + (size_t)b * g.cap + start;
    const int L4 = g.L & ~3;
    double acc = 0.0;
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0) {
        for (int i = 4 * threadIdx.x; i < L4; i += 4 * 256) {
            const float4 v = *reinterpret_cast<const float4 *>(x + i);
            acc += (double)v.x * (double)v.x;
            acc += (double)v.y * (double)v.y;
            acc += (double)v.z * (double)v.z;
            acc += (double)v.w * (double)v.w;
        }
    } else {
        for (int i = 4 * threadIdx.x; i < L4; i += 4 * 256) {
            const float v0 = x[i], v1 = x[i + 1], v2 = x[i + 2], v3 = x[i + 3];
            acc += (double)v0 * (double)v0;
            acc += (double)v1 * (double)v1;
            acc += (double)v2 * (double)v2;
            acc += (double)v3 * (double)v3;
        }
    }
    if (L4 + (int)threadIdx.x < g.L) {
        const float v = x[L4 + threadIdx.x];
        acc += (double)v * (double)v;
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
        t.lev[(size_t)b * g.cols_stride + m] = (((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3]) / (double)g.L;
}

// One workgroup per stream.  Wave 0 runs the recurrence, 64 columns at a time: with the ballot of the loud columns, lane
// i's run of quiet columns is its distance from the last loud lane at or below it, or the incoming q + i + 1 when there
// is none, capped at hold + 1; the column passes iff that is <= hold.  In diff mode the column handed on is the
// difference of chroma columns (m - 1, m), and it goes iff both passed: the ballot of the passes shifted by one lane,
// with the carried word for lane 0 (zero whenever the stream has no carry, and then live_diff_kernel has made no
// difference column for m = 0 either: its columns start `skip` = n - n_cols rows late).  A prefix count over the ballot
// of the columns handed on gives each its row in the gated buffer.  Rows go to LDS, kGateBlock columns at a time, and
// all lanes copy the kept columns over the flat (column, pitch class) index: contiguous 8-byte loads, and stores that are
// contiguous within every run of kept columns.  Thread 0 carries the state on and publishes the meter words; the
// compaction, which writes the feed number last, follows in the same stream.
__global__ void __launch_bounds__(256) live_gate_kernel(LiveArgs g, GateArgs t) {
    __shared__ int32_t dest[kGateBlock];  // row in the gated buffer, -1: not handed on
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63;
    int n = g.n_frames[b];
    if (n > g.cols_stride) n = g.cols_stride;
    const int skip = t.diff ? n - g.n_cols[b] : 0;
    const double *in = (t.diff ? g.dcols : g.cols) + (size_t)b * g.cols_stride * kLiveF;
    double *out = t.gcols + (size_t)b * g.cols_stride * kLiveF;
    const double *lev = t.lev + (size_t)b * g.cols_stride;
    int32_t *ord = t.ord + (size_t)b * t.ord_len;
    const int seen0 = t.seen[b], passed0 = t.passed[b];
    int q = t.q[b], prev = t.prev[b], kept = 0;  // carried by wave 0, the same in all its lanes
    for (int base = 0; base < n; base += kGateBlock) {
        const int nb = n - base < kGateBlock ? n - base : kGateBlock;
        if (threadIdx.x < 64) {
            for (int c0 = 0; c0 < nb; c0 += 64) {
                const int i = c0 + lane, m = base + i;
                const bool live = i < nb;
                const bool loud = live && lev[m] >= t.min_level;
                const unsigned long long loud_mask = __ballot(loud);
                const unsigned long long at_or_below = loud_mask & (~0ull >> (63 - lane));
                int qi = at_or_below ? lane - (63 - __clzll(at_or_below)) : q + lane + 1;
                if (qi > t.hold + 1) qi = t.hold + 1;
                const bool pass = live && qi <= t.hold;
                const unsigned long long pass_mask = __ballot(pass);
                bool hand = pass;
                if (t.diff) hand = pass && m >= skip && (lane ? (int)((pass_mask >> (lane - 1)) & 1) : prev);
                const unsigned long long hand_mask = __ballot(hand);
                const int d = kept + __popcll(hand_mask & ((1ull << lane) - 1));
                if (live) {
                    dest[i] = hand ? d : -1;
                    if (hand && passed0 + d < t.ord_len) ord[passed0 + d] = seen0 + m;
                }
                const int last = (nb - c0 < 64 ? nb - c0 : 64) - 1;
                q = __shfl(qi, last, 64);
                prev = (int)((pass_mask >> last) & 1);
                kept += __popcll(hand_mask);
            }
        }
        __syncthreads();
        for (int e = threadIdx.x; e < nb * kLiveF; e += blockDim.x) {
            const int col = e / kLiveF, f = e - col * kLiveF;
            const int d = dest[col];
            if (d >= 0) out[(size_t)d * kLiveF + f] = in[(size_t)(base + col - skip) * kLiveF + f];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        t.n_gated[b] = kept;
        t.q[b] = q;
        t.prev[b] = prev;
        t.seen[b] = seen0 + n;
        t.passed[b] = passed0 + kept;
        volatile int32_t *w = t.pub_words + (size_t)b * kGateWords;
        if (n > 0) {  // a feed without a column leaves the meter on the stream's last one
            *(volatile double *)(t.pub_level + b) = lev[n - 1];
            w[0] = prev;
        }
        w[1] = seen0 + n;
        w[2] = passed0 + kept;
        __threadfence_system();
    }
}

// live_restart_kernel's share: the stream is closed again and has seen nothing.  (Its meter words are emptied with every
// other block's, through the table of csrc/live_pub.h.)
__device__ __forceinline__ void live_gate_restart(const GateArgs &t, int b) {
    t.q[b] = kGateClosed;
    t.prev[b] = 0;
    t.seen[b] = 0;
    t.passed[b] = 0;
}

}  // namespace rts
