// Plan and commit of one live feed (csrc/live.hip, whose header tells what the mirror is for): integer arithmetic on
// counts, no HIP, so tests/sanitize/live_plan_driver.cpp runs it stand-alone.  live_plan_feed writes scratch only;
// live_mirror_commit is the one writer of the mirror between two resets / restarts.
#pragma once
#include <stdint.h>
#include <string.h>

namespace rts {

// Outputs whose last input sample, floor((k M + half) / L), is among the first in_total (rts_resample_avail).
inline long long resample_avail(long long in_total, int L, int M, int half) {
    if (in_total <= 0 || L < 1 || M < 1) return 0;
    const long long a = in_total * L - half;
    return a > 0 ? (a + M - 1) / M : 0;
}

struct LiveGeom {
    int B, L, hop, cap;       // streams, fft_len, hop, max_pending (plan-rate samples per stream)
    int diff;                 // RTS_FEATURE_CHROMA_DIFF
    int rs_L, rs_M, rs_half;  // the resampling plan's ratio and half length; rs_L == 0: no resampler
    long long in_cap;         // input-rate samples a staging slot holds per stream (resampler only)
};

struct LiveMirror {
    long long *pending;  // [B]
    uint8_t *has_carry;  // [B]     (read and written in diff mode only)
    long long *rs_tot;   // [B][2]  input samples taken, output samples made (with a resampler only)
};

enum LiveRefusal { kLiveFeedOk = 0, kLiveNegativeCount, kLiveOverStaging, kLiveOverPending };

struct FeedPlan {
    int32_t *offs;     // [B] exclusive prefix sum of counts, for the second table of the staging slot
    int32_t *rs_nout;  // [B] plan-rate samples the resampling launch makes per stream (with a resampler only)
    LiveMirror next;   // the mirror once the feed's chain has run
    long long total;   // samples in the slot
    int n_max;         // most chroma columns of a stream
    int n_max_diff;    // most columns a stream hands to the tracker in diff mode
    int n_out_max;     // largest rs_nout
    int stream;        // of a refusal: the first stream that breaks a rule, and its new plan-rate samples
    long long n_new;
};

// Writes `*p` and the arrays it points to, nothing else; a refused feed leaves them half written.
inline LiveRefusal live_plan_feed(const LiveGeom &g, const LiveMirror &cur, const int32_t *counts, FeedPlan *p) {
    const long long *pending = cur.pending, *rs_tot = cur.rs_tot;
    const uint8_t *has_carry = cur.has_carry;
    p->total = 0;
    p->n_max = p->n_max_diff = p->n_out_max = 0;
    for (int b = 0; b < g.B; b++) {
        p->stream = b;
        p->n_new = counts[b];
        if (counts[b] < 0) return kLiveNegativeCount;
        if (g.rs_L) {  // the tracker side sees what the resampling launch makes of these counts
            if (counts[b] > g.in_cap) return kLiveOverStaging;  // (more than any feed whose output fits max_pending)
            const long long in_next = rs_tot[2 * b] + counts[b];
            const long long out_next = resample_avail(in_next, g.rs_L, g.rs_M, g.rs_half);
            p->n_new = out_next - rs_tot[2 * b + 1];
            p->next.rs_tot[2 * b] = in_next;
            p->next.rs_tot[2 * b + 1] = out_next;
            p->rs_nout[b] = (int32_t)p->n_new;
            if (p->rs_nout[b] > p->n_out_max) p->n_out_max = p->rs_nout[b];
        }
        const long long q = pending[b] + p->n_new;
        if (q > g.cap) return kLiveOverPending;
        p->offs[b] = (int32_t)p->total;
        p->total += counts[b];
        // live_append_kernel: complete hops of q pending samples
        const int nf = q >= g.L ? (int)((q - g.L) / g.hop + 1) : 0;
        if (nf > p->n_max) p->n_max = nf;
        if (g.diff) {  // live_diff_kernel: a stream without a carry keeps its first column to itself
            const int nc = nf - (has_carry[b] ? 0 : 1);
            if (nc > p->n_max_diff) p->n_max_diff = nc;
            p->next.has_carry[b] = has_carry[b] || nf > 0;
        }
        // live_compact_kernel; hop > fft_len: a slice past the end leaves nothing
        const long long used = (long long)nf * g.hop;
        p->next.pending[b] = q > used ? q - used : 0;
    }
    return kLiveFeedOk;
}

inline void live_mirror_commit(const LiveGeom &g, const LiveMirror &cur, const LiveMirror &next) {
    memcpy(cur.pending, next.pending, sizeof(long long) * (size_t)g.B);
    if (g.diff) memcpy(cur.has_carry, next.has_carry, (size_t)g.B);
    if (g.rs_L) memcpy(cur.rs_tot, next.rs_tot, sizeof(long long) * 2 * (size_t)g.B);
}

// rts_live_import: the mirror entries of the slots that took a record, from the two words per stream an export handed
// out (pending samples, carry flag).  The one other writer of the mirror beside live_mirror_commit; entries of streams
// that are not listed, and the resampler's totals, are not touched.
inline void live_mirror_import(const LiveGeom &g, const LiveMirror &cur, int n, const int32_t *slots, const int32_t *words) {
    for (int i = 0; i < n; i++) {
        cur.pending[slots[i]] = words[2 * i];
        if (g.diff) cur.has_carry[slots[i]] = words[2 * i + 1] != 0;
    }
}

}  // namespace rts
