// Snapshot records (include/rtsync.h, rts_otw_export / rts_otw_import, their WTW and live counterparts): where
// the sections of a record lie, what a record's header must say before a slot takes it, how a selection is checked and
// cut into launches, and which desc field keeps a blob out of a handle.  Integer arithmetic only, no HIP, so that
// tests/sanitize/snapshot_plan_driver.cpp runs it stand-alone; the kernels (csrc/snapshot.h) call the same functions.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/rtsync.h"

#if defined(__HIPCC__)
#define RTS_SNAP_HD __host__ __device__
#else
#define RTS_SNAP_HD
#endif

namespace rts {
namespace snap {

constexpr int32_t kMagic = 0x31534E53;  // "SNS1"
constexpr int kFrameBytes = 96;         // 12 float64 chroma bins
constexpr int kPairBytes = 8;           // one (live, ref) int32 pair
constexpr int kOtwStateBytes = 64;      // RTS_STATE_LEN int32 words
constexpr int kWtwStateBytes = 32;      // RTS_WTW_STATE_LEN int32 words

// The header: 16 int32 words in front of every record.
enum Word {
    kWMagic = 0, kWVersion, kWKind,
    kWNb, kWMb,             // the stream's own reference length: N_b of an OTW record, M_b of a WTW record, the other 0
    kWHistValid,            // history frames in the record: min(raw count, 2 N_b)
    kWPathValid,            // path pairs in the record: min(n_path, the exporter's path capacity)
    kWHistLen,              // the history count the slot gets (OTW: raw, it runs past 2 N_b on RTS_LIVE_OVERFLOW)
    kWParam,                // what sizes the middle section: OTW the band width c; WTW the window W if D is carried, else 0
    kWOffState, kWOffMid, kWOffPath, kWOffHist,  // byte offsets from the record's start
    kWUsed,                 // bytes of the record that carry state; zeros from here to rec_stride
    kWPathCount,            // the stream's n_path word: above kWPathValid only where the exporter's path was truncated
    kHeaderWords = 16       // (word 15 is zero)
};
constexpr int kHeaderBytes = 4 * kHeaderWords;

RTS_SNAP_HD inline long long align16(long long v) { return (v + 15) & ~15LL; }

// A record packed by its valid counts: header, state words, the middle section (OTW: the two persisted bands; WTW: the
// last window's D where the handle keeps it), the path pairs, the history frames; every section on a multiple of 16.
struct Layout {
    long long off_state, off_mid, off_path, off_hist, used;
};
RTS_SNAP_HD inline Layout layout(int state_bytes, long long mid_bytes, long long hist_valid, long long path_valid) {
    Layout l;
    l.off_state = kHeaderBytes;
    l.off_mid = l.off_state + state_bytes;
    l.off_path = align16(l.off_mid + mid_bytes);
    l.off_hist = align16(l.off_path + kPairBytes * path_valid);
    l.used = l.off_hist + kFrameBytes * hist_valid;  // 96 = 6 * 16
    return l;
}
RTS_SNAP_HD inline long long mid_bytes(int kind, int param) {
    return kind == RTS_SNAPSHOT_OTW ? 16LL * (param + 1)  // two bands of c + 1 doubles
                                    : 8LL * param * param;  // D of W x W doubles
}
RTS_SNAP_HD inline Layout record_layout(int kind, int param, long long hist_valid, long long path_valid) {
    return layout(kind == RTS_SNAPSHOT_OTW ? kOtwStateBytes : kWtwStateBytes, mid_bytes(kind, param), hist_valid, path_valid);
}
// The stride a handle needs: its fullest possible record.  OTW: 2 N_max frames, 3 N_max + 8 pairs.  WTW: 2 M_max
// columns and the handle's path capacity.
inline long long otw_rec_stride(int N_max, int c) { return record_layout(RTS_SNAPSHOT_OTW, c, 2LL * N_max, 3LL * N_max + 8).used; }
inline long long wtw_rec_stride(int M_max, int W, int keep_last_d, long long path_cap) {
    return record_layout(RTS_SNAPSHOT_WTW, keep_last_d ? W : 0, 2LL * M_max, path_cap).used;
}
constexpr long long kMaxStride = 0x7fffffffLL;  // the header's offsets are int32

// A live session's record: the bound tracker's record in front, and at the END of the stride (so that both sides find
// it from rec_stride and max_pending alone) the live tail: four int32 words (pending count, carry flag, kLiveMagic,
// max_pending), the pending samples as float32 (zeros behind the count, up to max_pending, padded to 16 bytes), and
// the carried chroma column of difference features, 12 doubles (zeros without a carry and in chroma mode).
constexpr int32_t kLiveMagic = 0x3156494C;  // "LIV1"
constexpr int kLiveTailHeader = 16, kLiveCarryBytes = 96;
RTS_SNAP_HD inline long long live_tail_bytes(int max_pending) { return kLiveTailHeader + align16(4LL * max_pending) + kLiveCarryBytes; }
inline long long live_rec_stride(long long tracker_stride, int max_pending) { return tracker_stride + live_tail_bytes(max_pending); }

// What a slot makes of a record's header; every workgroup of an import computes it alike, from the header and the
// slot's own numbers.  `param`: the slot's c (OTW), or its W where it keeps D and 0 where not (WTW; a record without D
// -- no window yet -- fits both).  0, or the RTS_SNAP_* reason.  A header that passes describes sections that lie
// inside rec_stride and inside the slot's buffers, so the copy that follows needs no further bounds.
RTS_SNAP_HD inline int record_status(const int32_t *hdr, int kind, int param, int slot_len, long long slot_hist_cap,
                                     long long slot_path_cap, long long rec_stride) {
    if (hdr[kWMagic] != kMagic) return RTS_SNAP_BAD_MAGIC;
    if (hdr[kWVersion] != RTS_SNAPSHOT_VERSION) return RTS_SNAP_BAD_VERSION;
    if (hdr[kWKind] != kind) return RTS_SNAP_BAD_KIND;
    const bool otw = kind == RTS_SNAPSHOT_OTW;
    if (hdr[otw ? kWNb : kWMb] != slot_len) return RTS_SNAP_BAD_RANGE;
    const long long hv = hdr[kWHistValid], pv = hdr[kWPathValid];
    if (hv < 0 || hv > slot_hist_cap || hv > 2LL * slot_len) return RTS_SNAP_BAD_HISTORY;
    if (pv < 0 || pv > slot_path_cap) return RTS_SNAP_BAD_PATH;
    // a truncated path (n_path above the stored pairs) cannot move: a slot with more room would take pairs that were
    // never written for recorded ones and go on recording where the exporter stays truncated
    if (hdr[kWPathCount] != pv) return RTS_SNAP_BAD_PATH;
    const int rp = hdr[kWParam];
    if (hdr[otw ? kWMb : kWNb] != 0 || hdr[kWHistLen] < hv || (rp != param && (otw || rp != 0))) return RTS_SNAP_BAD_LAYOUT;
    const Layout l = record_layout(kind, rp, hv, pv);
    if (l.used > rec_stride || hdr[kWOffState] != l.off_state || hdr[kWOffMid] != l.off_mid || hdr[kWOffPath] != l.off_path ||
        hdr[kWOffHist] != l.off_hist || hdr[kWUsed] != l.used)
        return RTS_SNAP_BAD_LAYOUT;
    return 0;
}

// How a selection reaches the device: by value like RestartSel (csrc/common.h), kSelChunk streams per launch, in the
// caller's order.  rec[i] is the record's index in the blob.
constexpr int kSelChunk = 128;
struct SnapSel {
    int n;        // streams in this chunk
    int set_ref;  // import: first[] / len[] are given
    int32_t idx[kSelChunk];
    int32_t rec[kSelChunk];
    int32_t len[kSelChunk];
    long long first[kSelChunk];
};

// A selection names each stream once.  -1, or the position of the first entry that is out of [0, B) (*dup = 0) or
// repeats an earlier one (*dup = 1).
inline int sel_check(int B, const int32_t *idx, int n, int *dup) {
    std::vector<uint8_t> seen((size_t)(B > 0 ? B : 0), 0);
    for (int i = 0; i < n; i++) {
        *dup = 0;
        if (idx[i] < 0 || idx[i] >= B) return i;
        *dup = 1;
        if (seen[(size_t)idx[i]]) return i;
        seen[(size_t)idx[i]] = 1;
    }
    return -1;
}

// Fills `sel` with entries [*pos, *pos + kSelChunk) of the selection and advances *pos; returns sel->n.
inline int sel_next_chunk(int n, const int32_t *idx, const long long *first, const int32_t *len, int *pos, SnapSel *sel) {
    int k = 0;
    sel->set_ref = first != nullptr;
    for (; *pos < n && k < kSelChunk; ++*pos, ++k) {
        sel->idx[k] = idx[*pos];
        sel->rec[k] = *pos;
        sel->first[k] = first ? first[*pos] : 0;
        sel->len[k] = len ? len[*pos] : 0;
    }
    sel->n = k;
    return k;
}

// The first field of `d` a handle with the parameters `mine` (a desc filled as its own export would fill it, n and
// rec_stride those of the call) cannot take, or NULL.  Fields of another kind are not the handle's business.
inline const char *desc_mismatch(const rts_snapshot_desc &d, const rts_snapshot_desc &mine) {
    if (d.kind != mine.kind) return "kind";
    if (d.version != mine.version) return "version";
    if (d.n != mine.n) return "n";
    if (d.rec_stride != mine.rec_stride) return "rec_stride";
    if (d.ref_dtype != mine.ref_dtype) return "ref_dtype";
    if (d.F != mine.F) return "F";
    int tracker = mine.kind;
    if (mine.kind == RTS_SNAPSHOT_LIVE) {
        if (d.fft_len != mine.fft_len) return "fft_len";
        if (d.live_hop != mine.live_hop) return "live_hop";
        if (d.feature_kind != mine.feature_kind) return "feature_kind";
        if (d.max_pending != mine.max_pending) return "max_pending";
        if (d.tracker != mine.tracker) return "tracker";
        tracker = mine.tracker;
    }
    if (tracker == RTS_SNAPSHOT_OTW) {
        if (d.c != mine.c) return "c";
        if (d.max_run_count != mine.max_run_count) return "max_run_count";
        if (d.variant != mine.variant) return "variant";
        if (d.cost_kind != mine.cost_kind) return "cost_kind";
    } else if (tracker == RTS_SNAPSHOT_WTW) {
        if (d.window != mine.window) return "window";
        if (d.hop != mine.hop) return "hop";
        if (d.keep_last_d != mine.keep_last_d) return "keep_last_d";
    }
    return nullptr;
}

}  // namespace snap
}  // namespace rts
