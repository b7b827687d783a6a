// Snapshots of single tracker streams (include/rtsync.h, rts_otw_export / rts_otw_import, rts_wtw_export /
// rts_wtw_import): the gather of one stream's carried state into a self-contained record and the scatter
// of a record into a slot of another handle.  Where things lie and what a header must say is csrc/snapshot_plan.h's
// (host-only, tested on the CPU); here are the two kernels, which serve both trackers through a description of the
// handle's buffers, and what the entry points share.  The entry points themselves are beside their handles (otw_host.h,
// wtw.hip).  Everything is static: the header is compiled into more than one translation unit.
// Live sessions put their tail behind a tracker's record: csrc/snapshot_live.h.
#pragma once
#include "common.h"
#include "snapshot_plan.h"

namespace rts {

// A tracker handle as the snapshot kernels see it.  Both trackers keep, per stream: int32 state words, a path of int32
// pairs, a float64 history of 12-bin frames with its count, the length of the reference range, and a middle section
// (OTW: the two persisted bands, 2 (c + 1) doubles; WTW: the last window's D, W * W doubles, on a keep_last_d handle once
// a window has run).  State and history of a stream start on a multiple of 16 bytes in the handle (32 / 64 bytes of
// state, 96-byte frames behind hipMalloc'd bases); the path (an odd number of pairs per stream at odd N_max) and D (odd
// W) need not, so those two move as 8-byte elements on the handle's side and as 16-byte units on the record's.
struct SnapView {
    int kind;  // RTS_SNAPSHOT_OTW / RTS_SNAPSHOT_WTW
    int32_t *state;
    int state_words, st_n_path;
    unsigned long long *mid;  // bands / D as 8-byte elements, mid_stride of them per stream
    long long mid_stride;
    int param;     // c; W on a keep_last_d handle, else 0
    int mid_gate;  // the state word that must be > 0 for the middle section to exist (WTW: windows run), -1: always
    int32_t *path;
    int path_cap;
    double *hist;  // NULL (OTW before its first frame): every stream's history is empty
    int hist_stride;
    int32_t *count, *count2;  // the history count; WTW: both of its count arrays (an import writes both)
    long long *ref_first;
    int32_t *ref_len;
    int len_default;          // N / M of a single-reference handle
    int32_t *ctl, *ticket;    // WTW strip-DP handles: zeroed by an import, as by a restart (no window is pending between
                              // two pushes, so nothing in them survives a push; wtw_ctl_body rewrites them)
    int zero_hist;            // import: the slot's history behind the record's frames reads zero again (wtw.py:55)
    int dry;                  // import: write the status words and nothing else (rts_live_import asks before it changes anything)
    unsigned char *blob;
    long long rec_stride;
    int32_t *status;  // import
};

constexpr int kSnapThreads = 256;
constexpr int kSnapSlices = 64;  // at most; a launch takes one workgroup per 32 KB of rec_stride

// Grid (slices, sel.n): the workgroups of a stream share its record in 16-byte units, unit u going to thread u modulo
// the stream's threads, so slice 0 writes the header; the zero tail up to rec_stride is written by the same lanes.  Every
// lane derives the layout from the same few words of the handle, which the kernel does not write.
static __global__ void __launch_bounds__(kSnapThreads) snap_export_kernel(snap::SnapSel sel, SnapView a) {
    if ((int)blockIdx.y >= sel.n) return;
    const int b = sel.idx[blockIdx.y];
    const bool otw = a.kind == RTS_SNAPSHOT_OTW;
    const int32_t *st = a.state + (size_t)b * a.state_words;
    const int Nb = a.ref_len ? a.ref_len[b] : a.len_default;
    const int n_path = st[a.st_n_path];  // counts past path_cap once the path is truncated: such a record no slot takes
    const int pv = n_path < 0 ? 0 : (n_path > a.path_cap ? a.path_cap : n_path);
    int raw = a.hist ? a.count[b] : 0;
    raw = raw < 0 ? 0 : raw;
    int hv = raw > 2 * Nb ? 2 * Nb : raw;  // frames past 2 N_b are never read by anything (otw_recent_kernel's rule)
    hv = hv > a.hist_stride ? a.hist_stride : hv;
    // OTW: t keeps counting the raw count past RTS_LIVE_OVERFLOW.  WTW: past 2 M_b only "more than 2 M_b" is ever asked
    // (wtw_ctl_body), and how far the count ran depends on the exporter's stride: 2 M_b + 1 says it for every handle.
    const int cnt = otw ? raw : (raw > 2 * Nb + 1 ? 2 * Nb + 1 : raw);
    const int rp = (a.mid_gate >= 0 && st[a.mid_gate] <= 0) ? 0 : a.param;
    const long long mid_elems = snap::mid_bytes(a.kind, rp) >> 3;
    const snap::Layout l = snap::record_layout(a.kind, rp, hv, pv);
    unsigned char *rec = a.blob + (long long)sel.rec[blockIdx.y] * a.rec_stride;
    const unsigned char *state_b = reinterpret_cast<const unsigned char *>(st);
    const unsigned long long *mid_b = a.mid + (long long)b * a.mid_stride;
    const unsigned long long *path_b = reinterpret_cast<const unsigned long long *>(a.path) + (size_t)b * a.path_cap;
    const unsigned char *hist_b =  // (hv = 0 without a history: never used then)
        a.hist ? reinterpret_cast<const unsigned char *>(a.hist) + (long long)b * a.hist_stride * snap::kFrameBytes : nullptr;
    const long long step = 16LL * gridDim.x * blockDim.x;
    for (long long o = 16LL * (blockIdx.x * blockDim.x + threadIdx.x); o < a.rec_stride; o += step) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (o < snap::kHeaderBytes) {
            switch ((int)(o >> 4)) {  // the words of snap::Word, four to a unit
                case 0: v = make_uint4((unsigned)snap::kMagic, RTS_SNAPSHOT_VERSION, (unsigned)a.kind, (unsigned)(otw ? Nb : 0)); break;
                case 1: v = make_uint4((unsigned)(otw ? 0 : Nb), (unsigned)hv, (unsigned)pv, (unsigned)cnt); break;
                case 2: v = make_uint4((unsigned)rp, (unsigned)l.off_state, (unsigned)l.off_mid, (unsigned)l.off_path); break;
                default: v = make_uint4((unsigned)l.off_hist, (unsigned)l.used, (unsigned)n_path, 0u); break;
            }
        } else if (o < l.off_mid) {
            v = *reinterpret_cast<const uint4 *>(state_b + (o - l.off_state));
        } else if (o < l.off_hist) {  // 8-byte elements: the middle section, then the path
            const bool mid = o < l.off_path;
            const long long e = (o - (mid ? l.off_mid : l.off_path)) >> 3, n = mid ? mid_elems : pv;
            const unsigned long long *src = mid ? mid_b : path_b;
            const unsigned long long lo = e < n ? src[e] : 0ULL, hi = e + 1 < n ? src[e + 1] : 0ULL;
            v = make_uint4((unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32));
        } else if (o < l.used) {
            v = *reinterpret_cast<const uint4 *>(hist_b + (o - l.off_hist));
        }
        *reinterpret_cast<uint4 *>(rec + o) = v;
    }
}

// The same grid the other way round.  Whether the slot takes the record is decided from the record's header and the
// length of the slot's range (its new one where the call gives ranges: the kernel then reads sel.len and never the table
// it writes), by every workgroup of the stream alike: nothing is handed from one workgroup to another.  A refused slot
// gets its reason and nothing else; otherwise thread 0 of slice 0 stores the history count, the range and status 0 beside
// the copy.  OTW: bytes of the slot behind the record's valid counts stay as they are, nothing reads them.
static __global__ void __launch_bounds__(kSnapThreads) snap_import_kernel(snap::SnapSel sel, SnapView a) {
    if ((int)blockIdx.y >= sel.n) return;
    const int b = sel.idx[blockIdx.y];
    const unsigned char *rec = a.blob + (long long)sel.rec[blockIdx.y] * a.rec_stride;
    const int32_t *hdr = reinterpret_cast<const int32_t *>(rec);
    const int Nb = sel.set_ref ? sel.len[blockIdx.y] : (a.ref_len ? a.ref_len[b] : a.len_default);
    const int status = snap::record_status(hdr, a.kind, a.param, Nb, a.hist_stride, a.path_cap, a.rec_stride);
    const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
    if (status != 0 || a.dry) {
        if (lead) a.status[sel.rec[blockIdx.y]] = status;
        return;
    }
    const int hv = hdr[snap::kWHistValid], pv = hdr[snap::kWPathValid], rp = hdr[snap::kWParam];
    const long long mid_elems = snap::mid_bytes(a.kind, rp) >> 3;
    const snap::Layout l = snap::record_layout(a.kind, rp, hv, pv);  // == the header's offsets (record_status)
    unsigned char *state_b = reinterpret_cast<unsigned char *>(a.state + (size_t)b * a.state_words);
    unsigned long long *mid_b = a.mid + (long long)b * a.mid_stride;
    unsigned long long *path_b = reinterpret_cast<unsigned long long *>(a.path) + (size_t)b * a.path_cap;
    unsigned char *hist_b =  // (an import that writes has its history: rts_otw_import allocates it first)
        a.hist ? reinterpret_cast<unsigned char *>(a.hist) + (long long)b * a.hist_stride * snap::kFrameBytes : nullptr;
    const long long end = a.zero_hist ? l.off_hist + (long long)a.hist_stride * snap::kFrameBytes : l.used;
    const long long step = 16LL * gridDim.x * blockDim.x;
    for (long long o = l.off_state + 16LL * (blockIdx.x * blockDim.x + threadIdx.x); o < end; o += step) {
        const uint4 v = o < l.used ? *reinterpret_cast<const uint4 *>(rec + o) : make_uint4(0u, 0u, 0u, 0u);
        if (o < l.off_mid) {
            *reinterpret_cast<uint4 *>(state_b + (o - l.off_state)) = v;
        } else if (o < l.off_hist) {
            const bool mid = o < l.off_path;
            const long long e = (o - (mid ? l.off_mid : l.off_path)) >> 3, n = mid ? mid_elems : pv;
            unsigned long long *dst = mid ? mid_b : path_b;
            if (e < n) dst[e] = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
            if (e + 1 < n) dst[e + 1] = (unsigned long long)v.z | ((unsigned long long)v.w << 32);
        } else {
            *reinterpret_cast<uint4 *>(hist_b + (o - l.off_hist)) = v;
        }
    }
    if (lead) {
        a.count[b] = hdr[snap::kWHistLen];
        if (a.count2) a.count2[b] = hdr[snap::kWHistLen];
        if (a.ticket) a.ticket[b] = 0;
        if (sel.set_ref) {
            a.ref_first[b] = sel.first[blockIdx.y];
            a.ref_len[b] = sel.len[blockIdx.y];
        }
        a.status[sel.rec[blockIdx.y]] = 0;
    }
    if (a.ctl && blockIdx.x == 0 && threadIdx.x < 8) a.ctl[(size_t)b * 8 + threadIdx.x] = 0;
}

static int snap_slices(long long rec_stride) {
    const long long s = (rec_stride + 32767) / 32768;
    return (int)(s < 1 ? 1 : (s > kSnapSlices ? kSnapSlices : s));
}

// What export and import check alike of the selection and the blob (`what`: "idx_host" / "slot_host").
static int snap_check_sel(int B, const int32_t *idx, int n, const char *what, const void *blob, long long rec_stride) {
    if (!idx) return set_error(RTS_ERR_INVALID, "%s is NULL", what);
    if (n < 0) return set_error(RTS_ERR_INVALID, "n must be >= 0 (got %d)", n);
    if (!blob) return set_error(RTS_ERR_INVALID, "blob_dev is NULL");
    if ((uintptr_t)blob & 15) return set_error(RTS_ERR_INVALID, "blob_dev must be 16-byte aligned");
    if (rec_stride < snap::kHeaderBytes || (rec_stride & 15) || rec_stride > snap::kMaxStride)
        return set_error(RTS_ERR_INVALID, "rec_stride must be a multiple of 16 in [%d, 2^31) (got %lld)", snap::kHeaderBytes, rec_stride);
    int dup = 0;
    if (const int i = snap::sel_check(B, idx, n, &dup); i >= 0)
        return dup ? set_error(RTS_ERR_INVALID, "%s[%d]: stream %d is selected twice", what, i, idx[i])
                   : set_error(RTS_ERR_INVALID, "%s[%d]: stream index %d out of range [0, %d)", what, i, idx[i], B);
    return RTS_OK;
}

static int snap_stride_check(long long need, long long rec_stride, const char *len_name, int len_max) {
    if (need > snap::kMaxStride)
        return set_error(RTS_ERR_UNSUPPORTED, "a record of %s = %d frames takes %lld bytes: snapshots hold less than 2^31", len_name, len_max, need);
    if (rec_stride >= 0 && rec_stride < need)
        return set_error(RTS_ERR_INVALID, "rec_stride %lld is below the %lld bytes a record of this handle can take", rec_stride, need);
    return RTS_OK;
}

// An import's desc and ranges against its handle (`mine`: what the handle's own export would say, n and rec_stride
// those of the call).  The ranges follow the rule of ref_ranges_check, for tables with one entry per selected slot.
static int snap_check_import(const rts_snapshot_desc &d, const rts_snapshot_desc &mine, const int32_t *slot_host,
                             const long long *first_host, const int32_t *len_host, const RefTable &refs, int len_max,
                             const char *len_name) {
    if (const char *f = snap::desc_mismatch(d, mine))
        return set_error(RTS_ERR_INVALID, "the snapshot does not fit this handle: desc field %s differs", f);
    if ((first_host == nullptr) != (len_host == nullptr))
        return set_error(RTS_ERR_INVALID, "first_host and len_host must both be given or both be NULL");
    if (!first_host) return RTS_OK;
    if (!refs.first)
        return set_error(RTS_ERR_INVALID, "new reference ranges need a handle with per-stream references (rts_*_create_refs)");
    for (int i = 0; i < mine.n; i++) {
        const long long f = first_host[i];
        const int len = len_host[i];
        if (len < 1 || f < 0 || f > refs.n_frames - len || len > len_max)
            return set_error(RTS_ERR_INVALID, "stream %d: frames [%lld, %lld) must be at least one frame inside the %lld "
                                              "reference frames and at most %s = %d long", slot_host[i], f, f + len,
                             refs.n_frames, len_name, len_max);
    }
    return RTS_OK;
}

static int snap_enqueue(bool import, const SnapView &v, const int32_t *idx, int n, const long long *first_host,
                        const int32_t *len_host, hipStream_t s) {
    snap::SnapSel sel;
    for (int pos = 0; snap::sel_next_chunk(n, idx, first_host, len_host, &pos, &sel) > 0;) {
        const dim3 grid(snap_slices(v.rec_stride), sel.n);
        if (import) hipLaunchKernelGGL(snap_import_kernel, grid, dim3(kSnapThreads), 0, s, sel, v);
        else hipLaunchKernelGGL(snap_export_kernel, grid, dim3(kSnapThreads), 0, s, sel, v);
        RTS_HIP(hipGetLastError());
    }
    return RTS_OK;
}

}  // namespace rts
