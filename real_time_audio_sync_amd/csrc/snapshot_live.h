// Snapshots of single streams of a live session (include/rtsync.h, rts_live_export / rts_live_import):
// the bound tracker's record in front, written and read through the tracker's own export and import, and the live tail
// at the end of the stride (csrc/snapshot_plan.h: pending samples with their count, the diff carry with its flag).
// Included by live.hip behind its handle.  Sessions with a resampler or with the gate on are refused by both calls: the
// resampler's tail and totals and the gate's queue, ordinals and counters are the follow-up.
#pragma once
#include <vector>

#include "snapshot_plan.h"

namespace rts {

constexpr int kLiveSnapThreads = 256;

// Grid (slices, sel.n), like live_append_kernel's kAppendSlices: the workgroups of a stream share its tail in 16-byte
// units; unit 0 is the four header words, then four samples to a unit (zeros behind the pending count), then the carry
// two pitch classes to a unit (zeros without one).  The sample rows of the handle ([B][cap] float32) start on a multiple
// of 4 bytes only, so samples move as floats on the handle's side.  Only reads the handle.
__global__ void __launch_bounds__(kLiveSnapThreads) live_export_kernel(snap::SnapSel sel, LiveArgs g, unsigned char *blob,
                                                                       long long rec_stride) {
    if ((int)blockIdx.y >= sel.n) return;
    const int b = sel.idx[blockIdx.y];
    const long long tail = snap::live_tail_bytes(g.cap), off_carry = tail - snap::kLiveCarryBytes;
    unsigned char *rec = blob + (long long)sel.rec[blockIdx.y] * rec_stride + (rec_stride - tail);
    int p = g.pending[b];
    p = p < 0 ? 0 : (p > g.cap ? g.cap : p);
    const int has = g.has_carry ? (g.has_carry[b] != 0) : 0;
    const float *buf = g.buf + (size_t)b * g.cap;
    const long long step = 16LL * gridDim.x * blockDim.x;
    for (long long o = 16LL * (blockIdx.x * blockDim.x + threadIdx.x); o < tail; o += step) {
        if (o < snap::kLiveTailHeader) {
            *reinterpret_cast<int4 *>(rec) = make_int4(p, has, snap::kLiveMagic, g.cap);
        } else if (o < off_carry) {
            const long long i = (o - snap::kLiveTailHeader) >> 2;
            float4 v;
            v.x = i < p ? buf[i] : 0.0f;
            v.y = i + 1 < p ? buf[i + 1] : 0.0f;
            v.z = i + 2 < p ? buf[i + 2] : 0.0f;
            v.w = i + 3 < p ? buf[i + 3] : 0.0f;
            *reinterpret_cast<float4 *>(rec + o) = v;
        } else {
            const int e = (int)((o - off_carry) >> 3);
            double2 v;
            v.x = has ? g.carry[(size_t)b * kLiveF + e] : 0.0;
            v.y = has ? g.carry[(size_t)b * kLiveF + e + 1] : 0.0;
            *reinterpret_cast<double2 *>(rec + o) = v;
        }
    }
}

// The same grid the other way round, behind the tracker's import on the same stream.  The count is clamped to the
// buffer (the host has held the mirror words against max_pending before anything was enqueued).  Thread 0 of slice 0
// stores the count and the carry flag and publishes like live_restart_kernel: status and position words from the
// imported tracker state, the per-stream words of `blocks` (bit k: PubBlock k of csrc/live_pub.h) empty until the next
// feed, the bound ensemble's strikes 0, the feed number untouched.
__global__ void __launch_bounds__(kLiveSnapThreads) live_import_kernel(snap::SnapSel sel, LiveArgs g, unsigned blocks,
                                                                       const unsigned char *blob, long long rec_stride) {
    if ((int)blockIdx.y >= sel.n) return;
    const int b = sel.idx[blockIdx.y];
    const long long tail = snap::live_tail_bytes(g.cap), off_carry = tail - snap::kLiveCarryBytes;
    const unsigned char *rec = blob + (long long)sel.rec[blockIdx.y] * rec_stride + (rec_stride - tail);
    const int4 hd = *reinterpret_cast<const int4 *>(rec);
    const int p = hd.x < 0 ? 0 : (hd.x > g.cap ? g.cap : hd.x);
    const int has = g.has_carry ? (hd.y != 0) : 0;
    float *buf = g.buf + (size_t)b * g.cap;
    const long long step = 16LL * gridDim.x * blockDim.x;
    for (long long o = snap::kLiveTailHeader + 16LL * (blockIdx.x * blockDim.x + threadIdx.x); o < tail; o += step) {
        if (o < off_carry) {
            const long long i = (o - snap::kLiveTailHeader) >> 2;
            if (i >= p) continue;
            const float4 v = *reinterpret_cast<const float4 *>(rec + o);
            buf[i] = v.x;
            if (i + 1 < p) buf[i + 1] = v.y;
            if (i + 2 < p) buf[i + 2] = v.z;
            if (i + 3 < p) buf[i + 3] = v.w;
        } else if (has) {
            const int e = (int)((o - off_carry) >> 3);
            const double2 v = *reinterpret_cast<const double2 *>(rec + o);
            g.carry[(size_t)b * kLiveF + e] = v.x;
            g.carry[(size_t)b * kLiveF + e + 1] = v.y;
        }
    }
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    g.pending[b] = p;
    if (g.has_carry) g.has_carry[b] = has;
    live_publish_status(g, b);
    if (g.ens_state) g.ens_state[b] = g.ens_state[g.B + b] = 0;
    live_clear_published(g.pubs, blocks, g.B, b);
    __threadfence_system();
}

static int live_snap_usable(const rts_live *h, const char *what) {
    if (int rc = live_usable(h); rc != RTS_OK) return rc;
    if (h->rs)
        return set_error(RTS_ERR_UNSUPPORTED, "%s: the session resamples its input, and a record does not carry the resampler's tail and totals", what);
    if (h->gate_on)
        return set_error(RTS_ERR_UNSUPPORTED, "%s: the level gate is on, and a record does not carry its queue and counters", what);
    if (h->acc_on)
        return set_error(RTS_ERR_UNSUPPORTED, "%s: the accompaniment is on, and a record does not carry a stream's clock, time map and renderer state", what);
    return check_device(h->device, "handle");
}

static int live_tracker_bytes(const rts_live *h, size_t *bytes) {
    return h->otw ? rts_otw_snapshot_bytes(h->otw, bytes) : rts_wtw_snapshot_bytes(h->wtw, bytes);
}

static int live_snap_slices(long long tail) {
    const long long s = (tail + 32767) / 32768;
    return (int)(s < 1 ? 1 : (s > 16 ? 16 : s));
}

// What the session's own export says, for n records rec_stride apart: the tracker's desc with the live fields on top.
static void live_snap_desc(const rts_live *h, const rts_snapshot_desc &tracker, rts_snapshot_desc *d) {
    *d = tracker;
    d->tracker = tracker.kind;
    d->kind = RTS_SNAPSHOT_LIVE;
    d->fft_len = h->geo.L;
    d->live_hop = h->geo.hop;
    d->feature_kind = h->geo.diff ? RTS_FEATURE_CHROMA_DIFF : RTS_FEATURE_CHROMA;
    d->max_pending = h->geo.cap;
}

}  // namespace rts

extern "C" {

int rts_live_snapshot_bytes(const rts_live *h, size_t *bytes) {
    using namespace rts;
    if (!h || !bytes) return set_error(RTS_ERR_INVALID, "NULL argument");
    size_t t = 0;
    if (int rc = live_tracker_bytes(h, &t); rc != RTS_OK) return rc;
    const long long need = snap::live_rec_stride((long long)t, h->geo.cap);
    if (need > snap::kMaxStride)
        return set_error(RTS_ERR_UNSUPPORTED, "a record of this session takes %lld bytes: snapshots hold less than 2^31", need);
    *bytes = (size_t)need;
    return RTS_OK;
}

int rts_live_export(rts_live *h, const int32_t *idx_host, int n, void *blob_dev, long long rec_stride,
                    rts_snapshot_desc *desc_out, int32_t *mirror_out, void *stream) {
    using namespace rts;
    if (int rc = live_snap_usable(h, "rts_live_export"); rc != RTS_OK) return rc;
    if (!desc_out || !mirror_out) return set_error(RTS_ERR_INVALID, "desc_out / mirror_out is NULL");
    size_t need = 0;
    if (int rc = rts_live_snapshot_bytes(h, &need); rc != RTS_OK) return rc;
    if (rec_stride < (long long)need)
        return set_error(RTS_ERR_INVALID, "rec_stride %lld is below the %zu bytes a record of this session can take", rec_stride, need);
    // the tracker makes every check of the selection and the blob before it enqueues anything, and writes zeros up to
    // rec_stride behind its record; the tail goes on top of them
    rts_snapshot_desc td;
    if (int rc = h->otw ? rts_otw_export(h->otw, idx_host, n, blob_dev, rec_stride, &td, stream)
                        : rts_wtw_export(h->wtw, idx_host, n, blob_dev, rec_stride, &td, stream);
        rc != RTS_OK)
        return rc;
    live_snap_desc(h, td, desc_out);
    const long long tail = snap::live_tail_bytes(h->geo.cap);
    snap::SnapSel sel;
    for (int pos = 0; snap::sel_next_chunk(n, idx_host, nullptr, nullptr, &pos, &sel) > 0;) {
        hipLaunchKernelGGL(live_export_kernel, dim3(live_snap_slices(tail), sel.n), dim3(kLiveSnapThreads), 0, (hipStream_t)stream, sel,
                           h->args, static_cast<unsigned char *>(blob_dev), rec_stride);
        RTS_HIP(hipGetLastError());
    }
    for (int i = 0; i < n; i++) {  // from the host mirror: what the device holds once everything submitted has run
        mirror_out[2 * i] = (int32_t)h->cur.pending[idx_host[i]];
        mirror_out[2 * i + 1] = h->geo.diff ? h->cur.has_carry[idx_host[i]] != 0 : 0;
    }
    return RTS_OK;
}

int rts_live_import(rts_live *h, const int32_t *slot_host, int n, const void *blob_dev, long long rec_stride,
                    const rts_snapshot_desc *desc, const int32_t *mirror_host, const long long *first_host,
                    const int32_t *len_host, int32_t *status_dev, void *stream) {
    using namespace rts;
    if (int rc = live_snap_usable(h, "rts_live_import"); rc != RTS_OK) return rc;
    if (!desc || !mirror_host || !status_dev) return set_error(RTS_ERR_INVALID, "desc / mirror_host / status_dev is NULL");
    if (n < 0) return set_error(RTS_ERR_INVALID, "n must be >= 0 (got %d)", n);
    // the live fields first, the tracker's own through its import below
    rts_snapshot_desc mine = *desc;
    {
        rts_snapshot_desc t = *desc;
        t.kind = h->otw ? RTS_SNAPSHOT_OTW : RTS_SNAPSHOT_WTW;
        live_snap_desc(h, t, &mine);
    }
    if (desc->kind != RTS_SNAPSHOT_LIVE) return set_error(RTS_ERR_INVALID, "the snapshot does not fit this handle: desc field kind differs");
    for (const char *f : {desc->fft_len != mine.fft_len ? "fft_len" : nullptr, desc->live_hop != mine.live_hop ? "live_hop" : nullptr,
                          desc->feature_kind != mine.feature_kind ? "feature_kind" : nullptr,
                          desc->max_pending != mine.max_pending ? "max_pending" : nullptr, desc->tracker != mine.tracker ? "tracker" : nullptr})
        if (f) return set_error(RTS_ERR_INVALID, "the snapshot does not fit this handle: desc field %s differs", f);
    if (rec_stride < snap::live_tail_bytes(h->geo.cap) + snap::kHeaderBytes)
        return set_error(RTS_ERR_INVALID, "rec_stride %lld holds no tracker record in front of the live tail", rec_stride);
    for (int i = 0; i < n; i++)
        if (mirror_host[2 * i] < 0 || mirror_host[2 * i] > h->geo.cap || (mirror_host[2 * i + 1] != 0 && mirror_host[2 * i + 1] != 1))
            return set_error(RTS_ERR_INVALID, "record %d: mirror words (%d, %d) are no pending count within max_pending = %d and carry flag", i,
                             mirror_host[2 * i], mirror_host[2 * i + 1], h->geo.cap);
    rts_snapshot_desc td = *desc;
    td.kind = desc->tracker;
    // ask first: every check of the tracker's import and the device's decision per record, nothing written but status_dev
    for (int dry = 1; dry >= 0; dry--) {
        if (int rc = h->otw ? otw_import_records(h->otw, slot_host, n, blob_dev, rec_stride, &td, first_host, len_host, status_dev, stream, dry)
                            : wtw_import_records(h->wtw, slot_host, n, blob_dev, rec_stride, &td, first_host, len_host, status_dev, stream, dry);
            rc != RTS_OK)
            return rc;
        if (!dry || n == 0) break;
        std::vector<int32_t> status((size_t)n);
        RTS_HIP(hipMemcpyAsync(status.data(), status_dev, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, (hipStream_t)stream));
        RTS_HIP(hipStreamSynchronize((hipStream_t)stream));
        for (int i = 0; i < n; i++)
            if (status[(size_t)i] != 0)
                return set_error(RTS_ERR_INVALID, "stream %d refused record %d (status %d): nothing was changed", slot_host[i], i, status[(size_t)i]);
    }
    const long long tail = snap::live_tail_bytes(h->geo.cap);
    // What a restart empties, but not the gate block: an import is refused while the gate is on (live_snap_usable), and a
    // gate that is off keeps its meter words with its queue and counters, which a record does not carry either.
    const unsigned blocks = kPubRestartBlocks & ~(1u << kPubGate);
    snap::SnapSel sel;
    for (int pos = 0; snap::sel_next_chunk(n, slot_host, nullptr, nullptr, &pos, &sel) > 0;) {
        hipLaunchKernelGGL(live_import_kernel, dim3(live_snap_slices(tail), sel.n), dim3(kLiveSnapThreads), 0, (hipStream_t)stream, sel,
                           h->args, blocks, static_cast<const unsigned char *>(blob_dev), rec_stride);
        if (hipGetLastError() != hipSuccess) {
            h->failed = 1;  // the tracker took the records, the session did not: the mirror no longer describes the device
            return set_error(RTS_ERR_HIP, "launch of live_import_kernel failed");
        }
    }
    live_mirror_import(h->geo, h->cur, n, slot_host, mirror_host);
    RTS_HIP(hipStreamSynchronize((hipStream_t)stream));
    return RTS_OK;
}

}  // extern "C"
