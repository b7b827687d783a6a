// Shared host-side helpers for librtsync.so (error reporting, HIP call checking).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include "../../include/rtsync.h"

namespace rts {

char *last_error_buf();  // thread-local, 512 bytes
int set_error(int code, const char *fmt, ...);

inline bool dtype_ok(int dtype) { return dtype == RTS_F32 || dtype == RTS_F64; }  // a floating-point dtype code of the ABI

// Streams of a tracker handle (rts_live_create checks that it binds one of its own size).  Library-internal.
__attribute__((visibility("hidden"))) int otw_batch(const rts_otw *h);
__attribute__((visibility("hidden"))) int wtw_batch(const rts_wtw *h);
// Frames per stream of a tracker's own history, 2 N_max / 2 M_max (rts_live_gate keeps one ordinal per history frame).
__attribute__((visibility("hidden"))) int otw_history(const rts_otw *h);
__attribute__((visibility("hidden"))) int wtw_history(const rts_wtw *h);

// A handle (`noun`: "handle", or "plan" for rts_chroma) belongs to the device that was current when it was created;
// driving it with another device current would launch against foreign buffers.
__attribute__((visibility("hidden"))) int check_device(int handle_device, const char *noun);

// Host memory the device writes and the host reads without a copy: `bytes` of mapped, coherent host memory in *host and the
// same block as the device sees it in *dev -- or, on failure, nothing allocated and both NULL.  Freed with hipHostFree(*host).
__attribute__((visibility("hidden"))) hipError_t mapped_alloc(size_t bytes, void **host, void **dev);

// The one rule for per-stream reference ranges (rts_*_create_refs, rts_*_restart): len >= 1, first >= 0, [first, first +
// len) inside the pool of n_ref_frames and, where `len_name` is given, len <= len_max (the handle's buffers were sized by
// it).  `mask_host` (may be NULL) restricts the check to the selected streams.  Returns the largest length seen, or
// RTS_ERR_INVALID (< 0) with the message naming the stream.
__attribute__((visibility("hidden"))) int ref_ranges_check(int B, const uint8_t *mask_host, const long long *first_host,
                                                           const int32_t *len_host, long long n_ref_frames, int len_max,
                                                           const char *len_name);

// Per-stream references of a tracker handle: [B] first frames and [B] lengths on the device (NULL on a single-reference
// handle) and the size of the pool they index.  The kernels receive the two pointers as they are.
struct RefTable {
    long long *first;
    int32_t *len;
    long long n_frames;
};
__attribute__((visibility("hidden"))) hipError_t ref_table_upload(RefTable *t, const long long *first_host,
                                                                  const int32_t *len_host, int B);
__attribute__((visibility("hidden"))) void ref_table_free(RefTable *t);

// rts_*_read_path: the n_path word of stream b's state (`state_len` words per stream, n_path in slot `n_path_slot`) into
// *n, then min(*n, path_cap, cap_pairs) pairs into `pairs` (may be NULL).
__attribute__((visibility("hidden"))) int read_path(const int32_t *state, int state_len, int n_path_slot,
                                                    const int32_t *path, int path_cap, int b, int B, int32_t *pairs,
                                                    int cap_pairs, int *n, hipStream_t s);

// rts_*_restart: how the selection reaches the device.  The selected stream indices and (optionally) their new
// reference ranges travel as BY-VALUE kernel arguments, kRestartChunk streams per launch: the launch copies them, so
// the caller's host tables are consumed when the call returns, nothing is allocated or pinned, no later restart can
// overwrite what an earlier one still has to read, and a captured graph replays the values it was captured with.
constexpr int kRestartChunk = 128;
struct RestartSel {
    int n;        // selected streams in this chunk
    int set_ref;  // first[] / len[] are given: the streams move to these ranges of the reference pool
    int32_t idx[kRestartChunk];
    int32_t len[kRestartChunk];
    long long first[kRestartChunk];
};
// The checks every rts_*_restart makes before anything is enqueued (`len_name`: "N_max" / "M_max", `len_max` its value;
// n_ref_frames < 0: the handle has no per-stream references).  RTS_OK, or RTS_ERR_INVALID with the message set.
__attribute__((visibility("hidden"))) int restart_check(int B, const uint8_t *mask_host, const long long *first_host,
                                                        const int32_t *len_host, long long n_ref_frames, int len_max,
                                                        const char *len_name);
// Fills `sel` with the next selected streams from *pos on (at most kRestartChunk) and advances *pos; returns sel->n.
__attribute__((visibility("hidden"))) int restart_next_chunk(int B, const uint8_t *mask_host, const long long *first_host,
                                                             const int32_t *len_host, int *pos, RestartSel *sel);

// A resampling plan as the live handle uses it (csrc/resample.hip).  resample_info: the ratio, the table's half length,
// T = ceil(2 half / L), the input samples a stream carries from feed to feed, and the device the plan lives on.
// resample_live_enqueue: one launch that resamples every stream's (tail [B][T], staged feed) into `out_stage`, a buffer
// laid out like a staging slot (int32 counts[B], int32 offs[B] = b * cap, float32 samples at samples_off), reading tail
// and totals ([B][2]: input samples taken, output samples made) of this feed and writing those of the next into
// `tail_next` / `tot_next`: the caller keeps two copies and alternates.  n_out_max: the most new output samples of a
// stream (from the host mirror), which sizes the grid.  resample_live_restart_enqueue zeroes both copies ([2][B][T],
// [2][B][2]) for the selected streams.
__attribute__((visibility("hidden"))) int resample_info(const rts_resample *p, int *L, int *M, int *half, int *T,
                                                        int *device);
__attribute__((visibility("hidden"))) int resample_live_enqueue(const rts_resample *p, const unsigned char *stage,
                                                                size_t samples_off, int sample_kind, int B, int cap,
                                                                unsigned char *out_stage, const float *tail,
                                                                const long long *tot, float *tail_next,
                                                                long long *tot_next, int n_out_max, hipStream_t s);
__attribute__((visibility("hidden"))) int resample_live_restart_enqueue(const rts_resample *p, const RestartSel &sel,
                                                                        int B, float *tail, long long *tot,
                                                                        hipStream_t s);

// The annotation tables as the live handle uses them (csrc/annot.hip).  annot_select_enqueue: piece and frame offset of the
// selected streams into two [B] device tables, the values travelling by value like a restart's selection.
// annot_live_enqueue: the one launch a feed adds with annotations on -- per stream the reference index of the last stored
// point of the tracker's path ([B][path_cap][2], its count in word st_n_path of the stream's state), offset by frame0 and
// looked up in the stream's piece, into three host-mapped tables (sticky: see include/rtsync.h, rts_live_annotate).
struct AnnotLive {
    const int32_t *state;  // the tracker's state words, state_len per stream
    int state_len, st_n_path;
    const int32_t *path;
    int path_cap;
    const int32_t *piece, *frame0;  // [B] device
    double *beat;                   // [B] host-mapped
    int32_t *label, *ref_frame;     // [B] host-mapped
    int B;
};
__attribute__((visibility("hidden"))) int annot_pieces(const rts_annot *a);
__attribute__((visibility("hidden"))) int annot_device(const rts_annot *a);
__attribute__((visibility("hidden"))) int annot_longest(const rts_annot *a);  // rows of the handle's longest table
__attribute__((visibility("hidden"))) int annot_select_enqueue(int B, const uint8_t *mask_host, const int32_t *piece_host,
                                                               const int32_t *frame0_host, int32_t *piece_dev,
                                                               int32_t *frame0_dev, hipStream_t s);
__attribute__((visibility("hidden"))) int annot_live_enqueue(const rts_annot *a, const AnnotLive &g, hipStream_t s);

// The tail kernel of csrc/tempo.hip as the trackers and the live handle launch it: the regression window over the last
// min(K, stored) points of every stream's own path (rts_otw_tempo in include/rtsync.h has the definition).  otw_tempo_view /
// wtw_tempo_view fill in what describes the handle -- state, path, and the reference lengths the limits x_limit = 2 N_b,
// y_limit = N_b come from -- and return the handle's longest reference; the caller adds K, ahead and the outputs.
// bpm != NULL (the live handle): beats per minute through the tables `annot` at frame0[b] + the last point's reference
// index in piece[b]; NaN where annot, piece or frame0 is NULL.  The stores end with a system-scope fence: the live handle's
// outputs are host-mapped.
struct AnnotTables;
struct TempoTail {
    const int32_t *state;  // the tracker's state words, state_len per stream
    int state_len, st_n_path;
    const int32_t *path;  // [B][path_cap][2]
    int path_cap;
    const int32_t *ref_len;  // [B] per-stream reference lengths, NULL: N for every stream
    int N;
    int K;
    double ahead;
    double *slope, *pos, *bpm;  // [B]; pos and bpm may be NULL
    int32_t *n_out;             // [B]
    const int32_t *piece, *frame0;  // [B] device, for bpm
    int B;
};
__attribute__((visibility("hidden"))) int otw_tempo_view(const rts_otw *h, TempoTail *t);
__attribute__((visibility("hidden"))) int wtw_tempo_view(const rts_wtw *h, TempoTail *t);
// The checks rts_otw_tempo / rts_wtw_tempo / rts_live_follow_tempo share: K, ahead and, with the handle's longest
// reference N_max, the overflow rule.  RTS_OK or the error, the message set.
__attribute__((visibility("hidden"))) int tempo_tail_check(int K, double ahead, int N_max);
__attribute__((visibility("hidden"))) int tempo_tail_enqueue(const TempoTail &t, const rts_annot *annot, hipStream_t s);
__attribute__((visibility("hidden"))) const AnnotTables *annot_tables(const rts_annot *a);

// The fusion kernel of csrc/ensemble.hip as rts_otw_consensus / rts_wtw_consensus and the live handle launch it: one
// fusion step (include/rtsync.h, rts_ensemble_create) over every group of `e`, the member beats taken from the tracker that
// `view` describes (otw_tempo_view / wtw_tempo_view: state, path, B) at frame0[b] + the last stored point's reference index
// in piece[b] of `annot`.  Advances e's strikes / out.  The stores end with a system-scope fence: the live handle's outputs
// are host-mapped.
struct EnsembleOut {
    double *consensus, *spread;  // [n_groups]
    int32_t *n_in, *n_valid;     // [n_groups]
    double *dev;                 // [B]
    int32_t *strikes, *out;      // [B]
};
__attribute__((visibility("hidden"))) int ensemble_batch(const rts_ensemble *e);
__attribute__((visibility("hidden"))) int ensemble_groups(const rts_ensemble *e);
__attribute__((visibility("hidden"))) int ensemble_device(const rts_ensemble *e);
// the handle's carried state on the device, strikes[B] then out[B] (live_restart_kernel clears the selected streams')
__attribute__((visibility("hidden"))) int32_t *ensemble_state(const rts_ensemble *e);
__attribute__((visibility("hidden"))) int ensemble_fuse_enqueue(rts_ensemble *e, const rts_annot *annot, const TempoTail &view,
                                                                const int32_t *piece, const int32_t *frame0,
                                                                const EnsembleOut &o, hipStream_t s);

// The live accompaniment as the live handle drives it (csrc/accomp.hip; include/rtsync.h, rts_live_accompany, has the law).
// accomp_check: every parameter refusal, and the geometry (the plan's hop, the chroma plan's `hop`) on success.
// accomp_create: the per-stream device state, the seventh host-mapped block and the ring of chunks, every stream disarmed.
// accomp_arm notes the masked streams, which the next accomp_enqueue arms in its feed's chain; accomp_off drops what was
// noted and has the next accomp_enqueue disarm every stream first.  accomp_enqueue: the steering launch and one
// rts_warp_run into slot feed_no % 4 of the ring, `view` as otw_tempo_view / wtw_tempo_view fill it, n_samples / pending the
// live handle's own [B] words between its append and its compaction.  accomp_look reads slot feed % 4 of both host-mapped
// blocks; accomp_map synchronises.
struct Accomp;
struct AccompGeom;
__attribute__((visibility("hidden"))) int accomp_check(const rts_accomp_params *q, const rts_warp *plan, int hop, int device,
                                                       AccompGeom *out);
__attribute__((visibility("hidden"))) bool accomp_same(const Accomp *a, const AccompGeom &p, const rts_warp *plan,
                                                       const void *tracks, int dtype);
__attribute__((visibility("hidden"))) int accomp_create(const AccompGeom &p, rts_warp *plan, const void *tracks, int dtype, int B,
                                                        int device, Accomp **out);
__attribute__((visibility("hidden"))) void accomp_destroy(Accomp *a);
__attribute__((visibility("hidden"))) int accomp_tracks_check(int B, const uint8_t *mask, const long long *first,
                                                              const long long *len, const long long *origin);
__attribute__((visibility("hidden"))) void accomp_arm(Accomp *a, const uint8_t *mask, const long long *first, const long long *len,
                                                      const long long *origin);
__attribute__((visibility("hidden"))) void accomp_off(Accomp *a);
__attribute__((visibility("hidden"))) int accomp_restart(Accomp *a, const RestartSel &sel, hipStream_t s);
__attribute__((visibility("hidden"))) int accomp_reset(Accomp *a, hipStream_t s);
__attribute__((visibility("hidden"))) int accomp_enqueue(Accomp *a, const TempoTail &view, const int32_t *n_samples,
                                                         const int32_t *pending, int feed_no, hipStream_t s);
__attribute__((visibility("hidden"))) void accomp_look(const Accomp *a, int feed, const float **chunk_host, long long *row_stride,
                                                       int32_t *blocks, long long *out_total, long long *in_pos, double *rate,
                                                       int32_t *status, int32_t *warp_status);
__attribute__((visibility("hidden"))) int accomp_map(const Accomp *a, int b, long long *anchors_host, int cap, int *n,
                                                     long long state[2], hipStream_t s);

// rts_otw_import / rts_wtw_import with `dry` != 0: every check is made and status_dev is written, nothing else -- neither
// on the device nor in the handle.  rts_live_import asks this way first, so that a refused record leaves the session as
// it was.  dry == 0 is the public call.
__attribute__((visibility("hidden"))) int otw_import_records(rts_otw *h, const int32_t *slot_host, int n, const void *blob_dev,
                                                             long long rec_stride, const rts_snapshot_desc *desc,
                                                             const long long *first_host, const int32_t *len_host,
                                                             int32_t *status_dev, void *stream, int dry);
__attribute__((visibility("hidden"))) int wtw_import_records(rts_wtw *h, const int32_t *slot_host, int n, const void *blob_dev,
                                                             long long rec_stride, const rts_snapshot_desc *desc,
                                                             const long long *first_host, const int32_t *len_host,
                                                             int32_t *status_dev, void *stream, int dry);

#define RTS_HIP(call)                                                                       \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return ::rts::set_error(RTS_ERR_HIP, "%s failed: %s (%s:%d)", #call,              \
                                    hipGetErrorString(e_), __FILE__, __LINE__);               \
    } while (0)

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains every outstanding global store
// (a full release fence), which costs a memory round trip per call in loops that stream results to HBM while the
// threads talk to each other through LDS alone.
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

}  // namespace rts
