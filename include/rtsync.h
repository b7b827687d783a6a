/*
 * rtsync.h -- C-ABI of librtsync.so: the MI355X (gfx950) implementation of the chroma + DTW /
 * online-time-warping / windowed-time-warping hot path of smritip/real-time-audio-sync.
 *
 * The reference has no FFI boundary of its own (it is plain in-process Python); each entry point
 * below names the reference interface it replaces (file:line under /root/reference).  The Python
 * classes in real_time_audio_sync_amd/ bind these symbols with ctypes and keep the reference's
 * call surface (INTEGRATION.md shows the binding a maintainer would add).
 *
 * Conventions
 *   - All `*_dev` pointers are device (HIP) pointers on the current device; the library never
 *     frees or reallocates caller memory.  `stream` is a hipStream_t passed as void* (NULL =
 *     the default stream).  Calls taking a stream are asynchronous on it; `*_read_*` getters
 *     synchronise that stream and copy to host memory.
 *   - Feature matrices are FRAME-MAJOR: [frame][feature], feature stride 1 (the reference's
 *     numpy arrays are feature-major (12, N); the Python layer transposes once at upload).
 *   - Return value: 0 = ok, < 0 = error (message via rts_last_error(), thread-local).
 *   - One handle must not be driven from two host threads at once.
 *   - There is no CPU fallback anywhere behind this header.
 */
#ifndef RTSYNC_H
#define RTSYNC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTS_OK 0
#define RTS_ERR_INVALID (-1)     /* bad argument (message says which) */
#define RTS_ERR_UNSUPPORTED (-2) /* valid in the reference, not supported by this build (e.g. c too large) */
#define RTS_ERR_HIP (-3)         /* a HIP runtime call failed */
#define RTS_ERR_NO_DEVICE (-4)   /* no gfx950 device visible */

/* dtype of feature / sample buffers handed to the library */
#define RTS_F32 0
#define RTS_F64 1
#define RTS_I16 2 /* PCM16 samples, rts_live_* only: value / 32768 in float32, exactly what librosa.load returns for a WAV */

/* which reference class an OTW handle follows */
#define RTS_VARIANT_OTW 0         /* otw_eran.py:5   OnlineTimeWarping (sentinel 1e10, run_count starts 1) */
#define RTS_VARIANT_LIVENOTE 1    /* livenote.py:3   LiveNote          (sentinel inf,  run_count starts 0) */
#define RTS_VARIANT_LIVENOTE_V2 2 /* livenote_v2.py:3 LiveNoteV2       (+ forward-only path filter)       */

#define RTS_COST_DOT 0    /* 1 - <live, ref>            otw_eran.py:220, livenote_v2.py:170 */
#define RTS_COST_EUCLID 1 /* ||live - ref||_2           livenote_v2.py:168 (chroma_diff=True) */

/* direction / previous codes in the state vector */
#define RTS_DIR_NONE (-1)
#define RTS_DIR_BOTH 0
#define RTS_DIR_ROW 1
#define RTS_DIR_COLUMN 2

/* per-stream status (replaces insert()'s return value) */
#define RTS_RUNNING 0
#define RTS_STOP_REF_END 1  /* insert() returned "stop": otw_eran.py:69-71, livenote_v2.py:80-82 */
#define RTS_LIVE_OVERFLOW 2 /* "ran out of room in pre-allocated live-sequence": otw_eran.py:53-55 */
#define RTS_DEVICE_FAULT 3  /* an in-launch hand-off between workgroups ran into its bound (never expected) */

/* how rts_otw_run walks the live sequence */
#define RTS_MODE_INSERT_LOOP 0 /* for i: insert(live[:, i])  (tests.py:160-163, test_simple.py:122-125) */
#define RTS_MODE_SET_LIVE 1    /* set_live(live)             (otw_eran.py:91-142, livenote_v2.py:108-155) */

/* layout of the int32 state vector returned by rts_otw_read_state (RTS_STATE_LEN entries) */
#define RTS_STATE_LEN 16
#define RTS_ST_T 0            /* t / live_ptr */
#define RTS_ST_J 1            /* j / ref_ptr */
#define RTS_ST_DIRECTION 2
#define RTS_ST_PREVIOUS 3
#define RTS_ST_RUN_COUNT 4
#define RTS_ST_STATUS 5
#define RTS_ST_FIRST_INSERT 6
#define RTS_ST_N_PATH 7       /* path points recorded */
#define RTS_ST_CONSUMED 8     /* live frames consumed (inserts made, incl. the one that stopped) */
#define RTS_ST_ROW_STRIPS 9
#define RTS_ST_COL_STRIPS 10
#define RTS_ST_CELLS_LO 11    /* cells evaluated, low/high 32 bits */
#define RTS_ST_CELLS_HI 12
#define RTS_ST_PATH_TRUNCATED 13
#define RTS_ST_BAND_RECOMPUTES 15 /* times a band minimum left the window and was recomputed (diagnostic) */

const char *rts_last_error(void);
int rts_version(void);
/* Number of visible HIP devices that are gfx950; < 0 on HIP failure. */
int rts_device_count(void);

/* ------------------------------------------------------------------------------------------
 * Online time warping, batched over B independent live streams against one reference (or one each).
 * ------------------------------------------------------------------------------------------ */
typedef struct rts_otw rts_otw;

/* Replaces OnlineTimeWarping.__init__ (otw_eran.py:6-36) / LiveNote.__init__ (livenote.py:5-35) /
 * LiveNoteV2.__init__ (livenote_v2.py:8-40) for B streams at once.  `ref_dev` ([N][F], dtype
 * `ref_dtype`) is held by reference like otw_eran.py:17 and must outlive the handle.  Instead of the
 * reference's dense (2N x N) cost/acc matrices the handle keeps two (c+1)-cell bands per stream.
 * F must be 12.  Supported band widths: 1 <= c <= 2036 (LDS windows of 512 cells up to c = 500, 1024 up to 1012, 2048
 * above).  Above c = 500 no frame ring fits in LDS beside the bands: the default pipelined kernel and the dense mirror
 * (rts_otw_set_dense / rts_otw_replay_dense: the plain 8-wave kernel) read every frame from global memory, live buffers
 * must be 16-byte aligned, and RTS_OTW_SPEC=0 (the plain kernel without the dense mirror: an A/B knob) returns
 * RTS_ERR_UNSUPPORTED with a message. */
int rts_otw_create(const void *ref_dev, int ref_dtype, int F, int N, int B, int c, int max_run_count,
                   int variant, int cost_kind, rts_otw **out);
/* The same for B streams that each follow their own reference (one piece per microphone): stream b behaves exactly like
 * stream 0 of an rts_otw_create handle made with ref_dev = frames [first_host[b], first_host[b] + len_host[b]) of
 * `refs_dev` ([n_ref_frames][F] frame-major, dtype `ref_dtype`, held by reference) and N = len_host[b]; every limit the
 * reference derives from N (live capacity 2N_b, the stop at j + 1 >= N_b) is the stream's own.  The host tables are
 * copied at create; ranges may overlap or repeat.  Buffers are sized by the longest reference N_max (path capacity
 * 3 N_max + 8, insert history [B][2 N_max][F]); every getter is unchanged.  RTS_ERR_INVALID for a NULL pointer, len < 1,
 * first < 0 or a range past n_ref_frames (the message names the stream); the rules of rts_otw_create apply otherwise.
 * The dense mirror (rts_otw_set_dense, rts_otw_replay_dense) returns RTS_ERR_UNSUPPORTED on such a handle.
 * N_max is the longest range given here and never grows: to reserve room for a longer piece that rts_otw_restart
 * may move a stream on to later, create one stream on that piece and restart it onto its own range right away. */
int rts_otw_create_refs(const void *refs_dev, int ref_dtype, int F, long long n_ref_frames,
                        const long long *first_host, const int32_t *len_host, int B, int c, int max_run_count,
                        int variant, int cost_kind, rts_otw **out);
int rts_otw_destroy(rts_otw *h);
/* Back to the freshly-constructed state (all streams). */
int rts_otw_reset(rts_otw *h, void *stream);

/* Restart single streams while the others keep running: what constructing a new OnlineTimeWarping / LiveNote /
 * LiveNoteV2 object (otw_eran.py:6-36, livenote.py:5-35, livenote_v2.py:8-40) for that one microphone is in the
 * reference.  `mask_host`: uint8[B] in HOST memory; streams with a non-zero entry are selected.  From here on a selected
 * stream behaves exactly like stream 0 of a handle freshly created for it alone (same c, max_run_count, variant, cost
 * kind): state as after create, RTS_RUNNING, empty path and insert history, counters at zero, bands NaN until its first
 * frame; with a dense mirror attached its [2N][N] slices read sentinel / -1 again (otw_eran.py:23,27).  Nothing an
 * unselected stream owns is written.
 *   first_host / len_host both NULL: the selected streams keep their reference.  Both given (allowed only on an
 * rts_otw_create_refs handle): int64[B] / int32[B] host tables, read for selected streams only; stream b then follows
 * frames [first_host[b], first_host[b] + len_host[b]) of the pool given at create, path indices relative to that range
 * (a range that starts inside a piece is "follow from bar 50").  Checks as in rts_otw_create_refs, plus len_host[b] <=
 * N_max of the handle, whose buffers were sized by it.
 *   Asynchronous on `stream`, in stream order; no synchronisation and no allocation.  Mask and ranges travel as
 * by-value kernel arguments, so the host tables may be freed as soon as the call returns and the call can be captured
 * into a graph (a replay restarts the same streams onto the same ranges).  After an rts_otw_run a restart is allowed;
 * frames a restarted stream then receives through rts_otw_insert / rts_otw_push put the handle in the state in which
 * rts_otw_replay_dense answers RTS_ERR_UNSUPPORTED; until then (a restart after rts_otw_run and no frame since)
 * rts_otw_replay_dense still replays that whole run for every stream, the restarted ones included, because the buffers
 * it is handed are that run's.  After insert / push only, rts_otw_replay_dense shows for a
 * restarted stream the matrices of what it consumed since its restart.
 *   RTS_ERR_INVALID, with nothing enqueued and nothing changed: NULL handle or mask, only one of first_host /
 * len_host, ranges on a handle without per-stream references, len < 1, first < 0, a range past the pool, len > N_max
 * (the message names the stream), wrong current device.  An all-zero mask is RTS_OK and does nothing. */
int rts_otw_restart(rts_otw *h, const uint8_t *mask_host, const long long *first_host, const int32_t *len_host,
                    void *stream);

/* Whole live sequences, one launch.  `live_dev`: [B][T_max][F] (dtype `live_dtype`, frame-major);
 * `live_len_dev`: int32[B] valid frames per stream (<= T_max).  Resets the handle, then behaves like
 * the harness loop `for i in range(T): if ln.insert(live[:, i]) == "stop": break`
 * (RTS_MODE_INSERT_LOOP) or like `ln.set_live(live)` (RTS_MODE_SET_LIVE).  The live buffer is read
 * in place and must stay valid until the stream has finished. */
int rts_otw_run(rts_otw *h, const void *live_dev, int live_dtype, int T_max, const int32_t *live_len_dev,
                int mode, void *stream);

/* One new frame per stream: replaces insert(live_sample) (otw_eran.py:38-85, livenote_v2.py:43-104).
 * `frames_dev`: [B][F].  `active_dev`: optional uint8[B]; streams with 0 receive no frame (NULL = all).
 * Frames are appended to a handle-owned history of 2N frames per stream (the reference's
 * pre-allocated self.live, otw_eran.py:14,20). */
int rts_otw_insert(rts_otw *h, const void *frames_dev, int frames_dtype, const uint8_t *active_dev,
                   void *stream);

/* Several new frames per stream in one call: the loop `while len(data) >= 4096: ... ln.insert(col);
 * data = data[2048:]` of livenote_live.py:185-208 when a microphone buffer yields more than one hop.
 * `frames_dev`: [B][n_max][F]; `n_new_dev`: int32[B] frames to take per stream (NULL = n_max for all). */
int rts_otw_push(rts_otw *h, const void *frames_dev, int frames_dtype, int n_max, const int32_t *n_new_dev,
                 void *stream);

/* The tail of the tracker's own history: what a stream last heard, as the (queries_dev, q_len_dev) pair rts_locate takes.
 * The reference has nothing comparable (its self.live, otw_eran.py:14,20, is never read back as an excerpt).  Stream b has
 * consumed n frames through rts_otw_insert / rts_otw_push since create, reset or its last restart, n capped at the
 * history capacity of its own range, 2 N_b (the count runs past it on RTS_LIVE_OVERFLOW).  len_dev[b] = min(M_max, n);
 * out_dev[b][0 .. len) are frames n - len .. n - 1 in order, as float64 whatever dtype they were pushed in; rows
 * [len, M_max) are written as zeros.  `mask_dev`: optional uint8[B] DEVICE array, a stream with a zero entry gets len 0 and
 * all-zero rows (rts_locate then spends nothing on it: its kernel leaves on M < 1); NULL = all streams.
 *   out_dev double [B][M_max][12], len_dev int32 [B].  A fresh handle, whose history is not allocated yet, gives len 0
 * everywhere.  The handle is only read.  Asynchronous on `stream`; no allocation, no synchronisation (graph-capturable).
 *   RTS_ERR_INVALID, naming the argument: NULL handle, out_dev or len_dev, M_max < 1.  RTS_ERR_UNSUPPORTED: M_max > 256 (the
 * bound of rts_locate), and a handle that has consumed an rts_otw_run since its last reset -- those frames are the
 * caller's memory, not the handle's. */
int rts_otw_recent(rts_otw *h, int M_max, double *out_dev /* [B][M_max][12] */, int32_t *len_dev /* [B] */,
                   const uint8_t *mask_dev /* optional uint8[B], DEVICE */, void *stream);

/* Tracking confidence: the handle's own cell cost along the path it recorded.  The reference has nothing comparable (it
 * plots acc_cost after the fact, livenote_v2.ipynb).  Stream b has stored path points (t_i, j_i) -- min(n_path, path
 * capacity) of them once RTS_ST_PATH_TRUNCATED is set; n = min(K, stored) and the last n points count, in recording order.
 * costs_dev[b][k] is the cost between history frame t and frame j of the stream's current reference range (pool frame
 * first_b + j on an rts_otw_create_refs handle, also after a restart onto an offset range), bit for bit what the tracker
 * computes: RTS_COST_DOT 1 - <live, ref> in the strided-dot order of otw_eran.py:220, RTS_COST_EUCLID the norm of
 * livenote_v2.py:168, a float32 reference widened as the tracker widens it.  costs_dev[b][n .. K) are NaN.
 * mean_dev[b] is the sequential float64 sum of the n costs, oldest first, divided by (double)n -- NaN for n = 0 -- and
 * n_dev[b] = n.  A NaN cost (a silent column normalises to NaN) stays NaN and makes that stream's mean NaN, nothing else.
 * The mean is in the unit of rts_locate's cost / (M + end - start + 1).
 *   mean_dev double [B], n_dev int32 [B], costs_dev optional double [B][K].  1 <= K <= 256.  The handle is only read.
 * Asynchronous on `stream`; no allocation, no synchronisation (graph-capturable).
 *   RTS_ERR_INVALID, naming the argument: NULL handle, mean_dev or n_dev, K outside [1, 256].  RTS_ERR_UNSUPPORTED after an
 * rts_otw_run, as for rts_otw_recent.
 *   There is no WTW counterpart: its cosine cost is NaN on silent frames, and its windows re-decide the path. */
int rts_otw_path_cost(rts_otw *h, int K, double *mean_dev /* [B] */, int32_t *n_dev /* [B] */,
                      double *costs_dev /* optional [B][K] */, void *stream);

/* Getters (synchronise `stream`). */
int rts_otw_read_state(rts_otw *h, int b, int32_t *state /* RTS_STATE_LEN */, void *stream);
int rts_otw_read_states(rts_otw *h, int32_t *states /* [B][RTS_STATE_LEN] */, void *stream);
/* .path: (live_idx, ref_idx) int32 pairs in recording order.  `cap_pairs` = capacity of `pairs`;
 * *n receives the full length (copy is truncated to cap_pairs). */
int rts_otw_read_path(rts_otw *h, int b, int32_t *pairs, int cap_pairs, int *n, void *stream);
/* The live part of .acc_cost: row t over columns [j-c, j] and column j over rows [t-c, t]
 * (c+1 doubles each, index i <-> offset i-c; NaN where the index is negative, and everywhere for a stream that has
 * not consumed a frame since create / rts_otw_restart; rts_otw_reset and rts_otw_run leave the bands of such a stream as
 * they were). */
int rts_otw_read_bands(rts_otw *h, int b, double *row_band, double *col_band, void *stream);
/* Which streams had their band filled by the dense wavefront kernel in the handle's last rts_otw_run / rts_otw_insert /
 * rts_otw_push: took[b] = 1 if stream b was fresh and that call brought it at least c frames (c <= 500, reference of at
 * least c frames, no dense mirror; set_live: more than c frames), so that otw_bandfill_kernel evaluated the square
 * [0, c-1] x [0, c-1] in front of the step loop; 0 where the step loop ran alone.  Results do not depend on it: the
 * environment variable RTS_OTW_FILL=0, read by rts_otw_create, leaves every stream to the step loop (A/B measurements,
 * tests).  `took`: host int32 [B]. */
int rts_otw_read_fill(rts_otw *h, int32_t *took /* [B] */, void *stream);
/* Device-side views for zero-copy consumers (torch): path buffer [B][path_cap][2] int32 and state
 * [B][RTS_STATE_LEN] int32. */
int rts_otw_device_views(rts_otw *h, int32_t **path_dev, int *path_cap, int32_t **state_dev);
/* Optional mirror of the reference's dense matrices (otw_eran.py:23,27; plotted by livenote_v2.ipynb):
 * acc_dev / cost_dev are caller-owned double [B][2N][N] buffers that every evaluated cell is also
 * written to (never-evaluated cells hold the sentinel 1e10 / +inf, resp. -1).  NULL, NULL switches it
 * off.  Resets the handle (the matrices are re-initialised on every reset / run). */
int rts_otw_set_dense(rts_otw *h, double *acc_dev, double *cost_dev, void *stream);
/* The same matrices on demand, without slowing the tracker down: recomputes them, from everything the handle has
 * consumed since its last reset, into caller-owned double [B][2N][N] buffers.  Frames that came through rts_otw_insert /
 * rts_otw_push are kept by the handle: pass live_dev = NULL (live_dtype, T_max, live_len_dev ignored).  Frames of an
 * rts_otw_run are the caller's memory and the library keeps no pointer to them: pass that call's live_dev, live_dtype,
 * T_max and live_len_dev again (dtype and T_max are checked against the run being replayed).  The handle's own state is
 * not touched, so the streams keep running on the pipelined kernel.  Every supported band width.  Synchronises `stream`.
 * Every argument is checked before anything is enqueued, as in rts_otw_backward, whose source rules these are: a refused
 * call (live_dev must also be 16-byte aligned) leaves acc_dev / cost_dev untouched.
 * What the drop-in classes' .acc_cost / .cost
 * (otw_eran.py:23,27) are made of. */
int rts_otw_replay_dense(rts_otw *h, const void *live_dev, int live_dtype, int T_max, const int32_t *live_len_dev,
                         double *acc_dev, double *cost_dev, void *stream);
/* The backward path (Dixon's MATCH): from a stream's current best point back to (0, 0) over the
 * accumulated-cost cells the tracker has evaluated -- a monotone, gap-free warping path, optimal inside the explored
 * band, where .path is causal and may jump.  Defined on the reference's dense matrices acc / cost (otw_eran.py:23,27):
 *   end cell: best_point (otw_eran.py:192-211) at the end position (t, j), t clamped to the last row consumed and j to
 *     N - 1 (a stop or an overflow leaves one index one past the end);
 *   predecessor of (x, y) != (0, 0), d = cost[x][y]: the first of (x, y-1) with acc + d, (x-1, y) with acc + d and
 *     (x-1, y-1) with acc + 2 d, in-range candidates only, whose sum == acc[x][y];
 *   path: the predecessors from the end cell down to (0, 0), in forward order; total = acc[end].
 * The matrices are never built: the call replays what the handle has consumed (the source rules of rts_otw_replay_dense:
 * live_dev = NULL after rts_otw_insert / rts_otw_push or on a fresh handle, that call's buffers again after rts_otw_run,
 * RTS_ERR_UNSUPPORTED for the mixed state; a restarted stream shows what it consumed since its restart) on scratch state
 * into a per-strip log in the caller's workspace, 8 bytes per evaluated cell, and walks the log on the device.  Works on
 * rts_otw_create_refs handles: each stream uses its own range and N_b, indices are relative to the range.  Every
 * supported band width; not affected by RTS_OTW_SPEC.  The handle's state, path, bands and history are only read.
 *   path_dev [B][3 N_max + 8][2] (8-byte aligned): stream b gets path_len_dev[b] rows from (0, 0) to end_dev[b]; rows
 *     behind them are left untouched.  total_dev[b] = acc[end] bit for bit.  acc_dev: optional [B][3 N_max + 8], acc at
 *     every path point.  A stream that has consumed no frame: path_len 0, total NaN, end (-1, -1).
 *   ws_dev / ws_bytes: caller-owned, 16-byte aligned scratch of at least rts_otw_backward_workspace_bytes(N_max, c, B)
 *     (pure host arithmetic, linear in N_max: at most B (3 N_max + 8) (8 (c + 1) + 16) bytes plus a fixed header).
 * Features must be finite: a NaN frame makes that stream's result unspecified (path_len stays within [0, 3 N_max + 8],
 * nothing is read or written out of bounds).  Asynchronous on `stream`; the first call on a handle allocates its scratch
 * state, later calls neither allocate nor synchronise.  Every argument is checked before anything is enqueued. */
int rts_otw_backward_workspace_bytes(int N_max, int c, int B, size_t *bytes);
int rts_otw_backward(rts_otw *h, const void *live_dev, int live_dtype, int T_max, const int32_t *live_len_dev,
                     int32_t *path_dev /* [B][3 N_max + 8][2] */, int32_t *path_len_dev /* [B] */,
                     double *total_dev /* [B] */, int32_t *end_dev /* [B][2] */,
                     double *acc_dev /* optional [B][3 N_max + 8] */, void *ws_dev, size_t ws_bytes, void *stream);
/* Device time of the handle's last rts_otw_backward, split into its two parts (HIP events the call records on its
 * stream): the trace replay and the backtrace.  Waits for that call to finish. */
int rts_otw_backward_times(rts_otw *h, float *replay_ms, float *backtrace_ms);
/* Formerly a tuning knob (waves per stream workgroup); the library now chooses the count itself (8 everywhere but for
 * the wide forms, rts_otw_read_kernel_waves).  8 is accepted and changes
 * nothing, the retired counts 1, 2 and 4 return RTS_ERR_UNSUPPORTED, anything else RTS_ERR_INVALID.
 * Without a dense mirror the library runs its pipelined kernel (the next step's strips are computed
 * beside this step's control work); the environment variable RTS_OTW_SPEC=0, read by rts_otw_create, selects
 * the plain kernel instead (A/B measurements, tests). */
int rts_otw_set_waves(rts_otw *h, int waves);
/* Average device time of the last kernel launches is measured by the caller with HIP events on
 * `stream`; this returns the kernel's name as it appears in rocprofv3 traces. */
const char *rts_otw_kernel_name(const rts_otw *h);
/* Which instantiation of that kernel a launch of this handle gets: chosen at create from the band width, RTS_OTW_SPEC,
 * the feature dtypes and the batch size relative to the device's compute units.  `live_dtype`: the dtype
 * of the live input of the launch asked about -- rts_otw_run's own; RTS_F64 for rts_otw_insert, rts_otw_push and every
 * rts_live_* session, whose frames are read from the handle's float64 history.
 *   out[0]: the LDS window in cells (64 ... 2048);  out[1]: where the kernel keeps the frames it reads more than once,
 *   RTS_OTW_RING_*;  out[2]: 1 the pipelined kernel, 0 the plain one (RTS_OTW_SPEC=0, or a dense mirror is attached);
 *   out[3]: 1 if a launch that can bring a fresh stream at least c frames runs otw_bandfill_kernel first (rts_otw_read_fill
 *   says which streams then took it), 0 if every launch runs the step loop alone.
 * Host-side only: no GPU call, nothing is enqueued or synchronised.  RTS_ERR_INVALID: NULL argument, bad live_dtype.
 * RTS_ERR_UNSUPPORTED where the launch itself is refused (RTS_OTW_SPEC=0 at c > 500 without a dense mirror). */
#define RTS_OTW_RING_FLOAT 0     /* float32 frames in an LDS ring */
#define RTS_OTW_RING_DOUBLE 1    /* float64 frames in an LDS ring */
#define RTS_OTW_RING_NONE 2      /* no ring: frames come from global memory */
#define RTS_OTW_RING_NONE_LEAN 3 /* the same, the residency-oriented flavour of batches of RTS_OTW_TP_FROM streams per CU */
int rts_otw_read_kernel(const rts_otw *h, int live_dtype, int32_t out[4]);
/* The waves per stream of that instantiation: 8, or 12 / 16 for the wide forms of the pipelined kernel with a ring at band
 * widths 245..500, which a handle takes when every stream has a compute unit to itself (B <= CUs) and which
 * spend the further waves on the cost strips.  Results do not depend on it.  The environment variable RTS_OTW_WAVES=8, 12
 * or 16, read by rts_otw_create, fixes the count wherever the kernel has such a form (A/B measurements, tests); any other
 * value makes rts_otw_create return RTS_ERR_INVALID.  Same arguments, same errors as rts_otw_read_kernel, whose four
 * words stay as they are. */
int rts_otw_read_kernel_waves(const rts_otw *h, int live_dtype, int32_t *waves);

/* ------------------------------------------------------------------------------------------
 * Snapshots: single streams move from one handle to another.
 * ------------------------------------------------------------------------------------------ */

/* What an export knows on the host about the records it wrote, filled synchronously from the exporting handle's own
 * parameters (nothing is read back), and what an import holds against its target before anything is enqueued.  Fields
 * of another kind than `kind` are 0; a live session's desc (RTS_SNAPSHOT_LIVE) carries the fields of its bound tracker
 * too and names it in `tracker`. */
#define RTS_SNAPSHOT_VERSION 1
#define RTS_SNAPSHOT_OTW 1
#define RTS_SNAPSHOT_WTW 2
#define RTS_SNAPSHOT_LIVE 3
typedef struct rts_snapshot_desc {
    int32_t kind, version;  /* RTS_SNAPSHOT_*, RTS_SNAPSHOT_VERSION */
    int32_t n;              /* records in the blob */
    int32_t ref_dtype;      /* RTS_F32 / RTS_F64 of the exporting handle's reference: the cost of a cell depends on it */
    long long rec_stride;   /* bytes from one record to the next */
    int32_t F, c, max_run_count, variant, cost_kind;        /* RTS_SNAPSHOT_OTW */
    int32_t window, hop, keep_last_d;                       /* RTS_SNAPSHOT_WTW */
    int32_t fft_len, live_hop, feature_kind, max_pending;   /* RTS_SNAPSHOT_LIVE */
    int32_t tracker;        /* RTS_SNAPSHOT_LIVE: RTS_SNAPSHOT_OTW / _WTW of the bound tracker, whose fields are filled too; else 0 */
} rts_snapshot_desc;

/* Why the device refused a record (status_dev of rts_otw_import); 0 = imported. */
#define RTS_SNAP_BAD_MAGIC 1   /* not a record (or not written yet) */
#define RTS_SNAP_BAD_VERSION 2
#define RTS_SNAP_BAD_KIND 3
#define RTS_SNAP_BAD_RANGE 4   /* the record's N_b differs from the length of the slot's reference range */
#define RTS_SNAP_BAD_HISTORY 5 /* more history frames than the slot's buffer holds */
#define RTS_SNAP_BAD_PATH 6    /* more path pairs than the slot's buffer holds, or a path the exporter had truncated */
#define RTS_SNAP_BAD_LAYOUT 7  /* counts, section offsets, band width / window or used_bytes disagree with each other or with rec_stride */

/* Bytes a record of this handle can take: the stride rts_otw_export needs (a multiple of 16).  A record is
 *   64 bytes of int32 header words (magic, version, kind, N_b, M_b = 0, valid history frames, valid path pairs, the raw
 *     history count, c, the byte offsets of the four sections, used_bytes, the n_path word, one zero word),
 *   the 16 state words, the two persisted bands (2 (c + 1) doubles), the path pairs and the history frames (96 bytes each),
 * every section starting on a multiple of 16 bytes, packed by the VALID counts: used_bytes is a function of (c, history
 * frames, path pairs) alone, and the stride is used_bytes at 2 N_max frames and 3 N_max + 8 pairs.  RTS_ERR_UNSUPPORTED
 * where that reaches 2^31 bytes. */
int rts_otw_snapshot_bytes(const rts_otw *h, size_t *bytes);

/* Writes one self-contained record per selected stream into caller-owned device memory: record i, at blob_dev +
 * i * rec_stride, is stream idx_host[i].  A record is a function of the stream's state alone: it holds no slot index and
 * no pointer, and every byte behind used_bytes up to rec_stride is written as zero, so two exports of an unchanged
 * stream give the same rec_stride bytes whatever the blob held before.  Carried is exactly what rts_otw_restart resets
 * (state words, persisted bands, path, insert history and its count, the length of the reference range); everything
 * else is rebuilt by every launch.  The reference has nothing comparable (its objects live and die with the process).
 *   idx_host: int32[n] in HOST memory, consumed when the call returns (the selection travels by value, 128 streams per
 * launch, like a restart's).  blob_dev: 16-byte aligned, n * rec_stride bytes; rec_stride a multiple of 16 and at least
 * rts_otw_snapshot_bytes.  desc_out: filled on the host from the handle's parameters.  The handle is only read.
 * Asynchronous on `stream`, in stream order; no allocation, no synchronisation (graph-capturable).
 *   RTS_ERR_INVALID, naming the argument, with nothing enqueued: NULL handle, idx_host, blob_dev or desc_out, n < 0, an
 * index outside [0, B), a repeated index, a misaligned blob, a stride too small or no multiple of 16, wrong current
 * device.  RTS_ERR_UNSUPPORTED: a handle that has consumed an rts_otw_run since its last reset (those frames are the
 * caller's memory, as for rts_otw_recent), and a handle with the dense mirror attached.  n = 0 is RTS_OK. */
int rts_otw_export(rts_otw *h, const int32_t *idx_host /* [n] */, int n, void *blob_dev, long long rec_stride,
                   rts_snapshot_desc *desc_out, void *stream);

/* Reads record i into slot slot_host[i]: from here on that slot behaves exactly like the exported stream would have,
 * bit for bit -- rts_otw_insert / rts_otw_push continue it, rts_otw_recent, rts_otw_path_cost, rts_otw_tempo,
 * rts_otw_backward and rts_otw_replay_dense answer as for a stream that was restarted and then fed the same frames.
 * The target may differ in B, N_max, slot layout and kernel flavour (RTS_OTW_SPEC, RTS_OTW_TP_FROM, RTS_OTW_WAVES);
 * F, c, max_run_count, variant, cost kind and the reference's dtype must be the exporter's: `desc` is held against the
 * handle before anything is enqueued.  That the slot follows the same recording is the caller's business (the Python
 * layer offers a digest); the device checks its length.
 *   first_host / len_host: both NULL keeps every slot's reference range; both given (rts_otw_create_refs handles
 * only): int64[n] / int32[n] host tables, entry i the range slot_host[i] moves to, checked as in rts_otw_restart.
 *   status_dev: int32[n] device memory; entry i is 0 or the RTS_SNAP_* reason for which record i was refused.  The
 * decision is taken from the record's header and the slot's range length alone; a refused slot keeps everything it owns
 * (its range too).  Slots that are not selected are never written.
 *   Asynchronous on `stream`.  The first import into a handle without history allocates it, as the first rts_otw_insert
 * does; no other allocation, no synchronisation.
 *   RTS_ERR_INVALID, with nothing enqueued and nothing changed: NULL handle, slot_host, blob_dev, desc or status_dev,
 * n != desc->n, a slot outside [0, B), a repeated slot, a misaligned blob, rec_stride != desc->rec_stride, a desc field
 * that differs from the handle (the message names the field), a bad range (the message names the stream), wrong current
 * device.  RTS_ERR_UNSUPPORTED: a handle with the dense mirror attached. */
int rts_otw_import(rts_otw *h, const int32_t *slot_host /* [n] */, int n, const void *blob_dev, long long rec_stride,
                   const rts_snapshot_desc *desc, const long long *first_host /* [n] or NULL */,
                   const int32_t *len_host /* [n] or NULL */, int32_t *status_dev /* [n] */, void *stream);
/* The WTW counterparts are declared with the WTW handle below (rts_wtw_export / rts_wtw_import). */

/* ------------------------------------------------------------------------------------------
 * Offline DTW, batched over B independent (a, b) pairs.
 * ------------------------------------------------------------------------------------------ */

/* Bytes of the device workspace rts_dtw needs for (M, N, B): packed step codes (2 bits per cell), the rows
 * handed between the workgroups of one pair's pipeline, and a status word. */
int rts_dtw_workspace_bytes(int M, int N, int B, size_t *bytes);

/* Replaces dtw.DTW(seq_a, seq_b) -> (cost, acc_cost, path) (dtw.py:5-53).
 *   a_dev: [B][M][F] frames of seq_a (rows of the matrices), `a_stride` = frames between
 *          consecutive pairs (0 = every pair shares one a); b_dev / b_stride likewise, [B][N][F].
 *   cost_dev, acc_dev: double [B][M][N] outputs (dtw.py:11, :14); back_dev: optional (may be NULL) int8
 *          [B][M][N], the reference's internal `back` matrix: step codes 0 = (0,-1), 1 = (-1,0),
 *          2 = (-1,-1) (dtw.py:30); path_dev: int32 [B][M+N][2], pairs (i, j) from (0,0) to (M-1,N-1) in the first
 *          path_len_dev[k] rows of pair k, the rows behind them are left untouched;
 *          path_len_dev: int32 [B] (-1 if the device pipeline reported a fault).
 *   ws_dev / ws_bytes: caller-owned, 16-byte aligned scratch of at least rts_dtw_workspace_bytes(M, N, B).  16 bytes is
 *          all the alignment it needs (ws_dev + 16 is as good as a 256-byte aligned address), ws_bytes is all the room:
 *          nothing is written outside [ws_dev, ws_dev + rts_dtw_workspace_bytes), and no result depends on what the
 *          workspace or the outputs held before the call.
 *   Alignment of the outputs: path_dev 8 bytes (the path is stored as (i, j) pairs, RTS_ERR_INVALID otherwise); every
 *          other output that of its element type.  The same holds for rts_dtw_paths and rts_dtw_subseq_paths.
 * Any M, N >= 1 (a long pair is spread over many workgroups).  B <= 65535.  Asynchronous on `stream`;
 * no allocation, no synchronisation (graph-capturable). */
int rts_dtw(const void *a_dev, int a_dtype, long long a_stride, const void *b_dev, int b_dtype,
            long long b_stride, int F, int M, int N, int B, double *cost_dev, double *acc_dev,
            int8_t *back_dev, int32_t *path_dev, int32_t *path_len_dev, void *ws_dev, size_t ws_bytes,
            void *stream);

/* Bytes of the device workspace rts_dtw_paths needs for B pairs of at most M_max x N_max: per-pair slices sized by the
 * maxima (2-bit step codes, boundary rows, entry columns, column records: about 0.45 bytes per cell), no [M][N] array
 * of 8-byte elements. */
int rts_dtw_paths_workspace_bytes(int M_max, int N_max, int B, size_t *bytes);

/* dtw.DTW (dtw.py:5-53) for callers who want the alignment path and its total cost and never read the matrices, over
 * pairs of different lengths in one call: what the reference's corpus harness does one pair at a time (tests.py:199-262,
 * test_all(..., DTW) -> test_dtw(wav_ref, wav_live), every recording of a piece against every other).  Neither cost nor
 * acc_cost is written anywhere, so a 30-minute pair (19 380 x 19 380) needs about 165 MB instead of 6 GB.
 *   a_dev: [B][M_max][F] padded frames of the seq_a's, `a_stride` = frames between consecutive pairs (0 = every pair
 *          shares one a; otherwise >= M_max); a_len_dev: int32[B] DEVICE array, pair k uses frames [0, a_len_dev[k]);
 *          NULL = M_max for every pair, values above M_max are clamped to it (the convention of rts_locate's
 *          q_len_dev).  b_dev / b_stride / b_len_dev likewise with N_max.  Frames beyond a pair's length are not read.
 *   Pair k, with M_k x N_k its own lengths, gets exactly what rts_dtw gives for (M_k, N_k) -- same recurrence, same
 *          first-minimum rule, same backtrack (dtw.py:32-52):
 *   path_dev: int32 [B][M_max + N_max][2]; the first path_len_dev[k] rows of pair k are the pairs (i, j) from (0, 0) to
 *          (M_k - 1, N_k - 1); the rows behind them are left untouched.
 *   path_len_dev: int32 [B]; total_dev: double [B], acc_cost[M_k - 1][N_k - 1] bit for bit.
 *   A pair with M_k < 1 or N_k < 1 gets path_len = 0 and total = +inf; nothing of it is read.
 *   If the device pipeline reports a fault (as in rts_dtw), path_len = -1 and total = NaN for the call's pairs.
 *   ws_dev / ws_bytes: caller-owned, 16-byte aligned scratch of at least rts_dtw_paths_workspace_bytes(M_max, N_max, B).
 * Limits and errors as rts_dtw: F == 12 (RTS_ERR_UNSUPPORTED otherwise), M_max, N_max, B >= 1, B <= 65535, the same
 * bound on M_max * N_max; RTS_ERR_INVALID names the argument (a NULL a_dev, b_dev, path_dev, path_len_dev, total_dev or
 * ws_dev, a stride between 1 and the maximum, a short or misaligned workspace, a path_dev that is not 8-byte aligned).
 * Asynchronous on `stream`; no allocation, no synchronisation (graph-capturable). */
int rts_dtw_paths(const void *a_dev, int a_dtype, long long a_stride, const int32_t *a_len_dev, const void *b_dev,
                  int b_dtype, long long b_stride, const int32_t *b_len_dev, int F, int M_max, int N_max, int B,
                  int32_t *path_dev, int32_t *path_len_dev, double *total_dev, void *ws_dev, size_t ws_bytes,
                  void *stream);

/* Bytes of the device workspace rts_dtw_subseq_paths needs for B pairs of at most M_max x N_max: the layout and the size
 * of rts_dtw_paths_workspace_bytes (the last row lives in a boundary row that call leaves unused). */
int rts_dtw_subseq_paths_workspace_bytes(int M_max, int N_max, int B, size_t *bytes);

/* Subsequence DTW with the path: rts_dtw_paths with both ends of b free, for aligning an excerpt (a restarted or
 * re-acquired stream's history, a rehearsal take, a cut of a recording) against a whole piece offline.  The reference
 * has no such function; the recurrence is dtw.DTW's (dtw.py:32-52: same cell cost, same step weights, same
 * first-minimum rule) with the first row freed, and it serves the same corpus harness (tests.py:199-262) once the
 * recordings on one side are excerpts.  For one pair, a ([M][F], rows, matched entirely) and b ([N][F], columns),
 * c(i, j) = 1 - <a_i, b_j> as one fma chain (the cost of rts_dtw), float64, float32 inputs widened:
 *   D[0][j] = c(0, j)
 *   D[i][0] = D[i-1][0] + c(i, 0)
 *   D[i][j] = first minimum of (D[i][j-1] + c, D[i-1][j] + c, D[i-1][j-1] + 2c)
 *   end = first j minimising D[M-1][j], total = D[M-1][end]
 *   path = from (M-1, end) the chosen predecessor of every cell until a cell of row 0 is reached, in forward order;
 *          start = the column of that row-0 cell
 * This is rts_locate's recurrence with RTS_COST_DOT -- (total, end, start) are its (cost, end, start) bit for bit --
 * without its bound on M and with the path; total equals rts_dtw_paths' total of a against b[start .. end].  Features
 * must be finite: a NaN frame makes that pair's results unspecified, nothing else (nothing is read or written out of
 * bounds, path_len stays within [0, M_max + N_max]).
 *   a_dev / a_dtype / a_stride / a_len_dev, b_dev / b_dtype / b_stride / b_len_dev, F, M_max, N_max, B: as rts_dtw_paths
 *          (padding, 0 = shared -- typically many excerpts against one b --, device length tables or NULL, clamping).
 *   path_dev: int32 [B][M_max + N_max][2]; the first path_len_dev[k] rows of pair k are the pairs (i, j) from
 *          (0, start) to (M_k - 1, end); the rows behind them are left untouched.
 *   path_len_dev: int32 [B]; total_dev: double [B]; start_dev, end_dev: int32 [B].
 *   row_dev: optional (may be NULL) double [B][N_max]: row_dev[k][0 .. N_k) = D[M_k - 1][:], the rest is left untouched.
 *   A pair with M_k < 1 or N_k < 1 gets path_len = 0, total = +inf and start = end = -1; nothing of it is read.
 *   If the device pipeline reports a fault (as in rts_dtw), path_len = -1, total = NaN and start = end = -1.
 *   ws_dev / ws_bytes: caller-owned, 16-byte aligned scratch of at least
 *          rts_dtw_subseq_paths_workspace_bytes(M_max, N_max, B).
 * Limits and errors as rts_dtw_paths: F == 12 (RTS_ERR_UNSUPPORTED otherwise), M_max, N_max, B >= 1, B <= 65535;
 * RTS_ERR_INVALID names the argument (a NULL a_dev, b_dev, path_dev, path_len_dev, total_dev, start_dev, end_dev or
 * ws_dev, a stride between 1 and the maximum, a short or misaligned workspace, a path_dev that is not 8-byte aligned);
 * all of them are reported before any HIP call.
 * Asynchronous on `stream`; no allocation, no synchronisation (graph-capturable). */
int rts_dtw_subseq_paths(const void *a_dev, int a_dtype, long long a_stride, const int32_t *a_len_dev,
                         const void *b_dev, int b_dtype, long long b_stride, const int32_t *b_len_dev,
                         int F, int M_max, int N_max, int B,
                         int32_t *path_dev, int32_t *path_len_dev, double *total_dev,
                         int32_t *start_dev, int32_t *end_dev, double *row_dev /* optional [B][N_max] */,
                         void *ws_dev, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Locate: subsequence DTW of B live excerpts against P pieces of a reference pool.
 * ------------------------------------------------------------------------------------------ */

/* Where in the repertoire is this microphone?  The reference has no such function; the recurrence is dtw.DTW's
 * (dtw.py:32-40: same cell cost, same step weights, same first-minimum rule) with the first row freed, so that a match
 * may begin and end anywhere on the piece.  For one query x ([M][F], rows) and one piece y ([N][F], columns), c(i, j)
 * the cell cost:
 *   D[0][j] = c(0, j),               S[0][j] = j
 *   D[i][0] = D[i-1][0] + c(i, 0),   S[i][0] = S[i-1][0]
 *   D[i][j] = first minimum of (D[i][j-1] + c, D[i-1][j] + c, D[i-1][j-1] + 2c), S[i][j] = S of the chosen predecessor
 *   end = first j minimising D[M-1][j], cost = D[M-1][end], start = S[M-1][end]   (frame indices inside the piece)
 * All arithmetic is float64, float32 inputs widened.  cost equals acc_cost[-1][-1] of rts_dtw of the query against frames
 * [start, end] of the piece, bit for bit.  cost_kind: RTS_COST_DOT is 1 - <x_i, y_j> as one fma chain (the cost of
 * rts_dtw), RTS_COST_EUCLID is ||x_i - y_j||_2 in the order of the Euclidean tracker.  Features must be finite; a NaN
 * frame makes the results of the (stream, piece) pairs it takes part in unspecified, nothing else.
 *   queries_dev: [B][M_max][F] (q_dtype); q_len_dev: int32[B] DEVICE array of valid frames per stream, NULL = M_max for
 *          all, values above M_max are clamped to it.
 *   pool_dev: [n_pool_frames][F] (pool_dtype), e.g. the pool given to rts_otw_create_refs; piece p is frames
 *          [piece_first_dev[p], piece_first_dev[p] + piece_len_dev[p]).  The two tables are DEVICE arrays (int64[P],
 *          int32[P]) and only checked for NULL on the host.  Pieces may overlap or repeat.
 *   cost_dev double[B][P], end_dev / start_dev int32[B][P].  A piece with len < 1 or a range outside the pool gives
 *          cost = +inf, end = start = -1 for every stream (nothing is read out of bounds); so does a stream with
 *          q_len <= 0 for every piece.
 *   row_dev / rowstart_dev: optional (either may be NULL) double / int32 [B][n_pool_frames]: D[M-1][:] / S[M-1][:] of
 *          every valid piece at its pool position.  Cells that belong to no piece are left untouched; where pieces
 *          overlap, a cell holds the value of one of them.
 * One workgroup works on one (piece, stream) pair from end to end -- the recurrence is a chain along the piece and a
 * split would not be exact -- so the call is built for many pairs: a caller with one very long piece gets one
 * workgroup per stream.
 * Limits: F == 12 and M_max <= 256 (RTS_ERR_UNSUPPORTED otherwise), 1 <= B, P <= 65535.  RTS_ERR_INVALID, naming the
 * argument: a NULL pointer other than q_len_dev / row_dev / rowstart_dev, M_max < 1, B or P out of range,
 * n_pool_frames < 1, a bad q_dtype, pool_dtype or cost_kind.
 * Asynchronous on `stream`; no allocation, no synchronisation (graph-capturable). */
int rts_locate(const void *queries_dev, int q_dtype, int M_max, const int32_t *q_len_dev, int B, const void *pool_dev,
               int pool_dtype, int F, long long n_pool_frames, const long long *piece_first_dev,
               const int32_t *piece_len_dev, int P, int cost_kind, double *cost_dev, int32_t *end_dev,
               int32_t *start_dev, double *row_dev, int32_t *rowstart_dev, void *stream);

/* Ranked non-overlapping matches per (stream, piece): music repeats, and an excerpt of a repeated section matches every
 * pass equally well, of which rts_locate reports the earliest only.  For one query, one piece of N columns, its last
 * row D = D[M-1][:] and its starts S = S[M-1][:] exactly as rts_locate defines them:
 *   rank r = 0, 1, ..., K-1: among the columns j with D[j] finite that are not suppressed, the first minimum of D[j]
 *          (strict <, columns ascending): end_r = j, cost_r = D[j], start_r = S[j].  Column j is suppressed when its own
 *          match range [S[j], j] intersects the range of an earlier rank: S[j] <= end_q && j >= start_q for some q < r.
 *   The list ends at the first rank where no column is left or where cost_r > max_cost (+inf: no cut-off).
 * Rank 0 is rts_locate's (cost, end, start) bit for bit; costs are non-decreasing in rank, ranges pairwise disjoint; with
 * M = 1 the ranks are the K cheapest columns in stable order.
 *   queries_dev ... cost_kind: rts_locate's arguments, unchanged.
 *   cost_dev double[B][P][K], end_dev / start_dev int32[B][P][K], n_dev int32[B][P]: n = ranks written; slots from n on
 *          hold +inf, -1, -1.  A piece with len < 1 or outside the pool gives n = 0 and empty slots for every stream; so
 *          does a stream with q_len <= 0 for every piece.
 *   Overlapping pieces: rts_locate's row holds "the value of one of them" in shared cells, so a valid piece whose pool
 *          range intersects the range of another valid piece (identical ranges included) gets n = -1: slot 0 holds
 *          rts_locate's own answer for it, the other slots are empty.  (q_len <= 0 comes first: n = 0.)  The flag is
 *          decided on the device, by one workgroup that tests every piece against the table: P * P / 1024 tests per
 *          thread, meant for a repertoire's few hundred pieces.
 *   ws_dev: rts_locate_matches_workspace_bytes(B, n_pool_frames) bytes of the caller's device memory, any alignment.  It
 *          holds the rows and the starts: 256 + (8 B n_pool_frames rounded up to 256) + (4 B n_pool_frames rounded up to
 *          256) bytes.  It needs no initialisation and no result depends on what it held before.
 * Three launches on `stream`: the kernel of rts_locate with both row outputs in the workspace, the overlap flags, the
 * ranks (one workgroup per (piece, stream): K rounds of a first-minimum reduction over the piece's row).
 * Limits and errors as rts_locate, and: 1 <= K <= 32 (K < 1 RTS_ERR_INVALID, K > 32 RTS_ERR_UNSUPPORTED); a NaN max_cost,
 * n_dev or ws_dev NULL, ws_bytes too small, n_pool_frames > 2^40: RTS_ERR_INVALID naming the argument.  All checks come
 * before the first HIP call.
 * Asynchronous on `stream`; no allocation, no synchronisation (graph-capturable). */
int rts_locate_matches_workspace_bytes(int B, long long n_pool_frames, size_t *bytes);
int rts_locate_matches(const void *queries_dev, int q_dtype, int M_max, const int32_t *q_len_dev, int B,
                       const void *pool_dev, int pool_dtype, int F, long long n_pool_frames,
                       const long long *piece_first_dev, const int32_t *piece_len_dev, int P, int cost_kind, int K,
                       double max_cost, double *cost_dev, int32_t *end_dev, int32_t *start_dev, int32_t *n_dev,
                       void *ws_dev, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Chroma front end: frame -> window -> rFFT -> power -> 12-bin filterbank -> L2 normalise.
 * ------------------------------------------------------------------------------------------ */
typedef struct rts_chroma rts_chroma;

/* num_hops of chroma.create_stft (chroma.py:49-54): floor((n_samples + pad_left - fft_len) / hop) + 1,
 * 0 if the (padded) signal is shorter than one frame. */
long long rts_chroma_num_frames(long long n_samples, int fft_len, int hop, int pad_left);

/* A plan = window + twiddles + filterbank on the device.  `fb_host`: 12 x (fft_len/2+1) doubles, row
 * = pitch class (what librosa.filters.chroma(fs, fft_len) returns at chroma.py:69 / wtw.py:39);
 * `window_host`: fft_len doubles or NULL for np.hanning(fft_len) (chroma.py:39,:62).  fft_len: power
 * of two in [64, 8192] (the reference uses 4096, chroma.py:20). */
int rts_chroma_create(int fft_len, int hop, const double *window_host, const double *fb_host, rts_chroma **out);
int rts_chroma_destroy(rts_chroma *h);

/* Replaces create_stft + create_chroma (chroma.py:44-75), wav_to_chroma_col (chroma.py:35-42) and the
 * per-hop chroma of WTW.insert (wtw.py:81-90).  Frame m covers samples [m*hop - pad_left, +fft_len),
 * indices < 0 read as zero (pad_left = fft_len/2 for create_stft's centred framing, 0 for live
 * buffers).  `chroma_out_dev`: [n_frames][12] (out_dtype) or NULL; `stft_out_dev`: optional
 * [n_frames][fft_len/2+1] complex doubles (re, im) -- create_stft's return value, frame-major; 16-byte aligned, the
 * alignment of one complex double (RTS_ERR_INVALID otherwise).  chroma_out_dev needs the alignment of its element type.
 * normalize = 0 gives create_chroma(ft, normalize=False). */
int rts_chroma_frames(rts_chroma *h, const void *samples_dev, int sample_dtype, long long n_samples,
                      int pad_left, int n_frames, int normalize, void *chroma_out_dev, int out_dtype,
                      double *stft_out_dev, void *stream);

/* The same for B independent sample buffers in one launch (many live microphones): samples_dev is
 * [B][sample_stride]; stream b holds n_samples_dev[b] valid samples and gets n_frames_dev[b]
 * (<= n_frames_max) frames written to chroma_out_dev [B][n_frames_max][12]. */
int rts_chroma_frames_batch(rts_chroma *h, const void *samples_dev, int sample_dtype, long long sample_stride,
                            const int32_t *n_samples_dev, int pad_left, int B, int n_frames_max,
                            const int32_t *n_frames_dev, int normalize, void *chroma_out_dev, int out_dtype,
                            void *stream);

/* fft_len and hop of a plan (either pointer may be NULL). */
int rts_chroma_plan_info(const rts_chroma *h, int *fft_len, int *hop);

/* create_chroma(ft) for a power spectrum that is already on the device: spec_dev [n_frames][fft_len/2+1].  Like
 * rts_chroma_frames and rts_chroma_frames_batch it refuses (RTS_ERR_INVALID) a plan whose device is not the current
 * one. */
int rts_chroma_project(rts_chroma *h, const double *spec_dev, int n_frames, int normalize, void *chroma_out_dev,
                       int out_dtype, void *stream);

/* wav_to_chroma_diff's last step (chroma.py:85-90): out[m][f] = max(chroma[m+1][f] - chroma[m][f], 0),
 * out has n_frames-1 frames. */
int rts_chroma_diff(const void *chroma_dev, int dtype, int n_frames, void *out_dev, void *stream);

/* ------------------------------------------------------------------------------------------
 * Resampler: audio at any rate to the plan's rate, by a rational ratio L / M = fs_out / fs_in (reduced).
 * ------------------------------------------------------------------------------------------ */
typedef struct rts_resample rts_resample;

/* Replaces the resampling librosa.load does silently when a file is not at 22 050 Hz (chroma.py:27, wtw.py:23).  It is
 * not that resampler (a third-party dependency the reference does not pin) but one this project defines to the bit.
 * With taps h[-half .. half] (host doubles, e.g. filters.resample_taps) and input samples x[n] (float32, or PCM16 scaled
 * by 1/32768 exactly as rts_live_* scales it; x[n] = 0 for n < 0 and past the end), output sample k is
 *   c    = k * M + half                                                              (64-bit)
 *   y[k] = (float) sum over n = ceil((c - 2 half) / L) .. floor(c / L) of h[c - n L - half] * (double)x[n]
 * with n ascending, every term one float64 multiply followed by one float64 add (no fused multiply-add), and the sum
 * rounded once to float32: the result does not depend on how the input was cut into feeds. */

/* Output samples of a one-shot run over n_in input samples, ceil(n_in L / M) (chroma.py:27: len(librosa.load(path)[0])).
 * Pure host arithmetic; 0 for n_in <= 0. */
long long rts_resample_out_len(long long n_in, int L, int M);
/* Output samples that exist once in_total input samples have arrived: max(0, ceil((in_total L - half) / M)), i.e. every
 * k whose last input floor((k M + half) / L) has been seen.  They are the first samples of the one-shot result on the
 * same input, bit for bit; the latency is half / L input samples.  Pure host arithmetic (the microphone loops of
 * livenote_live.py:161-209 have no counterpart: PyAudio is opened at the rate they need). */
long long rts_resample_avail(long long in_total, int L, int M, int half);
/* The plan: the table on the current device, phase-major (librosa.load's resampling filter, chroma.py:27 / wtw.py:23; the
 * library is filter-agnostic like rts_chroma_create).  taps_host: 2 half + 1 doubles, h[-half] first.
 * RTS_ERR_INVALID, naming the argument, before any GPU call: NULL out or taps_host, L < 1, M < 1, gcd(L, M) != 1,
 * half < 1.  RTS_ERR_UNSUPPORTED: 2 half + 1 > 4 194 304 taps, ceil(2 half / L) > 4096 input samples under one output,
 * or floor((12 288 - floor(2 half / L) - 1) * L / M) < 64, the outputs whose inputs fit a workgroup's 12 288-sample
 * window (with filters.resample_taps' 16 zero crossings both mean fs_in above about 128 fs_out). */
int rts_resample_create(int L, int M, const double *taps_host, int half, rts_resample **out);
int rts_resample_destroy(rts_resample *p);
/* One-shot, ragged over B streams (librosa.load's resampling of whole files, chroma.py:27 / wtw.py:23): samples_dev is
 * [B][sample_stride] of sample_dtype (RTS_F32 | RTS_I16), stream b holds n_in_dev[b] (int32, DEVICE) samples and gets
 * n_out_dev[b] = min(rts_resample_out_len(n_in_dev[b]), n_out_max) samples written to out_dev[b][0 .. n_out_dev[b]);
 * samples behind them are left untouched.  out_dev float32 [B][n_out_max], n_out_dev int32 [B].  1 <= B <= 65535.
 * Asynchronous on `stream`; no allocation, no synchronisation (graph-capturable). */
int rts_resample_run(rts_resample *p, const void *samples_dev, int sample_dtype, long long sample_stride,
                     const int32_t *n_in_dev, int B, int n_out_max, float *out_dev, int32_t *n_out_dev, void *stream);

/* ------------------------------------------------------------------------------------------
 * Windowed time warping, batched over B live streams against one reference chroma (or one each).
 * ------------------------------------------------------------------------------------------ */
typedef struct rts_wtw rts_wtw;

/* layout of the int32 WTW state vector (8 entries per stream) */
#define RTS_WTW_STATE_LEN 8
#define RTS_WTW_ST_CHROMA_PTR 0
#define RTS_WTW_ST_LIVE_PTR 1
#define RTS_WTW_ST_REF_PTR 2
#define RTS_WTW_ST_STATUS 3
#define RTS_WTW_ST_N_PATH 4
#define RTS_WTW_ST_N_WINDOWS 5
#define RTS_WTW_ST_CELLS_LO 6
#define RTS_WTW_ST_CELLS_HI 7

/* Replaces the chroma-level state of WTW.__init__ (wtw.py:50-68): `chroma_ref_dev` is the reference
 * chroma [M][F] float64 (what wtw.py:37-41 computes; use rts_chroma_frames with pad_left =
 * fft_len/2), held by reference.  win_frames = dtw_win_size / hop_size, hop_frames = dtw_hop_size /
 * hop_size (wtw.py:100,:107), 1 <= win_frames <= 16384 (one workgroup per stream up to 64 frames; a
 * pipeline of workgroups per window above), hop_frames >= 1.  The handle owns a live
 * chroma history of 2M frames per stream (wtw.py:52,:55).  keep_last_d != 0 also keeps the last
 * window's accumulated-cost matrix D for inspection (the reference stores it into self.acc_cost,
 * wtw.py:105). */
int rts_wtw_create(const double *chroma_ref_dev, int F, int M, int B, int win_frames, int hop_frames,
                   int keep_last_d, rts_wtw **out);
/* The same for B streams that each follow their own reference chroma: stream b behaves exactly like stream 0 of an
 * rts_wtw_create handle made with chroma_ref_dev = frames [first_host[b], first_host[b] + len_host[b]) of
 * `chroma_refs_dev` ([n_ref_frames][F] float64) and M = len_host[b], so its N = 2 M_b, its boundary checks and the
 * truncation of its reference windows are its own.  Tables copied at create, ranges may overlap or repeat; the live
 * history is [B][2 M_max][F] (rts_wtw_device_views reports 2 M_max).  Errors as for rts_otw_create_refs.  M_max is the
 * longest range given here; room for a longer piece is reserved as described at rts_otw_create_refs. */
int rts_wtw_create_refs(const double *chroma_refs_dev, int F, long long n_ref_frames,
                        const long long *first_host, const int32_t *len_host, int B, int win_frames,
                        int hop_frames, int keep_last_d, rts_wtw **out);
int rts_wtw_destroy(rts_wtw *h);
int rts_wtw_reset(rts_wtw *h, void *stream);

/* Restart single streams (a new WTW object, wtw.py:50-68, for that one microphone) while the others keep running.
 * Arguments, ordering, by-value transport and errors exactly as for rts_otw_restart (len_host[b] <= M_max).  A selected
 * stream's state vector is zero again (RTS_RUNNING), its path empty, its live chroma history reads as zeros (wtw.py:55)
 * and its appended-column count is zero, on the one-workgroup window kernels and on the strip-DP pipeline alike.  With
 * keep_last_d the kept D of a restarted stream is unspecified until its next window, as on a fresh handle. */
int rts_wtw_restart(rts_wtw *h, const uint8_t *mask_host, const long long *first_host, const int32_t *len_host,
                    void *stream);

/* Replaces the part of WTW.insert below the per-hop chroma (wtw.py:92-128): appends n_new[b] (or
 * n_max when n_new_dev is NULL) already-normalised live chroma columns per stream -- cols_dev is
 * [B][n_max][F] -- then, column by column, applies the boundary check (wtw.py:96-97) and runs every
 * window that has become available (get_cost_matrix, run_dtw, find_path, hand-over).  precheck != 0
 * first applies insert()'s entry check (wtw.py:76-77).  Status STOP_REF_END replaces the "stop"
 * return value and is sticky.  Asynchronous on `stream`. */
int rts_wtw_push(rts_wtw *h, const void *cols_dev, int cols_dtype, int n_max, const int32_t *n_new_dev,
                 int precheck, void *stream);

/* rts_otw_recent for the live chroma history (wtw.py:52,:55) of a WTW handle: same contract, n being the columns appended
 * since create, reset or the stream's last restart, capped at 2 M_b.  rts_wtw_push alternates between two count arrays, and
 * a captured call reads the one that was current at capture: capture it behind the pushes it follows, in one graph. */
int rts_wtw_recent(rts_wtw *h, int M_max, double *out_dev, int32_t *len_dev, const uint8_t *mask_dev, void *stream);

int rts_wtw_read_states(rts_wtw *h, int32_t *states /* [B][RTS_WTW_STATE_LEN] */, void *stream);
int rts_wtw_read_path(rts_wtw *h, int b, int32_t *pairs, int cap_pairs, int *n, void *stream);
/* The last window's accumulated-cost matrix D, [W][W] doubles (needs keep_last_d).  A window of n live frames against m
 * reference frames writes D[i][j] for i < n, j < m with leading dimension W and nothing else.  Today every window is
 * W x W: wtw.py:96-97 stops a stream while ref_ptr + W is still inside the reference, so the slice wtw.py:102 takes is
 * never cut short.  Were one cut short (m < W), the cells outside its n x m part would keep what the stream's earlier
 * windows wrote there -- within a run m only shrinks, so column j >= m holds the D of the last window that reached
 * it.  Before a stream's first window since create the buffer is unspecified. */
int rts_wtw_read_last_d(rts_wtw *h, int b, double *d_host, void *stream);
/* Device views: live chroma history [B][2M][F] float64 and (if kept) the last window's D [B][W][W]. */
int rts_wtw_device_views(rts_wtw *h, double **live_chroma_dev, int *live_capacity, double **last_d_dev);

/* Snapshots of single WTW streams: rts_otw_snapshot_bytes / rts_otw_export / rts_otw_import for this tracker, with the
 * same arguments, the same refusals and the same per-record status words.  A record is the 64-byte header (kind
 * RTS_SNAPSHOT_WTW, M_b in the word after N_b, which is 0), the eight state words, the last window's D (W * W doubles) on
 * a keep_last_d handle once a window has run, the path pairs and the live chroma columns up to the appended count
 * (capped at 2 M_b) -- what rts_wtw_restart resets, plus D.  The appended count is carried capped at 2 M_b + 1: past
 * 2 M_b the tracker only ever asks whether a column was dropped, and how far the count ran depends on the exporter's
 * history stride.  Nothing of the strip-DP pipeline's control or ticket words is carried: no window is pending between
 * two pushes, the control step rewrites every word it later reads, and a handle that runs the window kernel has none;
 * an import zeroes them like a restart, so a stream may move between a window-kernel handle and a strip-DP handle
 * (RTS_WTW_WIN=0).  An import writes the count into both of the handle's count arrays, and the slot's history behind
 * the record's columns reads zero again (wtw.py:55).  The desc must agree in window, hop and keep_last_d; the stride is
 * the record at 2 M_max columns and the handle's path capacity.  Calls are in stream order between two rts_wtw_push;
 * an export in the middle of a partly filled window carries the columns that wait for it. */
int rts_wtw_snapshot_bytes(const rts_wtw *h, size_t *bytes);
int rts_wtw_export(rts_wtw *h, const int32_t *idx_host /* [n] */, int n, void *blob_dev, long long rec_stride,
                   rts_snapshot_desc *desc_out, void *stream);
int rts_wtw_import(rts_wtw *h, const int32_t *slot_host /* [n] */, int n, const void *blob_dev, long long rec_stride,
                   const rts_snapshot_desc *desc, const long long *first_host /* [n] or NULL */,
                   const int32_t *len_host /* [n] or NULL */, int32_t *status_dev /* [n] */, void *stream);

/* Device view of the state vectors, [B][RTS_WTW_STATE_LEN] int32 (zero-copy consumers; rts_live_* publishes from it). */
int rts_wtw_state_view(rts_wtw *h, int32_t **state_dev);

/* ------------------------------------------------------------------------------------------
 * Live ingestion: raw audio buffers of B microphones -> chroma columns -> alignment state, all on the device.
 * ------------------------------------------------------------------------------------------ */
typedef struct rts_live rts_live;

/* Replaces the audio loops that feed the trackers, for B streams per call:
 *   livenote_live.py:161-209  receive_audio / _process_input: once >= fft_len samples are pending,
 *                             `while len(data) >= 4096: col = wav_to_chroma_col(data[:4096]); ln.insert(col); data = data[2048:]`
 *   wtw.py:71-93              WTW.insert(list): self.buf += list; `while len(self.buf) >= fft_len:` one column per hop
 * Binds a chroma plan (its fft_len / hop; un-padded framing, chroma.py:35-42) and exactly one of `otw` (created with
 * the same B; columns go through rts_otw_push) or `wtw` (rts_wtw_push with precheck, i.e. wtw.py:76-77 once per feed);
 * a tracker created for another number of streams is refused with RTS_ERR_INVALID.
 * The plan and the tracker must outlive the handle and live on the current device.  max_pending: capacity in samples of
 * each stream's pending buffer (>= fft_len + hop); a feed that would exceed it is refused with RTS_ERR_INVALID.
 * A plan with hop > fft_len is accepted and follows the reference's slicing: a column is taken as soon as fft_len
 * samples are pending, and `buf = buf[hop:]` on fewer than hop samples leaves none, so pending after the drop is
 * max(0, pending - columns * hop) -- the samples between a column's end and its hop are skipped only as far as they
 * have arrived, and the next column starts at the next sample delivered.
 * All calls of one handle must use the same `stream`. */
int rts_live_create(rts_chroma *plan, rts_otw *otw, rts_wtw *wtw, int B, int max_pending, rts_live **out);

/* What a live handle hands to its tracker. */
#define RTS_FEATURE_CHROMA 0      /* the normalised chroma columns themselves */
#define RTS_FEATURE_CHROMA_DIFF 1 /* max(chroma[m+1] - chroma[m], 0) per pitch class: wav_to_chroma_diff, chroma.py:77-90 */

/* rts_live_create with a feature kind (rts_live_create is this with RTS_FEATURE_CHROMA).
 * RTS_FEATURE_CHROMA_DIFF is the microphone form of the reference's headline configuration (tests.py:145-163,
 * LiveNoteV2(..., chroma_diff=True) on wav_to_chroma_diff features): column m handed to the tracker is
 * np.clip(np.diff(chroma), 0, inf)[:, m] of the columns the ingestion makes (un-padded hop framing), not renormalised,
 * a NaN difference stays NaN.  The difference needs the previous chroma column of every stream, which the handle
 * carries on the device from feed to feed: a stream's tracker receives its first frame when the stream's second chroma
 * column is complete, and a feed in which no stream completes a difference column is an ordinary feed.
 * The tracker's reference must itself be difference features (wav_to_chroma_diff(ref) / rts_chroma_diff of the
 * reference's chroma).  The cost kind is the tracker's own choice at its create: tests.py:156 pairs RTS_COST_EUCLID
 * with either feature kind, and livenote_v2.py:168 uses it for chroma_diff=True.
 * RTS_FEATURE_CHROMA_DIFF with a `wtw` tracker returns RTS_ERR_UNSUPPORTED: the reference never runs WTW on difference
 * features, and its cosine cost is NaN on the zero columns they contain.  Any other feature_kind: RTS_ERR_INVALID. */
int rts_live_create_features(rts_chroma *plan, rts_otw *otw, rts_wtw *wtw, int B, int max_pending, int feature_kind,
                             rts_live **out);
/* rts_live_create_features for microphones at another rate than the plan's: what librosa.load's resampling (chroma.py:27 /
 * wtw.py:23) is for files, for the live loops, whose reference form opens PyAudio at the rate it needs.  The handle takes
 * INPUT-rate samples in rts_live_staging / rts_live_submit / rts_live_feed.  Per feed one more launch sits between the copy
 * and the append: it resamples (the stream's carried tail + the staged samples) with `resample_plan` -- held by
 * reference, it must outlive the handle -- into a second device buffer laid out like a staging slot, from which the
 * unchanged chain goes on.  Per stream the device carries the last ceil(2 half / L) input samples (float32, after
 * scaling) and two int64 totals; the host mirrors the totals with rts_resample_avail, which is how it knows every
 * stream's new sample count without a read-back: a stream that has been fed in_total samples has handed
 * rts_resample_avail(in_total) plan-rate samples on, the first that many of a one-shot run, bit for bit, however the
 * input was cut into feeds.  max_pending stays a capacity in plan-rate samples; a feed whose OUTPUT would exceed it is
 * refused with RTS_ERR_INVALID and changes nothing (totals, tail, pending).  rts_live_staging reports the input-rate
 * capacity, B * in_cap with in_cap = ceil((max_pending + 1) M / L) + ceil(2 half / L) + 2 samples per stream: no feed
 * whose output fits max_pending is longer than in_cap, whatever table the plan holds; a stream's count above in_cap is
 * refused with RTS_ERR_INVALID naming the staging capacity, like a feed that exceeds the slot as a whole.  rts_live_reset zeroes tail and totals of all
 * streams and rts_live_restart those of the selected ones (device and mirror): the new run starts on silence.
 * resample_plan NULL: RTS_ERR_INVALID (equal rates never build a resampler: use rts_live_create_features); a
 * resample_plan created on another device than the current one: RTS_ERR_INVALID; B * in_cap >= 2^31: RTS_ERR_INVALID
 * naming max_pending; everything else as rts_live_create_features. */
int rts_live_create_resampled(rts_chroma *plan, rts_otw *otw, rts_wtw *wtw, int B, int max_pending, int feature_kind,
                              rts_resample *resample_plan, rts_live **out);
int rts_live_destroy(rts_live *h);
/* Drops pending samples (and, with RTS_FEATURE_CHROMA_DIFF, the carried chroma column of every stream: each stream
 * is fresh again and skips its first chroma column) and resets the bound tracker.  Synchronises `stream`. */
int rts_live_reset(rts_live *h, void *stream);
/* Restart single streams of a session: drops the selected streams' pending samples (device buffer and host mirror:
 * rts_live_pending reads 0 for them), restarts them in the bound tracker (rts_otw_restart / rts_wtw_restart, same
 * arguments and errors) and republishes their status / position words, so that rts_live_poll shows RTS_RUNNING and the
 * positions of a fresh session for them; feeds_done does not go backwards.  Ordered after the feeds already submitted:
 * samples submitted before the call belong to the stream's old run, samples submitted after it to the new one.  A
 * staging slot handed out by rts_live_staging and not yet submitted stays valid.  With RTS_FEATURE_CHROMA_DIFF the
 * carried chroma column of a selected stream is dropped with its samples: its next chroma column only becomes the new
 * carry, so the first feed that completes columns for it hands the tracker one column fewer than it completes.
 * Unlike rts_live_reset it does not synchronise anything. */
int rts_live_restart(rts_live *h, const uint8_t *mask_host, const long long *first_host, const int32_t *len_host,
                     void *stream);

/* One feed, zero-copy form.  rts_live_staging hands out the next pinned host staging slot (it waits only if the feed
 * that used the slot four feeds ago has not been consumed by the device yet): the producer writes counts_host[b] = new
 * samples of stream b and the samples of all streams packed back to back in stream order (float32 or int16) to
 * samples_host (capacity_samples = B * max_pending).  rts_live_submit then enqueues, without synchronising anything:
 * one host-to-device copy of the used part of the slot (on an internal copy stream, so that it overlaps the kernels of
 * the previous feed), append to the per-stream pending buffers, chroma of every complete hop, with
 * RTS_FEATURE_CHROMA_DIFF the difference against the previous column (the carried one for a feed's first), push into
 * the tracker, drop of the consumed samples (hop per column, livenote_live.py:208 / wtw.py:83), publication of the
 * status words.  A refused feed (RTS_ERR_INVALID) changes neither the pending counts nor the carry.
 * If one of those enqueues itself fails (RTS_ERR_HIP, or the tracker's error), the device may have run a part of the
 * feed, and the handle no longer knows what its buffers hold: from then on rts_live_staging, rts_live_submit,
 * rts_live_feed and rts_live_restart return RTS_ERR_INVALID (the message says that an earlier feed failed while it was
 * being enqueued) until rts_live_reset, which starts every stream afresh, has succeeded. */
int rts_live_staging(rts_live *h, int32_t **counts_host, void **samples_host, long long *capacity_samples);
int rts_live_submit(rts_live *h, int sample_kind /* RTS_F32 | RTS_I16 */, void *stream);
/* The same from caller-owned host arrays (one memcpy into the staging slot): samples_host packed like above. */
int rts_live_feed(rts_live *h, const void *samples_host, int sample_kind, const int32_t *counts_host, void *stream);

/* Non-blocking look at what the device last published (host-mapped memory, written at the end of every feed):
 * status[b] (RTS_RUNNING / RTS_STOP_REF_END = insert() returned "stop" / ...), positions[2b] = live frame index
 * (t / live_ptr), positions[2b+1] = reference frame index (j / ref_ptr); *feeds_done = feeds whose results these words
 * reflect for every stream, *feeds_submitted = feeds enqueued so far.  Any pointer may be NULL. */
int rts_live_poll(rts_live *h, int32_t *status /* [B] */, int32_t *positions /* [B][2] */, int *feeds_done,
                  int *feeds_submitted);
/* The confidence of rts_otw_path_cost without a read-back.  rts_live_watch(K): 0 = off (the default), 1..256 = on.
 * With watch on, every rts_live_submit enqueues one more launch, between the tracker push and the publication of the
 * status words (in a feed without columns too): rts_otw_path_cost over the last K path points, its mean / n written to a
 * second host-mapped block, which the first rts_live_watch(K > 0) allocates.  With watch off a feed enqueues exactly what
 * it enqueues without this function.  rts_live_confidence is the non-blocking look at those words: mean_cost[b], n_points[b]
 * and *feeds_done, computed as by rts_live_poll, with the same guarantee: when *feeds_done >= k, every word read reflects a
 * feed >= k in which watch was on.  rts_live_watch(0) leaves the words as they are.  rts_live_restart republishes n = 0,
 * mean = NaN for the selected streams, rts_live_reset for all.  Any output pointer may be NULL.
 *   RTS_ERR_INVALID: NULL handle, K outside [0, 256], rts_live_confidence before any rts_live_watch(K > 0).
 * RTS_ERR_UNSUPPORTED: rts_live_watch on a handle bound to a WTW tracker (there is no WTW path cost). */
int rts_live_watch(rts_live *h, int K);
int rts_live_confidence(rts_live *h, double *mean_cost /* [B] */, int32_t *n_points /* [B] */, int *feeds_done);

/* The level gate: keeps the columns of a microphone nobody plays into away from its tracker, per stream, without a
 * read-back.  The reference never tracks silence: an operator presses `r` when the music starts (livenote_live.py:145-150,
 * :162) and watches a microphone meter (livenote_live.py:170-177, wtw_live.py:192-197).  On a silent column every
 * reference frame costs the same, so the OTW family ties and walks the diagonal while nothing is played, and WTW's cosine
 * cost is NaN; a session opened before the downbeat, or running across the gap between two movements, loses its place.
 *
 * Level of a column: column m of stream b in a feed is framed from the L = fft_len pending samples x[0..L) at offset
 * m * hop of the stream's buffer (after PCM scaling and after the resampler: on a resampling handle these are plan-rate
 * samples; the same offset in the hop > fft_len geometry).  Its level is (sum_i (double)x[i] * (double)x[i]) / L, the mean
 * square, un-windowed; 10 log10(level) is the reference meter's 20 log10(rms).  Every product is exact in float64 and the
 * order of the sum depends on the index i alone, so the same frame has the same level however the audio was cut into feeds.
 * Decision: every stream carries q, the length of its current run of quiet columns, saturating at hold + 1; a fresh stream
 * is closed (q = hold + 1), waiting for the first sound.  For every new chroma column in order: loud = level >= min_level
 * (a NaN level is quiet); loud: q = 0 and the column passes; otherwise q = min(q + 1, hold + 1) and the column passes iff
 * q <= hold.  So with hold = 0 a column passes iff it is loud, a rest of up to `hold` columns inside the music is kept
 * whole, a longer rest passes its first `hold` columns and then pauses the stream until the next loud column, and a stream
 * that has never heard a loud column passes nothing.
 * What the tracker gets.  RTS_FEATURE_CHROMA: the passing columns in order, packed to the front of a second buffer with
 * the feed's row stride, their counts as the push's n_new_dev.  RTS_FEATURE_CHROMA_DIFF: the difference step runs unchanged
 * on all chroma columns (carry and first-column skip as without the gate); the difference column of chroma columns
 * (m - 1, m) is handed on iff both passed, "the previous column passed" being one more device word per stream for a
 * feed's first column, zero whenever the stream has no carry.  Samples dropped per column, rts_live_pending and the
 * staging ring are as without the gate.  A feed in which every column of every stream is dropped still calls the push,
 * with counts of zero, which leaves the trackers alone.
 * Ordinals.  seen[b] counts the chroma columns stream b has completed since create, reset or its last restart, passed[b]
 * the columns handed to its tracker in that time.  The handle keeps the ordinal (the value of `seen` before the column,
 * for a difference column that of the later chroma column) of every column handed on, as long as the bound tracker's
 * history (2 N_max for OTW, 2 M_max for WTW): the counts run on past it, nothing is stored past it.  Live frame t of a
 * tracker's path thus ended at (ordinal[t] * hop + fft_len) / fs seconds of the stream's run.
 *
 * rts_live_gate: min_level > 0 and finite switches the gate on (buffers are made on first use), min_level == 0 off;
 * 0 <= hold <= 65535.  Allowed only before the first feed after create or after rts_live_reset: later it returns
 * RTS_ERR_INVALID, the message says so, and nothing changes.  With the gate on every feed enqueues two more launches
 * between the chroma (difference) step and the push (one in a feed without a column); with it off, or never called, a
 * feed enqueues exactly what it enqueues without this function.  Either tracker, either feature kind, resampling
 * handles too.  rts_live_reset keeps the setting and closes every stream; rts_live_restart closes the selected
 * streams: q, the previous-passed word, seen and passed start again, their ordinals are empty, their words republished.
 *   RTS_ERR_INVALID: NULL handle, negative / NaN / infinite min_level, hold out of range, after a feed, a failed handle.
 * rts_live_levels: the non-blocking look at a third host-mapped block, like rts_live_confidence and with the same
 * guarantee (when *feeds_done >= k, every word read reflects a feed >= k): level[b] of the stream's most recent chroma
 * column (NaN before its first), open[b] whether that column passed, seen[b], passed[b].  Any pointer may be NULL.
 * RTS_ERR_INVALID before the first rts_live_gate(min_level > 0).
 * rts_live_gate_columns: synchronises `stream`; *n = passed[b]; copies min(*n, cap, history length) ordinals of stream b
 * to ordinals_host (may be NULL).  RTS_ERR_INVALID: NULL handle or n, b out of range, before the first
 * rts_live_gate(min_level > 0). */
int rts_live_gate(rts_live *h, double min_level, int hold);
int rts_live_levels(rts_live *h, double *level /* [B] */, int32_t *open /* [B] */, int32_t *seen /* [B] */,
                    int32_t *passed /* [B] */, int *feeds_done);
int rts_live_gate_columns(rts_live *h, int b, int32_t *ordinals_host, int cap, int *n, void *stream);

/* Device views of the columns the most recently submitted feed handed to the tracker, and of their per-stream counts
 * (zero-copy consumers, tests): *cols_dev is float64, stream b's column i at cols_dev[(b * *cols_stride + i) * 12],
 * i < (*n_cols_dev)[b].  *cols_stride, the rows per stream, is the largest number of chroma columns any stream completed
 * in that feed (0: the feed completed none, or nothing was fed since create / reset) -- the layout the chroma kernel
 * and the tracker push share, so it changes from feed to feed and is returned here from the host mirror; it never
 * exceeds *cols_cap = (max_pending - fft_len) / hop + 1, the rows per stream the buffer has room for.  Valid for both
 * feature kinds: RTS_FEATURE_CHROMA views the chroma columns and the counts rts_chroma_frames_batch was given,
 * RTS_FEATURE_CHROMA_DIFF the difference columns and their counts; with the gate on (rts_live_gate) either kind views
 * the gated buffer and its counts, at the same row stride -- the columns the feed handed to the tracker.  The pointers
 * stay the same for the handle's life (two sets: gate off, gate on); the contents belong to the last feed in stream
 * order, the caller synchronises.  Any pointer may be NULL. */
int rts_live_columns_view(rts_live *h, double **cols_dev, int *cols_cap, int *cols_stride, int32_t **n_cols_dev);
/* Samples pending per stream after everything submitted so far (the host-side mirror; exact). */
int rts_live_pending(rts_live *h, long long *pending_host /* [B] */);

/* Snapshots of single streams of a live session in chroma or chroma-difference mode, over OTW or WTW.
 * A record is the bound tracker's record in front, written and read through rts_otw_export / rts_otw_import (or the
 * WTW pair) with all their rules, and at the END of the stride the live tail: four int32 words (pending count, carry
 * flag, a magic word, max_pending), max_pending float32 samples (zeros behind the count) padded to 16 bytes, and the 12
 * doubles of the carried chroma column of difference features (zeros without a carry and in chroma mode).
 * rts_live_snapshot_bytes = the tracker's + 16 + 4 max_pending rounded up to 16 + 96.
 *   rts_live_export: asynchronous on `stream`, behind the feeds already submitted; reads the session only and does not
 * allocate.  idx_host, blob_dev, rec_stride, desc_out as for rts_otw_export.  mirror_out: int32[n][2] HOST memory, filled
 * synchronously from the session's host mirror with each stream's pending count and carry flag (no read-back): hand them
 * to the import.
 *   rts_live_import: the one synchronous call here.  `desc` is held against the session (fft_len, live_hop,
 * feature_kind, max_pending, tracker; then the tracker's own fields) and the mirror words against max_pending before
 * anything is enqueued.  Then the tracker's import is asked without writing: it fills status_dev, the call waits for it,
 * and if any record was refused it returns RTS_ERR_INVALID naming that stream, with nothing changed -- neither the
 * tracker's slots nor pending buffers, carry, mirror or published words.  Otherwise the tracker's import and the live
 * tail are enqueued, the mirror entries of those slots are set, and the call returns when they have run.  The slots'
 * words are published like after rts_live_restart: status and positions from the imported tracker state, confidence,
 * beat and tempo words empty until the next feed, consensus strikes 0, the feed number untouched.  first_host / len_host
 * as for rts_otw_import.  Unselected streams are never written.
 *   RTS_ERR_UNSUPPORTED from both: a session with a resampler (its tail and totals are not carried) or with the level
 * gate on (nor are its queue, ordinals and counters); the tracker's own refusals (after rts_otw_run, dense mirror).
 * RTS_ERR_INVALID: NULL arguments, a failed handle, wrong current device, a desc mismatch (naming the field), mirror words
 * outside [0, max_pending] / {0, 1}, and everything rts_otw_export / rts_otw_import refuse. */
int rts_live_snapshot_bytes(const rts_live *h, size_t *bytes);
int rts_live_export(rts_live *h, const int32_t *idx_host /* [n] */, int n, void *blob_dev, long long rec_stride,
                    rts_snapshot_desc *desc_out, int32_t *mirror_out /* [n][2], host */, void *stream);
int rts_live_import(rts_live *h, const int32_t *slot_host /* [n] */, int n, const void *blob_dev, long long rec_stride,
                    const rts_snapshot_desc *desc, const int32_t *mirror_host /* [n][2] */,
                    const long long *first_host /* [n] or NULL */, const int32_t *len_host /* [n] or NULL */,
                    int32_t *status_dev /* [n] */, void *stream);

/* ------------------------------------------------------------------------------------------
 * Beats and labels: ground-truth tables on the device, the live beat words, the batched accuracy metric.
 * ------------------------------------------------------------------------------------------ */
typedef struct rts_annot rts_annot;

/* What the reference does with an alignment once it has one:
 *   livenote_live.py:197-202  after every insert: (beat, label) = get_beat_and_label(ln.path[-1][1], ...) (:211-227);
 *                             `if beat: self.beat = beat`, `if mus_label: self.mus_label = mus_label` -- both sticky
 *   tests.py:59-137           test_simple.get_error: get_beat (:112-128) of every path point of a recording pair, the
 *                             squared beat error and the percentages of points off by more than 1 / 3 / 5 / 10 beats / seconds
 * The table of a piece: n >= 1 rows (time_s double, beat int32) of its ground-truth CSV (tests.py:45-57), optionally one
 * flag per row: the row's label is a non-empty string (the label strings stay with the caller).  P tables lie back to back
 * in one pool of n_rows rows, piece p being rows [first[p], first[p] + len[p]).
 *
 * Lookup of frame f >= 0 in a table (float64, the operations of get_beat in their order):
 *   time = (double)f * frame_seconds                 (frame_seconds: 2048 / 22050. in the reference, computed by the caller)
 *   i = the first row with time <= times[i]          (the reference's linear search for the first closed interval that holds
 *                                                     the time finds the same row, the times being non-decreasing)
 *   no such row:                 no beat (NaN), seg = -1
 *   i == 0 and times[0] == 0:    beat = beats[0]
 *   otherwise:                   beat = beats[i] - (times[i] - time) / (times[i] - start), start = 0.0 for i == 0, else times[i-1]
 *   seg = 0 for i == 0, else i - 1                   (the label index of livenote_live.py:221, :225)
 *
 * rts_annot_create copies the tables to the current device, to which the handle then belongs, and returns when they are
 * there; label_ok_host may be NULL (no flags: every row counts as labelled).
 *   RTS_ERR_INVALID: NULL out or table pointer, frame_seconds not finite and > 0, n_rows outside [1, 2^31), P < 1, and per
 *   piece in order, the message naming the piece and the row: len < 1, rows outside the pool, a time that is not finite, a
 *   time below the one before it, a negative beat. */
int rts_annot_create(int P, long long n_rows, const long long *first_host /* [P] */, const int32_t *len_host /* [P] */,
                     const double *times_host /* [n_rows] */, const int32_t *beats_host /* [n_rows] */,
                     const uint8_t *label_ok_host /* [n_rows] or NULL */, double frame_seconds, rts_annot **out);
int rts_annot_destroy(rts_annot *h);

/* The lookup for B streams of up to n_max frames each: entry (b, k), k < n_dev[b] (n_dev NULL: n_max; larger values are
 * clamped to n_max), is frame frames_dev[b][k] + frame0_dev[b] (frame0_dev NULL: 0) looked up in piece piece_dev[b]; beat_dev
 * [B][n_max] gets the beat, seg_dev (may be NULL) the label index.  A negative frames_dev entry or a piece outside [0, P)
 * gives NaN / -1.  Entries behind n_dev[b] are not written.  Asynchronous on `stream`; allocates nothing, does not
 * synchronise, writes only beat_dev and seg_dev.  n_max == 0 enqueues nothing.
 *   RTS_ERR_INVALID: NULL handle, frames_dev, piece_dev or beat_dev, B outside [1, 65535], n_max < 0, another device current. */
int rts_annot_beats(rts_annot *h, const int32_t *frames_dev /* [B][n_max] */, int n_max, const int32_t *n_dev /* [B] or NULL */,
                    const int32_t *piece_dev /* [B] */, const int32_t *frame0_dev /* [B] or NULL */, int B,
                    double *beat_dev /* [B][n_max] */, int32_t *seg_dev /* [B][n_max] or NULL */, void *stream);

/* The metric of tests.py:59-137 (AlignmentError.stats in evaluate.py) for B paths in one launch.  path_dev / path_len_dev
 * are laid out like the outputs of rts_dtw_paths and rts_otw_read_path: column 0 the live side (a), column 1 the reference
 * side (b).  For the points (l, r) of pair b in order: l_beat from the table of piece0_dev[b], r_beat from that of
 * piece1_dev[b]; a point is skipped when either beat is none or equal to 0.0 (`if l_beat and r_beat`); diff = |l_beat -
 * r_beat|; sq_err_dev[b] is the sum of diff * diff in path order, one float64 addition after the other, bit for bit the
 * Python loop's; seconds_off = |get_time(r_beat) - get_time(l_beat)| with get_time(x) read off the table of piece0 (the
 * live side, for both beats: tests.py:130-137): whole = (int)x toward zero, sec = times[whole], and if whole + 1 < n, sec +=
 * (x mod 1) * (times[whole + 1] - times[whole]), x mod 1 taking the sign of the divisor like Python's %.
 * counts_dev[b] = { count of points that passed the skip rule, points with diff > 1, 3, 5, 10, points with seconds_off > 1,
 * 3, 5, 10, index_errors }.  Deviation from the reference: a point one of whose `whole` is < 0 or >= n is counted in
 * index_errors and in nothing else, the sum included (the reference raises IndexError for >= n and wraps round through
 * Python's negative indexing at a beat of exactly -1.0).
 * One workgroup per pair loops over the path; path_len <= 0 (the -1 fault marker of rts_dtw_paths included) gives zeros,
 * larger than P_max is clamped to it.  A piece outside [0, P) has no beats.  Asynchronous, allocates nothing, does not
 * synchronise, writes only sq_err_dev and counts_dev.
 *   RTS_ERR_INVALID: NULL handle or table pointer, path_dev NULL with P_max > 0, P_max < 0, B < 1, another device current. */
#define RTS_ANNOT_COUNTS 10
int rts_annot_path_error(rts_annot *h, const int32_t *path_dev /* [B][P_max][2] */, int P_max,
                         const int32_t *path_len_dev /* [B] */, const int32_t *piece0_dev /* [B] */,
                         const int32_t *piece1_dev /* [B] */, int B, double *sq_err_dev /* [B] */,
                         int32_t *counts_dev /* [B][RTS_ANNOT_COUNTS] */, void *stream);

/* Beat and label of every microphone without a read-back: the last step of livenote_live.py's loop (:197-202).
 * rts_live_annotate(h, annot, mask, piece, frame0): annot NULL switches annotations off (the other arguments are ignored and
 * the words stay as they are).  Otherwise `annot` -- held by reference, it must outlive the handle or the next
 * rts_live_annotate -- becomes the handle's tables, and every stream with mask_host[b] != 0 gets piece_host[b] (in [0, P)) and
 * frame0_host[b] (>= 0; frame0_host NULL: 0), the frame of its piece at which its reference range starts: after a restart
 * onto a range that starts inside a piece the path's indices are relative to the range.  A stream that was never selected has
 * no piece.  The host tables are consumed when the call returns; the change is ordered on `stream` behind the feeds already
 * submitted, like rts_live_restart.  Allowed at any time.  The first call with tables allocates a fourth host-mapped block
 * (NaN / -1 / -1 for every stream) and two [B] device tables.
 * With annotations on, every rts_live_submit enqueues ONE more launch, after the tracker push (and the watch launch) and
 * before the publication of the status words, in a feed without columns too.  Per stream it takes the reference index of
 * the last stored point of the tracker's path, as rts_otw_read_path / rts_wtw_read_path would return it (ln.path[-1][1]),
 * looks frame0 + that index up in the stream's piece and updates the block:
 *   beat[b]       changes iff the new beat is not none and != 0.0      (`if beat:`)
 *   label[b]      the label index seg; changes iff seg >= 0 and the flag of row seg is set (no flags: always)   (`if mus_label:`)
 *   ref_frame[b]  the frame of the piece just looked up, or -1 while the stream has no path point.
 * rts_live_restart republishes NaN / -1 / -1 for the selected streams, rts_live_reset for all; both keep pieces and offsets.
 * Either tracker, either feature kind, with the gate and on resampling handles.  With annotations off, or never switched
 * on, a feed enqueues exactly what it enqueues without this function.
 * rts_live_beats: the non-blocking look, like rts_live_confidence and with the same guarantee: when *feeds_done >= k, every
 * word read reflects a feed >= k.  Any output pointer may be NULL.
 *   RTS_ERR_INVALID: NULL handle; with tables: NULL mask_host or piece_host, a selected stream's piece outside [0, P) or
 *   negative frame0, tables of another device, a failed handle; rts_live_beats before the first rts_live_annotate with tables. */
int rts_live_annotate(rts_live *h, rts_annot *annot, const uint8_t *mask_host /* [B] */, const int32_t *piece_host /* [B] */,
                      const int32_t *frame0_host /* [B] or NULL */, void *stream);
int rts_live_beats(rts_live *h, double *beat /* [B] */, int32_t *label /* [B] */, int32_t *ref_frame /* [B] */, int *feeds_done);

/* ------------------------------------------------------------------------------------------
 * Tempo: the slope of a path over a trailing window, for offline paths, trackers and live feeds.
 * ------------------------------------------------------------------------------------------ */
/* The engine says where a performer is; this says how fast.  The reference's live loop prints the wall-clock frame next to
 * ln.path[-1] after every insert (livenote_live.py:203-206) and leaves the comparison to the operator.
 *
 * A path is n_pts stored points (x_k, y_k) = (live, reference) of int32.  The window at point i with length K is the points
 * p0 = max(0, i - K + 1) .. i, n = i - p0 + 1 of them.  A point is bad when x is outside [0, x_limit) or y outside
 * [0, y_limit); a window that contains a bad point has slope = pos = NaN.  Otherwise, all sums exact integers:
 *   Sx = sum x, Sy = sum y, Sxx = sum x^2, Sxy = sum x y over the window
 *   den = n Sxx - Sx^2, num = n Sxy - Sx Sy            (translation invariant)
 *   slope = den > 0 ? (double)num / (double)den : NaN    (two int64 -> float64 conversions, round to nearest even, one
 *                                                         division; den == 0: n < 2, or the live index never moves)
 *   Sx' = Sx - n x_i, Sy' = Sy - n y_i                   (relative to the newest point)
 *   pos = ((double)y_i + ((double)Sy' - slope * (double)Sx') / (double)n) + slope * ahead
 * every operation rounded on its own, in this order: the regression line read at the newest live frame plus `ahead` frames.
 * NaN is the canonical quiet NaN 0x7ff8000000000000.  The windows are trailing, so entry i of a curve is what a live
 * tracker would have published when point i was its newest.  2 <= K <= 1024; `ahead` finite.
 * The results are exact while num and den fit in int64; K^2 * x_limit * y_limit >= 2^63 is refused (RTS_ERR_UNSUPPORTED) on
 * the host, from the limits alone.
 *
 * rts_path_tempo: the curve of B paths laid out like the outputs of rts_dtw_paths and rts_otw_read_path.  slope_dev[b][i]
 * and pos_dev[b][i] (pos_dev may be NULL) for i < len_dev[b]; entries behind are not written; len <= 0 (the -1 fault marker
 * of rts_dtw_paths included) writes nothing, len > P_max is clamped.  One workgroup per path.  Asynchronous on `stream`;
 * allocates nothing, does not synchronise, writes only the two outputs.  P_max == 0 enqueues nothing.
 *   RTS_ERR_INVALID: NULL len_dev or slope_dev, path_dev NULL with P_max > 0, P_max < 0, B < 1, K outside [2, 1024], `ahead`
 *   not finite, a limit < 1. */
int rts_path_tempo(const int32_t *path_dev /* [B][P_max][2] */, int P_max, const int32_t *len_dev /* [B] */, int B, int K,
                   double ahead, long long x_limit, long long y_limit, double *slope_dev /* [B][P_max] */,
                   double *pos_dev /* [B][P_max] or NULL */, void *stream);

/* The window over the last n = min(K, stored points) points of every stream's own path, as rts_otw_read_path /
 * rts_wtw_read_path would return it (the stored count clamped to the path's capacity): slope_dev[b], pos_dev[b] (may be
 * NULL) and n_dev[b], the window length used -- 0 for a fresh or just-restarted stream, whose outputs are NaN.  Limits:
 * x_limit = 2 N_b, y_limit = N_b, N_b the length of the stream's own reference (per-stream references included); for WTW
 * that is the stream's live capacity 2 M_b and its reference length M_b.  Reads the handle only; one launch, asynchronous.
 *   RTS_ERR_INVALID: NULL handle, slope_dev or n_dev, K outside [2, 1024], `ahead` not finite, another device current.
 *   RTS_ERR_UNSUPPORTED: the overflow rule with the handle's longest reference. */
int rts_otw_tempo(rts_otw *h, int K, double ahead, double *slope_dev /* [B] */, double *pos_dev /* [B] or NULL */,
                  int32_t *n_dev /* [B] */, void *stream);
int rts_wtw_tempo(rts_wtw *h, int K, double ahead, double *slope_dev /* [B] */, double *pos_dev /* [B] or NULL */,
                  int32_t *n_dev /* [B] */, void *stream);

/* Slope to beats per minute through the annotation tables, conventions as rts_annot_beats: entry (b, k), k < n_dev[b], is
 * frame frames_dev[b][k] + frame0_dev[b] of piece piece_dev[b] with slope slope_dev[b][k] (reference frames per live frame).
 * With i, start, times[i] what the lookup of that frame uses: bpm = (slope * 60.0) / (times[i] - start), one beat per table
 * segment like get_beat.  NaN: no row, i == 0 and times[0] == 0, times[i] == start, a NaN slope, a negative frames_dev entry,
 * a piece outside [0, P).  Entries behind n_dev[b] are not written.  Asynchronous, allocates nothing, writes only bpm_dev.
 *   RTS_ERR_INVALID: NULL handle, frames_dev, slope_dev, piece_dev or bpm_dev, B outside [1, 65535], n_max < 0, another
 *   device current. */
int rts_annot_bpm(rts_annot *h, const int32_t *frames_dev /* [B][n_max] */, const double *slope_dev /* [B][n_max] */, int n_max,
                  const int32_t *n_dev /* [B] or NULL */, const int32_t *piece_dev /* [B] */,
                  const int32_t *frame0_dev /* [B] or NULL */, int B, double *bpm_dev /* [B][n_max] */, void *stream);

/* Tempo of every microphone without a read-back.  rts_live_follow_tempo(h, K, ahead): K = 0 switches it off (the words stay
 * as they are), 2 <= K <= 1024 on.  The first call with K > 0 allocates a fifth host-mapped block, double slope[B], pos[B],
 * bpm[B] then int32 n[B], NaN / NaN / NaN / 0 for every stream.  With it on, every rts_live_submit enqueues ONE more launch,
 * after the tracker push, the watch launch and the beat launch and before the publication of the status words, in a feed
 * without columns too: rts_otw_tempo / rts_wtw_tempo of the bound tracker into that block, and bpm[b] by the rule of
 * rts_annot_bpm from the stream's piece and frame0 as rts_live_annotate set them, at frame0 + the last stored point's
 * reference index -- the frame rts_live_beats reports; NaN while annotations are off or the stream has no piece.  With the
 * gate on (rts_live_gate) live indices count the columns the tracker received, so the slope is in reference frames per
 * column handed on; rts_live_gate_columns maps them back.  rts_live_restart republishes NaN / NaN / NaN / 0 for the selected
 * streams, rts_live_reset for all.  A handle that never calls it enqueues exactly what it enqueues without this function.
 * rts_live_tempo: the non-blocking look, like rts_live_confidence and with the same guarantee: when *feeds_done >= k, every
 * word read reflects a feed >= k.  Any output pointer may be NULL.
 *   RTS_ERR_INVALID: NULL handle, a failed handle, K outside {0} and [2, 1024], `ahead` not finite, another device current;
 *   rts_live_tempo before the first rts_live_follow_tempo(K > 0).  RTS_ERR_UNSUPPORTED: the overflow rule. */
int rts_live_follow_tempo(rts_live *h, int K, double ahead);
int rts_live_tempo(rts_live *h, double *slope /* [B] */, double *pos /* [B] */, double *bpm /* [B] */, int32_t *n /* [B] */,
                   int *feeds_done);

/* ------------------------------------------------------------------------------------------
 * Tuning: the offset of a source from A4 = 440 Hz, estimated on the device from its STFT.
 * ------------------------------------------------------------------------------------------ */
/* The chroma filterbank handed to rts_chroma_create is built for one A4; the reference builds it for 440 Hz and leaves the
 * rest open (chroma.py:24, "# TODO: check additions (tuning, normalization, etc.)").  A source that is off by a quarter tone
 * smears every partial over two chroma bins.  This estimates the offset without taking the STFT to the host: a histogram of
 * the spectral peaks' distances from the nearest equal-tempered pitch, R bins to the semitone, and a pick from it.  The
 * filterbank for the offset found is the caller's to build (filters.chroma_filterbank(a440=filters.tuning_a440(cents))).
 *
 * Input: the complex STFT rts_chroma_frames writes into stft_out_dev, [n_frames][fft_len/2+1] pairs of doubles (re, im).
 * Every float64 operation below is rounded on its own, in the order written; sqrt and / are the correctly rounded ones.
 * Per frame m:
 *   P[k] = re*re + im*im                for every bin (two products, one sum)
 *   Pmax = max_k P[k],  lim = thr_pow * Pmax
 *   bin k in [k_lo, k_hi] is a peak when P[k] > P[k-1] and P[k] >= P[k+1] and P[k] >= lim   (an all-zero frame has none)
 * and for a peak:
 *   a = sqrt(P[k-1]), b = sqrt(P[k]), c = sqrt(P[k+1])
 *   avg = 0.5*(c - a),  sh = (2.0*b - c) - a,  d = sh > 0 ? avg/sh : 0.0
 *   f = ((double)k + d) * bin_hz
 *   n = the largest index with E[n] <= f in the handle's ascending edge table E[0 .. n_edges)      (binary search)
 *   dropped when there is no such n or n >= n_edges - 1; otherwise hist[seg[m]][n mod R] += 1.
 * NaN input leaves the counts undefined; every index stays bounded.  The table is the host's (filters.tuning_edges):
 * E[n] = 440 * 2^((s_lo - 0.5 + n/R)/12), so histogram bin i holds offsets in [-50 + 100 i/R, -50 + 100 (i+1)/R) cents and
 * the device takes no logarithm -- which is what lets the histogram equal a serial restatement bit for bit.
 *
 * rts_tuning_create validates on the host, before any device call:
 *   RTS_ERR_UNSUPPORTED: fft_len not a power of two in [64, 8192]; R > 1024.
 *   RTS_ERR_INVALID: not 1 <= k_lo <= k_hi <= fft_len/2 - 1; R < 1; n_edges < 2; NULL edges_host or out; an edge that is
 *   not finite, positive and above the one before it; thr_pow outside [0, 1]; bin_hz not finite and > 0.
 * The handle belongs to the device that is current at create; rts_tuning_destroy(NULL) is RTS_OK.
 *
 * rts_tuning_accumulate ADDS the counts of n_frames frames to hist_dev [S][R] uint64 and never clears it: frame m goes to
 * row seg_dev[m] (int32; a value outside [0, S) drops the frame), every frame to row 0 when seg_dev is NULL.  Counts are
 * integers, so calls over any split of the frames give the same histogram.  One launch of persistent workgroups, each
 * owning a contiguous range of frames and adding to hist_dev only when its segment changes and at its end.  Asynchronous
 * on `stream`; allocates nothing, does not synchronise, writes only hist_dev.  n_frames == 0 enqueues nothing.
 *   RTS_ERR_INVALID: NULL handle; n_frames < 0; S < 1; with n_frames > 0: NULL stft_dev or hist_dev, stft_dev not 16-byte
 *   aligned, another device current.
 *
 * rts_tuning_pick: per row s of hist_dev, N = sum hist[s]; N == 0 gives cents 0.0 and n 0.  Otherwise, all integers,
 *   score[i] = sum_{d=-W..W} (W + 1 - |d|) * hist[s][(i + d) mod R]       (circular: -50 and +49 cents are neighbours)
 *   i* = the first maximum of score
 *   cents_dev[s] = ((double)i* + 0.5) * 100.0 / (double)R - 50.0,  n_dev[s] = N.
 * One workgroup per row; asynchronous, allocates nothing, writes only the two outputs.
 *   RTS_ERR_INVALID: NULL handle, hist_dev, cents_dev or n_dev; S < 1; W < 0 or 2 W + 1 > R; another device current. */
typedef struct rts_tuning rts_tuning;
int rts_tuning_create(int fft_len, int k_lo, int k_hi, int R, int n_edges, const double *edges_host /* [n_edges] */,
                      double bin_hz, double thr_pow, rts_tuning **out);
int rts_tuning_destroy(rts_tuning *p);
int rts_tuning_accumulate(rts_tuning *p, const double *stft_dev /* [n_frames][fft_len/2+1][2] */, long long n_frames,
                          const int32_t *seg_dev /* [n_frames] or NULL */, int S, unsigned long long *hist_dev /* [S][R] */,
                          void *stream);
int rts_tuning_pick(rts_tuning *p, const unsigned long long *hist_dev /* [S][R] */, int S, int W, double *cents_dev /* [S] */,
                    long long *n_dev /* [S] */, void *stream);

/* ------------------------------------------------------------------------------------------
 * Ensemble following: one microphone against several recordings of its piece, fused in beats.
 * ------------------------------------------------------------------------------------------ */
/* Every answer of a stream depends on its one recording resembling tonight's performance.  The reference ships two or three
 * performances of almost every piece, each with its own beat table, and its harness compares performances in beats, the
 * scale the recordings share (tests.py:59-137).  Here a microphone is followed against all recordings of its piece at once
 * (one stream each, a "group"), the group's position is the median beat of its members, and a member that loses its place is
 * outvoted, marked, and can be restarted where the others are (Arzt and Widmer, "Real-time music tracking using multiple
 * performances as a reference", ISMIR 2015).
 *
 * Every float64 operation below is rounded on its own, in the order written.  NaN is the canonical quiet NaN
 * 0x7ff8000000000000.
 *
 * Inverse lookup, beat x -> frame of piece p with rows (times[i], beats[i]), n of them (rts_annot_frames).  A piece is
 * invertible when its beats are strictly increasing; rts_annot_create decides that once per piece.
 *   x is NaN, p outside [0, P), p not invertible:                                   frame = -1
 *   i = the first row with x <= (double)beats[i] (bisection); none:                   frame = -1
 *   x < (double)beats[i] - 1.0:                                                       frame = -1   (a gap of the table, or
 *                                                         before the stretch get_beat interpolates from time zero)
 *   end = times[i], start = i == 0 ? 0.0 : times[i-1]
 *   time = end - ((double)beats[i] - x) * (end - start)
 *   f = floor(time / frame_seconds + 0.5);  f < 0: frame = 0;  f > INT32_MAX: frame = -1;  else frame = f
 * With floor(. + 0.5) the round trip frame -> get_beat -> frame is the identity on every frame that has a beat, in the
 * reference's 22 tables (Songs/) as in the two under tests/golden/.  rts_annot_frames has the geometry and conventions of
 * rts_annot_beats: entry (b, k), k < n_dev[b] (NULL: n_max; clamped to n_max), is beats_dev[b][k] in piece piece_dev[b];
 * entries behind n_dev[b] are not written.  Asynchronous, allocates nothing, writes only frame_dev.  n_max == 0 enqueues
 * nothing.
 *   RTS_ERR_INVALID: NULL handle, beats_dev, piece_dev or frame_dev, B outside [1, 65535], n_max < 0, another device current.
 *
 * Member beat.  Member b is stream b of a tracker with piece[b] and frame0[b] as rts_live_annotate takes them: the lookup of
 * rts_annot_beats of frame0[b] + y_last, y_last the reference index of the last stored path point (ln.path[-1][1],
 * livenote_live.py:197).  NaN while the stream has no path point, y_last < 0, or the stream has no piece.  Not sticky; a
 * beat of 0.0 is a position, only NaN is "none".
 *
 * Fusion step, once per group and step.  A group has 1 to 64 members in ascending stream order; parameters max_dev (beats,
 * > 0, +inf allowed) and patience in [1, 65535]; every member carries strikes and out, 0 when fresh.
 *   1. valid_i: beta_i is not NaN.
 *   2. in_i = valid_i && !out_i; when no member is in: in_i = valid_i (everyone valid is heard again).
 *   3. n_in == 0: consensus = spread = NaN, every dev_i = NaN, strikes and out unchanged; the step ends.
 *   4. v = the in-set sorted ascending by (value, member index), `<` on float64 (-0.0 and 0.0 tie, the index decides):
 *      consensus = n odd ? v[(n-1)/2] : (v[n/2-1] + v[n/2]) * 0.5;  spread = v[n-1] - v[0].
 *   5. every valid member: dev_i = beta_i - consensus; fabs(dev_i) > max_dev ? strikes_i = min(strikes_i + 1, patience)
 *      : strikes_i = 0;  out_i = strikes_i >= patience.  An invalid member: dev_i = NaN, strikes and out unchanged.
 * Published per group: consensus, spread, n_in, n_valid; per stream: dev, strikes, out.  A stream in no group reads NaN / 0 / 0.
 *
 * rts_ensemble_create: group_host[b] in [-1, n_groups) is stream b's group (-1: none).  Builds the CSR tables and the [B]
 * strikes / out state (zero) on the current device, to which the handle then belongs.
 *   RTS_ERR_INVALID, the message naming the argument: NULL out or group_host, B < 1, n_groups outside [1, B], max_dev NaN or
 *   <= 0, patience outside [1, 65535], an entry outside [-1, n_groups), a group without a member or with more than 64.
 * rts_ensemble_reset clears strikes and out of the streams with mask_host[b] != 0 (NULL: all), ordered on `stream`; the
 * mask travels by value and is consumed when the call returns.
 *
 * rts_otw_consensus / rts_wtw_consensus: one fusion step over every group from the tracker's paths as they stand, one
 * launch of one wave per group (ranks by counting across the wave, no LDS, no atomics).  group_dev = consensus[n_groups] then
 * spread[n_groups]; group_n_dev = n_in[n_groups] then n_valid[n_groups]; dev_dev[B]; member_dev = strikes[B] then out[B].
 * frame0_dev NULL: 0.  Advances the ensemble's state and writes the five outputs, nothing else; asynchronous, allocates
 * nothing.
 *   RTS_ERR_INVALID: a NULL handle, tables or output; B of the ensemble != B of the tracker; a handle on another device.
 *
 * rts_path_consensus, the offline curve over live frames t = 0 .. T-1 of B paths laid out like the outputs of rts_dtw_paths
 * (len <= 0 gives an empty path, len > P_max is clamped; the live index must not decrease along a path): at frame t member
 * b stands at the y of its last point k with x_k <= t (none, or y < 0: invalid at t); beta by the member-beat rule; the
 * fusion step runs with state that is zero at t = 0 and carries from t to t + 1 -- private state: the handle's own is
 * neither read nor written, only its groups and parameters are used.  With max_dev = +inf this is the plain median per
 * frame.  consensus_dev[g][t]; spread_dev, n_in_dev (same shape) and out_dev[b][t], out of stream b after step t (0 for a
 * stream in no group), may be NULL.  One wave per group, a cursor per lane: O(len + T) per member.  T == 0 enqueues nothing.
 *   RTS_ERR_INVALID: a NULL handle, tables, len_dev, piece_dev or consensus_dev; path_dev NULL with P_max > 0; P_max < 0;
 *   T < 0; a handle on another device.
 *
 * Live.  rts_live_follow_consensus(h, e): e NULL switches it off (the words stay as they are).  Otherwise `e` -- held by
 * reference like the tables of rts_live_annotate -- becomes the handle's ensemble; the first call allocates a sixth
 * host-mapped block.  With it on, every rts_live_submit enqueues ONE more launch, after the beat and tempo launches and
 * before the publication of the status words, in a feed without columns too: the fusion step of rts_otw_consensus /
 * rts_wtw_consensus with piece and frame0 as rts_live_annotate set them.  While annotations are switched off the launch is
 * skipped and the words stay.  rts_live_restart clears strikes and out of the selected streams and republishes NaN / 0 / 0
 * for them; rts_live_reset does so for all and publishes NaN / NaN / 0 / 0 per group.  A handle that never calls it enqueues
 * exactly what it enqueues without this function.
 * rts_live_consensus: the non-blocking look, like rts_live_confidence and with the same guarantee: when *feeds_done >= k,
 * every word read reflects a feed >= k.  Group outputs have n_groups entries of the ensemble bound last.  Any output pointer
 * may be NULL.
 *   RTS_ERR_INVALID: NULL handle, a failed handle, B of the ensemble != B of the handle, an ensemble of another device,
 *   rts_live_follow_consensus before any rts_live_annotate with tables; rts_live_consensus before the first
 *   rts_live_follow_consensus with an ensemble. */
typedef struct rts_ensemble rts_ensemble;
int rts_ensemble_create(int B, const int32_t *group_host /* [B] */, int n_groups, double max_dev, int patience, rts_ensemble **out);
int rts_ensemble_destroy(rts_ensemble *h);
int rts_ensemble_reset(rts_ensemble *h, const uint8_t *mask_host /* [B], NULL: all */, void *stream);
int rts_annot_frames(rts_annot *h, const double *beats_dev /* [B][n_max] */, int n_max, const int32_t *n_dev /* [B] or NULL */,
                     const int32_t *piece_dev /* [B] */, int B, int32_t *frame_dev /* [B][n_max] */, void *stream);
int rts_otw_consensus(rts_otw *h, rts_ensemble *e, rts_annot *a, const int32_t *piece_dev /* [B] */,
                      const int32_t *frame0_dev /* [B] or NULL */, double *group_dev /* [2][n_groups] */,
                      int32_t *group_n_dev /* [2][n_groups] */, double *dev_dev /* [B] */, int32_t *member_dev /* [2][B] */,
                      void *stream);
int rts_wtw_consensus(rts_wtw *h, rts_ensemble *e, rts_annot *a, const int32_t *piece_dev /* [B] */,
                      const int32_t *frame0_dev /* [B] or NULL */, double *group_dev /* [2][n_groups] */,
                      int32_t *group_n_dev /* [2][n_groups] */, double *dev_dev /* [B] */, int32_t *member_dev /* [2][B] */,
                      void *stream);
int rts_path_consensus(rts_ensemble *e, rts_annot *a, const int32_t *path_dev /* [B][P_max][2] */, int P_max,
                       const int32_t *len_dev /* [B] */, const int32_t *piece_dev /* [B] */,
                       const int32_t *frame0_dev /* [B] or NULL */, int T, double *consensus_dev /* [n_groups][T] */,
                       double *spread_dev /* [n_groups][T] or NULL */, int32_t *n_in_dev /* [n_groups][T] or NULL */,
                       int32_t *out_dev /* [B][T] or NULL */, void *stream);
int rts_live_follow_consensus(rts_live *h, rts_ensemble *e /* NULL: off */);
int rts_live_consensus(rts_live *h, double *consensus, double *spread, int32_t *n_in, int32_t *n_valid /* [n_groups] */,
                       double *dev, int32_t *strikes, int32_t *out /* [B] */, int *feeds_done);

/* ------------------------------------------------------------------------------------------
 * Render: one recording on another's time axis, along an alignment path.
 * ------------------------------------------------------------------------------------------ */
/* The reference stops at the path (its harness takes error statistics of it, tests.py:59-137); nothing in it plays a
 * recording along one, so no reference interface is replaced here.  This is time-scale modification by waveform-similarity overlap-add (WSOLA; Verhelst and Roelands,
 * ICASSP 1993) along a piecewise-linear integer time map, defined by this project to the bit like the resampler above.
 *
 * Plan.  Frames of N samples (N % 16 == 0, 64 <= N <= 4096) at a hop of H = N / 2, a search tolerance of delta samples
 * (0 <= delta <= 1024) and a window w[0 .. N) of host doubles (filters.hann_window_periodic(N): w[m] + w[m + H] = 1, so
 * the identity map gives the input back).  Input samples x[n] are float32, or PCM16 scaled by 1/32768 exactly as
 * rts_resample_run scales it; x[n] = 0 for n < 0 and for n >= n_in.
 *
 * Time map of a stream: A >= 2 anchors (out_pos[s], in_pos[s]), int64 pairs, out_pos[0] = 0, out_pos strictly increasing,
 * in_pos not decreasing, every segment shorter than 2^31 on both axes and every position below 2^62 in magnitude.  Block k
 * begins at output position t = k H; with s the last anchor with out_pos[s] <= t, at most A - 2,
 *   a_k = in_pos[s] + floor((t - out_pos[s]) * (in_pos[s+1] - in_pos[s]) / (out_pos[s+1] - out_pos[s]))
 * in exact 64-bit integer arithmetic.  (A block that begins at or behind the last anchor continues the last segment; n_out
 * may then lie at most 2^31 behind out_pos[A-2].)
 *
 * Frame positions.  p_0 = a_0.  For k >= 1 the frame is sought near a_k so that it continues the frame before it: with the
 * target x[p_{k-1} + H + n], n = 0 .. N-1, candidate delta in [-delta, delta] scores
 *   c(delta) = ((s_0 + s_1) + (s_2 + s_3)) + ((s_4 + s_5) + (s_6 + s_7))
 *   s_r      = sum over q = 0 .. N/8 - 1, q ascending, from 0.0, of (double)x[a_k + delta + 8 q + r] * (double)x[p_{k-1} + H + 8 q + r]
 * (the products are exact in float64, every add rounds once).  The winner is the first maximum in the order delta = 0,
 * -delta, -delta + 1, .., delta: a candidate replaces the best so far only when it is strictly greater, so a NaN score never
 * wins, a NaN score at 0 keeps 0, and digital silence gives 0.  p_k = a_k + the winner.
 *
 * Output, block k, m = 0 .. H-1:
 *   y[k H + m] = (float)( w[m + H] * (double)x[p_{k-1} + H + m]  +  w[m] * (double)x[p_k + m] )
 * each product one float64 multiply, one float64 add of the two (the earlier frame's product first, no fused multiply-add),
 * one rounding to float32.  Block 0 has the single term (float)(w[m] * (double)x[p_0 + m]).  rts_warp_blocks(n_out, N) =
 * ceil(n_out / H) blocks exist; samples at or behind n_out are not written.
 *
 * State of a stream: (k, p_{k-1}), two int64, zeros before the first block.  Nothing else is carried: rendering blocks
 * [0, k1) and then [k1, K) gives the bits of one run. */
typedef struct rts_warp rts_warp;

/* per-stream status words: rts_warp_anchors writes the first six (a sum of them), rts_warp_run the last three */
#define RTS_WARP_PATH_EMPTY 1      /* path_len < 1 */
#define RTS_WARP_PATH_START 2      /* the path does not begin at u = 0 */
#define RTS_WARP_PATH_BACKWARD 4   /* u or v steps backwards (or v begins below 0) */
#define RTS_WARP_PATH_SHORT_OUT 8  /* n_out <= the last u * hop_f */
#define RTS_WARP_PATH_SHORT_IN 16  /* n_in < the last v * hop_f */
#define RTS_WARP_PATH_TOO_MANY 32  /* more anchors than A_max */
#define RTS_WARP_NO_MAP 64         /* n_anchor outside [2, A_max]: rts_warp_anchors refused the path */
#define RTS_WARP_BAD_MAP 128       /* the anchors break a rule of the time map */
#define RTS_WARP_BAD_STATE 256     /* n_out < 0 or >= 2^62, k < 0 or > rts_warp_blocks(n_out), |p| >= 2^62 */

/* ceil(n_out / (N / 2)); 0 for n_out <= 0; -1 for an N that rts_warp_create does not take.  Pure host arithmetic. */
long long rts_warp_blocks(long long n_out, int N);
/* The plan: the window on the current device, to which the plan then belongs.  window_host: N doubles.
 * RTS_ERR_INVALID, naming the argument, before any GPU call: NULL out or window_host, N odd or < 2, delta < 0.
 * RTS_ERR_UNSUPPORTED: N not a multiple of 16 or outside [64, 4096] (48 and 4112 are refused), delta > 1024. */
int rts_warp_create(int N, int delta, const double *window_host, rts_warp **out);
int rts_warp_destroy(rts_warp *plan);
/* Time maps from monotone paths, on the device: path_dev int32 [B][P_max][2] and path_len_dev int32 [B] as rts_dtw_paths
 * writes them (a length above P_max is clamped to it).  With u = path[t][onto], v = path[t][1 - onto] -- `onto` in {0, 1}
 * is the column whose time axis the output gets -- every t with t == 0 or u_t != u_{t-1} gives the anchor (u_t * hop_f,
 * v_t * hop_f), hop_f the samples per feature frame; the closing anchor (n_out_dev[b], n_in_dev[b]) (int64 [B] each, the
 * output and input sample counts) follows.  anchors_dev int64 [B][A_max][2], n_anchor_dev int32 [B], status_dev int32 [B].
 * A stream with any of path_len < 1, u_0 != 0, a step backwards in u or v, n_out <= the last u * hop_f, n_in < the last
 * v * hop_f or more than A_max anchors gets the sum of the RTS_WARP_PATH_* words as its status and n_anchor 0 (its row of
 * anchors_dev is then undefined within its A_max entries); every other stream status 0.  One workgroup per path: flags, a
 * workgroup prefix sum, a scatter.  Asynchronous on `stream`; no allocation, no synchronisation (graph-capturable).
 *   RTS_ERR_INVALID, naming the argument, before any GPU call: a NULL pointer (path_dev may be NULL when P_max == 0),
 *   P_max < 0, onto outside {0, 1}, hop_f < 1, B outside [1, 65535], A_max < 2. */
int rts_warp_anchors(const int32_t *path_dev, int P_max, const int32_t *path_len_dev, int onto, int hop_f,
                     const long long *n_out_dev, const long long *n_in_dev, int B, long long *anchors_dev, int A_max,
                     int32_t *n_anchor_dev, int32_t *status_dev, void *stream);
/* Renders up to k_count further blocks of each of B streams, beginning at the stream's own k = state_dev[b][0]:
 * samples_dev is [B][sample_stride] of sample_dtype (RTS_F32 | RTS_I16) with n_in_dev[b] (int64) samples in stream b,
 * anchors_dev / n_anchor_dev / A_max as rts_warp_anchors leaves them (or made by the caller), n_out_dev int64 [B].  Block k
 * is written to out_dev[b][(k - k_start) * H ..], k_start the stream's k when the call began -- relative to the call, so
 * that a caller streams into a chunk buffer of k_count * H samples per stream however far the stream has come; out_dev
 * float32 [B][out_stride].  Rows that begin on a 16-byte boundary are written with 16-byte stores.  state_dev int64 [B][2]
 * moves on to (min(k + k_count, K), p of the last block rendered).  A stream whose n_anchor is outside [2, A_max], whose
 * anchors break a rule of the map, or whose state is impossible gets RTS_WARP_NO_MAP / RTS_WARP_BAD_MAP /
 * RTS_WARP_BAD_STATE in status_dev[b]: nothing is written for it and its state stays; every other stream status 0.  One
 * workgroup per stream walks its blocks in order.  Asynchronous on `stream`; no allocation, no synchronisation
 * (graph-capturable).
 *   RTS_ERR_INVALID, naming the argument, before any GPU call: a NULL plan or pointer (out_dev may be NULL when k_count ==
 *   0), sample_dtype, sample_stride < 0, A_max < 2, k_count < 0, out_stride < 0, B outside [1, 65535], a plan of another
 *   device. */
int rts_warp_run(rts_warp *plan, const void *samples_dev, int sample_dtype, long long sample_stride,
                 const long long *n_in_dev, const long long *anchors_dev, const int32_t *n_anchor_dev, int A_max,
                 const long long *n_out_dev, long long *state_dev /* [B][2]: k, p_prev */, long long k_count,
                 float *out_dev, long long out_stride, int32_t *status_dev, int B, void *stream);

/* ------------------------------------------------------------------------------------------
 * Live accompaniment: a track rendered along every tracker, feed by feed.
 * ------------------------------------------------------------------------------------------ */
/* Playing a track so that it follows the musician at the microphone is what a score follower is for.  With it on, every
 * rts_live_submit turns the tail of each armed stream's path into the next anchor of that stream's time map (the steering
 * law below) and renders the blocks that have become due with rts_warp_run, in the feed's own chain, into host-mapped
 * memory: nothing is read back and nothing synchronises.  The reference has nothing of the kind; the law is this
 * project's, to the bit (tests/accomp_model.py restates it).
 *
 * Parameters of a session (rts_accomp_params, with the two plans):
 *   N, H = N / 2    the warp plan's frame and hop; `hop`: the chroma plan's hop, microphone samples per live frame
 *   hop_track       track samples per reference frame, 1 .. 65536
 *   K               points of the regression window, 2 .. 1024 (the range of rts_otw_tempo)
 *   glide  G        samples over which a correction is spread, 0 <= G < 2^31
 *   lead            signed, |lead| < 2^31: what the output path adds between a sample leaving here and sounding, plus the
 *                   offset between a live index and the microphone sample its frame is centred on
 *   rate_min_pm, rate_max_pm   limits of the rate in track samples per 1000 output samples at equal hops,
 *                   0 <= min <= max <= 4000, max >= 1
 *   chunk_blocks    the most blocks rendered per feed and stream, >= 1
 *   A_max           anchors per stream, >= 2
 * The track pool tracks_dev (RTS_F32 | RTS_I16) is one run of samples that stays the caller's, like references; stream b's
 * track is its samples [first_b, first_b + len_b), and origin_b -- origin_host[b], or 0 -- is the track sample, counted
 * from first_b, that belongs to reference frame 0 of the range the stream's tracker follows.  All positions of a stream's
 * map are pool samples: x[n] = 0 for n >= first_b + len_b and for n < 0, and a frame or a search window that reaches in
 * front of first_b reads the pool there (leave N + delta samples of silence between tracks that must not meet).
 *
 * State of stream b on the device: fed (samples the append has taken since the stream was armed), base (-1: waiting), the
 * renderer's (k, p_prev), the anchors and their count, n_out.  Arming sets fed = 0, base = -1, the state zero, the one
 * anchor (0, first_b + origin_b), n_out = 0.
 *
 * Steering, once per feed and armed stream, behind the tracker's push; every integer exact int64, every float64
 * operation rounded on its own:
 *   1. fed_prev = fed; fed += n_b, the samples the feed's append took for the stream.
 *   2. base < 0: a tracker that has stored no path point leaves the stream waiting -- status WAIT, no block.  Otherwise
 *      base = fed_prev: output sample t sounds at microphone sample base + t, the clock starting with the feed that
 *      produced the first point.
 *   3. k_due = min((fed - base) / H, k + chunk_blocks), LATE when the min cut it.  k_due == k: no block.  Otherwise, with
 *      A_max anchors stored: status FULL, no block.
 *   4. (o0, i0) the last anchor (o0 == k H); o1 = k_due H; Ls = o1 - o0.
 *   5. lo = (Ls hop_track rate_min_pm) / (hop 1000), hi the same with rate_max_pm, nominal = (Ls hop_track) / hop.
 *   6. slope and pos of the last n = min(K, stored) points as rts_otw_tempo / rts_wtw_tempo define them with ahead = 0 and
 *      their limits; x_i the newest point's live index.  A NaN slope or slope <= 0: step_raw = nominal, status FREE.
 *   7. otherwise x1 = (double)(base + o1 + G + lead) / (double)hop;  y1 = pos + slope * (x1 - (double)x_i);
 *      tgt_f = floor(y1 * (double)hop_track); not finite or |tgt_f| >= 2^52: FREE as above; else
 *      d = clamp((int64)tgt_f + first_b + origin_b - i0, 0, 2^31 - 1);  step_raw = (d Ls) / (Ls + G).
 *   8. step = clamp(step_raw, lo, hi), status LO / HI when it clamped;  i1 = min(i0 + step, max(i0, first_b + len_b)),
 *      status END when that cut it.
 *   9. the anchor (o1, i1) is appended and n_out = o1: blocks [k, k_due) lie in the last segment.
 *  10. published: out_total = o1, in_pos = i1, rate = (double)(i1 - i0) / (double)Ls, blocks = k_due - k, the status.
 *      A feed without a block publishes out_total and in_pos of the last anchor, the rate published last (NaN before the
 *      first block), blocks 0; a stream that is not armed 0, 0, NaN, 0 and status 0.
 * The map keeps every rule of rts_warp_run's time map, and the audio is by definition what rts_warp_run renders for those
 * anchors, k_count = chunk_blocks, block k at sample (k - k_start) H of the stream's row.
 *
 * Delivery.  Feed f (counted from 1, the number rts_live_poll reports) renders into chunk f % 4 of a ring of four
 * host-mapped chunks [B][chunk_blocks H] float32 (rows begin on 32-byte boundaries) and publishes its words into slot f % 4
 * of a seventh host-mapped block.  When *feeds_done >= f the chunk and the words of feed f are complete; feed f + 4 writes
 * over them, so a consumer looks at least once in three feeds (out_total tells it when it did not).  Samples of a row
 * behind blocks H are left from earlier feeds. */
typedef struct rts_accomp_params {
    int32_t hop_track, K;
    long long glide, lead;
    int32_t rate_min_pm, rate_max_pm, chunk_blocks, A_max;
} rts_accomp_params;

#define RTS_ACC_ON 1     /* the stream is armed */
#define RTS_ACC_WAIT 2   /* its tracker has no path point yet: the clock has not started */
#define RTS_ACC_FREE 4   /* no usable slope: the segment runs at the nominal rate */
#define RTS_ACC_LO 8     /* the step was raised to the lower rate limit */
#define RTS_ACC_HI 16    /* the step was cut to the upper rate limit */
#define RTS_ACC_END 32   /* the anchor was held at the end of the track */
#define RTS_ACC_FULL 64  /* A_max anchors are stored: nothing more is rendered */
#define RTS_ACC_LATE 128 /* more than chunk_blocks blocks were due: the rest follows with the next feeds */

/* Arms the streams with mask_host[b] != 0 (again, when they are armed already: from output sample 0), switching the
 * accompaniment on; a NULL warp_plan switches it off, and the next time it is switched on every stream starts disarmed.
 * The streams are armed in the chain of the next rts_live_submit, in front of its steering.  The first call with a plan
 * allocates the per-stream state, the seventh host-mapped block and the ring; a later call with another plan, pool, dtype
 * or parameters waits for the device, frees them and starts over with every stream disarmed.  The plan and the pool must
 * outlive their use here.  rts_live_restart disarms the restarted streams (status 0, nothing rendered until they are
 * armed again), rts_live_reset all streams; rts_live_export / rts_live_import refuse a session with the accompaniment on,
 * rts_live_gate(min_level > 0) too.  A session that never calls this allocates none of it and enqueues exactly what it
 * enqueues without this function; with it on a feed enqueues two more launches.
 *   RTS_ERR_UNSUPPORTED: a session with the level gate on or with a resampler (live indices are not microphone time there);
 *   chunk_blocks H >= 2^31 or (chunk_blocks H hop_track rate_max_pm) / (hop 1000) >= 2^31 (a segment of the map could
 *   reach 2^31); the overflow rule of rts_otw_tempo for K.
 *   RTS_ERR_INVALID: NULL handle, a failed handle, NULL tracks_dev, mask_host, first_host, len_host or params, track_dtype,
 *   every parameter limit above, a masked stream with first or len < 0 or a position at or beyond 2^61, more than 65535
 *   streams, a plan of another device, another device current. */
int rts_live_accompany(rts_live *h, rts_warp *warp_plan, const void *tracks_dev, int track_dtype /* RTS_F32 | RTS_I16 */,
                       const uint8_t *mask_host /* [B] */, const long long *first_host /* [B] */,
                       const long long *len_host /* [B] */, const long long *origin_host /* [B] or NULL */,
                       const rts_accomp_params *params);
/* The non-blocking look, like rts_live_tempo and with its guarantee: *feeds_done = f is the newest feed every stream has
 * published, *chunk_host the chunk of feed f ([B] rows *row_stride samples apart, stream b's audio its first blocks[b] * H
 * samples) and the [B] words those of feed f.  A stream whose slot holds another feed's words -- the accompaniment was off
 * in feed f, or four more feeds have been submitted -- reads blocks 0, status 0, rate NaN.  warp_status: what rts_warp_run
 * left for the stream (RTS_WARP_NO_MAP while it has fewer than two anchors).  Any output pointer may be NULL.
 *   RTS_ERR_INVALID: NULL handle; before the first rts_live_accompany with a plan. */
int rts_live_accompaniment(rts_live *h, const float **chunk_host, long long *row_stride, int32_t *blocks /* [B] */,
                           long long *out_total /* [B] */, long long *in_pos /* [B] */, double *rate /* [B] */,
                           int32_t *status /* [B] */, int32_t *warp_status /* [B] */, int *feeds_done);
/* For tests and tools, like rts_otw_read_path: waits for `stream`, then *n = the anchors stream b has stored, the first
 * min(*n, cap) of them as (out_pos, in_pos) pairs in anchors_host (may be NULL) and the renderer's (k, p_prev) in state
 * (may be NULL).
 *   RTS_ERR_INVALID: NULL handle or n, b outside [0, B), cap < 0, before the first rts_live_accompany with a plan, another
 *   device current. */
int rts_live_accomp_map(rts_live *h, int b, long long *anchors_host, int cap, int *n, long long state[2], void *stream);

/* ------------------------------------------------------------------------------------------
 * The time map of a path: positions of one recording on the other, annotation tables carried over.
 * ------------------------------------------------------------------------------------------ */
/* The reference stops at the path here too (tests.py:59-137 takes error statistics of it); reading a time of one
 * recording and saying where that moment lies on the other is this project's definition, to the bit, like the resampler's
 * and the renderer's.  tests/pathmap_model.py holds it in plain Python.
 *
 * Knots.  A path of P points (p[t][0], p[t][1]), int32, in the layout of rts_dtw_paths; a side `from` in {0, 1} and two
 * int32 offsets per pair, off[0] added to column 0 and off[1] to column 1 (NULL: zeros; where a restarted stream's or a
 * subsequence path's own range begins): u_t = p[t][from] + off[from], v_t = p[t][1 - from] + off[1 - from], in 64 bits.
 * The path is usable when P >= 1, u and v do not decrease in t and no u_t or v_t is below 0; steps larger than 1 are
 * allowed.  The knots k_0 < k_1 < .. < k_{K-1} are the distinct values of u.  lo_i is v at the first point with u = k_i,
 * hi_i v at the last, and m_i = (double)(lo_i + hi_i) * 0.5, exact: the middle of the vertical run (rts_warp_anchors keeps
 * its first-point rule).  m_i does not decrease in i, since lo_{i+1} >= hi_i.
 *
 * A position x, float64, in frames (fractions allowed), maps to
 *   NaN                                                                  if x is NaN, x < k_0 or x > k_{K-1}
 *                                                                        (compared as doubles, before any conversion)
 *   m_i                                                                  if x == k_i
 *   m_i + ((x - k_i) * (m_{i+1} - m_i)) / (double)(k_{i+1} - k_i)        otherwise, i the last knot with k_i <= x
 * every operation float64 and rounded on its own, no fused multiply-add.  y does not decrease in x (the product of the
 * largest x - k_i with m_{i+1} - m_i divides exactly), y == x to the bit on the identity path, and y(k_i) == m_i.
 *
 * Status of a pair, a sum of: */
#define RTS_PATHMAP_OK 0
#define RTS_PATHMAP_EMPTY 1    /* len < 1 (the -1 of rts_dtw_paths' fault contract included); rts_annot_transfer: no such piece */
#define RTS_PATHMAP_BACKWARD 2 /* a column steps back */
#define RTS_PATHMAP_NEGATIVE 4 /* an index is below 0 after the offsets */
/* A pair whose status is not 0 gets NaN in all of its valid entries; its neighbours are unaffected.
 *
 * rts_path_map: y_dev[b][e] = the image of x_dev[b][e] for e < n_dev[b] (NULL: n_max; clamped to [0, n_max]); entries
 * behind it are not written.  path_dev int32 [B][P_max][2], len_dev int32 [B] (a length above P_max is clamped to it),
 * off_dev int32 [B][2] or NULL, x_dev / y_dev float64 [B][n_max], status_dev int32 [B].  One workgroup of 256 lanes per
 * pair: it walks the path once and reduces the status, then every lane maps entries with at most three bisections of
 * column `from`.  Asynchronous on `stream`; no allocation, no synchronisation (graph-capturable); writes y_dev and
 * status_dev only, and no result depends on what they held.
 *   RTS_ERR_INVALID, naming the argument, before any GPU call: a NULL pointer (path_dev may be NULL when P_max == 0, x_dev
 *   and y_dev when n_max == 0), P_max or n_max outside [0, 2^30], `from` outside {0, 1}, B outside [1, 65535]. */
int rts_path_map(const int32_t *path_dev /* [B][P_max][2] */, int P_max, const int32_t *len_dev /* [B] */,
                 const int32_t *off_dev /* [B][2] or NULL */, int from, const double *x_dev /* [B][n_max] */, int n_max,
                 const int32_t *n_dev /* [B] or NULL */, int B, double *y_dev /* [B][n_max] */, int32_t *status_dev /* [B] */,
                 void *stream);
/* A table carried along a path: for pair b and row r of table piece_dev[b] of `h`, x = times[r] / frame_seconds (one
 * division, the handle's own frame_seconds), times_dev[b][r] = y(x) * frame_seconds, or NaN where x has no image or the
 * path is refused; n_rows_dev[b] = the table's length, entries behind it are not written.  A piece outside [0, P) gives
 * n_rows 0 and status RTS_PATHMAP_EMPTY (its path is not looked at).  Path, offsets, `from`, status and launch shape as
 * rts_path_map.  The map does not decrease, so the finite images of a table's times are non-decreasing and finite: with
 * the beats of the same rows they pass rts_annot_create's rules.
 *   RTS_ERR_INVALID before any GPU call: a NULL handle or pointer (path_dev may be NULL when P_max == 0), P_max or
 *   rows_max outside [0, 2^30], `from` outside {0, 1}, B outside [1, 65535], rows_max below the longest table of the handle (piece_dev
 *   lies on the device, so every table counts as selected), another device current. */
int rts_annot_transfer(rts_annot *h, const int32_t *path_dev /* [B][P_max][2] */, int P_max, const int32_t *len_dev /* [B] */,
                       const int32_t *off_dev /* [B][2] or NULL */, int from, const int32_t *piece_dev /* [B] */, int B,
                       int rows_max, double *times_dev /* [B][rows_max] */, int32_t *n_rows_dev /* [B] */,
                       int32_t *status_dev /* [B] */, void *stream);

/* ------------------------------------------------------------------------------------------
 * Following a score: note lists to reference chroma.
 * ------------------------------------------------------------------------------------------ */
/* The reference follows recordings only; what a note list sounds like to the chroma chain is this project's definition, to
 * the bit, like the resampler's and the renderer's.  tests/score_model.py holds it in plain numpy.
 *
 * A plan holds fft_len L (a power of two in [64, 8192], as a chroma plan), hop H in [1, 2^24], pad_left in [0, L] (L/2 for
 * the reference's centred framing, chroma.py:44-65) and three host tables, copied at create:
 *   T [128][12] float64   the chroma a steady tone of MIDI pitch p leaves
 *   CW[L + 1]   float64   CW[0] = 0, CW[n] = CW[n-1] + w[n-1]^2: the window's cumulative energy, summed by the host
 *   DK[K + 1]   float64   K in [0, 2^20]: the energy left k frames after the onset
 * every entry finite and >= 0, CW[0] == 0 and CW not decreasing.
 *
 * Notes lie in one pool, piece by piece, each piece's notes in ascending onset order: onset and end (int64 samples, end
 * exclusive), pitch (int32), energy (float64).  Piece p has notes [note_first[p], note_first[p] + note_len[p]) and writes
 * frames [frame_first[p], frame_first[p] + n_frames[p]) of an output pool [n_pool_frames][12], the layout
 * rts_otw_create_refs and rts_locate take.  Frame m of a piece, every float64 operation rounded on its own:
 *   w0 = m H - pad_left
 *   for every note n of the piece in ascending index, acc[0..11] starting at +0.0:
 *       a = clamp(onset - w0, 0, L);  b = clamp(end - w0, 0, L);  if b <= a: the note takes no part
 *       k = clamp(m - floor((onset + pad_left) / H), 0, K)
 *       wgt = (energy * DK[k]) * (CW[b] - CW[a])
 *       acc[c] = acc[c] + wgt * T[pitch][c]                        c = 0..11
 *   s = sum of acc[c] * acc[c], c ascending, from +0.0;  len = sqrt(s)
 *   if !normalize or len < 2.2250738585072014e-308: len = 1.0     (the rule of the chroma kernels)
 *   out[c] = acc[c] / len                                          (float32 output: that value converted)
 * in exact integers: no onset or end of 64 bits overflows a step of it.  A note takes no part in any frame when its pitch
 * lies outside 0..127, onset < 0, end < onset, or its energy is negative or not finite; such notes are counted per piece
 * in skipped_dev[p].  A piece without notes gives all-zero frames; a piece with n_frames < 1 writes nothing.
 *
 * Status of a piece, a sum of: */
#define RTS_SCORE_OK 0
#define RTS_SCORE_FRAMES 1 /* n_frames >= 1 and its frame range leaves the pool: nothing is written */
#define RTS_SCORE_NOTES 2  /* its note range leaves [0, n_notes): nothing is written, no note is read, skipped is 0 */
/* The result is a function of the notes and the tables alone, whatever order the notes have: the kernel leaves out notes
 * that cannot reach a wave's frames by two per-piece tables that hold for any order (the largest end up to a note, the
 * smallest onset from a note on), which a prepare kernel writes into the workspace, 24 bytes per note.  The note ranges of
 * two pieces are either the same or disjoint.
 *
 * rts_score_chroma: asynchronous on `stream`, no allocation, no synchronisation (graph-capturable), two launches; writes
 * the frames of the pieces, skipped_dev, status_dev and the workspace only, and no result depends on what they held.
 *   RTS_ERR_UNSUPPORTED: fft_len no power of two in [64, 8192].
 *   RTS_ERR_INVALID, naming the argument, before any GPU call: a NULL handle, table or pointer (the four note pointers
 *   and the workspace may be NULL when n_notes == 0; skipped_dev and status_dev always), hop, pad_left or K outside their
 *   limits, a table entry that breaks the rules above, n_notes outside [0, 2^31), P outside [1, 65535], n_pool_frames
 *   outside [1, 2^31), out_dtype, a workspace below rts_score_workspace_bytes, another device current. */
typedef struct rts_score rts_score;
int rts_score_create(int fft_len, int hop, int pad_left, int K, const double *T_host /* [128][12] */,
                     const double *CW_host /* [fft_len + 1] */, const double *DK_host /* [K + 1] */, rts_score **out);
int rts_score_destroy(rts_score *h);
int rts_score_workspace_bytes(long long n_notes, size_t *bytes);
int rts_score_chroma(rts_score *h, const long long *onset_dev, const long long *end_dev, const int32_t *pitch_dev,
                     const double *energy_dev, long long n_notes, const long long *note_first_dev /* [P] */,
                     const int32_t *note_len_dev /* [P] */, const long long *frame_first_dev /* [P] */,
                     const int32_t *n_frames_dev /* [P] */, int P, int normalize, void *out_dev /* [n_pool_frames][12] */,
                     int out_dtype, long long n_pool_frames, int32_t *skipped_dev /* [P] or NULL */,
                     int32_t *status_dev /* [P] or NULL */, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RTSYNC_H */
