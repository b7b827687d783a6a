// Beats and labels: the ground-truth tables of P pieces on the device, and three kernels that read them.
//   livenote_live.py:197-202, :211-227   after every insert: get_beat_and_label(ln.path[-1][1]) -> the beat and the bar
//                                        label shown, both sticky                          -> annot_live_kernel (one launch
//                                                                                            per feed of a live handle)
//   tests.py:112-128                     get_beat of every path point                      -> rts_annot_beats
//   tests.py:59-137                      test_simple.get_error: the accuracy metric        -> rts_annot_path_error
//   the way back, beat -> frame of a piece (annot_frame_of in csrc/annot_device.h)         -> rts_annot_frames
// The definition is include/rtsync.h's; the checks of the tables and the launch geometry are csrc/annot_plan.h's.
//
// Lookup of frame f in a table of n rows (annot_lookup): time = (double)f * frame_seconds, i = the first row with time <=
// times[i] by bisection; none: no beat (NaN on the device) and seg = -1.  i == 0 and times[0] == 0: beats[0].  Otherwise
// beats[i] - (times[i] - time) / (times[i] - start), start = 0.0 for i == 0 and times[i - 1] behind it: the operations of
// evaluate.get_beat in their order (the build compiles with -ffp-contract=off).  seg = 0 for i == 0, else i - 1.
//
// Every kernel bounds what it reads: a piece outside [0, P) or a negative frame has no beat, rows are indexed inside the
// piece's own range, path points inside P_max, a stream's last path point inside the tracker's path_cap.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "annot_device.h"
#include "annot_plan.h"
#include "common.h"

namespace rts {

// grid (ceil(n_max / 256), B): one lane per entry.
__global__ void __launch_bounds__(kAnnotThreads)
annot_beats_kernel(AnnotTables t, const int32_t *frames, int n_max, const int32_t *n_dev, const int32_t *piece_dev,
                   const int32_t *frame0_dev, double *beat_out, int32_t *seg_out) {
    const int b = blockIdx.y;
    const int k = blockIdx.x * kAnnotThreads + threadIdx.x;
    int n = n_dev ? n_dev[b] : n_max;
    if (n > n_max) n = n_max;
    if (k >= n) return;
    const size_t e = (size_t)b * n_max + k;
    const int32_t f = frames[e];
    const long long frame = f < 0 ? -1 : (long long)f + (frame0_dev ? frame0_dev[b] : 0);
    int seg;
    const double beat = annot_lookup(annot_piece(t, piece_dev[b]), frame, t.frame_seconds, &seg);
    beat_out[e] = beat;
    if (seg_out) seg_out[e] = seg;
}

// grid (ceil(n_max / 256), B): one lane per entry, the other way round: beat -> frame of the stream's piece.
__global__ void __launch_bounds__(kAnnotThreads)
annot_frames_kernel(AnnotTables t, const double *beats, int n_max, const int32_t *n_dev, const int32_t *piece_dev,
                    int32_t *frame_out) {
    const int b = blockIdx.y;
    const int k = blockIdx.x * kAnnotThreads + threadIdx.x;
    int n = n_dev ? n_dev[b] : n_max;
    if (n > n_max) n = n_max;
    if (k >= n) return;
    const size_t e = (size_t)b * n_max + k;
    frame_out[e] = annot_frame_of(t, piece_dev[b], beats[e]);
}

// AlignmentError.get_time (tests.py:130-134) on the live table: *bad when the beat's integer part is no row of it
__device__ __forceinline__ double annot_time_of(const AnnotPiece &p, double beat, bool *bad) {
    if (!(beat > -1.0 && beat < (double)p.n)) {  // (int)beat < 0 or >= n
        *bad = true;
        return 0.0;
    }
    const int whole = (int)beat;  // toward zero, like Python's int()
    double sec = p.times[whole];
    if (whole + 1 < p.n) {
        double r = fmod(beat, 1.0);  // Python's float %: the sign of the divisor
        if (r != 0.0 && r < 0.0) r += 1.0;
        sec += r * (p.times[whole + 1] - p.times[whole]);
    }
    return sec;
}

// One workgroup per pair.  Per chunk of kAnnotChunk path points every lane looks its points up and leaves diff * diff (0.0
// for a point that does not count: error + 0.0 == error for every error >= +0.0) in LDS; lane 0 then adds the chunk to the
// pair's sum in path order -- the one float64 chain of the metric, equal to the Python loop bit for bit.  The counters are
// integers: each lane keeps its own, and they meet in LDS at the end.
__global__ void __launch_bounds__(kAnnotThreads)
annot_path_error_kernel(AnnotTables t, const int32_t *path, int P_max, const int32_t *path_len, const int32_t *piece0,
                        const int32_t *piece1, double *sq_err, int32_t *counts) {
    __shared__ double sq[kAnnotChunk];
    __shared__ int32_t total[RTS_ANNOT_COUNTS];
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    int n = path_len[b];
    if (n > P_max) n = P_max;
    if (n < 0) n = 0;
    const AnnotPiece live = annot_piece(t, piece0[b]), ref = annot_piece(t, piece1[b]);
    const int32_t *pts = path + (size_t)b * P_max * 2;
    if (tid < RTS_ANNOT_COUNTS) total[tid] = 0;
    int32_t cnt = 0, bad = 0, off_b[4] = {0, 0, 0, 0}, off_s[4] = {0, 0, 0, 0};
    double err = 0.0;  // lane 0's
    const double thr[4] = {1.0, 3.0, 5.0, 10.0};
    for (int base = 0; base < n; base += kAnnotChunk) {
        const int m = n - base < kAnnotChunk ? n - base : kAnnotChunk;
        for (int k = tid; k < m; k += kAnnotThreads) {
            const int32_t l = pts[2 * (size_t)(base + k)], r = pts[2 * (size_t)(base + k) + 1];
            int seg;
            const double l_beat = annot_lookup(live, l, t.frame_seconds, &seg);
            const double r_beat = annot_lookup(ref, r, t.frame_seconds, &seg);
            double d2 = 0.0;
            // `if l_beat and r_beat` (tests.py:71): None and 0.0 are both falsy
            if (l_beat == l_beat && r_beat == r_beat && l_beat != 0.0 && r_beat != 0.0) {
                bool oob = false;
                const double tr = annot_time_of(live, r_beat, &oob);
                const double tl = annot_time_of(live, l_beat, &oob);
                if (oob) {
                    bad++;
                } else {
                    const double diff = fabs(l_beat - r_beat);
                    const double secs = fabs(tr - tl);
                    d2 = diff * diff;
                    for (int q = 0; q < 4; q++) {
                        off_b[q] += diff > thr[q];
                        off_s[q] += secs > thr[q];
                    }
                    cnt++;
                }
            }
            sq[k] = d2;
        }
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < m; k++) err += sq[k];
        __syncthreads();
    }
    __syncthreads();  // total[] is zero (n == 0 runs no chunk)
    if (cnt) atomicAdd(&total[0], cnt);
    for (int q = 0; q < 4; q++) {
        if (off_b[q]) atomicAdd(&total[1 + q], off_b[q]);
        if (off_s[q]) atomicAdd(&total[5 + q], off_s[q]);
    }
    if (bad) atomicAdd(&total[9], bad);
    __syncthreads();
    if (tid < RTS_ANNOT_COUNTS) counts[(size_t)b * RTS_ANNOT_COUNTS + tid] = total[tid];
    if (tid == 0) sq_err[b] = err;
}

// rts_live_annotate: piece and frame offset of the selected streams, by value like a restart's selection.
struct AnnotSel {
    int n;
    int32_t idx[kRestartChunk], piece[kRestartChunk], frame0[kRestartChunk];
};

__global__ void annot_select_kernel(AnnotSel sel, int32_t *piece, int32_t *frame0) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= sel.n) return;
    piece[sel.idx[i]] = sel.piece[i];
    frame0[sel.idx[i]] = sel.frame0[i];
}

// One lane per stream, once per feed: ln.path[-1][1] of the stream's tracker, looked up, into the sticky words
// (livenote_live.py:197-202).  The words lie in host-mapped memory and are only written here, never read.
__global__ void __launch_bounds__(kAnnotLiveThreads) annot_live_kernel(AnnotTables t, AnnotLive g) {
    const int b = blockIdx.x * kAnnotLiveThreads + threadIdx.x;
    if (b >= g.B) return;
    int m = g.state[(size_t)b * g.state_len + g.st_n_path];
    if (m > g.path_cap) m = g.path_cap;
    if (m < 1) {
        g.ref_frame[b] = -1;
        return;
    }
    const int32_t j = g.path[((size_t)b * g.path_cap + (m - 1)) * 2 + 1];
    const long long frame = j < 0 ? -1 : (long long)j + g.frame0[b];
    const int piece = g.piece[b];
    int seg;
    const double beat = annot_lookup(annot_piece(t, piece), frame, t.frame_seconds, &seg);
    if (beat == beat && beat != 0.0) g.beat[b] = beat;  // `if beat:`
    if (seg >= 0 && (!t.label_ok || t.label_ok[t.first[piece] + seg])) g.label[b] = seg;  // `if mus_label:`
    g.ref_frame[b] = frame < 0 ? -1 : (int32_t)frame;
}

}  // namespace rts

struct rts_annot {
    rts::AnnotTables t;  // device pointers
    long long n_rows;
    int longest;  // rows of the longest table
    int device;
    void *block;  // the one allocation behind them
};

namespace rts {

int annot_pieces(const rts_annot *a) { return a->t.P; }
int annot_device(const rts_annot *a) { return a->device; }
int annot_longest(const rts_annot *a) { return a->longest; }
const AnnotTables *annot_tables(const rts_annot *a) { return &a->t; }

int annot_select_enqueue(int B, const uint8_t *mask_host, const int32_t *piece_host, const int32_t *frame0_host,
                         int32_t *piece_dev, int32_t *frame0_dev, hipStream_t s) {
    AnnotSel sel;
    for (int pos = 0; pos < B;) {
        sel.n = 0;
        for (; pos < B && sel.n < kRestartChunk; pos++)
            if (mask_host[pos]) {
                sel.idx[sel.n] = pos;
                sel.piece[sel.n] = piece_host[pos];
                sel.frame0[sel.n] = frame0_host ? frame0_host[pos] : 0;
                sel.n++;
            }
        if (sel.n == 0) break;
        hipLaunchKernelGGL(annot_select_kernel, dim3((sel.n + 63) / 64), dim3(64), 0, s, sel, piece_dev, frame0_dev);
        RTS_HIP(hipGetLastError());
    }
    return RTS_OK;
}

int annot_live_enqueue(const rts_annot *a, const AnnotLive &g, hipStream_t s) {
    hipLaunchKernelGGL(annot_live_kernel, dim3(annot_live_grid(g.B)), dim3(kAnnotLiveThreads), 0, s, a->t, g);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

}  // namespace rts

extern "C" {

int rts_annot_destroy(rts_annot *h) {
    if (!h) return RTS_OK;
    if (h->block) (void)hipFree(h->block);
    free(h);
    return RTS_OK;
}

int rts_annot_create(int P, long long n_rows, const long long *first_host, const int32_t *len_host, const double *times_host,
                     const int32_t *beats_host, const uint8_t *label_ok_host, double frame_seconds, rts_annot **out) {
    using namespace rts;
    if (!out) return set_error(RTS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!first_host || !len_host || !times_host || !beats_host)
        return set_error(RTS_ERR_INVALID, "first_host, len_host, times_host and beats_host must be given");
    if (!(frame_seconds > 0.0) || frame_seconds > 1.7976931348623157e308)
        return set_error(RTS_ERR_INVALID, "frame_seconds must be finite and > 0");
    if (n_rows < 1 || n_rows > 0x7fffffffLL) return set_error(RTS_ERR_INVALID, "n_rows must be in [1, 2^31)");
    AnnotFault where;
    if (const AnnotRefusal why = annot_check(P, n_rows, first_host, len_host, times_host, beats_host, &where); why != kAnnotOk) {
        char msg[256];
        annot_message(msg, sizeof(msg), why, where, n_rows);
        return set_error(RTS_ERR_INVALID, "%s", msg);
    }
    rts_annot *h = (rts_annot *)calloc(1, sizeof(rts_annot));
    if (!h) return set_error(RTS_ERR_INVALID, "out of host memory");
    // one block: times, first (8-byte values), beats, len, the pieces' invertible flags, the rows' label flags
    const size_t nr = (size_t)n_rows, np = (size_t)P;
    const size_t o_first = sizeof(double) * nr, o_beats = o_first + sizeof(long long) * np, o_len = o_beats + sizeof(int32_t) * nr,
                 o_inv = o_len + sizeof(int32_t) * np, o_flags = o_inv + np, bytes = o_flags + (label_ok_host ? nr : 0);
    uint8_t *inv = (uint8_t *)malloc(np);
    if (!inv) {
        free(h);
        return set_error(RTS_ERR_INVALID, "out of host memory");
    }
    for (int p = 0; p < P; p++) inv[p] = annot_invertible(beats_host + first_host[p], len_host[p]) ? 1 : 0;
    hipError_t e = hipGetDevice(&h->device);
    if (e == hipSuccess) e = hipMalloc(&h->block, bytes);
    unsigned char *d = static_cast<unsigned char *>(h->block);
    if (e == hipSuccess) e = hipMemcpy(d, times_host, sizeof(double) * nr, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + o_first, first_host, sizeof(long long) * np, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + o_beats, beats_host, sizeof(int32_t) * nr, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + o_len, len_host, sizeof(int32_t) * np, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + o_inv, inv, np, hipMemcpyHostToDevice);
    if (e == hipSuccess && label_ok_host) e = hipMemcpy(d + o_flags, label_ok_host, nr, hipMemcpyHostToDevice);
    free(inv);
    if (e != hipSuccess) {
        rts_annot_destroy(h);
        return set_error(RTS_ERR_HIP, "rts_annot_create: %s", hipGetErrorString(e));
    }
    h->t.times = reinterpret_cast<const double *>(d);
    h->t.first = reinterpret_cast<const long long *>(d + o_first);
    h->t.beats = reinterpret_cast<const int32_t *>(d + o_beats);
    h->t.len = reinterpret_cast<const int32_t *>(d + o_len);
    h->t.invertible = d + o_inv;
    h->t.label_ok = label_ok_host ? d + o_flags : nullptr;
    h->t.P = P;
    h->t.frame_seconds = frame_seconds;
    h->n_rows = n_rows;
    for (int p = 0; p < P; p++)
        if (len_host[p] > h->longest) h->longest = len_host[p];
    *out = h;
    return RTS_OK;
}

int rts_annot_beats(rts_annot *h, const int32_t *frames_dev, int n_max, const int32_t *n_dev, const int32_t *piece_dev,
                    const int32_t *frame0_dev, int B, double *beat_dev, int32_t *seg_dev, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!frames_dev || !piece_dev || !beat_dev) return set_error(RTS_ERR_INVALID, "frames_dev, piece_dev and beat_dev must be given");
    if (B < 1 || B > 65535) return set_error(RTS_ERR_INVALID, "B must be in [1, 65535] (got %d)", B);
    if (n_max < 0) return set_error(RTS_ERR_INVALID, "n_max must be >= 0");
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    if (n_max == 0) return RTS_OK;
    const AnnotGrid g = annot_beats_grid(B, n_max);
    hipLaunchKernelGGL(annot_beats_kernel, dim3(g.x, g.y), dim3(kAnnotThreads), 0, (hipStream_t)stream, h->t, frames_dev, n_max,
                       n_dev, piece_dev, frame0_dev, beat_dev, seg_dev);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

int rts_annot_frames(rts_annot *h, const double *beats_dev, int n_max, const int32_t *n_dev, const int32_t *piece_dev, int B,
                     int32_t *frame_dev, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!beats_dev || !piece_dev || !frame_dev) return set_error(RTS_ERR_INVALID, "beats_dev, piece_dev and frame_dev must be given");
    if (B < 1 || B > 65535) return set_error(RTS_ERR_INVALID, "B must be in [1, 65535] (got %d)", B);
    if (n_max < 0) return set_error(RTS_ERR_INVALID, "n_max must be >= 0");
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    if (n_max == 0) return RTS_OK;
    const AnnotGrid g = annot_beats_grid(B, n_max);
    hipLaunchKernelGGL(annot_frames_kernel, dim3(g.x, g.y), dim3(kAnnotThreads), 0, (hipStream_t)stream, h->t, beats_dev, n_max,
                       n_dev, piece_dev, frame_dev);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

int rts_annot_path_error(rts_annot *h, const int32_t *path_dev, int P_max, const int32_t *path_len_dev, const int32_t *piece0_dev,
                         const int32_t *piece1_dev, int B, double *sq_err_dev, int32_t *counts_dev, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (!path_len_dev || !piece0_dev || !piece1_dev || !sq_err_dev || !counts_dev)
        return set_error(RTS_ERR_INVALID, "path_len_dev, piece0_dev, piece1_dev, sq_err_dev and counts_dev must be given");
    if (B < 1) return set_error(RTS_ERR_INVALID, "B must be >= 1");
    if (P_max < 0 || (P_max > 0 && !path_dev)) return set_error(RTS_ERR_INVALID, "path_dev is NULL or P_max < 0");
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    hipLaunchKernelGGL(annot_path_error_kernel, dim3(B), dim3(kAnnotThreads), 0, (hipStream_t)stream, h->t, path_dev, P_max,
                       path_len_dev, piece0_dev, piece1_dev, sq_err_dev, counts_dev);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

}  // extern "C"
