#pragma clang fp contract(off)
// Live accompaniment: a track rendered along every tracker, feed by feed (include/rtsync.h, rts_live_accompany; DESIGN.md
// 4.22; tests/accomp_model.py is the definition in Python).  Every float64 operation of the law is rounded on its own: the
// pragma above switches contraction off for the whole file, under the build's -ffp-contract=off and under hipcc's own
// default alike, like csrc/warp.hip's.
//
// What a feed adds to the chain of csrc/live.hip, between the consensus launch and live_compact_kernel:
//   accomp_arm_kernel / accomp_disarm_kernel   only in the first feed after rts_live_accompany armed streams or switched
//                         the accompaniment off and on again: the selection travels by value, like a restart's
//   accomp_steer_kernel   one wave per stream: the regression window over the tail of the tracker's path (the sums and
//                         tempo_fit of csrc/tempo_device.h), then on lane 0 the steering law, whose integer part is
//                         csrc/accomp_plan.h's: the next anchor of the stream's time map, n_out, and the published words
//   rts_warp_run          k_count = chunk_blocks, straight into this feed's chunk of the host-mapped ring: the blocks
//                         [k, k_due) the steering made due, 16-byte stores
// Nothing is read back and nothing synchronises.  The chunk and the words of feed f are complete when live_compact_kernel
// publishes f: both kernels have ended before it starts, the ring is fine-grained host memory, and the words were
// fenced at system scope.
//
// Every kernel bounds what it reads and writes: path points inside min(stored, path_cap), anchors inside A_max (a full list
// is reported, not extended), the selection inside its count, streams inside B.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "accomp_plan.h"
#include "common.h"
#include "tempo_device.h"
#include "tempo_plan.h"
#include "warp_plan.h"

namespace rts {

// The warp plan as csrc/warp.hip defines it (token for token: one definition in two translation units).  This file needs
// the hop and the device of a plan it is handed.
struct WarpGeom {
    const double *w;  // [N] on the device
    int N, H, delta;
};

}  // namespace rts

struct rts_warp {
    rts::WarpGeom g;
    int device;
};

namespace rts {

struct AccompDev {  // per-stream state on the device
    long long *fed, *base;  // [B]
    long long *wstate;      // [B][2]: the renderer's (k, p_prev)
    long long *anchors;     // [B][A_max][2]
    long long *n_out, *n_in, *origin;  // [B]: n_in = the end of the stream's track, origin = its reference frame 0 (pool samples)
    double *rate;           // [B] the rate published last
    int32_t *n_anchor, *armed;  // [B]
};

struct AccompWords {  // one slot of the seventh host-mapped block
    long long *out_total, *in_pos;
    double *rate;
    int32_t *blocks, *status, *warp_status, *seq;
};

struct AccompSteer {
    // the tracker, as TempoTail carries it
    const int32_t *state;
    int state_len, st_n_path;
    const int32_t *path;
    int path_cap;
    const int32_t *ref_len;
    int N;
    // the append: n_samples[b] - pending[b] samples were taken (live_append_kernel wrote the first, live_compact_kernel
    // writes the second behind this kernel)
    const int32_t *n_samples, *pending;
    AccompGeom p;
    AccompDev d;
    AccompWords w;
    int feed_no;
};

constexpr int kAccSelChunk = 128;
struct AccompSel {  // by value, like RestartSel
    int n;
    int32_t idx[kAccSelChunk];
    long long origin[kAccSelChunk], n_in[kAccSelChunk];
};

__global__ void accomp_arm_kernel(AccompSel sel, AccompDev d, int A_max) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= sel.n) return;
    const int b = sel.idx[i];
    d.fed[b] = 0;
    d.base[b] = -1;
    d.wstate[2 * b] = d.wstate[2 * b + 1] = 0;
    long long *an = d.anchors + (size_t)b * (size_t)A_max * 2;
    an[0] = 0;
    an[1] = sel.origin[i];
    d.n_anchor[b] = 1;
    d.n_out[b] = 0;
    d.n_in[b] = sel.n_in[i];
    d.origin[b] = sel.origin[i];
    d.rate[b] = annot_nan();
    d.armed[b] = 1;
}

// n < 0: every stream of B; otherwise the streams of the selection.
__global__ void accomp_disarm_kernel(RestartSel sel, int B, AccompDev d) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (sel.n < 0 ? B : sel.n)) return;
    const int b = sel.n < 0 ? i : sel.idx[i];
    d.armed[b] = 0;
    d.n_anchor[b] = 0;  // the renderer skips the stream (RTS_WARP_NO_MAP)
    d.n_out[b] = 0;
}

__device__ __forceinline__ void accomp_publish(const AccompWords &w, int b, long long out_total, long long in_pos, double rate,
                                               long long blocks, int status, int feed_no) {
    *(volatile long long *)(w.out_total + b) = out_total;
    *(volatile long long *)(w.in_pos + b) = in_pos;
    *(volatile double *)(w.rate + b) = rate;
    *(volatile int32_t *)(w.blocks + b) = (int32_t)blocks;
    *(volatile int32_t *)(w.status + b) = status;
    __threadfence_system();
    *(volatile int32_t *)(w.seq + b) = feed_no;  // written last, like live_publish
    __threadfence_system();
}

// One wave per stream, shaped like tempo_tail_kernel: lane l adds the terms of points l, l + 64, ... of the stream's last n =
// min(K, stored) points, a butterfly of shuffles adds the lanes, lane 0 fits, steers and stores.  No LDS, no barrier.
__global__ void __launch_bounds__(kAccThreads) accomp_steer_kernel(AccompSteer g) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int Nb = g.ref_len ? g.ref_len[b] : g.N;
    const long long y_limit = Nb, x_limit = 2 * (long long)Nb;
    int points = g.state[(size_t)b * g.state_len + g.st_n_path];  // counts on past path_cap once the path is truncated
    points = points > g.path_cap ? g.path_cap : (points < 0 ? 0 : points);
    const int n = points < g.p.K ? points : g.p.K;
    const int2 *pts = reinterpret_cast<const int2 *>(g.path) + (size_t)b * g.path_cap + (points - n);
    TempoSums v = {0, 0, 0, 0, 0};
    for (int k = lane; k < n; k += kAccThreads) {
        const int2 p = pts[k];
        tempo_add(v, tempo_point(p.x, p.y, x_limit, y_limit));
    }
    for (int m = 32; m >= 1; m >>= 1) {
        const TempoSums o = tempo_shfl_xor(v, m);
        tempo_add(v, o);
    }
    if (lane != 0) return;
    const AccompDev &d = g.d;
    const int A = d.n_anchor[b];  // 1 .. A_max while armed
    if (!d.armed[b] || A < 1 || A > g.p.A_max) {
        accomp_publish(g.w, b, 0, 0, annot_nan(), 0, 0, g.feed_no);
        return;
    }
    // 1. the clock
    const long long fed_prev = d.fed[b];
    int n_b = g.n_samples[b] - g.pending[b];
    if (n_b < 0) n_b = 0;
    const long long fed = fed_prev + n_b;
    d.fed[b] = fed;
    long long *an = d.anchors + (size_t)b * (size_t)g.p.A_max * 2;
    const long long o0 = an[2 * (A - 1)], i0 = an[2 * (A - 1) + 1];
    const long long k = d.wstate[2 * b];
    const double rate_last = d.rate[b];
    int status = kAccOn;
    // 2. waiting for the first path point
    long long base = d.base[b];
    if (base < 0) {
        if (points == 0) {
            accomp_publish(g.w, b, o0, i0, rate_last, 0, status | kAccWait, g.feed_no);
            return;
        }
        base = fed_prev;
        d.base[b] = base;
    }
    // 3. the blocks due
    int late;
    const long long k_due = accomp_due(fed, base, g.p.H, k, g.p.chunk_blocks, &late);
    if (late) status |= kAccLate;
    if (k_due == k || A >= g.p.A_max) {
        if (k_due != k) status |= kAccFull;
        accomp_publish(g.w, b, o0, i0, rate_last, 0, status, g.feed_no);
        return;
    }
    // 4. the segment, 5. its limits
    const long long o1 = k_due * g.p.H, Ls = o1 - o0, G = g.p.glide;
    const long long lo = accomp_rate_step(Ls, g.p.hop_track, g.p.hop, g.p.rate_min_pm);
    const long long hi = accomp_rate_step(Ls, g.p.hop_track, g.p.hop, g.p.rate_max_pm);
    // 6. the regression, 7. the target
    // (a point is stored: base was set with one, and a restart, which takes them away, disarms; n == 0 would run free)
    const int2 last = n > 0 ? pts[n - 1] : make_int2(0, 0);
    double sl, at;
    tempo_fit(n, v, last.x, last.y, 0.0, &sl, &at);
    long long step_raw = 0;
    bool steered = sl > 0.0;  // not NaN
    if (steered) {
        const double x1 = (double)(base + o1 + G + g.p.lead) / (double)g.p.hop;
        const double y1 = at + sl * (x1 - (double)last.x);
        const double tgt_f = floor(y1 * (double)g.p.hop_track);
        steered = fabs(tgt_f) < (double)kAccTargetLimit;  // not NaN, not infinite
        if (steered) step_raw = accomp_step_raw((long long)tgt_f, d.origin[b], i0, Ls, G);
    }
    if (!steered) {
        step_raw = accomp_nominal(Ls, g.p.hop_track, g.p.hop);
        status |= kAccFree;
    }
    // 8. - 10.
    const long long i1 = accomp_advance(i0, step_raw, lo, hi, d.n_in[b], &status);
    an[2 * A] = o1;
    an[2 * A + 1] = i1;
    d.n_anchor[b] = A + 1;
    d.n_out[b] = o1;
    const double rate = (double)(i1 - i0) / (double)Ls;
    d.rate[b] = rate;
    accomp_publish(g.w, b, o1, i1, rate, k_due - k, status, g.feed_no);
}

struct Accomp {
    AccompGeom p;
    rts_warp *plan;
    const void *tracks;
    int dtype, B, device;
    AccompDev d;
    unsigned char *words_host, *words_dev;  // kAccSlots slots of accomp_words_bytes(B)
    float *ring_host, *ring_dev;            // [kAccSlots][B][row]
    long long row;
    // what rts_live_accompany armed since the last feed, and whether the next feed disarms everyone first
    uint8_t *pend;
    long long *pend_origin, *pend_n_in;
    int pend_any, pend_disarm_all;
};

static AccompWords accomp_words(unsigned char *base, int B, int slot) {
    unsigned char *p = base + (size_t)slot * accomp_words_bytes(B);
    AccompWords w;
    w.out_total = reinterpret_cast<long long *>(p);
    w.in_pos = w.out_total + B;
    w.rate = reinterpret_cast<double *>(w.in_pos + B);
    w.blocks = reinterpret_cast<int32_t *>(w.rate + B);
    w.status = w.blocks + B;
    w.warp_status = w.status + B;
    w.seq = w.warp_status + B;
    return w;
}

static void accomp_words_clear(Accomp *a) {
    memset(a->words_host, 0, kAccSlots * accomp_words_bytes(a->B));
    for (int s = 0; s < kAccSlots; s++) {
        const AccompWords w = accomp_words(a->words_host, a->B, s);
        for (int b = 0; b < a->B; b++) w.rate[b] = __builtin_nan("");
    }
}

int accomp_check(const rts_accomp_params *q, const rts_warp *plan, int hop, int device, AccompGeom *out) {
    if (!q) return set_error(RTS_ERR_INVALID, "params is NULL");
    // the copy of the plan's layout above is held against what a plan must be: a drifted layout reads nonsense here
    if (!warp_n_ok(plan->g.N) || plan->g.H * 2 != plan->g.N || !warp_delta_ok(plan->g.delta) || !plan->g.w)
        return set_error(RTS_ERR_INVALID, "warp_plan is not a plan of rts_warp_create (N = %d, hop %d, delta %d)", plan->g.N, plan->g.H,
                         plan->g.delta);
    if (plan->device != device)
        return set_error(RTS_ERR_INVALID, "warp_plan lives on device %d, the handle on device %d", plan->device, device);
    AccompGeom p = {plan->g.H, hop, q->hop_track, q->K, q->glide, q->lead, q->rate_min_pm, q->rate_max_pm, q->chunk_blocks, q->A_max};
    switch (accomp_params_check(p)) {
    case kAccOk: break;
    case kAccBadHopTrack: return set_error(RTS_ERR_INVALID, "hop_track must be in [1, %d] (got %d)", kAccMaxHopTrack, p.hop_track);
    case kAccBadK: return set_error(RTS_ERR_INVALID, "K must be in [%d, %d] (got %d)", kAccMinK, kAccMaxK, p.K);
    case kAccBadGlide: return set_error(RTS_ERR_INVALID, "glide must be in [0, 2^31) (got %lld)", p.glide);
    case kAccBadLead: return set_error(RTS_ERR_INVALID, "|lead| must be below 2^31 (got %lld)", p.lead);
    case kAccBadRates:
        return set_error(RTS_ERR_INVALID, "rate_min_pm / rate_max_pm must satisfy 0 <= min <= max <= %d and max >= 1 (got %d, %d)",
                         kAccMaxRatePm, p.rate_min_pm, p.rate_max_pm);
    case kAccBadChunk: return set_error(RTS_ERR_INVALID, "chunk_blocks must be >= 1 (got %d)", p.chunk_blocks);
    case kAccBadAnchors: return set_error(RTS_ERR_INVALID, "A_max must be >= 2 (got %d)", p.A_max);
    case kAccOverflow:
        return set_error(RTS_ERR_UNSUPPORTED, "chunk_blocks = %d: a segment of %d blocks of %d samples could reach 2^31 samples of "
                         "output, or of the track at rate_max_pm = %d", p.chunk_blocks, p.chunk_blocks, p.H, p.rate_max_pm);
    }
    *out = p;
    return RTS_OK;
}

bool accomp_same(const Accomp *a, const AccompGeom &p, const rts_warp *plan, const void *tracks, int dtype) {
    const AccompGeom &q = a->p;
    return a->plan == plan && a->tracks == tracks && a->dtype == dtype && q.H == p.H && q.hop == p.hop && q.hop_track == p.hop_track &&
           q.K == p.K && q.glide == p.glide && q.lead == p.lead && q.rate_min_pm == p.rate_min_pm && q.rate_max_pm == p.rate_max_pm &&
           q.chunk_blocks == p.chunk_blocks && q.A_max == p.A_max;
}

void accomp_destroy(Accomp *a) {
    if (!a) return;
    void *dev[] = {a->d.fed, a->d.base, a->d.wstate, a->d.anchors, a->d.n_out, a->d.n_in, a->d.origin, a->d.rate, a->d.n_anchor,
                   a->d.armed};
    for (void *p : dev)
        if (p) (void)hipFree(p);
    if (a->words_host) (void)hipHostFree(a->words_host);
    if (a->ring_host) (void)hipHostFree(a->ring_host);
    free(a->pend);
    free(a->pend_origin);
    free(a->pend_n_in);
    free(a);
}

template <class T>
static hipError_t accomp_dev_zeroed(hipError_t e, T **p, size_t n) {
    if (e == hipSuccess) e = hipMalloc((void **)p, sizeof(T) * n);
    if (e == hipSuccess) e = hipMemset(*p, 0, sizeof(T) * n);
    return e;
}

int accomp_create(const AccompGeom &p, rts_warp *plan, const void *tracks, int dtype, int B, int device, Accomp **out) {
    Accomp *a = (Accomp *)calloc(1, sizeof(Accomp));
    if (!a) return set_error(RTS_ERR_INVALID, "out of host memory");
    a->p = p;
    a->plan = plan;
    a->tracks = tracks;
    a->dtype = dtype;
    a->B = B;
    a->device = device;
    a->row = (long long)p.chunk_blocks * p.H;  // H % 8 == 0: every row begins on a 32-byte boundary
    const size_t nB = (size_t)B;
    a->pend = (uint8_t *)calloc(nB, 1);
    a->pend_origin = (long long *)calloc(nB, sizeof(long long));
    a->pend_n_in = (long long *)calloc(nB, sizeof(long long));
    if (!a->pend || !a->pend_origin || !a->pend_n_in) {
        accomp_destroy(a);
        return set_error(RTS_ERR_INVALID, "out of host memory");
    }
    hipError_t e = hipSuccess;
    e = accomp_dev_zeroed(e, &a->d.fed, nB);
    e = accomp_dev_zeroed(e, &a->d.base, nB);
    e = accomp_dev_zeroed(e, &a->d.wstate, 2 * nB);
    e = accomp_dev_zeroed(e, &a->d.anchors, 2 * nB * (size_t)p.A_max);
    e = accomp_dev_zeroed(e, &a->d.n_out, nB);
    e = accomp_dev_zeroed(e, &a->d.n_in, nB);
    e = accomp_dev_zeroed(e, &a->d.origin, nB);
    e = accomp_dev_zeroed(e, &a->d.rate, nB);
    e = accomp_dev_zeroed(e, &a->d.n_anchor, nB);
    e = accomp_dev_zeroed(e, &a->d.armed, nB);
    const size_t ring_bytes = sizeof(float) * kAccSlots * nB * (size_t)a->row;
    if (e == hipSuccess) e = mapped_alloc(kAccSlots * accomp_words_bytes(B), (void **)&a->words_host, (void **)&a->words_dev);
    if (e == hipSuccess) e = mapped_alloc(ring_bytes, (void **)&a->ring_host, (void **)&a->ring_dev);
    if (e != hipSuccess) {
        accomp_destroy(a);
        return set_error(RTS_ERR_HIP, "rts_live_accompany: %s", hipGetErrorString(e));
    }
    accomp_words_clear(a);
    memset(a->ring_host, 0, ring_bytes);
    *out = a;
    return RTS_OK;
}

// rts_live_accompany's tables for the masked streams, checked before anything changes.
int accomp_tracks_check(int B, const uint8_t *mask, const long long *first, const long long *len, const long long *origin) {
    for (int b = 0; b < B; b++) {
        if (!mask[b]) continue;
        if (!accomp_track_ok(first[b], len[b], origin ? origin[b] : 0))
            return set_error(RTS_ERR_INVALID, "stream %d: track [%lld, %lld + %lld) with origin %lld: first and len must be >= 0 and "
                             "every position below 2^61 in magnitude", b, first[b], first[b], len[b], origin ? origin[b] : 0);
    }
    return RTS_OK;
}

// The masked streams are armed by the next feed, in whose chain the selection is enqueued.
void accomp_arm(Accomp *a, const uint8_t *mask, const long long *first, const long long *len, const long long *origin) {
    for (int b = 0; b < a->B; b++) {
        if (!mask[b]) continue;
        a->pend[b] = 1;
        a->pend_origin[b] = first[b] + (origin ? origin[b] : 0);
        a->pend_n_in[b] = first[b] + len[b];
        a->pend_any = 1;
    }
}

// Off: nothing armed is left waiting, and the first feed after it is switched on again disarms every stream.
void accomp_off(Accomp *a) {
    memset(a->pend, 0, (size_t)a->B);
    a->pend_any = 0;
    a->pend_disarm_all = 1;
}

static int accomp_disarm_all(Accomp *a, hipStream_t s) {
    RestartSel all;
    all.n = -1;
    all.set_ref = 0;
    hipLaunchKernelGGL(accomp_disarm_kernel, dim3((a->B + 63) / 64), dim3(64), 0, s, all, a->B, a->d);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

// rts_live_restart: the selected streams stop, and what was waiting to arm them is dropped.
int accomp_restart(Accomp *a, const RestartSel &sel, hipStream_t s) {
    hipLaunchKernelGGL(accomp_disarm_kernel, dim3((sel.n + 63) / 64), dim3(64), 0, s, sel, a->B, a->d);
    RTS_HIP(hipGetLastError());
    for (int i = 0; i < sel.n; i++) a->pend[sel.idx[i]] = 0;
    a->pend_any = 0;
    for (int b = 0; b < a->B; b++) a->pend_any |= a->pend[b];
    return RTS_OK;
}

// rts_live_reset, behind its synchronisation: every stream disarmed, the words as at create.
int accomp_reset(Accomp *a, hipStream_t s) {
    memset(a->pend, 0, (size_t)a->B);
    a->pend_any = 0;
    a->pend_disarm_all = 0;
    accomp_words_clear(a);
    return accomp_disarm_all(a, s);
}

// The three steps a feed adds (top of the file).  `view`: the bound tracker; n_samples / pending: the live handle's.
int accomp_enqueue(Accomp *a, const TempoTail &view, const int32_t *n_samples, const int32_t *pending, int feed_no,
                   hipStream_t s) {
    if (a->pend_disarm_all) {
        if (int rc = accomp_disarm_all(a, s); rc != RTS_OK) return rc;
        a->pend_disarm_all = 0;
    }
    if (a->pend_any) {
        AccompSel sel;
        sel.n = 0;
        for (int b = 0; b <= a->B; b++) {
            if (b < a->B && a->pend[b]) {
                sel.idx[sel.n] = b;
                sel.origin[sel.n] = a->pend_origin[b];
                sel.n_in[sel.n] = a->pend_n_in[b];
                sel.n++;
            }
            if (sel.n == kAccSelChunk || (b == a->B && sel.n > 0)) {
                hipLaunchKernelGGL(accomp_arm_kernel, dim3((sel.n + 63) / 64), dim3(64), 0, s, sel, a->d, a->p.A_max);
                RTS_HIP(hipGetLastError());
                sel.n = 0;
            }
        }
        memset(a->pend, 0, (size_t)a->B);
        a->pend_any = 0;
    }
    const int slot = feed_no % kAccSlots;
    AccompSteer g;
    g.state = view.state;
    g.state_len = view.state_len;
    g.st_n_path = view.st_n_path;
    g.path = view.path;
    g.path_cap = view.path_cap;
    g.ref_len = view.ref_len;
    g.N = view.N;
    g.n_samples = n_samples;
    g.pending = pending;
    g.p = a->p;
    g.d = a->d;
    g.w = accomp_words(a->words_dev, a->B, slot);
    g.feed_no = feed_no;
    hipLaunchKernelGGL(accomp_steer_kernel, dim3(a->B), dim3(kAccThreads), 0, s, g);
    RTS_HIP(hipGetLastError());
    return rts_warp_run(a->plan, a->tracks, a->dtype, 0, a->d.n_in, a->d.anchors, a->d.n_anchor, a->p.A_max, a->d.n_out, a->d.wstate,
                        a->p.chunk_blocks, a->ring_dev + (size_t)slot * (size_t)a->B * (size_t)a->row, a->row, g.w.warp_status,
                        a->B, s);
}

// rts_live_accompaniment: slot `feed` of the ring.  A stream whose words in that slot belong to another feed (the
// accompaniment was off in that feed, or the ring has gone round) reads blocks 0, status 0.
void accomp_look(const Accomp *a, int feed, const float **chunk_host, long long *row_stride, int32_t *blocks, long long *out_total,
                 long long *in_pos, double *rate, int32_t *status, int32_t *warp_status) {
    const int slot = feed % kAccSlots;
    const AccompWords w = accomp_words(a->words_host, a->B, slot);
    if (chunk_host) *chunk_host = a->ring_host + (size_t)slot * (size_t)a->B * (size_t)a->row;
    if (row_stride) *row_stride = a->row;
    for (int b = 0; b < a->B; b++) {
        const bool have = feed > 0 && *(const volatile int32_t *)(w.seq + b) == feed;
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        if (blocks) blocks[b] = have ? *(const volatile int32_t *)(w.blocks + b) : 0;
        if (out_total) out_total[b] = have ? *(const volatile long long *)(w.out_total + b) : 0;
        if (in_pos) in_pos[b] = have ? *(const volatile long long *)(w.in_pos + b) : 0;
        if (rate) rate[b] = have ? *(const volatile double *)(w.rate + b) : __builtin_nan("");
        if (status) status[b] = have ? *(const volatile int32_t *)(w.status + b) : 0;
        if (warp_status) warp_status[b] = have ? *(const volatile int32_t *)(w.warp_status + b) : 0;
    }
}

// rts_live_accomp_map: stream b's anchors and renderer state, synchronously.
int accomp_map(const Accomp *a, int b, long long *anchors_host, int cap, int *n, long long state[2], hipStream_t s) {
    int32_t A = 0;
    RTS_HIP(hipMemcpyAsync(&A, a->d.n_anchor + b, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (state) RTS_HIP(hipMemcpyAsync(state, a->d.wstate + 2 * (size_t)b, 2 * sizeof(long long), hipMemcpyDeviceToHost, s));
    RTS_HIP(hipStreamSynchronize(s));
    *n = A;
    int take = A < cap ? A : cap;
    if (take > a->p.A_max) take = a->p.A_max;
    if (take > 0 && anchors_host) {
        RTS_HIP(hipMemcpyAsync(anchors_host, a->d.anchors + (size_t)b * (size_t)a->p.A_max * 2, sizeof(long long) * 2 * (size_t)take,
                               hipMemcpyDeviceToHost, s));
        RTS_HIP(hipStreamSynchronize(s));
    }
    return RTS_OK;
}

}  // namespace rts
