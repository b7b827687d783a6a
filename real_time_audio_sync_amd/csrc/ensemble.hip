// Ensemble following: one microphone against several recordings of its piece, fused in beats.
//   tests.py:59-137            the harness compares two performances in beats, the scale the recordings share
//   livenote_live.py:197-202   get_beat_and_label(ln.path[-1][1]) after every insert: the member beat, here not sticky
//   the fusion step over the trackers' last path points   -> ensemble_fuse_kernel (rts_otw_consensus, rts_wtw_consensus, one
//                                                            launch per feed of a live handle)
//   the same step along offline paths, frame by frame      -> ensemble_curve_kernel (rts_path_consensus)
// The definition is include/rtsync.h's (rts_ensemble_create); the checks of the group table, its CSR form and the launch
// grids are csrc/ensemble_plan.h's.
//
// One wave per group, lane i its member i.  The sort of the definition is a rank count: lane i's rank is the number of
// in-set lanes j with v_j < v_i, or v_j == v_i and j < i, found by reading every member's value across the wave; ranks of
// the in-set are a permutation of 0 .. n-1, so median and extremes are picked by a ballot on the rank and one more
// cross-lane read.  No LDS, no atomics, no barrier.  Waves behind the groups' clear the outputs of the streams in no group.
//
// Every kernel bounds what it reads: a member's last path point inside the tracker's path_cap, path points inside min(len,
// P_max), rows inside the piece's own range (annot_lookup), members inside the CSR tables rts_ensemble_create built.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "annot_device.h"
#include "common.h"
#include "ensemble_plan.h"

namespace rts {

struct EnsembleTables {
    const int32_t *first;    // [n_groups + 1]
    const int32_t *members;  // [B]: the groups' members, then the streams in no group
    int n_groups, B;
    double max_dev;
    int patience;
};

__device__ __forceinline__ double ens_read(double v, int lane) {
    return __longlong_as_double(__shfl(__double_as_longlong(v), lane, 64));
}

struct FuseResult {
    double consensus, spread, dev;
    int n_in, n_valid;
};

// One fusion step of a wave: `beta` is this lane's member beat (lanes >= m hold no member), `strikes` / `out` its carried
// state, updated in place.  Every lane returns the group's words and its own dev.  Called by all 64 lanes.
__device__ __forceinline__ FuseResult ensemble_step(double beta, int m, int lane, double max_dev, int patience, int &strikes,
                                                    int &out) {
    const double qnan = annot_nan();
    const bool valid = lane < m && beta == beta;
    const unsigned long long vmask = __ballot(valid);
    unsigned long long inmask = __ballot(valid && !out);
    if (inmask == 0) inmask = vmask;  // everyone valid is heard again
    FuseResult r;
    r.n_valid = __popcll(vmask);
    r.n_in = __popcll(inmask);
    r.consensus = r.spread = r.dev = qnan;
    if (r.n_in == 0) return r;
    const bool in = (inmask >> lane) & 1;
    int rank = 0;
    for (int j = 0; j < m; j++) {
        const double vj = ens_read(beta, j);
        if (((inmask >> j) & 1) && (vj < beta || (vj == beta && j < lane))) rank++;
    }
    const int n = r.n_in;
    // the in-set's ranks are 0 .. n-1, each once: every ballot below has exactly one lane
    const double v_lo = ens_read(beta, __ffsll(__ballot(in && rank == (n - 1) / 2)) - 1);
    const double v_hi = ens_read(beta, __ffsll(__ballot(in && rank == n / 2)) - 1);
    const double v_min = ens_read(beta, __ffsll(__ballot(in && rank == 0)) - 1);
    const double v_max = ens_read(beta, __ffsll(__ballot(in && rank == n - 1)) - 1);
    const double c = (n & 1) ? v_lo : (v_lo + v_hi) * 0.5;
    const double sp = v_max - v_min;
    r.consensus = c == c ? c : qnan;
    r.spread = sp == sp ? sp : qnan;
    if (valid) {
        const double d = beta - c;
        r.dev = d == d ? d : qnan;
        if (fabs(d) > max_dev) strikes = strikes + 1 < patience ? strikes + 1 : patience;
        else strikes = 0;
        out = strikes >= patience ? 1 : 0;
    }
    return r;
}

struct EnsembleFuse {
    const int32_t *state;  // the tracker's state words, state_len per stream
    int state_len, st_n_path;
    const int32_t *path;  // [B][path_cap][2]
    int path_cap;
    const int32_t *piece, *frame0;  // [B] device; frame0 may be NULL
    int32_t *strikes, *out;         // [B] the ensemble's carried state
    EnsembleOut o;
};

// grid ensemble_grid(n_groups, loose) of kEnsembleThreads lanes: wave w < n_groups is group w, the waves behind take 64
// streams in no group each.
__global__ void __launch_bounds__(kEnsembleThreads) ensemble_fuse_kernel(EnsembleTables e, AnnotTables t, EnsembleFuse f) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * kEnsembleWaves + (threadIdx.x >> 6);
    const int grouped = e.first[e.n_groups];
    if (w >= e.n_groups) {
        const int at = grouped + (w - e.n_groups) * 64 + lane;
        if (at < e.B) {
            const int b = e.members[at];
            f.o.dev[b] = annot_nan();
            f.o.strikes[b] = 0;
            f.o.out[b] = 0;
        }
        __threadfence_system();
        return;
    }
    const int lo = e.first[w];
    int m = e.first[w + 1] - lo;
    if (m > kEnsembleMaxMembers) m = kEnsembleMaxMembers;  // (rts_ensemble_create refuses such a table)
    int b = -1, strikes = 0, out = 0;
    double beta = annot_nan();
    if (lane < m) {
        b = e.members[lo + lane];
        strikes = f.strikes[b];
        out = f.out[b];
        int pts = f.state[(size_t)b * f.state_len + f.st_n_path];  // counts on past path_cap once the path is truncated
        if (pts > f.path_cap) pts = f.path_cap;
        if (pts >= 1) {
            const int32_t j = f.path[((size_t)b * f.path_cap + (pts - 1)) * 2 + 1];
            const long long frame = j < 0 ? -1 : (long long)j + (f.frame0 ? f.frame0[b] : 0);
            int seg;
            beta = annot_lookup(annot_piece(t, f.piece[b]), frame, t.frame_seconds, &seg);
        }
    }
    const FuseResult r = ensemble_step(beta, m, lane, e.max_dev, e.patience, strikes, out);
    if (lane < m) {
        f.strikes[b] = strikes;
        f.out[b] = out;
        f.o.dev[b] = r.dev;
        f.o.strikes[b] = strikes;
        f.o.out[b] = out;
    }
    if (lane == 0) {
        f.o.consensus[w] = r.consensus;
        f.o.spread[w] = r.spread;
        f.o.n_in[w] = r.n_in;
        f.o.n_valid[w] = r.n_valid;
    }
    __threadfence_system();
}

struct EnsembleCurve {
    const int32_t *path;  // [B][P_max][2]
    int P_max;
    const int32_t *len;             // [B]
    const int32_t *piece, *frame0;  // [B]; frame0 may be NULL
    int T;
    double *consensus, *spread;  // [n_groups][T]; spread may be NULL
    int32_t *n_in;               // [n_groups][T] or NULL
    int32_t *out;                // [B][T] or NULL
};

// Same grid.  Per wave: frames in stretches of kEnsembleStage; lane i walks member i's path with a cursor (the last point
// with x <= t), looks its beat up when the cursor's y changed, and the wave runs the step; lane (t mod 64) keeps the group's
// words of frame t, every lane the 64 `out` bits of its member, and the stretch is stored with lanes along t.
__global__ void __launch_bounds__(kEnsembleThreads) ensemble_curve_kernel(EnsembleTables e, AnnotTables t, EnsembleCurve c) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * kEnsembleWaves + (threadIdx.x >> 6);
    const int grouped = e.first[e.n_groups];
    if (w >= e.n_groups) {
        if (!c.out) return;
        const int at0 = grouped + (w - e.n_groups) * 64;
        const int cnt = e.B - at0 < 64 ? e.B - at0 : 64;
        for (int i = 0; i < cnt; i++) {
            int32_t *row = c.out + (size_t)e.members[at0 + i] * c.T;
            for (int k = lane; k < c.T; k += 64) row[k] = 0;
        }
        return;
    }
    const int lo = e.first[w];
    int m = e.first[w + 1] - lo;
    if (m > kEnsembleMaxMembers) m = kEnsembleMaxMembers;
    int b = 0, n = 0, piece = -1, frame0 = 0;
    if (lane < m) {
        b = e.members[lo + lane];
        n = c.len[b];
        if (n > c.P_max) n = c.P_max;
        if (n < 0) n = 0;
        piece = c.piece[b];
        frame0 = c.frame0 ? c.frame0[b] : 0;
    }
    const AnnotPiece tab = annot_piece(t, piece);
    const int2 *pts = reinterpret_cast<const int2 *>(c.path) + (size_t)b * c.P_max;
    int k = -1;                                    // the cursor: the last point with x <= t
    int next_x = n > 0 ? pts[0].x : 0x7fffffff;    // x of point k + 1
    int y = -1, y_seen = -2;
    double beta = annot_nan();
    int strikes = 0, out = 0;
    for (int t0 = 0; t0 < c.T; t0 += kEnsembleStage) {
        const int span = c.T - t0 < kEnsembleStage ? c.T - t0 : kEnsembleStage;
        double my_c = annot_nan(), my_s = annot_nan();
        int my_n = 0;
        unsigned long long out_bits = 0;
        for (int q = 0; q < span; q++) {
            const int tt = t0 + q;
            while (k + 1 < n && next_x <= tt) {
                k++;
                y = pts[k].y;
                next_x = k + 1 < n ? pts[k + 1].x : 0x7fffffff;
            }
            if (y != y_seen) {
                int seg;
                beta = annot_lookup(tab, y < 0 ? -1 : (long long)y + frame0, t.frame_seconds, &seg);
                y_seen = y;
            }
            const FuseResult r = ensemble_step(beta, m, lane, e.max_dev, e.patience, strikes, out);
            if (lane == q) {
                my_c = r.consensus;
                my_s = r.spread;
                my_n = r.n_in;
            }
            out_bits |= (unsigned long long)out << q;
        }
        if (lane < span) {
            const size_t at = (size_t)w * c.T + t0 + lane;
            c.consensus[at] = my_c;
            if (c.spread) c.spread[at] = my_s;
            if (c.n_in) c.n_in[at] = my_n;
        }
        if (c.out) {
            for (int i = 0; i < m; i++) {
                const unsigned long long bits = __shfl(out_bits, i, 64);
                const int bi = __shfl(b, i, 64);
                if (lane < span) c.out[(size_t)bi * c.T + t0 + lane] = (int32_t)((bits >> lane) & 1);
            }
        }
    }
}

// rts_ensemble_reset with a mask: the selection by value, like a restart's
__global__ void ensemble_reset_kernel(RestartSel sel, int32_t *strikes, int32_t *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= sel.n) return;
    strikes[sel.idx[i]] = 0;
    out[sel.idx[i]] = 0;
}

}  // namespace rts

struct rts_ensemble {
    rts::EnsembleTables t;  // device pointers
    int loose;              // streams in no group
    int device;
    int32_t *block;    // the one allocation: first[n_groups + 1], members[B], strikes[B], out[B]
    int32_t *strikes;  // out = strikes + B
};

namespace rts {

int ensemble_batch(const rts_ensemble *e) { return e->t.B; }
int ensemble_groups(const rts_ensemble *e) { return e->t.n_groups; }
int ensemble_device(const rts_ensemble *e) { return e->device; }
int32_t *ensemble_state(const rts_ensemble *e) { return e->strikes; }

int ensemble_fuse_enqueue(rts_ensemble *e, const rts_annot *annot, const TempoTail &view, const int32_t *piece,
                          const int32_t *frame0, const EnsembleOut &o, hipStream_t s) {
    EnsembleFuse f = {};
    f.state = view.state;
    f.state_len = view.state_len;
    f.st_n_path = view.st_n_path;
    f.path = view.path;
    f.path_cap = view.path_cap;
    f.piece = piece;
    f.frame0 = frame0;
    f.strikes = e->strikes;
    f.out = e->strikes + e->t.B;
    f.o = o;
    hipLaunchKernelGGL(ensemble_fuse_kernel, dim3(ensemble_grid(e->t.n_groups, e->loose)), dim3(kEnsembleThreads), 0, s, e->t,
                       *annot_tables(annot), f);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

// rts_otw_consensus / rts_wtw_consensus behind their views
static int tracker_consensus(const TempoTail &view, rts_ensemble *e, rts_annot *a, const int32_t *piece_dev,
                             const int32_t *frame0_dev, double *group_dev, int32_t *group_n_dev, double *dev_dev,
                             int32_t *member_dev, void *stream) {
    if (!e) return set_error(RTS_ERR_INVALID, "the ensemble handle e is NULL");
    if (!a) return set_error(RTS_ERR_INVALID, "the tables a are NULL");
    if (!piece_dev) return set_error(RTS_ERR_INVALID, "piece_dev is NULL");
    if (!group_dev || !group_n_dev || !dev_dev || !member_dev)
        return set_error(RTS_ERR_INVALID, "group_dev, group_n_dev, dev_dev and member_dev must be given");
    if (e->t.B != view.B)
        return set_error(RTS_ERR_INVALID, "the ensemble e was created for B = %d streams, the tracker has %d", e->t.B, view.B);
    if (int rc = check_device(e->device, "ensemble handle e"); rc != RTS_OK) return rc;
    if (int rc = check_device(annot_device(a), "tables a"); rc != RTS_OK) return rc;
    const int G = e->t.n_groups, B = e->t.B;
    const EnsembleOut o = {group_dev, group_dev + G, group_n_dev, group_n_dev + G, dev_dev, member_dev, member_dev + B};
    return ensemble_fuse_enqueue(e, a, view, piece_dev, frame0_dev, o, (hipStream_t)stream);
}

}  // namespace rts

extern "C" {

int rts_ensemble_destroy(rts_ensemble *h) {
    if (!h) return RTS_OK;
    if (h->block) (void)hipFree(h->block);
    free(h);
    return RTS_OK;
}

int rts_ensemble_create(int B, const int32_t *group_host, int n_groups, double max_dev, int patience, rts_ensemble **out) {
    using namespace rts;
    if (!out) return set_error(RTS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!group_host) return set_error(RTS_ERR_INVALID, "group_host is NULL");
    EnsembleFault where;
    if (const EnsembleRefusal why = ensemble_check(B, group_host, n_groups, max_dev, patience, &where); why != kEnsembleOk) {
        char msg[256];
        ensemble_message(msg, sizeof(msg), why, where, B, n_groups);
        return set_error(RTS_ERR_INVALID, "%s", msg);
    }
    const size_t nB = (size_t)B, nG = (size_t)n_groups, words = nG + 1 + 3 * nB;
    rts_ensemble *h = (rts_ensemble *)calloc(1, sizeof(rts_ensemble));
    int32_t *host = (int32_t *)calloc(words, sizeof(int32_t));  // strikes and out start at zero
    if (!h || !host) {
        free(h);
        free(host);
        return set_error(RTS_ERR_INVALID, "out of host memory");
    }
    const int grouped = ensemble_csr(B, group_host, n_groups, host, host + nG + 1);
    hipError_t e = hipGetDevice(&h->device);
    if (e == hipSuccess) e = hipMalloc((void **)&h->block, sizeof(int32_t) * words);
    if (e == hipSuccess) e = hipMemcpy(h->block, host, sizeof(int32_t) * words, hipMemcpyHostToDevice);
    free(host);
    if (e != hipSuccess) {
        rts_ensemble_destroy(h);
        return set_error(RTS_ERR_HIP, "rts_ensemble_create: %s", hipGetErrorString(e));
    }
    h->t.first = h->block;
    h->t.members = h->block + nG + 1;
    h->t.n_groups = n_groups;
    h->t.B = B;
    h->t.max_dev = max_dev;
    h->t.patience = patience;
    h->strikes = h->block + nG + 1 + nB;
    h->loose = B - grouped;
    *out = h;
    return RTS_OK;
}

int rts_ensemble_reset(rts_ensemble *h, const uint8_t *mask_host, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    const int B = h->t.B;
    if (!mask_host) {
        RTS_HIP(hipMemsetAsync(h->strikes, 0, sizeof(int32_t) * 2 * (size_t)B, (hipStream_t)stream));
        return RTS_OK;
    }
    RestartSel sel;
    for (int pos = 0; restart_next_chunk(B, mask_host, nullptr, nullptr, &pos, &sel) > 0;) {
        hipLaunchKernelGGL(ensemble_reset_kernel, dim3((sel.n + 63) / 64), dim3(64), 0, (hipStream_t)stream, sel, h->strikes,
                           h->strikes + B);
        RTS_HIP(hipGetLastError());
    }
    return RTS_OK;
}

int rts_otw_consensus(rts_otw *h, rts_ensemble *e, rts_annot *a, const int32_t *piece_dev, const int32_t *frame0_dev,
                      double *group_dev, int32_t *group_n_dev, double *dev_dev, int32_t *member_dev, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    TempoTail view = {};
    otw_tempo_view(h, &view);
    return tracker_consensus(view, e, a, piece_dev, frame0_dev, group_dev, group_n_dev, dev_dev, member_dev, stream);
}

int rts_wtw_consensus(rts_wtw *h, rts_ensemble *e, rts_annot *a, const int32_t *piece_dev, const int32_t *frame0_dev,
                      double *group_dev, int32_t *group_n_dev, double *dev_dev, int32_t *member_dev, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    TempoTail view = {};
    wtw_tempo_view(h, &view);
    return tracker_consensus(view, e, a, piece_dev, frame0_dev, group_dev, group_n_dev, dev_dev, member_dev, stream);
}

int rts_path_consensus(rts_ensemble *e, rts_annot *a, const int32_t *path_dev, int P_max, const int32_t *len_dev,
                       const int32_t *piece_dev, const int32_t *frame0_dev, int T, double *consensus_dev, double *spread_dev,
                       int32_t *n_in_dev, int32_t *out_dev, void *stream) {
    using namespace rts;
    if (!e) return set_error(RTS_ERR_INVALID, "the ensemble handle e is NULL");
    if (!a) return set_error(RTS_ERR_INVALID, "the tables a are NULL");
    if (!len_dev) return set_error(RTS_ERR_INVALID, "len_dev is NULL");
    if (!piece_dev) return set_error(RTS_ERR_INVALID, "piece_dev is NULL");
    if (P_max < 0 || (P_max > 0 && !path_dev)) return set_error(RTS_ERR_INVALID, "path_dev is NULL or P_max < 0");
    if (T < 0) return set_error(RTS_ERR_INVALID, "T must be >= 0 (got %d)", T);
    if (T > 0 && !consensus_dev) return set_error(RTS_ERR_INVALID, "consensus_dev is NULL");
    if (int rc = check_device(e->device, "ensemble handle e"); rc != RTS_OK) return rc;
    if (int rc = check_device(annot_device(a), "tables a"); rc != RTS_OK) return rc;
    if (T == 0) return RTS_OK;
    const EnsembleCurve c = {path_dev, P_max, len_dev, piece_dev, frame0_dev, T, consensus_dev, spread_dev, n_in_dev, out_dev};
    hipLaunchKernelGGL(ensemble_curve_kernel, dim3(ensemble_grid(e->t.n_groups, e->loose)), dim3(kEnsembleThreads), 0,
                       (hipStream_t)stream, e->t, *annot_tables(a), c);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

}  // extern "C"
