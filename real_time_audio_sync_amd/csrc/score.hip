// Following a score: the chroma a note list leaves, frame by frame, as the chroma chain would hear it.
// The definition is include/rtsync.h's (rts_score_create); the limits, the table rules, the workspace layout and the grids are
// csrc/score_plan.h's; tests/score_model.py is the serial restatement.
//
// A frame's sum over the notes is one ordered float64 chain, so the parallelism is over frames: a wave takes 64 consecutive
// frames of one piece, one frame and twelve accumulators per lane, and walks the notes in index order, 64 at a time: every
// lane loads one note, and the notes that can reach the wave are handed round by readlane.  The note record and its row of
// T are then the same for every lane; each lane clamps the note to its own window, looks its two window energies and its
// decay up (CW is 32 KB at fft_len 4096 and stays in the caches) and adds.  No lane leaves the loop early, so the order of the
// additions is the definition's.
//
// Which notes a wave walks: those between the first note that may still sound in its first frame and the first note none of
// whose successors starts before its last frame's window ends.  Both ends come from tables that do not decrease along a piece
// whatever order its notes have -- the running maximum of the ends, the running minimum (from the back) of the onsets, valid
// notes only -- so each is one bisection, a pedal note that has ended costs later frames nothing, and leaving the other notes
// out never changes a sum: such a note has b <= a in every frame of the wave.  score_prepare_kernel writes the two tables and
// every valid note's onset frame into the workspace, counts the invalid notes and sets the status words.
//
// Every read is bounded here: a piece whose note range leaves [0, n_notes) reads no note, a piece whose frame range leaves
// the pool writes no frame, CW and DK are indexed by clamped values, T by a pitch that passed the check.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "common.h"
#include "score_plan.h"

namespace rts {

struct ScoreTables {
    const double *T, *CW, *DK;  // device
    int L, H, pad, K;
};

struct ScoreArgs {
    const long long *onset, *end;
    const int32_t *pitch;
    const double *energy;
    long long n_notes;
    const long long *note_first, *frame_first;
    const int32_t *note_len, *n_frames;
    long long n_pool;
    int normalize, out_f64;
    void *out;
    int32_t *skipped, *status;
    long long *emax, *omin;       // workspace (score_plan.h)
    unsigned long long *oframe;
};

constexpr long long kI64Min = (long long)0x8000000000000000ULL, kI64Max = 0x7fffffffffffffffLL;

__device__ __forceinline__ bool note_ok(long long on, long long en, int32_t pitch, double e) {
    return pitch >= 0 && pitch < kScorePitches && on >= 0 && en >= on && e >= 0.0 && e <= 1.7976931348623157e308;
}

// lane j's value of x in every lane; j is the same for every lane
__device__ __forceinline__ unsigned long long lane_u64(unsigned long long x, int j) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, j);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x >> 32), j);
    return ((unsigned long long)hi << 32) | lo;
}

struct ScorePiece {
    long long note_first, frame_first;
    int32_t note_len, n_frames;
    int status;
};
__device__ __forceinline__ ScorePiece score_piece(const ScoreArgs &g, int p) {
    ScorePiece q;
    q.note_first = g.note_first[p];
    q.note_len = g.note_len[p];
    q.frame_first = g.frame_first[p];
    q.n_frames = g.n_frames[p];
    q.status = RTS_SCORE_OK;
    if (q.note_first < 0 || q.note_len < 0 || q.note_first > g.n_notes - q.note_len) q.status |= RTS_SCORE_NOTES;
    if (q.n_frames >= 1 && (q.frame_first < 0 || q.frame_first > g.n_pool - q.n_frames)) q.status |= RTS_SCORE_FRAMES;
    return q;
}

// grid P, one wave: the piece's three workspace tables in chunks of 64 notes, a scan across the lanes and a carry.
__global__ void __launch_bounds__(kScoreWave) score_prepare_kernel(ScoreTables pl, ScoreArgs g) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const ScorePiece q = score_piece(g, p);
    int skipped = 0;
    if (!(q.status & RTS_SCORE_NOTES) && q.note_len > 0) {
        const long long nl = q.note_len;
        long long carry = kI64Min;
        for (long long base = 0; base < nl; base += kScoreWave) {
            const long long i = base + lane;
            const bool in = i < nl;
            long long e = kI64Min;
            unsigned long long of = 0;
            bool ok = false;
            if (in) {
                const long long n = q.note_first + i, on = g.onset[n], en = g.end[n];
                ok = note_ok(on, en, g.pitch[n], g.energy[n]);
                if (ok) {
                    e = en;
                    of = ((unsigned long long)on + (unsigned long long)pl.pad) / (unsigned long long)pl.H;
                }
            }
            skipped += __popcll(__ballot(in && !ok));
#pragma unroll
            for (int d = 1; d < kScoreWave; d <<= 1) {
                const long long o = __shfl_up(e, d);
                if (lane >= d && o > e) e = o;
            }
            if (carry > e) e = carry;
            if (in) {
                g.emax[q.note_first + i] = e;
                g.oframe[q.note_first + i] = of;
            }
            carry = __shfl(e, kScoreWave - 1);
        }
        carry = kI64Max;
        for (long long base = (nl - 1) / kScoreWave * kScoreWave; base >= 0; base -= kScoreWave) {
            const long long i = base + lane;
            const bool in = i < nl;
            long long o = kI64Max;
            if (in) {
                const long long n = q.note_first + i, on = g.onset[n];
                if (note_ok(on, g.end[n], g.pitch[n], g.energy[n])) o = on;
            }
#pragma unroll
            for (int d = 1; d < kScoreWave; d <<= 1) {
                const long long x = __shfl_down(o, d);
                if (lane + d < kScoreWave && x < o) o = x;
            }
            if (carry < o) o = carry;
            if (in) g.omin[q.note_first + i] = o;
            carry = __shfl(o, 0);
        }
    }
    if (lane == 0) {
        if (g.skipped) g.skipped[p] = skipped;
        if (g.status) g.status[p] = q.status;
    }
}

// grid (ceil(n_pool / 256), P), four waves: a wave takes frames [tile, tile + 64) of piece blockIdx.y.
__global__ void __launch_bounds__(kScoreThreads) score_main_kernel(ScoreTables pl, ScoreArgs g) {
    const int p = blockIdx.y, lane = threadIdx.x & (kScoreWave - 1), wave = threadIdx.x / kScoreWave;
    const ScorePiece q = score_piece(g, p);
    const long long tile = ((long long)blockIdx.x * kScoreWaves + wave) * kScoreWave;
    if (q.status != RTS_SCORE_OK || tile >= q.n_frames) return;
    const long long L = pl.L, H = pl.H;
    const long long m = tile + lane, m_last = q.n_frames - 1 < tile + kScoreWave - 1 ? q.n_frames - 1 : tile + kScoreWave - 1;
    const long long w0 = m * H - pl.pad, w1 = w0 + L;
    const long long first_w0 = tile * H - pl.pad, last_w1 = m_last * H - pl.pad + L;
    // the first note whose running maximum of ends lies behind the wave's first window start ...
    long long lo = 0, hi = q.note_len;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (g.emax[q.note_first + mid] > first_w0) hi = mid;
        else lo = mid + 1;
    }
    const int i_lo = __builtin_amdgcn_readfirstlane((int)lo);
    // ... and the first from which on no note starts before the wave's last window ends
    lo = i_lo;
    hi = q.note_len;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (g.omin[q.note_first + mid] >= last_w1) hi = mid;
        else lo = mid + 1;
    }
    const int i_hi = __builtin_amdgcn_readfirstlane((int)lo);

    double acc[kScoreCh];
#pragma unroll
    for (int c = 0; c < kScoreCh; c++) acc[c] = 0.0;
    const unsigned long long um = (unsigned long long)m, K = (unsigned long long)pl.K;
    // 64 notes at a time: lane l reads note base + l (one coalesced load per field) and says whether it can reach the wave at
    // all -- a note that cannot sound, or, behind a long note that keeps the running maximum up, one that has ended before the
    // wave's first window begins or starts behind its last, has b <= a in every lane.  The others are handed round in index
    // order, one broadcast each, so no lane waits on a load per note.
    for (int base = i_lo; base < i_hi; base += kScoreWave) {
        long long my_on = 0, my_en = 0;
        int32_t my_pitch = 0;
        double my_e = 0.0;
        unsigned long long my_of = 0;
        bool reach = false;
        if (base + lane < i_hi) {
            const long long n = q.note_first + base + lane;
            my_on = g.onset[n];
            my_en = g.end[n];
            my_pitch = g.pitch[n];
            my_e = g.energy[n];
            my_of = g.oframe[n];
            reach = note_ok(my_on, my_en, my_pitch, my_e) && my_en > first_w0 && my_on < last_w1;
        }
        for (unsigned long long todo = __ballot(reach); todo; todo &= todo - 1) {
            const int j = __builtin_ctzll(todo);
            const long long on = (long long)lane_u64((unsigned long long)my_on, j), en = (long long)lane_u64((unsigned long long)my_en, j);
            const unsigned long long of = lane_u64(my_of, j);
            const double e = __longlong_as_double((long long)lane_u64((unsigned long long)__double_as_longlong(my_e), j));
            const double *row = pl.T + (size_t)__builtin_amdgcn_readlane(my_pitch, j) * kScoreCh;
            const int a = on <= w0 ? 0 : on >= w1 ? (int)L : (int)(on - w0);
            const int b = en <= w0 ? 0 : en >= w1 ? (int)L : (int)(en - w0);
            if (b > a) {
                const unsigned long long k = um <= of ? 0 : um - of >= K ? K : um - of;
                const double wgt = (e * pl.DK[k]) * (pl.CW[b] - pl.CW[a]);
#pragma unroll
                for (int c = 0; c < kScoreCh; c++) acc[c] = acc[c] + wgt * row[c];
            }
        }
    }
    if (m >= q.n_frames) return;
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < kScoreCh; c++) s = s + acc[c] * acc[c];
    double len = sqrt(s);
    if (!g.normalize || len < 2.2250738585072014e-308) len = 1.0;  // the rule of the chroma kernels
    const size_t o = (size_t)(q.frame_first + m) * kScoreCh;
    if (g.out_f64) {
        double *out = reinterpret_cast<double *>(g.out) + o;
#pragma unroll
        for (int c = 0; c < kScoreCh; c++) out[c] = acc[c] / len;
    } else {
        float *out = reinterpret_cast<float *>(g.out) + o;
#pragma unroll
        for (int c = 0; c < kScoreCh; c++) out[c] = (float)(acc[c] / len);
    }
}

}  // namespace rts

struct rts_score {
    rts::ScoreTables t;  // device pointers
    int device;
    void *block;  // the one allocation behind them
};

extern "C" {

int rts_score_destroy(rts_score *h) {
    if (!h) return RTS_OK;
    if (h->block) (void)hipFree(h->block);
    free(h);
    return RTS_OK;
}

int rts_score_create(int fft_len, int hop, int pad_left, int K, const double *T_host, const double *CW_host,
                     const double *DK_host, rts_score **out) {
    using namespace rts;
    if (!out) return set_error(RTS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!T_host || !CW_host || !DK_host) return set_error(RTS_ERR_INVALID, "T_host, CW_host and DK_host must be given");
    long long where = -1;
    ScoreRefusal why = score_plan_check(fft_len, hop, pad_left, K);
    if (why == kScoreOk) why = score_tables_check(fft_len, K, T_host, CW_host, DK_host, &where);
    if (why != kScoreOk) {
        char msg[256];
        score_message(msg, sizeof(msg), why, where);
        return set_error(why == kScoreFftLen ? RTS_ERR_UNSUPPORTED : RTS_ERR_INVALID, "%s", msg);
    }
    rts_score *h = (rts_score *)calloc(1, sizeof(rts_score));
    if (!h) return set_error(RTS_ERR_INVALID, "out of host memory");
    const size_t n_t = (size_t)kScorePitches * kScoreCh, n_cw = (size_t)fft_len + 1, n_dk = (size_t)K + 1;
    hipError_t e = hipGetDevice(&h->device);
    if (e == hipSuccess) e = hipMalloc(&h->block, sizeof(double) * (n_t + n_cw + n_dk));
    double *d = static_cast<double *>(h->block);
    if (e == hipSuccess) e = hipMemcpy(d, T_host, sizeof(double) * n_t, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + n_t, CW_host, sizeof(double) * n_cw, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + n_t + n_cw, DK_host, sizeof(double) * n_dk, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        rts_score_destroy(h);
        return set_error(RTS_ERR_HIP, "rts_score_create: %s", hipGetErrorString(e));
    }
    h->t.T = d;
    h->t.CW = d + n_t;
    h->t.DK = d + n_t + n_cw;
    h->t.L = fft_len;
    h->t.H = hop;
    h->t.pad = pad_left;
    h->t.K = K;
    *out = h;
    return RTS_OK;
}

int rts_score_workspace_bytes(long long n_notes, size_t *bytes) {
    using namespace rts;
    if (!bytes) return set_error(RTS_ERR_INVALID, "bytes is NULL");
    if (n_notes < 0 || n_notes > kScoreLimit31 - 1) return set_error(RTS_ERR_INVALID, "n_notes must be in [0, 2^31)");
    *bytes = score_workspace_bytes(n_notes);
    return RTS_OK;
}

int rts_score_chroma(rts_score *h, const long long *onset_dev, const long long *end_dev, const int32_t *pitch_dev,
                     const double *energy_dev, long long n_notes, const long long *note_first_dev, const int32_t *note_len_dev,
                     const long long *frame_first_dev, const int32_t *n_frames_dev, int P, int normalize, void *out_dev,
                     int out_dtype, long long n_pool_frames, int32_t *skipped_dev, int32_t *status_dev, void *workspace,
                     size_t workspace_bytes, void *stream) {
    using namespace rts;
    if (!h) return set_error(RTS_ERR_INVALID, "handle is NULL");
    ScoreCall c;
    c.n_notes = n_notes;
    c.n_pool_frames = n_pool_frames;
    c.P = P;
    c.out_dtype = out_dtype;
    c.notes_given = onset_dev && end_dev && pitch_dev && energy_dev;
    c.pieces_given = note_first_dev && note_len_dev && frame_first_dev && n_frames_dev;
    c.out_given = out_dev != nullptr;
    c.workspace_given = workspace != nullptr;
    c.workspace_bytes = workspace_bytes;
    if (const ScoreRefusal why = score_call_check(c); why != kScoreOk) {
        char msg[256];
        score_message(msg, sizeof(msg), why, -1);
        return set_error(RTS_ERR_INVALID, "%s", msg);
    }
    if (reinterpret_cast<uintptr_t>(workspace) % sizeof(long long)) return set_error(RTS_ERR_INVALID, "workspace must be 8-byte aligned");
    if (int rc = check_device(h->device, "handle"); rc != RTS_OK) return rc;
    ScoreArgs g;
    g.onset = onset_dev;
    g.end = end_dev;
    g.pitch = pitch_dev;
    g.energy = energy_dev;
    g.n_notes = n_notes;
    g.note_first = note_first_dev;
    g.frame_first = frame_first_dev;
    g.note_len = note_len_dev;
    g.n_frames = n_frames_dev;
    g.n_pool = n_pool_frames;
    g.normalize = normalize != 0;
    g.out_f64 = out_dtype == RTS_F64;
    g.out = out_dev;
    g.skipped = skipped_dev;
    g.status = status_dev;
    g.emax = static_cast<long long *>(workspace);
    g.omin = g.emax ? g.emax + n_notes : nullptr;
    g.oframe = g.emax ? reinterpret_cast<unsigned long long *>(g.emax + 2 * n_notes) : nullptr;
    hipLaunchKernelGGL(score_prepare_kernel, dim3(P), dim3(kScoreWave), 0, (hipStream_t)stream, h->t, g);
    RTS_HIP(hipGetLastError());
    const ScoreGrid grid = score_main_grid(P, n_pool_frames);
    hipLaunchKernelGGL(score_main_kernel, dim3(grid.x, grid.y), dim3(kScoreThreads), 0, (hipStream_t)stream, h->t, g);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

}  // extern "C"
