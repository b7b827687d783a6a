// Host side of the annotation tables (csrc/annot.hip): the checks rts_annot_create makes on the tables before anything is
// allocated, and the launch geometry of the two batched kernels.  No HIP in it, so tests/sanitize/annot_driver.cpp runs it
// stand-alone.
//
// A table is n >= 1 rows (time_s, beat) of one piece's ground truth (Songs/<piece>/<recording>.csv, tests.py:45-57); P
// tables lie back to back in one pool, piece p being rows [first[p], first[p] + len[p]).  The reference looks a time up
// with a linear search for the first row whose closed interval [times[i-1], times[i]] ([.., times[0]] for the first)
// contains it (tests.py:112-128, livenote_live.py:211-227).  With non-decreasing times that row is the first i with
// time <= times[i], so the device searches by bisection; the interval's width times[i] - times[i-1] is then > 0 whenever
// the row is found (a zero-width row i > 0 is never the first), and the division of the interpolation is safe.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

namespace rts {

enum AnnotRefusal {
    kAnnotOk = 0,
    kAnnotNoPieces,   // P < 1
    kAnnotShort,      // len[p] < 1
    kAnnotRange,      // first[p] < 0 or first[p] + len[p] past the pool
    kAnnotTime,       // a NaN or infinite time
    kAnnotOrder,      // times[row] < times[row - 1]
    kAnnotBeat,       // a negative beat
};

struct AnnotFault {
    int piece;       // the piece that breaks a rule (-1 for kAnnotNoPieces)
    long long row;   // the row inside that piece (-1 where the rule is about the range)
};

// The first rule broken, pieces in order and rows in order inside a piece.  Reads rows of pieces whose range has passed
// its own check only.
inline AnnotRefusal annot_check(int P, long long n_rows, const long long *first, const int32_t *len, const double *times,
                                const int32_t *beats, AnnotFault *where) {
    where->piece = -1;
    where->row = -1;
    if (P < 1) return kAnnotNoPieces;
    for (int p = 0; p < P; p++) {
        where->piece = p;
        where->row = -1;
        if (len[p] < 1) return kAnnotShort;
        if (first[p] < 0 || first[p] > n_rows - len[p]) return kAnnotRange;
        const double *t = times + first[p];
        const int32_t *bt = beats + first[p];
        for (int32_t i = 0; i < len[p]; i++) {
            where->row = i;
            if (!isfinite(t[i])) return kAnnotTime;
            if (i > 0 && t[i] < t[i - 1]) return kAnnotOrder;
            if (bt[i] < 0) return kAnnotBeat;
        }
    }
    return kAnnotOk;
}

// A piece is invertible -- rts_annot_frames maps a beat back to a frame of it -- when its beats are strictly increasing.
// Decided once per piece at rts_annot_create, on tables that passed annot_check.
inline bool annot_invertible(const int32_t *beats, int32_t n) {
    for (int32_t i = 1; i < n; i++)
        if (beats[i] <= beats[i - 1]) return false;
    return n >= 1;
}

// The message of a refusal, naming piece and row.
inline void annot_message(char *buf, size_t size, AnnotRefusal why, const AnnotFault &w, long long n_rows) {
    switch (why) {
    case kAnnotOk: snprintf(buf, size, "ok"); break;
    case kAnnotNoPieces: snprintf(buf, size, "P must be >= 1"); break;
    case kAnnotShort: snprintf(buf, size, "piece %d: a table needs at least one row", w.piece); break;
    case kAnnotRange: snprintf(buf, size, "piece %d: its rows reach outside the pool of %lld rows", w.piece, n_rows); break;
    case kAnnotTime: snprintf(buf, size, "piece %d, row %lld: the time is not finite", w.piece, w.row); break;
    case kAnnotOrder:
        snprintf(buf, size, "piece %d, row %lld: the time is below that of row %lld (times must not decrease)", w.piece, w.row,
                 w.row - 1);
        break;
    case kAnnotBeat: snprintf(buf, size, "piece %d, row %lld: the beat is negative", w.piece, w.row); break;
    }
}

// ---- launch geometry ------------------------------------------------------------------------------------------------
constexpr int kAnnotThreads = 256;  // both batched kernels
// rts_annot_path_error: path points a workgroup looks up between two turns of the lane that carries the float64 sum
// (8 KB of LDS).  Four points per lane and turn.
constexpr int kAnnotChunk = 1024;
constexpr int kAnnotLiveThreads = 64;  // the per-feed kernel: one lane per stream

struct AnnotGrid {
    unsigned x, y;
};
// rts_annot_beats: one lane per (stream, entry), streams along y.
inline AnnotGrid annot_beats_grid(int B, int n_max) {
    const AnnotGrid g = {(unsigned)((n_max + kAnnotThreads - 1) / kAnnotThreads), (unsigned)B};
    return g;
}
// the per-feed kernel
inline unsigned annot_live_grid(int B) { return (unsigned)((B + kAnnotLiveThreads - 1) / kAnnotLiveThreads); }

}  // namespace rts
