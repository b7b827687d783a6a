// The annotation tables as the kernels see them, and the lookup of one frame (csrc/annot.hip has the definition's
// comment; csrc/tempo.hip reads the same rows for its beats-per-minute rule).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rts {

struct AnnotTables {
    const double *times;      // [n_rows]
    const int32_t *beats;     // [n_rows]
    const uint8_t *label_ok;  // [n_rows] the row's label is a non-empty string; NULL: no flags were given
    const long long *first;   // [P]
    const int32_t *len;       // [P]
    const uint8_t *invertible;  // [P] the piece's beats are strictly increasing (annot_invertible, csrc/annot_plan.h)
    int P;
    double frame_seconds;
};

struct AnnotPiece {
    const double *times;
    const int32_t *beats;
    int n;  // 0: no such piece
};

__device__ __forceinline__ AnnotPiece annot_piece(const AnnotTables &t, int piece) {
    AnnotPiece p = {nullptr, nullptr, 0};
    if (piece < 0 || piece >= t.P) return p;
    const long long first = t.first[piece];
    p.times = t.times + first;
    p.beats = t.beats + first;
    p.n = t.len[piece];
    return p;
}

__device__ __forceinline__ double annot_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// The first i in [0, n] with time <= times[i]; n: none.
__device__ __forceinline__ int annot_row(const AnnotPiece &p, double time) {
    int lo = 0, hi = p.n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (time <= p.times[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// -> the beat (NaN: none) and *seg
__device__ __forceinline__ double annot_lookup(const AnnotPiece &p, long long frame, double frame_seconds, int *seg) {
    *seg = -1;
    if (p.n < 1 || frame < 0) return annot_nan();
    const double time = (double)frame * frame_seconds;
    const int i = annot_row(p, time);
    if (i >= p.n) return annot_nan();
    const double end = p.times[i];
    const double beat = (double)p.beats[i];
    *seg = i == 0 ? 0 : i - 1;
    if (i == 0 && end == 0.0) return beat - 0.0;
    const double start = i == 0 ? 0.0 : p.times[i - 1];
    return beat - (end - time) / (end - start);
}

// The inverse lookup, beat x -> frame of piece `piece` (include/rtsync.h, rts_annot_frames): -1 where there is none.
__device__ __forceinline__ int32_t annot_frame_of(const AnnotTables &t, int piece, double x) {
    if (!(x == x) || piece < 0 || piece >= t.P || !t.invertible[piece]) return -1;
    const AnnotPiece p = annot_piece(t, piece);
    int lo = 0, hi = p.n;  // the first i with x <= (double)beats[i]
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (x <= (double)p.beats[mid]) hi = mid;
        else lo = mid + 1;
    }
    const int i = lo;
    if (i >= p.n) return -1;
    const double beat = (double)p.beats[i];
    if (x < beat - 1.0) return -1;  // a gap of the table, or before the stretch get_beat interpolates from time zero
    const double end = p.times[i];
    const double start = i == 0 ? 0.0 : p.times[i - 1];
    const double time = end - (beat - x) * (end - start);
    const double f = floor(time / t.frame_seconds + 0.5);
    if (!(f >= 0.0)) return f == f ? 0 : -1;
    if (f > 2147483647.0) return -1;
    return (int32_t)f;
}

}  // namespace rts
