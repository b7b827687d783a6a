// Host side of the time map of a path (csrc/pathmap.hip): the argument checks rts_path_map and rts_annot_transfer make
// before anything is enqueued, the 64-bit element offsets of a pair's rows, and the launch geometry.  No HIP in it, so
// tests/sanitize/pathmap_plan_driver.cpp runs it stand-alone.
//
// Both entry points take a ragged batch: paths [B][P_max][2] with a length per pair, entries [B][n_max] (positions, or the
// rows of a table) with a count per pair.  B * P_max * 2 passes 2^31 at B = 27 000 half-hour paths, so a pair's rows are
// found through size_t offsets only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RTS_PATHMAP_HD __host__ __device__
#else
#define RTS_PATHMAP_HD
#endif

namespace rts {

constexpr int kPathmapThreads = 256;  // one workgroup per pair: the status walk's chunk, the entries' stride
constexpr int kPathmapWaves = kPathmapThreads / 64;
constexpr int kPathmapMaxBatch = 65535;
// P_max, n_max and rows_max stop here: the lanes' strided loops count in int, and t + kPathmapThreads must not leave it
constexpr int kPathmapMaxSize = 1 << 30;

enum PathmapRefusal {
    kPathmapOk = 0,
    kPathmapPmax,      // P_max outside [0, kPathmapMaxSize]
    kPathmapNoPath,    // path NULL with P_max > 0
    kPathmapNoLen,     // len NULL
    kPathmapFrom,      // from outside {0, 1}
    kPathmapEntries,   // n_max / rows_max outside [0, kPathmapMaxSize]
    kPathmapNoIn,      // x NULL with n_max > 0 / piece NULL
    kPathmapBatch,     // B outside [1, kPathmapMaxBatch]
    kPathmapNoOut,     // y / times NULL with entries to write
    kPathmapNoStatus,  // status NULL
};

// The first rule broken, in the order of the enum.  `in` / `out`: x_dev / y_dev of rts_path_map, which may be NULL when there
// is no entry; rts_annot_transfer passes in_needed = true for piece_dev.
inline PathmapRefusal pathmap_check(const void *path, int P_max, const void *len, int from, const void *in, bool in_needed,
                                    int n_max, int B, const void *out, const void *status) {
    if (P_max < 0 || P_max > kPathmapMaxSize) return kPathmapPmax;
    if (!path && P_max > 0) return kPathmapNoPath;
    if (!len) return kPathmapNoLen;
    if (from != 0 && from != 1) return kPathmapFrom;
    if (n_max < 0 || n_max > kPathmapMaxSize) return kPathmapEntries;
    if (!in && (in_needed || n_max > 0)) return kPathmapNoIn;
    if (B < 1 || B > kPathmapMaxBatch) return kPathmapBatch;
    if (!out && n_max > 0) return kPathmapNoOut;
    if (!status) return kPathmapNoStatus;
    return kPathmapOk;
}

// The refusal in words, with the argument names of rts_path_map or (transfer) rts_annot_transfer.
inline const char *pathmap_message(PathmapRefusal why, bool transfer) {
    switch (why) {
    case kPathmapOk: return "ok";
    case kPathmapPmax: return "P_max must be in [0, 2^30]";
    case kPathmapNoPath: return "path_dev is NULL";
    case kPathmapNoLen: return "len_dev is NULL";
    case kPathmapFrom: return "from must be 0 or 1";
    case kPathmapEntries: return transfer ? "rows_max must be in [0, 2^30]" : "n_max must be in [0, 2^30]";
    case kPathmapNoIn: return transfer ? "piece_dev is NULL" : "x_dev is NULL";
    case kPathmapBatch: return "B must be in [1, 65535]";
    case kPathmapNoOut: return transfer ? "times_dev is NULL" : "y_dev is NULL";
    case kPathmapNoStatus: return "status_dev is NULL";
    }
    return "?";
}

// Where pair b's rows begin, in elements: int32 words of the path, doubles of the entries.  b in [0, B), sizes >= 0.
RTS_PATHMAP_HD inline size_t pathmap_path_offset(int b, int P_max) { return (size_t)b * (size_t)P_max * 2; }
RTS_PATHMAP_HD inline size_t pathmap_entry_offset(int b, int n_max) { return (size_t)b * (size_t)n_max; }

// Points the status walk looks at (len clamped to [0, P_max]) and the turns of kPathmapThreads points it takes.
RTS_PATHMAP_HD inline int pathmap_points(int len, int P_max) { return len > P_max ? P_max : (len < 0 ? 0 : len); }
inline int pathmap_turns(int len, int P_max) {
    const int n = pathmap_points(len, P_max);
    return n / kPathmapThreads + (n % kPathmapThreads != 0);
}
// Valid entries of a pair: n (none given: n_max) clamped to [0, n_max].
RTS_PATHMAP_HD inline int pathmap_entries(bool given, int n, int n_max) { return !given || n > n_max ? n_max : (n < 0 ? 0 : n); }
// One workgroup per pair.
inline unsigned pathmap_grid(int B) { return (unsigned)B; }

}  // namespace rts
