// Host side of the score kernels (csrc/score.hip): the limits of a plan, the rules its three tables keep, the argument
// rules of rts_score_chroma, the workspace layout and the two grids.  No HIP in it, so tests/sanitize/score_plan_driver.cpp
// runs it stand-alone.
//
// The definition is include/rtsync.h's (rts_score_create).  What the host can check is what lies on the host: the plan, the
// tables and the sizes.  Notes and piece tables lie on the device; the kernels bound every read of them themselves.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

namespace rts {

constexpr int kScorePitches = 128;         // rows of T
constexpr int kScoreCh = 12;               // pitch classes
constexpr int kScoreMinL = 64, kScoreMaxL = 8192;  // a chroma plan's limits (rts_chroma_create)
constexpr int kScoreMaxHop = 1 << 24;
constexpr int kScoreMaxK = 1 << 20;
constexpr int kScoreMaxPieces = 65535;     // pieces lie along gridDim.y
constexpr long long kScoreLimit31 = 0x7fffffffLL;

enum ScoreRefusal {
    kScoreOk = 0,
    kScoreFftLen,    // L no power of two in [kScoreMinL, kScoreMaxL]           (RTS_ERR_UNSUPPORTED)
    kScoreHop,       // H outside [1, kScoreMaxHop]
    kScorePad,       // pad_left outside [0, L]
    kScoreK,         // K outside [0, kScoreMaxK]
    kScoreTableT,    // an entry of T negative or not finite
    kScoreTableCW,   // CW[0] != 0, an entry not finite, or CW decreasing
    kScoreTableDK,   // an entry of DK negative or not finite
    kScoreNotes,     // n_notes outside [0, 2^31)
    kScoreNotePtr,   // n_notes > 0 and one of the four note pointers NULL
    kScorePieces,    // P outside [1, kScoreMaxPieces]
    kScorePiecePtr,  // one of the four piece tables NULL
    kScorePool,      // n_pool_frames outside [1, 2^31)
    kScoreOut,       // out_dev NULL
    kScoreDtype,     // out_dtype neither RTS_F32 (0) nor RTS_F64 (1)
    kScoreWorkspace, // workspace NULL or too small with n_notes > 0
};

inline ScoreRefusal score_plan_check(int L, int hop, int pad_left, int K) {
    if (L < kScoreMinL || L > kScoreMaxL || (L & (L - 1))) return kScoreFftLen;
    if (hop < 1 || hop > kScoreMaxHop) return kScoreHop;
    if (pad_left < 0 || pad_left > L) return kScorePad;
    if (K < 0 || K > kScoreMaxK) return kScoreK;
    return kScoreOk;
}

// The rules of the tables, on a plan that passed score_plan_check.  *where: the first entry that breaks one.
inline ScoreRefusal score_tables_check(int L, int K, const double *T, const double *CW, const double *DK, long long *where) {
    for (int i = 0; i < kScorePitches * kScoreCh; i++)
        if (!isfinite(T[i]) || T[i] < 0.0) return *where = i, kScoreTableT;
    for (int i = 0; i <= L; i++)
        if (!isfinite(CW[i]) || (i == 0 ? CW[0] != 0.0 : CW[i] < CW[i - 1])) return *where = i, kScoreTableCW;
    for (int i = 0; i <= K; i++)
        if (!isfinite(DK[i]) || DK[i] < 0.0) return *where = i, kScoreTableDK;
    *where = -1;
    return kScoreOk;
}

// ---- workspace ------------------------------------------------------------------------------------------------------
// Three int64 tables of n_notes entries, one behind the other, indexed like the notes:
//   emax   the largest end of the piece's valid notes up to and including this one (INT64_MIN before the first)
//   omin   the smallest onset of the piece's valid notes from this one on         (INT64_MAX behind the last)
//   oframe floor((onset + pad_left) / H) of a valid note, 0 of any other
// emax and omin do not decrease along a piece, whatever order the notes have, so both can be bisected.
constexpr int kScoreWsTables = 3;
inline size_t score_workspace_bytes(long long n_notes) {
    return n_notes <= 0 ? 0 : (size_t)n_notes * kScoreWsTables * sizeof(long long);
}

struct ScoreCall {
    long long n_notes, n_pool_frames;
    int P, out_dtype;
    bool notes_given, pieces_given, out_given, workspace_given;
    size_t workspace_bytes;
};
inline ScoreRefusal score_call_check(const ScoreCall &c) {
    if (c.n_notes < 0 || c.n_notes > kScoreLimit31 - 1) return kScoreNotes;  // keeps 24 n_notes far below 2^63 as well
    if (c.n_notes > 0 && !c.notes_given) return kScoreNotePtr;
    if (c.P < 1 || c.P > kScoreMaxPieces) return kScorePieces;
    if (!c.pieces_given) return kScorePiecePtr;
    if (c.n_pool_frames < 1 || c.n_pool_frames > kScoreLimit31 - 1) return kScorePool;
    if (!c.out_given) return kScoreOut;
    if (c.out_dtype != 0 && c.out_dtype != 1) return kScoreDtype;
    if (c.n_notes > 0 && (!c.workspace_given || c.workspace_bytes < score_workspace_bytes(c.n_notes))) return kScoreWorkspace;
    return kScoreOk;
}

inline void score_message(char *buf, size_t size, ScoreRefusal why, long long where) {
    switch (why) {
    case kScoreOk: snprintf(buf, size, "ok"); break;
    case kScoreFftLen: snprintf(buf, size, "fft_len must be a power of two in [%d, %d], as for a chroma plan", kScoreMinL, kScoreMaxL); break;
    case kScoreHop: snprintf(buf, size, "hop must be in [1, %d]", kScoreMaxHop); break;
    case kScorePad: snprintf(buf, size, "pad_left must be in [0, fft_len]"); break;
    case kScoreK: snprintf(buf, size, "K must be in [0, %d]", kScoreMaxK); break;
    case kScoreTableT: snprintf(buf, size, "T_host: entry %lld is negative or not finite", where); break;
    case kScoreTableCW: snprintf(buf, size, "CW_host: entry %lld breaks CW[0] == 0, finite, not decreasing", where); break;
    case kScoreTableDK: snprintf(buf, size, "DK_host: entry %lld is negative or not finite", where); break;
    case kScoreNotes: snprintf(buf, size, "n_notes must be in [0, 2^31)"); break;
    case kScoreNotePtr: snprintf(buf, size, "onset_dev, end_dev, pitch_dev and energy_dev must be given when n_notes > 0"); break;
    case kScorePieces: snprintf(buf, size, "P must be in [1, %d]", kScoreMaxPieces); break;
    case kScorePiecePtr: snprintf(buf, size, "note_first_dev, note_len_dev, frame_first_dev and n_frames_dev must be given"); break;
    case kScorePool: snprintf(buf, size, "n_pool_frames must be in [1, 2^31)"); break;
    case kScoreOut: snprintf(buf, size, "out_dev is NULL"); break;
    case kScoreDtype: snprintf(buf, size, "out_dtype must be RTS_F32 or RTS_F64"); break;
    case kScoreWorkspace: snprintf(buf, size, "workspace is NULL or smaller than rts_score_workspace_bytes(n_notes)"); break;
    }
}

// ---- launch geometry ------------------------------------------------------------------------------------------------
// Prepare: one wave per piece.  Main: workgroups of four waves, a wave takes 64 consecutive frames of one piece (one frame
// per lane); pieces along y, tiles of 256 frames along x.  The pieces' frame counts lie on the device; a piece that fits the
// pool has at most n_pool_frames of them, which bounds x, and a wave whose tile lies behind its piece's end leaves at once.
constexpr int kScoreWave = 64;
constexpr int kScoreWaves = 4;
constexpr int kScoreThreads = kScoreWave * kScoreWaves;
struct ScoreGrid {
    unsigned x, y;
};
inline ScoreGrid score_main_grid(int P, long long n_pool_frames) {
    const ScoreGrid g = {(unsigned)((n_pool_frames + kScoreThreads - 1) / kScoreThreads), (unsigned)P};
    return g;
}

}  // namespace rts
