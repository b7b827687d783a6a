// Host side of ensemble following (csrc/ensemble.hip): the checks rts_ensemble_create makes on the group table and the
// parameters before anything is allocated, the CSR form of the table, and the launch grids of the two kernels.  No HIP in
// it, so tests/sanitize/ensemble_plan_driver.cpp runs it stand-alone.
//
// A group table gives every stream b of a tracker its group, group[b] in [0, n_groups), or -1 for a stream in no group.  A
// group is one microphone followed against several recordings of its piece: its members are the streams with that entry, in
// ascending stream order, 1 to 64 of them -- one lane of a wave each.  CSR: members[first[g] .. first[g + 1]) are group g's
// streams; behind the last group, members[first[n_groups] .. B) are the streams in no group, ascending, which the kernels
// only clear.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

namespace rts {

constexpr int kEnsembleMaxMembers = 64;      // one wave per group, one lane per member
constexpr int kEnsembleMaxPatience = 65535;

enum EnsembleRefusal {
    kEnsembleOk = 0,
    kEnsembleBatch,     // B < 1
    kEnsembleGroups,    // n_groups outside [1, B]
    kEnsembleMaxDev,    // max_dev NaN or <= 0
    kEnsemblePatience,  // patience outside [1, kEnsembleMaxPatience]
    kEnsembleEntry,     // group[stream] outside [-1, n_groups)
    kEnsembleEmpty,     // a group without a member
    kEnsembleLarge,     // a group of more than kEnsembleMaxMembers members
};

struct EnsembleFault {
    int stream;  // the stream whose entry breaks the rule (-1 where the rule is not about one)
    int group;   // the group that breaks the rule (-1 where the rule is not about one)
    int count;   // its members (kEnsembleLarge)
};

// The first rule broken: the scalars in the order of the enum, then the entries in stream order, then the groups in order
// (an empty group before a large one of a higher index).  Reads group[0 .. B) only once B and n_groups have passed.
inline EnsembleRefusal ensemble_check(int B, const int32_t *group, int n_groups, double max_dev, int patience,
                                      EnsembleFault *where) {
    where->stream = where->group = -1;
    where->count = 0;
    if (B < 1) return kEnsembleBatch;
    if (n_groups < 1 || n_groups > B) return kEnsembleGroups;
    if (!(max_dev > 0.0)) return kEnsembleMaxDev;  // NaN fails the comparison; +inf passes
    if (patience < 1 || patience > kEnsembleMaxPatience) return kEnsemblePatience;
    for (int b = 0; b < B; b++)
        if (group[b] < -1 || group[b] >= n_groups) {
            where->stream = b;
            where->group = group[b];
            return kEnsembleEntry;
        }
    for (int g = 0; g < n_groups; g++) {
        int count = 0;
        for (int b = 0; b < B; b++) count += group[b] == g;
        where->group = g;
        where->count = count;
        if (count < 1) return kEnsembleEmpty;
        if (count > kEnsembleMaxMembers) return kEnsembleLarge;
    }
    where->group = -1;
    where->count = 0;
    return kEnsembleOk;
}

inline void ensemble_message(char *buf, size_t size, EnsembleRefusal why, const EnsembleFault &w, int B, int n_groups) {
    switch (why) {
    case kEnsembleOk: snprintf(buf, size, "ok"); break;
    case kEnsembleBatch: snprintf(buf, size, "B must be >= 1 (got %d)", B); break;
    case kEnsembleGroups: snprintf(buf, size, "n_groups must be in [1, B = %d] (got %d)", B, n_groups); break;
    case kEnsembleMaxDev: snprintf(buf, size, "max_dev must be > 0 beats (+inf allowed, NaN not)"); break;
    case kEnsemblePatience: snprintf(buf, size, "patience must be in [1, %d]", kEnsembleMaxPatience); break;
    case kEnsembleEntry:
        snprintf(buf, size, "group_host: stream %d has entry %d outside [-1, %d)", w.stream, w.group, n_groups);
        break;
    case kEnsembleEmpty: snprintf(buf, size, "group_host: group %d has no member", w.group); break;
    case kEnsembleLarge:
        snprintf(buf, size, "group_host: group %d has %d members, more than %d", w.group, w.count, kEnsembleMaxMembers);
        break;
    }
}

// The CSR form of a table that passed ensemble_check: first[n_groups + 1], members[B].  Returns the number of grouped
// streams, first[n_groups]; the B - first[n_groups] streams in no group follow in members[], ascending.
inline int ensemble_csr(int B, const int32_t *group, int n_groups, int32_t *first, int32_t *members) {
    for (int g = 0; g <= n_groups; g++) first[g] = 0;
    for (int b = 0; b < B; b++)
        if (group[b] >= 0) first[group[b] + 1]++;
    for (int g = 0; g < n_groups; g++) first[g + 1] += first[g];
    const int grouped = first[n_groups];
    int loose = grouped;
    for (int b = 0; b < B; b++)
        if (group[b] < 0) members[loose++] = b;
    // one pass over the streams per group (ascending, so the members are): no cursor table, nothing allocated
    for (int g = 0; g < n_groups; g++) {
        int at = first[g];
        for (int b = 0; b < B; b++)
            if (group[b] == g) members[at++] = b;
    }
    return grouped;
}

// ---- launch geometry ------------------------------------------------------------------------------------------------
// Both kernels: one wave per group, kEnsembleWaves waves to a workgroup; behind the groups' waves, one wave per 64 streams
// in no group, which only clears their outputs.
constexpr int kEnsembleWaves = 4;
constexpr int kEnsembleThreads = 64 * kEnsembleWaves;
constexpr int kEnsembleStage = 64;  // curve kernel: live frames whose group results a wave keeps in registers between stores

inline int ensemble_waves(int n_groups, int loose) { return n_groups + (loose + 63) / 64; }
inline unsigned ensemble_grid(int n_groups, int loose) {
    return (unsigned)((ensemble_waves(n_groups, loose) + kEnsembleWaves - 1) / kEnsembleWaves);
}

}  // namespace rts
