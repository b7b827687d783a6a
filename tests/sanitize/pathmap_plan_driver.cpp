// Stand-alone driver for csrc/pathmap_plan.h (no HIP): the argument checks of rts_path_map / rts_annot_transfer, the 64-bit
// element offsets of a pair's rows, and the launch geometry.  Built with AddressSanitizer and UndefinedBehaviorSanitizer by
// tests/test_pathmap_cpu.py and run as a child process: an offset formed in 32 bits would be a "runtime error:" in its
// output or a wrong number in the sweep.
//
//   pathmap_plan_driver CASEFILE   lines:  C path P_max len from in in_needed n_max B out status   (pointers as 0 / 1)
//                                          O b P_max n_max | G len P_max | E given n n_max | B batch
//   output, one line per case:     C <the case> refusal | map message | transfer message
//                                  O b P_max n_max path_offset entry_offset | G len P_max points turns |
//                                  E given n n_max entries | B batch grid
//   then the driver's own sweep: the offsets against 128-bit products up to B = 65535 pairs of 2^31 - 1 points, and a ragged
//   batch walked the way the kernels walk it, every index inside its pair's rows.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../real_time_audio_sync_amd/csrc/pathmap_plan.h"

using namespace rts;

static int sweep() {
    const int sizes[] = {0, 1, 2, 255, 256, 257, 40000, 65536, 0x7fffffff};
    const int pairs[] = {0, 1, 2, 26843, 26844, 32768, 65534};
    for (int b : pairs)
        for (int s : sizes) {
            if ((unsigned __int128)pathmap_path_offset(b, s) != (unsigned __int128)b * (unsigned __int128)s * 2) return 1;
            if ((unsigned __int128)pathmap_entry_offset(b, s) != (unsigned __int128)b * (unsigned __int128)s) return 1;
        }
    if (pathmap_path_offset(65534, 40000) <= ((size_t)1 << 32)) return 2;  // B * P_max * 2 well beyond 2^31
    // a ragged batch, walked like the kernels: arrays of exactly B * P_max * 2 and B * n_max elements
    const int B = 5, P_max = 300, n_max = 70;
    const int lens[B] = {-1, 0, 1, 257, 5000}, ns[B] = {-3, 0, 1, 70, 1000};
    int32_t *path = (int32_t *)malloc(sizeof(int32_t) * B * P_max * 2);
    double *y = (double *)malloc(sizeof(double) * B * n_max);
    if (!path || !y) return 3;
    long long touched = 0;
    for (int b = 0; b < B; b++) {
        int32_t *pts = path + pathmap_path_offset(b, P_max);
        const int P = pathmap_points(lens[b], P_max);
        for (int turn = 0; turn < pathmap_turns(lens[b], P_max); turn++)
            for (int tid = 0; tid < kPathmapThreads; tid++) {
                const int t = turn * kPathmapThreads + tid;
                if (t < P) pts[2 * (size_t)t] = pts[2 * (size_t)t + 1] = t, touched++;
            }
        double *row = y + pathmap_entry_offset(b, n_max);
        const int n = pathmap_entries(true, ns[b], n_max);
        for (int e = 0; e < n; e++) row[e] = 0.0, touched++;
    }
    free(path);
    free(y);
    if (touched != (0 + 0 + 1 + 257 + 300) + (0 + 0 + 1 + 70 + 70)) return 4;
    if (pathmap_entries(false, -7, 9) != 9 || pathmap_grid(kPathmapMaxBatch) != 65535u) return 5;
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char kind[8];
    static const char token = 0;  // a non-NULL pointer that is never dereferenced
    while (fscanf(f, "%7s", kind) == 1) {
        if (!strcmp(kind, "C")) {
            int path, P_max, len, from, in, in_needed, n_max, B, out, status;
            if (fscanf(f, "%d %d %d %d %d %d %d %d %d %d", &path, &P_max, &len, &from, &in, &in_needed, &n_max, &B, &out, &status) != 10)
                return 2;
            const PathmapRefusal why = pathmap_check(path ? &token : nullptr, P_max, len ? &token : nullptr, from, in ? &token : nullptr,
                                                     in_needed != 0, n_max, B, out ? &token : nullptr, status ? &token : nullptr);
            printf("C %d %d %d %d %d %d %d %d %d %d %d | %s | %s\n", path, P_max, len, from, in, in_needed, n_max, B, out, status,
                   (int)why, pathmap_message(why, false), pathmap_message(why, true));
        } else if (!strcmp(kind, "O")) {
            int b, P_max, n_max;
            if (fscanf(f, "%d %d %d", &b, &P_max, &n_max) != 3) return 2;
            printf("O %d %d %d %zu %zu\n", b, P_max, n_max, pathmap_path_offset(b, P_max), pathmap_entry_offset(b, n_max));
        } else if (!strcmp(kind, "G")) {
            int len, P_max;
            if (fscanf(f, "%d %d", &len, &P_max) != 2) return 2;
            printf("G %d %d %d %d\n", len, P_max, pathmap_points(len, P_max), pathmap_turns(len, P_max));
        } else if (!strcmp(kind, "E")) {
            int given, n, n_max;
            if (fscanf(f, "%d %d %d", &given, &n, &n_max) != 3) return 2;
            printf("E %d %d %d %d\n", given, n, n_max, pathmap_entries(given != 0, n, n_max));
        } else if (!strcmp(kind, "B")) {
            int B;
            if (fscanf(f, "%d", &B) != 1) return 2;
            printf("B %d %u\n", B, pathmap_grid(B));
        } else {
            return 2;
        }
    }
    fclose(f);
    const int rc = sweep();
    if (rc) {
        printf("sweep failed %d\n", rc);
        return 1;
    }
    printf("sweep checked\n");
    return 0;
}
