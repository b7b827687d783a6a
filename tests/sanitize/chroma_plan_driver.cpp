// Stand-alone driver of csrc/chroma_plan.h for tests/test_chroma_plan_cpu.py, built with -fsanitize=address,undefined.
//   chroma_plan_driver CASE   CASE: lines "lds L", "flavour L hop span n_frames" and "grid kernel n_frames cus batched"
// Per "lds" line, one line for each kernel: every section's byte offset (each team's FFT buffer and scratch), the bytes
// of a team's buffer and scratch, the spectrum stride and the total.  Per "flavour" / "grid" line: the answer.
#include <stdio.h>
#include <string.h>

#include "../../real_time_audio_sync_amd/csrc/chroma_plan.h"

using namespace rts::chroma_plan;

int main(int argc, char **argv) {
    FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    char kind[16];
    while (fscanf(f, "%15s", kind) == 1) {
        if (!strcmp(kind, "lds")) {
            int L;
            if (fscanf(f, "%d", &L) != 1) return 2;
            for (int k = 0; k < kKernels; k++) {
                const Lds l = lds_layout((Kernel)k, L);
                printf("lds L=%d kernel=%d teams=%d group=%d z=%d", L, k, teams((Kernel)k), group((Kernel)k), 16 * l.z(0));
                for (int t = 1; t < teams((Kernel)k); t++) printf(",%d", 16 * l.z(t));
                printf(" z_bytes=%d tw=%d spec=%d sstride=%d red=%d", 16 * l.z_team, 16 * l.tw(), 16 * l.spec(), l.sstride, 16 * l.red(0));
                for (int t = 1; t < teams((Kernel)k); t++) printf(",%d", 16 * l.red(t));
                printf(" red_bytes=%d red_in_z=%d total=%zu\n", 8 * l.red_team, (int)l.red_in_z(), l.bytes());
            }
        } else if (!strcmp(kind, "flavour")) {
            int L, hop, n_frames;
            long long span;
            if (fscanf(f, "%d %d %lld %d", &L, &hop, &span, &n_frames) != 4) return 2;
            printf("flavour kernel=%d\n", (int)flavour(L, hop, span, n_frames));
        } else if (!strcmp(kind, "grid")) {
            int k, n_frames, cus, batched;
            if (fscanf(f, "%d %d %d %d", &k, &n_frames, &cus, &batched) != 4 || k < 0 || k >= kKernels) return 2;
            printf("grid x=%d\n", grid_x((Kernel)k, n_frames, cus, batched != 0));
        } else {
            return 2;
        }
    }
    fclose(f);
    return 0;
}
