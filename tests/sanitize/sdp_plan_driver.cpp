// Stand-alone driver of csrc/sdp_plan.h for tests/test_sdp_plan_cpu.py, built with -fsanitize=address,undefined.
//   sdp_plan_driver CASE   CASE: lines "ws M N B" and "plan strips B resident1 resident2 pad"
// (RTS_SDP_CONFIG / RTS_SDP_GRID come from the environment, as in the library).  Per "ws" line: every section's offset and
// byte length (the header first), the total, and where workspace_carve puts each pointer for a base address that is
// never dereferenced -- the carve must agree with the layout the size came from.  Per "plan" line: the Plan.
#include <stdio.h>
#include <string.h>

#include "../../real_time_audio_sync_amd/csrc/sdp_plan.h"

using namespace rts::sdp;

struct Fields {  // the workspace fields as DtwArgs / WtwArgs name and type them
    int32_t *err;
    unsigned long long *bnd;
    int32_t *entb, *cross, *lens, *scratch;
    double *yrec;
    uint32_t *codes;
    int32_t *ticket;
};

int main(int argc, char **argv) {
    FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    static const char *const names[kSections] = {"bnd", "entb", "cross", "lens", "yrec", "codes", "scratch", "ticket"};
    char kind[8];
    while (fscanf(f, "%7s", kind) == 1) {
        if (!strcmp(kind, "ws")) {
            int M, N, B;
            if (fscanf(f, "%d %d %d", &M, &N, &B) != 3) return 2;
            const WorkspaceLayout w = workspace_layout(M, N, B);
            printf("ws M=%d N=%d B=%d err=0,%zu", M, N, B, kWsHeader);
            for (int s = 0; s < kSections; s++) printf(" %s=%zu,%zu", names[s], w.off[s], w.len[s]);
            printf(" total=%zu bytes=%zu", w.total, workspace_bytes(M, N, B));
            unsigned char *const base = reinterpret_cast<unsigned char *>((uintptr_t)1 << 32);  // an address, not memory
            Fields c;
            const WorkspaceLayout v = workspace_carve(base, M, N, B, &c, &c.scratch);
            const void *const at[kSections] = {c.bnd, c.entb, c.cross, c.lens, c.yrec, c.codes, c.scratch, c.ticket};
            printf(" carve=%zu", (size_t)((uintptr_t)c.err - (uintptr_t)base));
            for (int s = 0; s < kSections; s++) printf(",%zu", (size_t)((uintptr_t)at[s] - (uintptr_t)base));
            printf(" bnd_bytes=%zu\n", v.len[kBnd]);
        } else if (!strcmp(kind, "plan")) {
            int strips, B, r1, r2;
            size_t pad;
            if (fscanf(f, "%d %d %d %d %zu", &strips, &B, &r1, &r2, &pad) != 5) return 2;
            const Plan p = pick_config(strips, B, r1, r2, pad);
            printf("plan NS=%d H=%d grid=%d n_rg=%d block=%d smem=%zu\n", p.NS, p.H, p.grid, p.n_rg, p.block, p.smem);
        } else {
            return 2;
        }
    }
    fclose(f);
    return 0;
}
