// Stand-alone driver for csrc/accomp_plan.h (no HIP): the parameter limits of the live accompaniment, the rule that keeps a
// segment below 2^31, and the integer part of the steering law (steps 3, 5, 7 tail and 8 of include/rtsync.h,
// rts_live_accompany).  Built with AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_accomp_cpu.py and run as a
// child process: a signed overflow in one of the law's products would be a "runtime error:" in its output.
//
//   accomp_plan_driver CASEFILE    lines:  P H hop hop_track K glide lead rate_min_pm rate_max_pm chunk_blocks A_max |
//                                          T first len origin | D fed base H k chunk_blocks | R Ls hop_track hop rate_pm |
//                                          S tgt origin i0 Ls G | A i0 step_raw lo hi track_end
//   output, one line per case:     the case, then  P: refusal | T: ok | D: k_due late | R: step nominal | S: step_raw |
//                                  A: i1 status
//   then the driver's own sweep: every piece agrees with 128-bit arithmetic at the parameter limits.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../real_time_audio_sync_amd/csrc/accomp_plan.h"

using namespace rts;

typedef __int128 i128;

static int sweep() {
    const long long top = kAccLimit31 - 1;
    // step 5 and the chunk rule: whatever the rule lets through keeps lo, hi and nominal exact and hi below 2^31
    const int Hs[] = {32, 64, 512, 2048}, hops[] = {1, 128, 2048, 65536}, hts[] = {1, 160, 2048, kAccMaxHopTrack};
    const int pms[] = {0, 1, 500, 1000, 2000, kAccMaxRatePm};
    const int chunks[] = {1, 3, 64, 1 << 20, (1 << 26) - 1, 0x7fffffff};
    for (int H : Hs)
        for (int hop : hops)
            for (int ht : hts)
                for (int chunk : chunks) {
                    const i128 Ls = (i128)chunk * H;
                    const bool over = accomp_chunk_overflows(chunk, H, ht, hop, kAccMaxRatePm);
                    const i128 hi128 = Ls * ht * kAccMaxRatePm / ((i128)hop * 1000);
                    if (over != (Ls >= kAccLimit31 || hi128 >= kAccLimit31)) return 1;
                    if (over) continue;
                    for (int pm : pms) {
                        if (accomp_rate_step((long long)Ls, ht, hop, pm) != (long long)(Ls * ht * pm / ((i128)hop * 1000))) return 2;
                        if (accomp_rate_step((long long)Ls, ht, hop, pm) >= kAccLimit31) return 3;
                    }
                    if (accomp_nominal((long long)Ls, ht, hop) != (long long)(Ls * ht / hop)) return 4;
                }
    // step 7: every target the float64 part lets through, every position a track may have
    const long long tgts[] = {-(kAccTargetLimit - 1), -1, 0, 1, 12345678901LL, kAccTargetLimit - 1};
    const long long poss[] = {-(kAccPosLimit - 1), -1, 0, 1LL << 40, kAccPosLimit - 1};
    const long long Lss[] = {1, 32, 1536, top}, Gs[] = {0, 1, 2205, top};
    for (long long tgt : tgts)
        for (long long origin : poss)
            for (long long i0 : poss)
                for (long long Ls : Lss)
                    for (long long G : Gs) {
                        i128 d = (i128)tgt + origin - i0;
                        d = d < 0 ? 0 : (d > top ? top : d);
                        if (accomp_step_raw(tgt, origin, i0, Ls, G) != (long long)(d * Ls / ((i128)Ls + G))) return 5;
                    }
    // step 8: the anchor never runs backwards, never leaves [i0, max(i0, end)], and the step stays inside [lo, hi] unless END
    const long long steps[] = {0, 1, 1000, top};
    for (long long i0 : poss)
        for (long long raw : steps)
            for (long long lo : steps)
                for (long long hi : steps) {
                    if (lo > hi) continue;
                    for (long long end : poss) {
                        int st = 0;
                        const long long i1 = accomp_advance(i0, raw, lo, hi, end, &st);
                        const long long stop = i0 > end ? i0 : end;
                        if (i1 < i0 || i1 > stop || (st & ~(kAccLo | kAccHi | kAccEnd))) return 6;
                        if (!(st & kAccEnd) && (i1 - i0 < lo || i1 - i0 > hi)) return 7;
                        if (((st & kAccLo) != 0) != (raw < lo) || ((st & kAccHi) != 0) != (raw > hi)) return 8;
                    }
                }
    // step 3
    int late = 0;
    if (accomp_due(1000, 0, 32, 0, 3, &late) != 3 || !late) return 9;
    if (accomp_due(95, 0, 32, 0, 3, &late) != 2 || late) return 9;
    if (accomp_due((1LL << 61) + 5, 5, 2048, (1LL << 50) - 2, 0x7fffffff, &late) != (1LL << 50) || late) return 9;
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char kind[8];
    while (fscanf(f, "%7s", kind) == 1) {
        if (!strcmp(kind, "P")) {
            AccompGeom p;
            if (fscanf(f, "%d %d %d %d %lld %lld %d %d %d %d", &p.H, &p.hop, &p.hop_track, &p.K, &p.glide, &p.lead, &p.rate_min_pm,
                       &p.rate_max_pm, &p.chunk_blocks, &p.A_max) != 10)
                return 2;
            printf("P %d %d %d %d %lld %lld %d %d %d %d %d\n", p.H, p.hop, p.hop_track, p.K, p.glide, p.lead, p.rate_min_pm,
                   p.rate_max_pm, p.chunk_blocks, p.A_max, (int)accomp_params_check(p));
        } else if (!strcmp(kind, "T")) {
            long long first, len, origin;
            if (fscanf(f, "%lld %lld %lld", &first, &len, &origin) != 3) return 2;
            printf("T %lld %lld %lld %d\n", first, len, origin, (int)accomp_track_ok(first, len, origin));
        } else if (!strcmp(kind, "D")) {
            long long fed, base, k;
            int H, chunk, late = 0;
            if (fscanf(f, "%lld %lld %d %lld %d", &fed, &base, &H, &k, &chunk) != 5) return 2;
            const long long k_due = accomp_due(fed, base, H, k, chunk, &late);
            printf("D %lld %lld %d %lld %d %lld %d\n", fed, base, H, k, chunk, k_due, late);
        } else if (!strcmp(kind, "R")) {
            long long Ls;
            int ht, hop, pm;
            if (fscanf(f, "%lld %d %d %d", &Ls, &ht, &hop, &pm) != 4) return 2;
            printf("R %lld %d %d %d %lld %lld\n", Ls, ht, hop, pm, accomp_rate_step(Ls, ht, hop, pm), accomp_nominal(Ls, ht, hop));
        } else if (!strcmp(kind, "S")) {
            long long tgt, origin, i0, Ls, G;
            if (fscanf(f, "%lld %lld %lld %lld %lld", &tgt, &origin, &i0, &Ls, &G) != 5) return 2;
            printf("S %lld %lld %lld %lld %lld %lld\n", tgt, origin, i0, Ls, G, accomp_step_raw(tgt, origin, i0, Ls, G));
        } else if (!strcmp(kind, "A")) {
            long long i0, raw, lo, hi, end;
            if (fscanf(f, "%lld %lld %lld %lld %lld", &i0, &raw, &lo, &hi, &end) != 5) return 2;
            int st = 0;
            const long long i1 = accomp_advance(i0, raw, lo, hi, end, &st);
            printf("A %lld %lld %lld %lld %lld %lld %d\n", i0, raw, lo, hi, end, i1, st);
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
