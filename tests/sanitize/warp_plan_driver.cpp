// Stand-alone driver for csrc/warp_plan.h (no HIP): the limits of a plan, block counts, LDS bytes, the turns of the anchors
// kernel and the two pieces of integer arithmetic the run kernel shares with the host, the segment rule and the time map.
// Built with AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_warp_cpu.py and run as a child process: a signed
// overflow in the map's product would be a "runtime error:" in its output.
//
//   warp_plan_driver CASEFILE      lines:  B n_out N | L N delta | T len P_max | S o0 i0 o1 i1 reach
//   output, one line per case:     B n_out N blocks | L N delta n_ok delta_ok lds_bytes | T len P_max turns |
//                                  S o0 i0 o1 i1 reach ok [map(o0) map(mid) map(reach - 1)]
//   then the driver's own sweep: every plan's LDS fits, and the map agrees with 128-bit arithmetic at the limits.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../real_time_audio_sync_amd/csrc/warp_plan.h"

using namespace rts;

static long long map128(long long t, long long o0, long long i0, long long o1, long long i1) {
    const __int128 num = (__int128)(t - o0) * (__int128)(i1 - i0);
    return (long long)((__int128)i0 + num / (__int128)(o1 - o0));
}

static int sweep() {
    for (int N = -16; N <= kWarpMaxN + 32; N++)
        for (int d = 0; d <= kWarpMaxDelta; d += 64)
            if (warp_n_ok(N) && (warp_lds_bytes(N, d) > 40 * 1024 || warp_lds_bytes(N, d) % 16 != 0 || (N / 2) % 8 != 0)) return 1;
    const long long top = kWarpSegLimit - 1, far = kWarpPosLimit - 1;
    const long long o0s[] = {0, 1, 1LL << 33, far - top}, i0s[] = {-far, -1, 0, 1LL << 40, far - top};
    const long long dos[] = {1, 2, 3, 511, top - 1, top}, dis[] = {0, 1, 2, 1000, top - 1, top};
    for (long long o0 : o0s)
        for (long long i0 : i0s)
            for (long long d_o : dos)
                for (long long d_i : dis) {
                    const long long o1 = o0 + d_o, i1 = i0 + d_i;
                    const long long reaches[] = {o1, o0 + kWarpSegLimit};
                    for (long long reach : reaches) {
                        if (!warp_segment_ok(o0, i0, o1, i1, reach)) continue;
                        const long long ts[] = {o0, o0 + (reach - o0) / 2, reach - 1};
                        for (long long t : ts)
                            if (warp_map_pos(t, o0, i0, o1, i1) != map128(t, o0, i0, o1, i1)) return 2;
                    }
                }
    // what the rule refuses
    if (warp_segment_ok(0, 0, 0, 0, 0) || warp_segment_ok(0, 5, 10, 4, 10) || warp_segment_ok(0, 0, kWarpSegLimit, 0, kWarpSegLimit) ||
        warp_segment_ok(0, 0, 1, kWarpSegLimit, 1) || warp_segment_ok(0, 0, 10, 10, kWarpSegLimit + 1) ||
        warp_segment_ok(-1, 0, 10, 10, 10) || warp_segment_ok(0, 0, 10, kWarpPosLimit, 10) ||
        warp_segment_ok(kWarpPosLimit - 1, 0, kWarpPosLimit, 0, kWarpPosLimit))
        return 3;
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char kind[8];
    while (fscanf(f, "%7s", kind) == 1) {
        if (!strcmp(kind, "B")) {
            long long n_out;
            int N;
            if (fscanf(f, "%lld %d", &n_out, &N) != 2) return 2;
            printf("B %lld %d %lld\n", n_out, N, warp_blocks(n_out, N));
        } else if (!strcmp(kind, "L")) {
            int N, d;
            if (fscanf(f, "%d %d", &N, &d) != 2) return 2;
            const bool ok = warp_n_ok(N) && warp_delta_ok(d);
            printf("L %d %d %d %d %zu\n", N, d, (int)warp_n_ok(N), (int)warp_delta_ok(d), ok ? warp_lds_bytes(N, d) : (size_t)0);
        } else if (!strcmp(kind, "T")) {
            int len, P_max;
            if (fscanf(f, "%d %d", &len, &P_max) != 2) return 2;
            printf("T %d %d %d\n", len, P_max, warp_anchor_turns(len, P_max));
        } else if (!strcmp(kind, "S")) {
            long long o0, i0, o1, i1, reach;
            if (fscanf(f, "%lld %lld %lld %lld %lld", &o0, &i0, &o1, &i1, &reach) != 5) return 2;
            const bool ok = warp_segment_ok(o0, i0, o1, i1, reach);
            printf("S %lld %lld %lld %lld %lld %d", o0, i0, o1, i1, reach, (int)ok);
            if (ok)
                printf(" %lld %lld %lld", warp_map_pos(o0, o0, i0, o1, i1), warp_map_pos(o0 + (reach - o0) / 2, o0, i0, o1, i1),
                       warp_map_pos(reach - 1, o0, i0, o1, i1));
            printf("\n");
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
