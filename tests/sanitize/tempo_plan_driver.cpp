// Stand-alone driver of csrc/tempo_plan.h for tests/test_tempo_cpu.py, built with -fsanitize=address,undefined.
//   tempo_plan_driver CASE   CASE: "n_limits n_rings n_grids", then n_limits lines "K x_limit y_limit", n_rings lines
//                            "K P_max len", n_grids lines "B n_max"
// Output, one line per input line:
//   "limit K x_limit y_limit k_ok overflows"
//   "ring K P_max len entries lds_bytes turns windows"   the curve kernel's ring walked on the host for a path of `len`
//                            points: every turn writes its kTempoChunk slots, then every point i >= K of the turn reads
//                            the slot K points back.  The ring is an array of exactly `entries` tags (the index of the point
//                            a slot holds), so a slot outside it is a sanitizer report; a slot that does not hold point
//                            i - K makes the driver exit 3.  `windows`: the reads made.
//   "grid B n_max x y"
// and a last line "sweep checked", after a sweep of its own: tempo_overflows against a 128-bit product for every K in
// [2, 1024] at limits on both sides of 2^63 / K^2, and the LDS bytes of every K against the launch limit.
#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>

#include "../../real_time_audio_sync_amd/csrc/tempo_plan.h"

static long long walk_ring(int K, int P_max, int len) {
    using namespace rts;
    const int R = tempo_ring_entries(K);
    long long *tag = (long long *)malloc(sizeof(long long) * (size_t)R);  // exactly R entries
    if (!tag) abort();
    for (int i = 0; i < R; i++) tag[i] = -1;
    const int n = len > P_max ? P_max : len;
    long long reads = 0;
    int s0 = 0, turns = 0;
    for (int base = 0; base < n; base += kTempoChunk, turns++) {
        for (int t = 0; t < kTempoChunk; t++) tag[tempo_ring_wrap(s0 + t, R)] = (long long)base + t;  // every lane writes
        for (int t = 0; t < kTempoChunk; t++) {
            const int i = base + t;
            if (i >= n || i < K) continue;
            const int slot = tempo_ring_wrap(s0 + t, R);
            if (tag[slot] != i) exit(3);
            if (tag[tempo_ring_back(slot, K, R)] != (long long)i - K) exit(3);
            reads++;
        }
        s0 = tempo_ring_wrap(s0 + kTempoChunk, R);
    }
    if (turns != tempo_curve_turns(len, P_max)) exit(4);
    free(tag);
    return reads;
}

static bool wide_overflows(int K, long long x, long long y) {
    // K^2 < 2^21 and x < 2^63: K^2 x < 2^84; times y < 2^63 would leave 128 bits, so compare by division instead
    const unsigned __int128 top = (unsigned __int128)1 << 63;
    const unsigned __int128 kx = (unsigned __int128)((unsigned long long)K * K) * (unsigned long long)x;
    return (top + kx - 1) / kx <= (unsigned __int128)(unsigned long long)y;  // y >= ceil(2^63 / (K^2 x))
}

int main(int argc, char **argv) {
    using namespace rts;
    FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    int n_limits = 0, n_rings = 0, n_grids = 0;
    if (fscanf(f, "%d %d %d", &n_limits, &n_rings, &n_grids) != 3) return 2;
    for (int c = 0; c < n_limits; c++) {
        int K = 0;
        long long x = 0, y = 0;
        if (fscanf(f, "%d %lld %lld", &K, &x, &y) != 3) return 2;
        printf("limit %d %lld %lld %d %d\n", K, x, y, (int)tempo_k_ok(K), (int)(tempo_k_ok(K) && tempo_overflows(K, x, y)));
    }
    for (int c = 0; c < n_rings; c++) {
        int K = 0, P_max = 0, len = 0;
        if (fscanf(f, "%d %d %d", &K, &P_max, &len) != 3 || !tempo_k_ok(K)) return 2;
        printf("ring %d %d %d %d %zu %d %lld\n", K, P_max, len, tempo_ring_entries(K), tempo_curve_lds_bytes(K),
               tempo_curve_turns(len, P_max), walk_ring(K, P_max, len));
    }
    for (int c = 0; c < n_grids; c++) {
        int B = 0, n_max = 0;
        if (fscanf(f, "%d %d", &B, &n_max) != 2) return 2;
        const TempoGrid g = tempo_bpm_grid(B, n_max);
        printf("grid %d %d %u %u\n", B, n_max, g.x, g.y);
    }
    fclose(f);
    const long long top = 0x7fffffffffffffffLL;
    for (int K = kTempoMinK; K <= kTempoMaxK; K++) {
        if (tempo_curve_lds_bytes(K) + kTempoWaves * (kTempoSums * sizeof(uint64_t) + sizeof(uint32_t)) > kTempoLdsLimit) return 5;
        const long long kk = (long long)K * K;
        for (long long x : {1LL, 2LL, 3LL, 1LL << 22, 1LL << 31, (1LL << 31) + 1, top / kk, top}) {
            // the smallest y that overflows with this K and x, and its neighbours
            const unsigned __int128 kx = (unsigned __int128)kk * (unsigned long long)x;
            const unsigned __int128 edge128 = (((unsigned __int128)1 << 63) + kx - 1) / kx;
            const long long edge = edge128 > (unsigned __int128)top ? top : (long long)edge128;
            for (long long y : {1LL, edge - 1, edge, edge < top ? edge + 1 : edge, top}) {
                if (y < 1) continue;
                if (tempo_overflows(K, x, y) != wide_overflows(K, x, y)) return 6;
                if (tempo_overflows(K, y, x) != wide_overflows(K, y, x)) return 6;
            }
        }
    }
    printf("sweep checked\n");
    return 0;
}
