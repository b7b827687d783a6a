// Stand-alone driver of csrc/tuning_plan.h for tests/test_tuning_cpu.py, built with -fsanitize=address,undefined.
//   tuning_plan_driver CASE   CASE: "n_picks n_creates n_pickchecks n_searches n_layouts", then
//     n_picks       blocks "R W" followed by R counts (unsigned 64-bit)
//     n_creates     lines  "fft_len k_lo k_hi R n_edges bin_hz thr_pow kind at": doubles as the hex of their bits; the edge
//                          table is E[n] = 100 * 1.001^n with, by `kind`, 0 nothing changed, 1 no table (NULL), 2 E[at] =
//                          E[at - 1], 3 E[at] = NaN, 4 E[at] = -E[at], 5 E[at] = inf, 6 E[at] = 0
//     n_pickchecks  lines  "R W"
//     n_searches    blocks "n_edges R n_f" followed by n_edges edges and n_f frequencies, all as hex bits
//     n_layouts     lines  "fft_len n_edges R"
// Output, one line per case:
//   "pick <hex bits of cents> <n>"
//   "create <refusal> <unsupported> <bad edge or -1>"
//   "pickcheck <refusal>"
//   "search" then per frequency " <edge index>:<histogram bin>"
//   "layout <p_doubles> <staged> <edges_off> <wmax_off> <hist_off> <bytes>"
// and a last line "sweep checked", after a sweep of its own: the frame ranges of the workgroups partition [0, n_frames)
// in order for every grid the launch can choose, and every layout fits the launch limit.
// Every table is an allocation of exactly its own size, so an index outside it is a sanitizer report.
#include <initializer_list>
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../real_time_audio_sync_amd/csrc/tuning_plan.h"

static double from_bits(uint64_t u) {
    double d;
    memcpy(&d, &u, sizeof d);
    return d;
}
static uint64_t to_bits(double d) {
    uint64_t u;
    memcpy(&u, &d, sizeof u);
    return u;
}
static bool read_double(FILE *f, double *d) {
    uint64_t u = 0;
    if (fscanf(f, "%" SCNx64, &u) != 1) return false;
    *d = from_bits(u);
    return true;
}

int main(int argc, char **argv) {
    using namespace rts;
    FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    int n_picks = 0, n_creates = 0, n_pickchecks = 0, n_searches = 0, n_layouts = 0;
    if (fscanf(f, "%d %d %d %d %d", &n_picks, &n_creates, &n_pickchecks, &n_searches, &n_layouts) != 5) return 2;
    for (int c = 0; c < n_picks; c++) {
        int R = 0, W = 0;
        if (fscanf(f, "%d %d", &R, &W) != 2 || R < 1 || tuning_pick_refusal(R, W) != kTuningOk) return 2;
        uint64_t *h = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)R);  // exactly R counters
        if (!h) abort();
        for (int i = 0; i < R; i++)
            if (fscanf(f, "%" SCNu64, &h[i]) != 1) return 2;
        double cents = -1.0;
        long long n = -1;
        tuning_pick(h, R, W, &cents, &n);
        printf("pick %016" PRIx64 " %lld\n", to_bits(cents), n);
        free(h);
    }
    for (int c = 0; c < n_creates; c++) {
        int fft_len = 0, k_lo = 0, k_hi = 0, R = 0, n_edges = 0, kind = 0, at = 0;
        double bin_hz = 0, thr_pow = 0;
        if (fscanf(f, "%d %d %d %d %d", &fft_len, &k_lo, &k_hi, &R, &n_edges) != 5 || !read_double(f, &bin_hz) ||
            !read_double(f, &thr_pow) || fscanf(f, "%d %d", &kind, &at) != 2)
            return 2;
        double *E = nullptr;
        if (kind != 1 && n_edges > 0) {
            E = (double *)malloc(sizeof(double) * (size_t)n_edges);
            if (!E) abort();
            double v = 100.0;
            for (int n = 0; n < n_edges; n++, v *= 1.001) E[n] = v;
            if (kind != 0 && (at < 0 || at >= n_edges || (kind == 2 && at < 1))) return 2;
            if (kind == 2) E[at] = E[at - 1];
            if (kind == 3) E[at] = from_bits(0x7ff8000000000000ULL);
            if (kind == 4) E[at] = -E[at];
            if (kind == 5) E[at] = from_bits(0x7ff0000000000000ULL);
            if (kind == 6) E[at] = 0.0;
        }
        int bad = -1;
        const int why = tuning_create_refusal(fft_len, k_lo, k_hi, R, n_edges, E, bin_hz, thr_pow, &bad);
        printf("create %d %d %d\n", why, (int)tuning_refusal_unsupported(why), why == kTuningBadEdges ? bad : -1);
        free(E);
    }
    for (int c = 0; c < n_pickchecks; c++) {
        int R = 0, W = 0;
        if (fscanf(f, "%d %d", &R, &W) != 2) return 2;
        printf("pickcheck %d\n", tuning_pick_refusal(R, W));
    }
    for (int c = 0; c < n_searches; c++) {
        int n_edges = 0, R = 0, n_f = 0;
        if (fscanf(f, "%d %d %d", &n_edges, &R, &n_f) != 3 || n_edges < 1 || R < 1) return 2;
        double *E = (double *)malloc(sizeof(double) * (size_t)n_edges);  // exactly n_edges edges
        if (!E) abort();
        for (int n = 0; n < n_edges; n++)
            if (!read_double(f, &E[n])) return 2;
        printf("search");
        for (int i = 0; i < n_f; i++) {
            double fr = 0;
            if (!read_double(f, &fr)) return 2;
            const int n = tuning_edge_index(E, n_edges, fr);
            printf(" %d:%d", n, tuning_hist_bin(n, n_edges, R));
        }
        printf("\n");
        free(E);
    }
    for (int c = 0; c < n_layouts; c++) {
        int fft_len = 0, n_edges = 0, R = 0;
        if (fscanf(f, "%d %d %d", &fft_len, &n_edges, &R) != 3) return 2;
        const TuningLds l = tuning_lds(fft_len, n_edges, R);
        printf("layout %d %d %zu %zu %zu %zu\n", l.p_doubles, l.edges_staged, l.edges_off, l.wmax_off, l.hist_off, l.bytes);
    }
    fclose(f);
    for (long long n_frames : {1LL, 2LL, 37LL, 511LL, 512LL, 513LL, 1023LL, 1025LL, 77777LL, (1LL << 31) + 5, (1LL << 40) + 3}) {
        const int G = tuning_groups(n_frames);
        if (G < 1 || G > kTuningMaxGroups || G > n_frames) return 5;
        if (tuning_first_frame(n_frames, G, 0) != 0 || tuning_first_frame(n_frames, G, G) != n_frames) return 5;
        for (int g = 0; g < G; g++) {
            const long long len = tuning_first_frame(n_frames, G, g + 1) - tuning_first_frame(n_frames, G, g);
            if (len < n_frames / G || len > n_frames / G + 1) return 5;  // no workgroup idle, none a frame ahead
        }
    }
    for (int fft_len = kTuningMinFft; fft_len <= kTuningMaxFft; fft_len *= 2)
        for (int R : {1, 7, 100, kTuningMaxR})
            for (int n_edges : {2, 601, 3500, 6001, 8000, 1 << 20}) {
                const TuningLds l = tuning_lds(fft_len, n_edges, R);
                if (l.bytes > kTuningLdsLimit || l.p_doubles < fft_len / 2 + 1 || (l.edges_off & 15) != 0) return 6;
                if (l.bytes != tuning_lds_bytes(fft_len, n_edges, R, l.edges_staged != 0)) return 6;
                if (!l.edges_staged && tuning_lds_bytes(fft_len, n_edges, R, true) <= kTuningLdsLimit) return 6;
            }
    printf("sweep checked\n");
    return 0;
}
