// Stand-alone driver of csrc/live_plan.h for tests/test_live_plan_cpu.py, built with -fsanitize=address,undefined.
//   live_plan_driver CASE   CASE: "B L hop cap diff rs_L rs_M rs_half in_cap n_feeds", then n_feeds lines of B counts
// Every array has exactly the size live_plan.h states for it (an array the mode does not use is NULL), so an index one
// past B is a sanitizer report.  Per feed one line: what live_plan_feed returned and planned, then -- after
// live_mirror_commit for an accepted feed -- the mirror; for a refused feed `same` tells whether its bytes are untouched.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../real_time_audio_sync_amd/csrc/live_plan.h"

template <class T>
static T *exact(size_t n) {
    T *p = (T *)calloc(n, sizeof(T));
    if (!p) abort();
    return p;
}

template <class T>
static void list(const char *key, const T *v, size_t n) {
    printf(" %s=", key);
    if (!v || !n) printf("-");
    for (size_t i = 0; v && i < n; i++) printf(i ? ",%lld" : "%lld", (long long)v[i]);
}

static rts::LiveMirror mirror(const rts::LiveGeom &g) {
    rts::LiveMirror m = {exact<long long>(g.B), g.diff ? exact<uint8_t>(g.B) : nullptr,
                         g.rs_L ? exact<long long>(2 * (size_t)g.B) : nullptr};
    return m;
}

static std::vector<unsigned char> bytes(const rts::LiveGeom &g, const rts::LiveMirror &m) {
    std::vector<unsigned char> v;
    const unsigned char *p = (const unsigned char *)m.pending;
    v.insert(v.end(), p, p + sizeof(long long) * g.B);
    if (g.diff) v.insert(v.end(), m.has_carry, m.has_carry + g.B);
    if (g.rs_L) v.insert(v.end(), (const unsigned char *)m.rs_tot, (const unsigned char *)(m.rs_tot + 2 * (size_t)g.B));
    return v;
}

int main(int argc, char **argv) {
    FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    rts::LiveGeom g = {};
    int n_feeds = 0;
    if (fscanf(f, "%d %d %d %d %d %d %d %d %lld %d", &g.B, &g.L, &g.hop, &g.cap, &g.diff, &g.rs_L, &g.rs_M, &g.rs_half,
               &g.in_cap, &n_feeds) != 10)
        return 2;
    const size_t B = (size_t)g.B;
    rts::LiveMirror cur = mirror(g);
    rts::FeedPlan p = {};
    p.next = mirror(g);
    p.offs = exact<int32_t>(B);
    p.rs_nout = g.rs_L ? exact<int32_t>(B) : nullptr;
    for (int i = 0; i < n_feeds; i++) {
        int32_t *counts = exact<int32_t>(B);
        for (size_t b = 0; b < B; b++)
            if (fscanf(f, "%d", &counts[b]) != 1) return 2;
        const std::vector<unsigned char> before = bytes(g, cur);
        const rts::LiveRefusal why = rts::live_plan_feed(g, cur, counts, &p);
        const int same = bytes(g, cur) == before;
        printf("feed=%d rule=%d stream=%d same=%d", i, (int)why, why == rts::kLiveFeedOk ? -1 : p.stream, same);
        if (why == rts::kLiveFeedOk) {
            printf(" total=%lld n_max=%d n_max_diff=%d n_out_max=%d", p.total, p.n_max, p.n_max_diff, p.n_out_max);
            list("offs", p.offs, B);
            list("nout", p.rs_nout, B);
            rts::live_mirror_commit(g, cur, p.next);
        }
        list("pending", cur.pending, B);
        list("carry", cur.has_carry, B);
        list("tot", cur.rs_tot, 2 * B);
        printf("\n");
        free(counts);
    }
    fclose(f);
    for (rts::LiveMirror *m : {&cur, &p.next}) {
        free(m->pending);
        free(m->has_carry);
        free(m->rs_tot);
    }
    free(p.offs);
    free(p.rs_nout);
    return 0;
}
