// Stand-alone driver of csrc/snapshot_plan.h for tests/test_snapshot_plan_cpu.py (built with ASan + UBSan): reads one
// command per line from the file named on the command line and prints one line of numbers per command.
//   layout kind N param hist path path_cap   -> off_state off_mid off_path off_hist used stride  (kind 1 OTW: param = c;
//                                               kind 2 WTW: N = M_max, param = W with D carried or 0, stride at keep_last_d)
//   status kind w0 .. w15 param len hist_cap path_cap rec_stride  -> the RTS_SNAP_* reason (0: taken)
//   desc kind field delta           -> the field desc_mismatch names when `field` of a fitting desc is off by delta, or -
//   sel B n with_ref i0 .. i(n-1)   -> bad dup, then per chunk " | n set_ref" and idx:rec:len:first of every entry
//   livetail max_pending tracker_stride  -> live_tail_bytes live_rec_stride
//   mirror B diff n slot pending carry (n times)  -> pending[B] / carry[B] / rs_tot[2B] after live_mirror_import on a
//                                      mirror that held 1000 + b, b % 2 and 7 b + 1, 7 b + 2
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../real_time_audio_sync_amd/csrc/live_plan.h"
#include "../../real_time_audio_sync_amd/csrc/snapshot_plan.h"

using namespace rts::snap;

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char cmd[32];
    while (fscanf(f, "%31s", cmd) == 1) {
        if (!strcmp(cmd, "layout")) {
            int kind, N, param;
            long long hist, path, path_cap;
            if (fscanf(f, "%d %d %d %lld %lld %lld", &kind, &N, &param, &hist, &path, &path_cap) != 6) return 3;
            const Layout l = record_layout(kind, param, hist, path);
            const long long stride = kind == RTS_SNAPSHOT_OTW ? otw_rec_stride(N, param) : wtw_rec_stride(N, param, param > 0, path_cap);
            printf("%lld %lld %lld %lld %lld %lld\n", l.off_state, l.off_mid, l.off_path, l.off_hist, l.used, stride);
        } else if (!strcmp(cmd, "status")) {
            int32_t w[kHeaderWords];
            int kind, c, N;
            long long hist_cap, path_cap, stride;
            if (fscanf(f, "%d", &kind) != 1) return 3;
            for (int i = 0; i < kHeaderWords; i++)
                if (fscanf(f, "%d", &w[i]) != 1) return 3;
            if (fscanf(f, "%d %d %lld %lld %lld", &c, &N, &hist_cap, &path_cap, &stride) != 5) return 3;
            printf("%d\n", record_status(w, kind, c, N, hist_cap, path_cap, stride));
        } else if (!strcmp(cmd, "desc")) {
            char field[32];
            int kind, delta;
            if (fscanf(f, "%d %31s %d", &kind, field, &delta) != 3) return 3;
            rts_snapshot_desc d;
            memset(&d, 0, sizeof(d));
            d.kind = kind;
            d.version = RTS_SNAPSHOT_VERSION;
            d.n = 5;
            d.ref_dtype = RTS_F64;
            d.rec_stride = 4096;
            d.F = 12;
            d.c = 40;
            d.max_run_count = 3;
            d.variant = RTS_VARIANT_LIVENOTE;
            d.cost_kind = RTS_COST_EUCLID;
            d.window = 100;
            d.hop = 50;
            d.keep_last_d = 1;
            d.fft_len = 1024;
            d.live_hop = 512;
            d.feature_kind = 1;
            d.max_pending = 6000;
            d.tracker = kind == RTS_SNAPSHOT_LIVE ? RTS_SNAPSHOT_WTW : 0;
            const rts_snapshot_desc mine = d;
            struct { const char *name; int32_t *p; } fields[] = {
                {"kind", &d.kind}, {"version", &d.version}, {"n", &d.n}, {"ref_dtype", &d.ref_dtype}, {"F", &d.F}, {"c", &d.c},
                {"max_run_count", &d.max_run_count}, {"variant", &d.variant}, {"cost_kind", &d.cost_kind},
                {"window", &d.window}, {"hop", &d.hop}, {"keep_last_d", &d.keep_last_d}, {"fft_len", &d.fft_len},
                {"live_hop", &d.live_hop}, {"feature_kind", &d.feature_kind}, {"max_pending", &d.max_pending},
                {"tracker", &d.tracker}};
            bool found = !strcmp(field, "rec_stride") || !strcmp(field, "none");
            if (!strcmp(field, "rec_stride")) d.rec_stride += delta;
            for (auto &e : fields)
                if (!strcmp(field, e.name)) {
                    *e.p += delta;
                    found = true;
                }
            if (!found) return 3;
            const char *m = desc_mismatch(d, mine);
            printf("%s\n", m ? m : "-");
        } else if (!strcmp(cmd, "livetail")) {
            int cap;
            long long tracker;
            if (fscanf(f, "%d %lld", &cap, &tracker) != 2) return 3;
            printf("%lld %lld\n", live_tail_bytes(cap), live_rec_stride(tracker, cap));
        } else if (!strcmp(cmd, "mirror")) {
            int B, diff, n;
            if (fscanf(f, "%d %d %d", &B, &diff, &n) != 3 || B < 1 || n < 0) return 3;
            std::vector<long long> pending((size_t)B), tot(2 * (size_t)B);
            std::vector<uint8_t> carry((size_t)B);
            for (int b = 0; b < B; b++) {
                pending[(size_t)b] = 1000 + b;
                carry[(size_t)b] = (uint8_t)(b % 2);
                tot[2 * (size_t)b] = 7 * b + 1;
                tot[2 * (size_t)b + 1] = 7 * b + 2;
            }
            std::vector<int32_t> slots((size_t)n), words(2 * (size_t)n);
            for (int i = 0; i < n; i++)
                if (fscanf(f, "%d %d %d", &slots[(size_t)i], &words[2 * (size_t)i], &words[2 * (size_t)i + 1]) != 3) return 3;
            rts::LiveGeom g;
            memset(&g, 0, sizeof(g));
            g.B = B;
            g.diff = diff;
            const rts::LiveMirror cur = {pending.data(), carry.data(), tot.data()};
            rts::live_mirror_import(g, cur, n, slots.data(), words.data());
            for (int b = 0; b < B; b++) printf("%s%lld", b ? "," : "", pending[(size_t)b]);
            printf(" ");
            for (int b = 0; b < B; b++) printf("%s%d", b ? "," : "", (int)carry[(size_t)b]);
            printf(" ");
            for (int b = 0; b < 2 * B; b++) printf("%s%lld", b ? "," : "", tot[(size_t)b]);
            printf("\n");
        } else if (!strcmp(cmd, "sel")) {
            int B, n, with_ref;
            if (fscanf(f, "%d %d %d", &B, &n, &with_ref) != 3 || n < 0) return 3;
            std::vector<int32_t> idx((size_t)n), len((size_t)n);
            std::vector<long long> first((size_t)n);
            for (int i = 0; i < n; i++) {
                if (fscanf(f, "%d", &idx[(size_t)i]) != 1) return 3;
                first[(size_t)i] = 1000LL * i;
                len[(size_t)i] = i + 1;
            }
            int dup = 0;
            const int bad = sel_check(B, idx.data(), n, &dup);
            printf("%d %d", bad, bad >= 0 ? dup : 0);
            if (bad < 0) {
                SnapSel sel;
                for (int pos = 0; sel_next_chunk(n, idx.data(), with_ref ? first.data() : nullptr, with_ref ? len.data() : nullptr, &pos, &sel) > 0;) {
                    printf(" | %d %d", sel.n, sel.set_ref);
                    for (int k = 0; k < sel.n; k++) printf(" %d:%d:%d:%lld", sel.idx[k], sel.rec[k], sel.len[k], sel.first[k]);
                }
            }
            printf("\n");
        } else {
            return 3;
        }
    }
    fclose(f);
    return 0;
}
