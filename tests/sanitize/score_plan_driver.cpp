// Stand-alone driver for csrc/score_plan.h (no HIP): the limits of a score plan, the rules of its three tables, the argument
// rules of rts_score_chroma, the workspace size and the main kernel's grid.  Built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_score_cpu.py and run as a child process: a read past a table or a signed overflow
// in a size would be an error in its output.
//
//   score_plan_driver CASEFILE    lines:  P L hop pad_left K | T L K table entry fault | C n_notes n_pool P dtype notes_given
//                                         pieces_given out_given ws_given ws_bytes | W n_notes P n_pool
//       T: valid tables (T all 1, CW[i] = i, DK all 1) with one fault put into `table` (0 T, 1 CW, 2 DK; -1 none) at `entry`:
//          0 a negative value, 1 NaN, 2 +infinity, 3 CW[0] = 1, 4 the entry one below its predecessor
//   output, one line per case:    the case, then  P: refusal | T: refusal where | C: refusal | W: bytes grid.x grid.y
//   then the driver's own check: every refusal has a message of its own.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "../../real_time_audio_sync_amd/csrc/score_plan.h"

using namespace rts;

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char kind[8];
    while (fscanf(f, "%7s", kind) == 1) {
        if (!strcmp(kind, "P")) {
            int L, hop, pad, K;
            if (fscanf(f, "%d %d %d %d", &L, &hop, &pad, &K) != 4) return 2;
            printf("P %d %d %d %d %d\n", L, hop, pad, K, (int)score_plan_check(L, hop, pad, K));
        } else if (!strcmp(kind, "T")) {
            int L, K, table, fault;
            long long entry;
            if (fscanf(f, "%d %d %d %lld %d", &L, &K, &table, &entry, &fault) != 5) return 2;
            if (score_plan_check(L, 1, 0, K) != kScoreOk) return 2;
            // exactly as long as the plan says: the sanitizer sees a read behind them
            std::vector<double> T((size_t)kScorePitches * kScoreCh, 1.0), CW((size_t)L + 1), DK((size_t)K + 1, 1.0);
            for (int i = 0; i <= L; i++) CW[i] = (double)i;
            std::vector<double> *which = table == 0 ? &T : table == 1 ? &CW : table == 2 ? &DK : nullptr;
            if (which) {
                if (entry < 0 || (size_t)entry >= which->size()) return 2;
                double &v = (*which)[(size_t)entry];
                if (fault == 0) v = -1.0;
                else if (fault == 1) v = NAN;
                else if (fault == 2) v = INFINITY;
                else if (fault == 3) v = 1.0;
                else if (fault == 4 && entry > 0) v = (*which)[(size_t)entry - 1] - 1.0;
                else return 2;
            }
            long long where = -2;
            const ScoreRefusal r = score_tables_check(L, K, T.data(), CW.data(), DK.data(), &where);
            printf("T %d %d %d %lld %d %d %lld\n", L, K, table, entry, fault, (int)r, where);
        } else if (!strcmp(kind, "C")) {
            ScoreCall c;
            int notes, pieces, out, ws;
            unsigned long long bytes;
            if (fscanf(f, "%lld %lld %d %d %d %d %d %d %llu", &c.n_notes, &c.n_pool_frames, &c.P, &c.out_dtype, &notes, &pieces, &out,
                       &ws, &bytes) != 9)
                return 2;
            c.notes_given = notes;
            c.pieces_given = pieces;
            c.out_given = out;
            c.workspace_given = ws;
            c.workspace_bytes = (size_t)bytes;
            printf("C %lld %lld %d %d %d %d %d %d %llu %d\n", c.n_notes, c.n_pool_frames, c.P, c.out_dtype, notes, pieces, out, ws,
                   bytes, (int)score_call_check(c));
        } else if (!strcmp(kind, "W")) {
            long long n_notes, n_pool;
            int P;
            if (fscanf(f, "%lld %d %lld", &n_notes, &P, &n_pool) != 3) return 2;
            const ScoreGrid g = score_main_grid(P, n_pool);
            printf("W %lld %d %lld %llu %u %u\n", n_notes, P, n_pool, (unsigned long long)score_workspace_bytes(n_notes), g.x, g.y);
        } else {
            return 2;
        }
    }
    fclose(f);
    std::set<std::string> seen;
    for (int r = kScoreOk; r <= kScoreWorkspace; r++) {
        char msg[256] = "";
        score_message(msg, sizeof(msg), (ScoreRefusal)r, 7);
        if (!msg[0] || !seen.insert(msg).second) {
            printf("messages failed %d\n", r);
            return 1;
        }
    }
    if (score_workspace_bytes(-5) != 0) return 1;
    printf("messages checked\n");
    return 0;
}
