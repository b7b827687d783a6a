// Stand-alone driver of otw_plan::threads (csrc/otw_plan.h) for tests/test_otw_wide_plan_cpu.py, built with
// -fsanitize=address,undefined.
//   otw_wide_plan_driver CASE   CASE: lines "c spec tp_from cus B ref_f64 live_f64 waves"
// Per line: the window of band width c, the table entry of a launch without mirror (ok, pipelined, ring kind by number), the
// threads per workgroup of that entry's kernel under the RTS_OTW_WAVES value `waves` (0: unset; -1: refused), the same for
// the mirror entry, and what `auto` takes where every stream has a CU to itself.
#include <stdio.h>

#include "../../real_time_audio_sync_amd/csrc/otw_plan.h"

using namespace rts::otw_plan;

int main(int argc, char **argv) {
    FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    int c, spec, tp, cus, B, r64, l64, waves, n;
    while ((n = fscanf(f, "%d %d %d %d %d %d %d %d", &c, &spec, &tp, &cus, &B, &r64, &l64, &waves)) == 8) {
        const int W = window(c);
        const Entry e = entry(W, spec, tp, cus, B, r64 != 0, l64 != 0);
        printf("W=%d ok=%d pipelined=%d ring=%d threads=%d mirror_threads=%d auto_waves=%d waves_ok=%d\n", W, e.ok, e.pipelined,
               e.ring, threads(W, e, B, cus, waves), threads(W, mirror_entry(W), B, cus, waves), kWideWaves, (int)waves_ok(waves));
    }
    fclose(f);
    return n == EOF ? 0 : 2;
}
