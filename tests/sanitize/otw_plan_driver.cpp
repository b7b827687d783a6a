// Stand-alone driver of csrc/otw_plan.h for tests/test_otw_plan_cpu.py, built with -fsanitize=address,undefined.
//   otw_plan_driver CASE   CASE: lines "c spec tp_from cus B ref_f64 live_f64 fill max_new mirror"
// Per line: the window of band width c, the table entry of a launch without mirror at that window (ok, pipelined, ring
// kind by number), the entry of a mirror launch, and whether a launch that can bring max_new frames enqueues the band fill.
#include <stdio.h>

#include "../../real_time_audio_sync_amd/csrc/otw_plan.h"

using namespace rts::otw_plan;

int main(int argc, char **argv) {
    FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    int c, spec, tp, cus, B, r64, l64, fill, max_new, mirror, n;
    while ((n = fscanf(f, "%d %d %d %d %d %d %d %d %d %d", &c, &spec, &tp, &cus, &B, &r64, &l64, &fill, &max_new, &mirror)) == 10) {
        const int W = window(c);
        const Entry e = entry(W, spec, tp, cus, B, r64 != 0, l64 != 0), m = mirror_entry(W);
        printf("W=%d ok=%d pipelined=%d ring=%d mirror=%d,%d,%d fill=%d\n", W, e.ok, e.pipelined, e.ring, m.ok, m.pipelined,
               m.ring, (int)fill_gate(fill, max_new, c, W, mirror != 0));
    }
    fclose(f);
    return n == EOF ? 0 : 2;
}
