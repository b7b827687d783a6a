// Host-computable decisions of the OTW tracker (otw_host.h): the band window of a handle, which instantiation of
// otw_advance_kernel a launch gets, and whether a launch enqueues otw_bandfill_kernel in front of it.  Integer
// arithmetic, no HIP headers, so tests/sanitize/otw_plan_driver.cpp runs it stand-alone; otw_host.h includes it and keeps
// only the table of instantiations (set_entry) and the launches.  The ring kinds are the RTS_OTW_RING_* of
// include/rtsync.h.
#pragma once

namespace rts {
namespace otw_plan {

// Where the step kernel keeps the frames it reads more than once.
enum Ring {
    kRingFloat = 0,     // float32 frames in an LDS ring
    kRingDouble = 1,    // float64 frames in an LDS ring
    kRingNone = 2,      // no ring: every frame is read from global memory (LiveFromGlobal)
    kRingNoneLean = 3,  // the same at 73 registers, three workgroups per CU (LiveFromGlobalLean)
};

constexpr int kMaxC = 2036;        // the widest band the LDS-resident kernel holds
constexpr int kWideWindow = 1024;  // from here on no ring fits beside the window's bands

// The LDS window of band width c: the power of two from 64 up that holds the band's c cells and 12 more.
// c <= 52 -> 64, then 128 / 256 / 512 / 1024 / 2048 up to c = 116 / 244 / 500 / 1012 / 2036.
inline int window(int c) {
    int W = 64;
    while (W < c + 12) W *= 2;
    return W;
}

// One entry of a handle's kernel table.  ok == 0: the handle has no kernel for that kind of launch, which is refused.
struct Entry {
    int ok, pipelined, ring;
};

// The entry of a launch without dense mirror and trace.  Fixed at create but for `live_f64`: rts_otw_run's dtype, and
// always 1 for the handle-owned history (rts_otw_insert, rts_otw_push and every rts_live_* session).
//   W >= 1024: the pipelined kernel without ring; RTS_OTW_SPEC=0 has no entry there.
//   W <= 512, RTS_OTW_SPEC=0: the plain kernel, float ring when both inputs are float32, else double.
//   W <= 512, pipelined:
//     B >= tp_from * cus (two streams per CU or more by default)   none-lean
//     below that, reference and live input both float32            float ring: every value widens back exactly
//     anything else, B <= cus                                      double ring (one workgroup per CU at W = 512) while
//                                                                  every stream has a CU to itself
//     anything else, cus < B < tp_from * cus                       none: up to four workgroups per CU
inline Entry entry(int W, int spec, int tp_from, int cus, int B, bool ref_f64, bool live_f64) {
    if (W >= kWideWindow) return spec ? Entry{1, 1, kRingNone} : Entry{0, 0, kRingNone};
    const bool f32 = !ref_f64 && !live_f64;
    if (!spec) return Entry{1, 0, f32 ? kRingFloat : kRingDouble};
    if (B >= tp_from * cus && B > 0) return Entry{1, 1, kRingNoneLean};
    if (f32) return Entry{1, 1, kRingFloat};
    return Entry{1, 1, B <= cus ? kRingDouble : kRingNone};
}

// Threads per workgroup of an entry's kernel: 512 (eight waves) but for the wide forms of the pipelined W = 512 ring
// kernels, which exist for the batches that leave every stream a CU of its own.  The 512-thread kernel is sized for two
// workgroups per CU; alone on a CU it leaves half of every SIMD's wave slots empty, and the wide forms fill them with
// helper waves (cost strips): 768 threads = 12 waves, 9 of them helpers, 1024 = 16 waves, 13 helpers.
//   `waves`: RTS_OTW_WAVES, read at create.  0 (unset): kWideWaves where B <= cus, else 8 -- a float32 handle with
//   cus < B < tp_from * cus shares a CU between two workgroups and keeps 512 threads.  8 / 12 / 16: that width at any B
//   (A/B runs, tests).  Anything else: -1, rts_otw_create refuses.
//   Every other kernel -- plain, none, none-lean, W != 512, the dense mirror -- has the 512-thread form alone, whatever
//   `waves` says: its residency or its tests depend on it.
constexpr int kWideWaves = 12;  // what `auto` takes where B <= cus: the measured winner over 8 and 16 (profiles/otw_wide_summary.md)
inline bool waves_ok(int waves) { return waves == 0 || waves == 8 || waves == 12 || waves == 16; }
inline int threads(int W, const Entry &e, int B, int cus, int waves) {
    if (!waves_ok(waves)) return -1;
    const bool has_wide = e.ok && e.pipelined && W == 512 && (e.ring == kRingFloat || e.ring == kRingDouble);
    if (!has_wide) return 512;
    if (waves == 0) waves = (B <= cus) ? kWideWaves : 8;
    return 64 * waves;
}

// The entry of a launch that writes the dense mirror or the backward trace: the plain kernel at every window, whatever
// RTS_OTW_SPEC, with the double ring where one fits.
constexpr Entry mirror_entry(int W) { return Entry{1, 0, W >= kWideWindow ? kRingNone : kRingDouble}; }

// Whether a launch enqueues otw_bandfill_kernel in front of the step kernel.  `fill`: RTS_OTW_FILL; `max_new`: the
// largest number of new frames the call can bring to any stream; `mirror`: the launch writes a dense mirror or a trace.
// Only a launch that can bring a fresh stream its first c frames pays for the kernel; it has no c = 1 and no wide-window
// form.  Which streams it then fills is decided on the device (otw_fill_eligible).
inline bool fill_gate(int fill, int max_new, int c, int W, bool mirror) {
    return fill && max_new >= c && c >= 2 && W < kWideWindow && !mirror;
}

}  // namespace otw_plan
}  // namespace rts
