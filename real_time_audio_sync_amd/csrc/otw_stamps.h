// In-kernel cycle stamps of otw_advance_kernel: everything that depends on RTS_OTW_STAMPS.  They exist only in the
// diagnostic build (tools/otw_phase_profile.py); the shipped library compiles every macro below to nothing and has none
// of the three entry points at the end.
//   -DRTS_OTW_STAMPS=1: per-phase stamps of wave 0 (they inflate what they measure).  [B][16] sums: slots 0..5 = hit
//     steps, 8..13 = other steps (0 end-of-step barrier wait, 1 chains, 2 mid-step barrier wait, 3 settle, 4 decide,
//     5 plan); 6 / 14 = their counts.  The plain kernel's wave 0 uses 0, 3, 5 and 8 for its four phases.
//   -DRTS_OTW_STAMPS=2: only the work / end-of-step wait split of the pipelined kernel, two stamps per step, by step
//     kind: 0 Row-only / Column-only hit, 1 Both hit while the band fills (planned as a hit), 2 Both hit with a full band
//     (planned "hit if", resolved to a hit), 3 every other step.  [B][128]: 32 words per step kind -- 0 wave-0 work, 1 its
//     end-of-step wait, 2 steps, 3..17 own work of waves 1..15 (as many as the instantiation has: NT / 64 - 1; the rest
//     stay 0); words 18, 19 of kind 0: the extra carry rounds of waves 1, 2 (all steps).
// These are macros because they name the kernel's locals (RTS_STAMP_LOCALS declares them; tid, lane, wave, a, e and the
// plan constants are the kernel's own), and the sums are separate scalars: an indexed array would go to scratch.
// RTS_W0_STEP_END contains the step's barrier (RTS_STEP_BARRIER, otw.hip) in every build.
#pragma once
#include "otw_host.h"  // rts_otw_set_debug writes the handle's `debug`

#if defined(RTS_OTW_STAMPS) && RTS_OTW_STAMPS == 1

#define RTS_STAMP_LOCALS()                                                              \
    long long stamp_sum[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};         \
    int stamp_base = 0;                                                                 \
    long long stamp_last = (long long)__builtin_amdgcn_s_memtime();                     \
    __builtin_amdgcn_s_waitcnt(0xC07F)
// the time since the last stamp goes to `slot`
#define RTS_STAMP(slot)                                                   \
    do {                                                                  \
        const long long now_ = (long long)__builtin_amdgcn_s_memtime();   \
        __builtin_amdgcn_s_waitcnt(0xC07F);                               \
        stamp_sum[slot] += now_ - stamp_last;                             \
        stamp_last = now_;                                                \
    } while (0)
// ... to `slot` of the hit steps or of the other steps, whichever the general loop's current step is
#define RTS_STAMP2(slot)      \
    do {                      \
        if (stamp_base)       \
            RTS_STAMP(8 + slot); \
        else                  \
            RTS_STAMP(slot);  \
    } while (0)
// A step loop of wave 0 entered a step -- its stamps go to the hit slots or to the other steps' -- and took it.  A step
// that the hit-step loop hands back to the general loop in between (the rare band reduction, a "hit if" that is none)
// leaves its entry in the hit slots.
#define RTS_STAMP_ENTER(hit) do { stamp_base = (hit) ? 0 : 8; } while (0)
#define RTS_STAMP_TAKEN() do { if (stamp_base) stamp_sum[14] += 1; else stamp_sum[6] += 1; } while (0)
#define RTS_STAMP_WRITE_BACK()                                                           \
    do {                                                                                 \
        if (tid == 0 && a.debug)                                                         \
            for (int i = 0; i < 16; i++) a.debug[(size_t)e.b * 16 + i] = stamp_sum[i];   \
    } while (0)

#else

#define RTS_STAMP(slot) do { } while (0)
#define RTS_STAMP2(slot) do { } while (0)
#define RTS_STAMP_ENTER(hit) do { } while (0)
#define RTS_STAMP_TAKEN() do { } while (0)

#endif

#if defined(RTS_OTW_STAMPS) && RTS_OTW_STAMPS == 2

#define RTS_STAMP_LOCALS()                                                                                              \
    long long lw_k0 = 0, lw_k1 = 0, lw_k2 = 0, lw_k3 = 0; /* wave 0: work */                                            \
    long long lb_k0 = 0, lb_k1 = 0, lb_k2 = 0, lb_k3 = 0; /* wave 0: end-of-step barrier wait */                        \
    long long ln_k0 = 0, ln_k1 = 0, ln_k2 = 0, ln_k3 = 0; /* wave 0: steps */                                           \
    long long l_last = 0;                                                                                               \
    long long lo_k0 = 0, lo_k1 = 0, lo_k2 = 0, lo_t0 = 0; /* waves 1..15: own work in hit steps */                      \
    long long lo_rounds = 0                               /* waves 1, 2: extra carry rounds of their speculative chains */
#define RTS_ROUNDS_ACC (&lo_rounds)
// the step kind from the plan flags as published (raw) and as resolved by otw_resolve_plan (res)
#define RTS_STEP_KIND(raw, res)                                                                          \
    (!((res) & kPlanHit) ? 3 : (((res) & (kPlanRow | kPlanCol)) != (kPlanRow | kPlanCol)) ? 0 : ((raw) & kPlanHitIf) ? 2 : 1)
// waves 1..NT/64-1: the wave's own work in a step, from the plan read to the end-of-step barrier
#define RTS_LW_BEGIN() do { lo_t0 = (long long)__builtin_amdgcn_s_memtime(); __builtin_amdgcn_s_waitcnt(0xC07F); } while (0)
#define RTS_LW_END(kind)                                                  \
    do {                                                                  \
        const long long t_ = (long long)__builtin_amdgcn_s_memtime();     \
        __builtin_amdgcn_s_waitcnt(0xC07F);                               \
        const int kd_ = (kind);                                           \
        if (kd_ == 0) lo_k0 += t_ - lo_t0;                                \
        if (kd_ == 1) lo_k1 += t_ - lo_t0;                                \
        if (kd_ == 2) lo_k2 += t_ - lo_t0;                                \
    } while (0)
// wave 0: the start of its step loops, and the end-of-step barrier with the time up to it and the time in it
#define RTS_W0_BEGIN()                                          \
    do {                                                        \
        l_last = (long long)__builtin_amdgcn_s_memtime();       \
        __builtin_amdgcn_s_waitcnt(0xC07F);                     \
    } while (0)
#define RTS_W0_STEP_END(kind)                                             \
    do {                                                                  \
        const long long t0_ = (long long)__builtin_amdgcn_s_memtime();    \
        __builtin_amdgcn_s_waitcnt(0xC07F);                               \
        RTS_STEP_BARRIER();                                               \
        const long long t1_ = (long long)__builtin_amdgcn_s_memtime();    \
        __builtin_amdgcn_s_waitcnt(0xC07F);                               \
        const int kd_ = (kind);                                           \
        if (kd_ == 0) lw_k0 += t0_ - l_last, lb_k0 += t1_ - t0_, ln_k0 += 1; \
        if (kd_ == 1) lw_k1 += t0_ - l_last, lb_k1 += t1_ - t0_, ln_k1 += 1; \
        if (kd_ == 2) lw_k2 += t0_ - l_last, lb_k2 += t1_ - t0_, ln_k2 += 1; \
        if (kd_ == 3) lw_k3 += t0_ - l_last, lb_k3 += t1_ - t0_, ln_k3 += 1; \
        l_last = t1_;                                                     \
    } while (0)
#define RTS_STAMP_WRITE_BACK()                                                                                          \
    do {                                                                                                                \
        if (a.debug) {                                                                                                  \
            long long *dbg = a.debug + (size_t)e.b * 128;                                                               \
            if (tid == 0) {                                                                                             \
                dbg[0] = lw_k0, dbg[1] = lb_k0, dbg[2] = ln_k0, dbg[32] = lw_k1, dbg[33] = lb_k1, dbg[34] = ln_k1;      \
                dbg[64] = lw_k2, dbg[65] = lb_k2, dbg[66] = ln_k2, dbg[96] = lw_k3, dbg[97] = lb_k3, dbg[98] = ln_k3;   \
            }                                                                                                           \
            if (lane == 0 && wave >= 1 && wave <= 15) dbg[2 + wave] = lo_k0, dbg[34 + wave] = lo_k1, dbg[66 + wave] = lo_k2; \
            if (lane == 0 && wave >= 1 && wave <= 2) dbg[17 + wave] = lo_rounds;                                        \
        }                                                                                                               \
    } while (0)

#else

#define RTS_ROUNDS_ACC nullptr
#define RTS_STEP_KIND(raw, res) 0
#define RTS_LW_BEGIN() do { } while (0)
#define RTS_LW_END(kind) do { } while (0)
#define RTS_W0_BEGIN() do { } while (0)
#define RTS_W0_STEP_END(kind) RTS_STEP_BARRIER()

#endif

#if !defined(RTS_OTW_STAMPS) || (RTS_OTW_STAMPS != 1 && RTS_OTW_STAMPS != 2)
#define RTS_STAMP_LOCALS() do { } while (0)
#define RTS_STAMP_WRITE_BACK() do { } while (0)
#endif

#ifdef RTS_OTW_STAMPS
extern "C" {

/* Diagnostic build only: caller-provided [B][rts_otw_debug_words()] int64 device buffer receiving per-phase cycle sums. */
int rts_otw_set_debug(rts_otw *h, long long *debug_dev) {
    if (!h) return rts::set_error(RTS_ERR_INVALID, "handle is NULL");
    h->debug = debug_dev;
    return RTS_OK;
}
/* What this library was built with, so that the caller sizes the buffer by the library and not by its own settings. */
int rts_otw_stamp_level(void) { return RTS_OTW_STAMPS; }
int rts_otw_debug_words(void) { return (RTS_OTW_STAMPS == 2) ? 128 : 16; }

}  // extern "C"
#endif
