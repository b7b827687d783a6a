#!/usr/bin/env python3
"""Diagnostic (not shipped): build librtsync with -DRTS_OTW_STAMPS into tools/_diag/ and print
the share of wave-0 cycles each phase of otw_advance_kernel takes on the bench workload.

    RTS_DIAG_LEVEL=1|2 [RTS_OTW_WAVES=8|12|16] python tools/otw_phase_profile.py [--build]

RTS_DIAG_LIB=<path> runs a
diagnostic library built earlier.  The stamp level and the size of the debug buffer are the library's own
(rts_otw_stamp_level / rts_otw_debug_words), whatever RTS_DIAG_LEVEL says when the tool runs."""
import ctypes, os, subprocess, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DIAG = os.path.join(ROOT, "tools", "_diag")
DEFAULT_SO = os.path.join(DIAG, "librtsync_diag.so")


def build():
    """otw.hip with the stamps, linked with the package's own objects of every other source (the tracker's ABI reaches into
    tempo.hip and from there on, so the library is only whole with all of them)."""
    from real_time_audio_sync_amd import _build
    _build.build()
    if not os.path.isdir(_build.OBJ_DIR):   # the library was there already, its objects were not
        _build.build(force=True)
    os.makedirs(DIAG, exist_ok=True)
    so = DEFAULT_SO
    obj = os.path.join(DIAG, "otw.hip.o")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc] + _build.HIPCC_FLAGS + _build.PER_SOURCE_FLAGS["otw.hip"] +
                          ["-DRTS_OTW_STAMPS=%s" % os.environ.get("RTS_DIAG_LEVEL", "1"), "-c", "-x", "hip",
                           os.path.join(_build.CSRC, "otw.hip"), "-o", obj])
    others = [os.path.join(_build.OBJ_DIR, os.path.basename(f) + ".o") for f in _build.sources() if os.path.basename(f) != "otw.hip"]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", so, obj] + others)
    return so


def main():
    so = os.environ.get("RTS_DIAG_LIB", DEFAULT_SO)  # a diagnostic library built earlier (A/B)
    if "--build" in sys.argv or not os.path.exists(so):
        build()
        if "--build" in sys.argv:
            return
    import torch
    from real_time_audio_sync_amd import synth
    L = ctypes.CDLL(so)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    L.rts_otw_create.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, i32, ctypes.POINTER(vp)]
    L.rts_otw_run.argtypes = [vp, vp, i32, i32, vp, i32, vp]
    L.rts_otw_set_debug.argtypes = [vp, vp]
    L.rts_otw_set_waves.argtypes = [vp, i32]
    L.rts_otw_read_states.argtypes = [vp, vp, vp]
    L.rts_otw_stamp_level.restype = L.rts_otw_debug_words.restype = i32
    LEVEL2 = L.rts_otw_stamp_level() == 2  # the library's, not this run's RTS_DIAG_LEVEL: the kernel writes what it was built for
    words = L.rts_otw_debug_words()
    B, N, c = 64, 2200, 500
    ref = synth.synth_ref(N, seed=1000)
    lives = [synth.synth_live(ref, seed=1001 + b) for b in range(B)]
    dev = torch.device("cuda:0")
    ref_d = torch.from_numpy(np.ascontiguousarray(ref.T)).float().to(dev)
    tmax = max(l.shape[1] for l in lives)
    buf = torch.zeros((B, tmax, 12), dtype=torch.float32)
    for b, l in enumerate(lives):
        buf[b, :l.shape[1]] = torch.from_numpy(l.T.copy()).float()
    live_d = buf.to(dev)
    len_d = torch.tensor([l.shape[1] for l in lives], dtype=torch.int32, device=dev)
    names = ["barrier 2 wait + plan", "-", "-", "phase A (chain / install)", "-", "barrier 1 wait", "-", "-", "control"]
    for waves in (8,):
        h = vp()
        assert L.rts_otw_create(ref_d.data_ptr(), 0, 12, N, B, c, 3, 0, 0, ctypes.byref(h)) == 0
        L.rts_otw_set_waves(h, waves)
        dbg = torch.zeros((B, words), dtype=torch.int64, device=dev)
        L.rts_otw_set_debug(h, dbg.data_ptr())
        for _ in range(2):
            L.rts_otw_run(h, live_d.data_ptr(), 0, tmax, len_d.data_ptr(), 0, None)
        torch.cuda.synchronize()
        st = np.zeros((B, 16), dtype=np.int32)
        L.rts_otw_read_states(h, st.ctypes.data, None)
        d = dbg.cpu().numpy().astype(np.float64)
        frames = st[:, 8].sum()
        if LEVEL2:
            # [B][128]: 32 words per step kind (0 wave-0 work, 1 its end-of-step wait, 2 steps, 3..17 own work of waves
            # 1..15: those past the kernel's own count stay 0 and are not printed)
            kinds = ("single hits (Row-only / Column-only)", "Both hits while the band fills", "Both hits with a full band (\"hit if\")")
            assert words == 128, "a level-2 library of another stamp layout (otw_stamps.h)"
            tot = d.reshape(B, 4, 32).sum(axis=0)
            nh = max((i for i in range(13) if tot[:3, 5 + i].any()), default=4) + 1  # helper waves that stamped: 5, 9 or 13
            hl = "helper waves 3-%d" % (2 + nh)
            hits = tot[:3].sum(axis=0)
            n = max(hits[2], 1)
            print("hit steps: %d  wave-0 work %.0f cycles, end-of-step barrier wait %.0f cycles" % (hits[2], hits[0] / n, hits[1] / n))
            n3 = max(tot[3, 2], 1)
            print("other steps: %d  wave-0 work %.0f cycles, end-of-step barrier wait %.0f cycles" % (tot[3, 2], tot[3, 0] / n3, tot[3, 1] / n3))
            print("hit steps, own work: wave 1 (row speculation) %.0f, wave 2 (column speculation) %.0f, %s: %s"
                  % (hits[3] / n, hits[4] / n, hl, ", ".join("%.0f" % (hits[5 + i] / n) for i in range(nh))))
            for kd, label in enumerate(kinds):
                nk = max(tot[kd, 2], 1)
                print("%s: %d  wave-0 work %.0f + wait %.0f, wave 1 %.0f, wave 2 %.0f, %s: %s"
                      % (label, tot[kd, 2], tot[kd, 0] / nk, tot[kd, 1] / nk, tot[kd, 3] / nk, tot[kd, 4] / nk, hl,
                         ", ".join("%.0f" % (tot[kd, 5 + i] / nk) for i in range(nh))))
            steps = max(tot[:, 2].sum(), 1)
            print("extra carry rounds per speculative chain: row %.2f, column %.2f" % (tot[0, 18] / steps, tot[0, 19] / steps))
            return
        nm = ["barrier-2 wait", "phase A (chain / install) | hit: step entry", "barrier-1 wait", "settle", "decide", "plan + refill"]
        for base, label in ((0, "hit steps"), (8, "other steps")):
            n = d[:, base + 6].sum()
            tot = d[:, base:base + 6].sum()
            print("%s: %d (%.1f per frame), %.0f cycles per step" % (label, n, n / frames, tot / max(n, 1)))
            for i, x in enumerate(nm):
                print("   %-28s %7.0f cycles  %5.1f %%" % (x, d[:, base + i].sum() / max(n, 1), 100 * d[:, base + i].sum() / max(tot, 1)))
        print("band argmin recomputes per frame: %.3f" % (st[:, 15].sum() / frames))


if __name__ == "__main__":
    main()
