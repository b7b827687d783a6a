#!/usr/bin/env python3
"""The device resampler (csrc/resample.hip) in the two shapes its users have, one JSON object per line:

  oneshot    a 30-minute mono file at 44.1 and at 48 kHz through chroma.ResamplePlan.run (rts_resample_run), device
             events around `reps` launches after a warm-up; ms per file, input samples per second, times real time.
  live       64 microphones deliver 100 ms per feed through LiveSession: `resampled` feeds 4800 samples per stream at
             48 kHz into LiveSession(fs_in=48000), `plain` feeds the same duration, 2205 samples, into an ordinary session.
             The microphones' audio is the ordinary session's, brought up to 48 kHz beforehand, so both trackers do the
             same work.  Wall time per feed over `feeds` feeds ending in a synchronise, `rounds` rounds, the two
             alternating inside one process; every round is printed, so the spread is on the page.
  plain      the ordinary session alone (what another build of the library is given: see --root).
  host_poly  scipy.signal.resample_poly of one 64 x 4800 feed with the same table on the host, if scipy is there:
             the CPU pass the device path saves, for comparison.

    python tools/bench_resample.py [oneshot|live|plain|host_poly|all] [--root TREE] [--label NAME] [--feeds N] [--rounds R]

--root: import the package from another checkout of this repository (e.g. the parent commit, built), so that the
ordinary 22 050 Hz feed of two commits can be timed side by side with one script; only `plain` makes sense there.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, FS, FS_MIC = 64, 22050, 48000


def emit(**kw):
    print(json.dumps(kw), flush=True)


def bench_oneshot(label, reps):
    import torch
    from real_time_audio_sync_amd import chroma
    for fs_in in (44100, 48000):
        n_in = 30 * 60 * fs_in
        plan = chroma.ResamplePlan(fs_in)
        x = (torch.rand(n_in, device=plan.device) - 0.5).reshape(1, -1)
        out = torch.empty((1, plan.out_len(n_in)), dtype=torch.float32, device=plan.device)
        for _ in range(3):
            plan.run(x, out=out)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(reps):
            t0.record()
            plan.run(x, out=out)
            t1.record()
            t1.synchronize()
            times.append(t0.elapsed_time(t1))
        med = float(np.median(times))
        emit(bench="oneshot", label=label, fs_in=fs_in, L=plan.L, M=plan.M, taps=len(plan.taps), n_in=n_in,
             n_out=int(out.shape[1]), reps=reps, ms_median=med, ms_min=float(min(times)), ms_max=float(max(times)),
             input_Msamples_per_s=n_in / med / 1e3, times_real_time=30 * 60 * 1e3 / med,
             GB_moved_per_s=4.0 * (n_in + out.shape[1]) / med / 1e6)
        plan.close()
        del x, out


def open_sessions(kinds):
    from real_time_audio_sync_amd import synth
    from real_time_audio_sync_amd.live import LiveSession
    ref, _ = synth.synth_batch(2200, 1, seed=1000)
    made = {}
    for kind in kinds:
        kw = dict(fs_in=FS_MIC) if kind == "resampled" else {}
        made[kind] = LiveSession(ref, batch=B, c=500, max_run_count=3, **kw)
    return made


def bench_live(label, kinds, feeds, rounds):
    rs = np.random.RandomState(5)
    blocks = {"plain": (rs.randint(-20000, 20000, size=(B, 8 * FS)) / 32768.0).astype(np.float32)}   # 8 s, cycled
    per = {"resampled": FS_MIC // 10, "plain": FS // 10}
    if "resampled" in kinds:
        # the microphones' audio is the same 8 s brought up to 48 kHz (on the device, before anything is timed), so that
        # both sessions' trackers hear the same music and do the same work
        from real_time_audio_sync_amd import chroma
        blocks["resampled"] = np.stack([chroma.resample(x, FS, FS_MIC)[:8 * FS_MIC] for x in blocks["plain"]])
    sess = open_sessions(kinds)

    def run(kind, n):
        s, blk, m = sess[kind], blocks[kind], per[kind]
        for i in range(n):
            j = (i % 80) * m
            s.feed_block(blk[:, j:j + m])
        s.sync()

    for kind in kinds:                      # every launch shape once, then a fresh start
        run(kind, 60)
        sess[kind].reset()
    for r in range(rounds):
        for kind in kinds:
            t0 = time.perf_counter()
            run(kind, feeds)
            dt = time.perf_counter() - t0
            done = sess[kind].poll()["feeds_done"]
            emit(bench="live_feed", label=label, kind=kind, round=r, streams=B, ms_audio_per_feed=100,
                 samples_per_stream_per_feed=per[kind], feeds=feeds, us_per_feed=dt / feeds * 1e6, feeds_done=done,
                 frames_consumed=int(sess[kind].otw.states()[:, 8].sum()))
            sess[kind].reset()
    for s in sess.values():
        s.close()


def bench_host_poly(label, reps):
    try:
        from scipy import signal
    except ImportError:
        emit(bench="host_poly", label=label, skipped="scipy is not installed")
        return
    from real_time_audio_sync_amd import filters
    L, M = filters.resample_ratio(FS_MIC)
    h = filters.resample_taps(FS_MIC) / L
    blk = (np.random.RandomState(5).rand(B, FS_MIC // 10) - 0.5).astype(np.float32)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        signal.resample_poly(blk, L, M, axis=1, window=h)
        times.append((time.perf_counter() - t0) * 1e6)
    emit(bench="host_poly", label=label, streams=B, samples_per_stream_per_feed=FS_MIC // 10, reps=reps,
         us_per_feed_median=float(np.median(times)), us_per_feed_min=float(min(times)), us_per_feed_max=float(max(times)),
         note="scipy.signal.resample_poly on one host thread pool as scipy runs it; no edge state carried between feeds")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all", choices=["oneshot", "live", "plain", "host_poly", "all"])
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--label", default="this")
    ap.add_argument("--feeds", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    if a.what in ("oneshot", "all"):
        bench_oneshot(a.label, a.reps)
    if a.what in ("live", "all"):
        bench_live(a.label, ["resampled", "plain"], a.feeds, a.rounds)
    if a.what == "plain":
        bench_live(a.label, ["plain"], a.feeds, a.rounds)
    if a.what in ("host_poly", "all"):
        bench_host_poly(a.label, a.reps)


if __name__ == "__main__":
    main()
