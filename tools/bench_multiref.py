#!/usr/bin/env python3
"""Per-stream references, cost on the OTW headline kernel: f32 features, c = 500, one 2200-frame reference, synthetic
lives (synth.synth_batch).  Per batch size B, in one process and alternated step by step (ABAB...):
  (a) single    BatchedOTW(ref, batch=B)                        -- today's handle
  (b) shared    BatchedOTW.with_references([ref] * B)            -- per-stream tables, every stream on one range
  (c) distinct  BatchedOTW.with_references([copy_b of ref ...])  -- B separate uploads of the reference
(c)'s references are copies with the same values, so every stream computes exactly what it computes in (a): the only
difference is the reference working set (B x 2200 x 48 B instead of 106 KB), i.e. what the cache hierarchy does with it.
All three must give identical states and paths (checked).  Device time of one run() per step from HIP events; one JSON
object per line, median and spread over the timed steps.

  python tools/bench_multiref.py [--batches 64,1024,4096] [--steps 10] [--warmup 3] [--out FILE]
(B = 64 measures all three, larger batches (a) and (c).)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,1024,4096")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-ref", type=int, default=2200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from real_time_audio_sync_amd import synth
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for B in [int(x) for x in args.batches.split(",")]:
        ref, lives = synth.synth_batch(args.n_ref, B, seed=11)
        engs = {"single": BatchedOTW(ref, 500, 3, batch=B, dtype=torch.float32)}
        if B <= 64:
            engs["shared"] = BatchedOTW.with_references([ref] * B, 500, 3, dtype=torch.float32)
        engs["distinct"] = BatchedOTW.with_references([ref.copy() for _ in range(B)], 500, 3, dtype=torch.float32)
        lv, ln = engs["single"].pack(lives)
        times = {k: [] for k in engs}
        for step in range(args.warmup + args.steps):
            for k, eng in engs.items():  # alternated inside every step
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                eng.run(lv, ln)
                e1.record()
                torch.cuda.synchronize()
                if step >= args.warmup:
                    times[k].append(e0.elapsed_time(e1))
        st0 = engs["single"].states()
        probe = (0, B // 2, B - 1)
        for k, eng in engs.items():
            assert np.array_equal(eng.states(), st0), (B, k)
            assert all(np.array_equal(eng.path(b), engs["single"].path(b)) for b in probe), (B, k)
        base = float(np.median(times["single"]))
        for k, ts in times.items():
            med = float(np.median(ts))
            emit(dict(B=B, variant=k, ms_median=round(med, 4), ms_min=round(float(np.min(ts)), 4),
                      ms_max=round(float(np.max(ts)), 4), vs_single=round(med / base, 4), steps=len(ts),
                      ref_bytes=int(engs[k].ref.numel() * engs[k].ref.element_size()),
                      frames=int(st0[:, 8].sum()), c=500, n_ref=args.n_ref, dtype="f32"))
        for eng in engs.values():
            eng.close()
        del engs, lv, ln
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
