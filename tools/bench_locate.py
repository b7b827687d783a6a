#!/usr/bin/env python3
"""Timings of rts_locate (csrc/locate.hip): B live excerpts of M frames against a pool of 64 pieces x 2200 frames of
synthetic chroma (float32).  Device time from HIP events on the launch stream, median of repeated launches.  One JSON
object per line: ms per call and DP cells per second.

    python tools/bench_locate.py [reps]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PIECES, PIECE_FRAMES = 64, 2200


def timed(fn, reps, warm=3):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(ts))


def main():
    import torch
    from real_time_audio_sync_amd import synth
    from real_time_audio_sync_amd.locate import locate_batch
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    dev = torch.device("cuda:0")
    pool_h = synth.synth_ref(PIECES * PIECE_FRAMES, seed=3)
    pool = torch.from_numpy(np.ascontiguousarray(pool_h.T)).to(torch.float32).to(dev)
    first = torch.arange(PIECES, dtype=torch.int64, device=dev) * PIECE_FRAMES
    lens = torch.full((PIECES,), PIECE_FRAMES, dtype=torch.int32, device=dev)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    for B, M in ((64, 64), (64, 256), (1, 64), (1, 256)):
        # stream b heard M frames from somewhere inside piece b
        q = torch.stack([pool[b * PIECE_FRAMES + 500 + 3 * b: b * PIECE_FRAMES + 500 + 3 * b + M] for b in range(B)])
        q = (q + 0.02 * torch.rand(q.shape, device=dev)).contiguous()
        out = locate_batch(q, None, pool, first, lens)
        found = int((out[0].argmin(dim=1).cpu() == torch.arange(B)).sum())
        t = timed(lambda: locate_batch(q, None, pool, first, lens), reps)
        cells = B * M * PIECES * PIECE_FRAMES
        print(json.dumps(dict(kernel="rts_locate", B=B, M=M, pieces=PIECES, piece_frames=PIECE_FRAMES,
                              workgroups=B * PIECES, compute_units=cus, ms_per_call=t * 1e3, cells_per_s=cells / t,
                              streams_that_found_their_piece=found)), flush=True)


if __name__ == "__main__":
    main()
