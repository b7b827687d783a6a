#!/usr/bin/env python3
"""Timings of rts_locate_matches (csrc/locate.hip) against rts_locate with both row outputs -- the same launch chain
without the overlap flags and the ranking kernel -- at the same shape, alternating in one session, on synthetic chroma
(float32).  Device time from HIP events on the launch stream around one call with preallocated buffers, median of
repeated launches.  One JSON object per line and shape: ms per call of both, their ratio, the difference (what the two
new launches cost) and the baseline's own max/min spread over its repetitions.

    python tools/bench_locate_matches.py [reps] [shape index] >> profiles/locate_matches_bench.jsonl

With a shape index only that shape runs (a kernel trace then holds the kernels of one shape).
"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (B, M, pieces, frames per piece, K): the repertoire search of tools/bench_locate.py; one long piece, one workgroup
SHAPES = ((64, 64, 64, 2200, 4), (1, 256, 1, 19380, 8))


def timed_pair(fns, reps, warm=3):
    """Alternating launches of the given calls -> one list of seconds per call."""
    import torch
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e-3)
    return ts


def main():
    import torch
    from real_time_audio_sync_amd import _native as nat, synth
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    shapes = SHAPES if len(sys.argv) < 3 else (SHAPES[int(sys.argv[2])],)
    for B, M, P, N, K in shapes:
        # every piece plays the same 550 frames four times over (with a little noise): K = 4 ranks exist
        sec = synth.synth_ref(550, seed=3)
        pool_h = np.concatenate([sec] * (P * N // 550 + 1), axis=1)[:, :P * N]
        pool = torch.from_numpy(np.ascontiguousarray(pool_h.T)).to(torch.float32).to(dev)
        pool = pool + 0.01 * torch.rand(pool.shape, device=dev)
        pool = (pool / pool.norm(dim=1, keepdim=True)).contiguous()
        first = torch.arange(P, dtype=torch.int64, device=dev) * N
        lens = torch.full((P,), N, dtype=torch.int32, device=dev)
        q = torch.stack([pool[(b % P) * N + 100 + 3 * b: (b % P) * N + 100 + 3 * b + M] for b in range(B)])
        q = (q + 0.02 * torch.rand(q.shape, device=dev)).contiguous()
        n_pool = P * N
        nbytes = ctypes.c_size_t()
        nat.check(nat.lib.rts_locate_matches_workspace_bytes(B, n_pool, ctypes.byref(nbytes)))
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        cost = torch.empty((B, P, K), dtype=torch.float64, device=dev)
        end = torch.empty((B, P, K), dtype=torch.int32, device=dev)
        start = torch.empty((B, P, K), dtype=torch.int32, device=dev)
        n = torch.empty((B, P), dtype=torch.int32, device=dev)
        row = torch.empty((B, n_pool), dtype=torch.float64, device=dev)
        rowstart = torch.empty((B, n_pool), dtype=torch.int32, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        head = (q.data_ptr(), nat.F32, M, None, B, pool.data_ptr(), nat.F32, 12, n_pool, first.data_ptr(), lens.data_ptr(), P,
                nat.COST_DOT)

        def matches():
            nat.check(nat.lib.rts_locate_matches(*head, K, float("inf"), cost.data_ptr(), end.data_ptr(), start.data_ptr(),
                                                 n.data_ptr(), ws.data_ptr(), nbytes.value, stream))

        def baseline():
            nat.check(nat.lib.rts_locate(*head, cost.data_ptr(), end.data_ptr(), start.data_ptr(), row.data_ptr(),
                                         rowstart.data_ptr(), stream))
        tb, tm = timed_pair((baseline, matches), reps)
        matches()
        torch.cuda.synchronize()
        mb, mm = float(np.median(tb)), float(np.median(tm))
        print(json.dumps(dict(kernel="rts_locate_matches", baseline="rts_locate with row_dev and rowstart_dev", B=B, M=M,
                              pieces=P, piece_frames=N, K=K, workgroups=B * P, compute_units=cus, reps=reps,
                              baseline_ms=mb * 1e3, matches_ms=mm * 1e3, ratio=mm / mb, extra_ms=(mm - mb) * 1e3,
                              baseline_spread_max_over_min=max(tb) / min(tb),
                              matches_spread_max_over_min=max(tm) / min(tm),
                              mean_ranks_found=float(n.clamp(min=0).double().mean()))), flush=True)


if __name__ == "__main__":
    main()
