#!/usr/bin/env python3
"""Timings of rts_dtw_subseq_paths (csrc/dtw.hip) next to rts_dtw_paths at the same shape in the same run: the
subsequence call evaluates the same cells through the same pipeline plus the last-row minimum, so rts_dtw_paths is its
yardstick.  Device time from HIP events on the launch stream, warm-up, then `reps` rounds in which the two calls
alternate; median per call, and the baseline's own spread (max over min of its repetitions) to read the ratio against.
Both sides are timed through their Python entry points (dtw_subseq_paths / dtw_paths), output and workspace allocation
from torch's caching allocator included.  One JSON object per line, printed and appended to
profiles/dtw_subseq_bench.jsonl.

    python tools/bench_dtw_subseq.py [reps]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "dtw_subseq_bench.jsonl")


def timed_alternating(fns, reps, warm=2):
    """-> one list of `reps` times (seconds) per function; round r times fns[0], fns[1], ... in turn."""
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


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def main():
    import torch
    from real_time_audio_sync_amd import synth
    from real_time_audio_sync_amd.dtw import dtw_paths, dtw_subseq_paths
    from real_time_audio_sync_amd.otw_batch import frames_tensor
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    dev = torch.device("cuda:0")

    def run(case, a, b, M, N, B, inside=None):
        path, plen, total, start, end = dtw_subseq_paths(a, b, check=True)
        _, plen_p, total_p = dtw_paths(a, b, check=True)
        first = path[:, 0, 1].cpu().numpy()
        last = np.array([int(path[k, int(plen[k]) - 1, 1]) for k in range(B)])
        sane = bool((first == start.cpu().numpy()).all() and (last == end.cpu().numpy()).all()
                    and bool((total <= total_p).all()))       # freeing the ends cannot cost more than pinning them
        if inside is not None:
            sane = sane and bool(inside(start.cpu().numpy(), end.cpu().numpy()))
        del path
        t_sub, t_paths = timed_alternating([lambda: dtw_subseq_paths(a, b), lambda: dtw_paths(a, b)], reps)
        ms, mp = float(np.median(t_sub)), float(np.median(t_paths))
        emit(kernel="rts_dtw_subseq_paths vs rts_dtw_paths", case=case, M=M, N=N, pairs=B, features="f32", reps=reps,
             seconds_subseq=ms, seconds_paths=mp, subseq_over_paths=ms / mp,
             paths_spread_max_over_min=max(t_paths) / min(t_paths), subseq_spread_max_over_min=max(t_sub) / min(t_sub),
             cells_per_s_subseq=B * M * N / ms, results_sane=sane)
        torch.cuda.empty_cache()

    # ---- the two shapes of tools/bench_dtw_paths.py
    for n_ref, B in ((1289, 64), (19380, 1)):
        ref = synth.synth_ref(n_ref, seed=n_ref)
        live = synth.synth_live(ref, seed=n_ref + 1, max_frames=1262 if n_ref == 1289 else None)
        b = frames_tensor(ref, dev, torch.float32)
        a = frames_tensor(live, dev, torch.float32).unsqueeze(0).repeat(B, 1, 1).contiguous()
        run("uniform", a, b, int(a.shape[1]), int(b.shape[0]), B)

    # ---- the use case: 64 excerpts of 646 frames (60 s) against one shared 19 380-frame piece
    n_ref, B, L = 19380, 64, 646
    ref = synth.synth_ref(n_ref, seed=n_ref)
    b = frames_tensor(ref, dev, torch.float32)
    at = np.linspace(0, n_ref - L, B).astype(np.int64)
    rs = np.random.RandomState(5)
    exc = []
    for A in at:
        q = ref[:, A:A + L] + 0.03 * rs.rand(12, L)
        exc.append(frames_tensor(q / np.sqrt((q * q).sum(axis=0, keepdims=True)), dev, torch.float32))
    a = torch.stack(exc).contiguous()
    run("64 excerpts of 60 s against one 30-minute piece", a, b, L, n_ref, B,
        inside=lambda s, e: (np.abs(s - at) <= 11).all() and (np.abs(e - (at + L - 1)) <= 11).all())


if __name__ == "__main__":
    main()
