#!/usr/bin/env python3
"""Timings of rts_dtw_paths (csrc/dtw.hip) next to rts_dtw at the same shape in the same run, and of one ragged batch the
dense call cannot hold.  Device time from HIP events on the launch stream, warm-up, median of repeated calls; both
sides are timed through their Python entry points (dtw_paths / dtw_batch(want_back=False)), output and workspace
allocation from torch's caching allocator included.  One JSON object per line, printed and appended to
profiles/dtw_paths_bench.jsonl.

    python tools/bench_dtw_paths.py [reps]
"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "dtw_paths_bench.jsonl")


def timed(fn, reps, warm=2):
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


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def workspace_bytes(nat, M, N, B):
    n = ctypes.c_size_t(0)
    nat.check(nat.lib.rts_dtw_paths_workspace_bytes(M, N, B, ctypes.byref(n)))
    return n.value


def main():
    import torch
    from real_time_audio_sync_amd import _native as nat, synth
    from real_time_audio_sync_amd.dtw import dtw_batch, dtw_paths
    from real_time_audio_sync_amd.otw_batch import frames_tensor
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    dev = torch.device("cuda:0")

    # ---- uniform shapes, path-only against dense
    for n_ref, B in ((1289, 64), (19380, 1)):
        ref = synth.synth_ref(n_ref, seed=n_ref)
        live = synth.synth_live(ref, seed=n_ref + 1, max_frames=1262 if n_ref == 1289 else None)
        b = frames_tensor(ref, dev, torch.float32)
        a1 = frames_tensor(live, dev, torch.float32)
        a = a1.unsqueeze(0).repeat(B, 1, 1).contiguous()
        M, N = int(a.shape[1]), int(b.shape[0])
        _, acc, _, dpath, dlen = dtw_batch(a, b, want_back=False, check=True)
        path, plen, total = dtw_paths(a, b, check=True)
        same = bool(torch.equal(plen, dlen) and torch.equal(path[0, :int(plen[0])], dpath[0, :int(dlen[0])])
                    and bool((total == acc[:, -1, -1]).all()))
        del acc, dpath, path
        t_dense = timed(lambda: dtw_batch(a, b, want_back=False), reps)
        t_paths = timed(lambda: dtw_paths(a, b), reps)
        cells = B * M * N
        emit(kernel="rts_dtw_paths vs rts_dtw", M=M, N=N, pairs=B, features="f32", reps=reps,
             seconds_paths=t_paths, seconds_dense=t_dense, paths_over_dense=t_paths / t_dense,
             cells_per_s_paths=cells / t_paths, cells_per_s_dense=cells / t_dense,
             workspace_bytes=workspace_bytes(nat, M, N, B), dense_output_bytes=16 * cells, same_result=same)
        torch.cuda.empty_cache()

    # ---- one ragged batch: 64 pairs of 5 000 .. 20 000 frames a side (random unit chroma made on the device)
    rs = np.random.RandomState(7)
    B = 64
    al = rs.randint(5000, 20001, size=B).astype(np.int32)
    bl = rs.randint(5000, 20001, size=B).astype(np.int32)
    M, N = int(al.max()), int(bl.max())
    g = torch.Generator(device=dev)
    g.manual_seed(7)

    def unit(shape):
        x = torch.rand(shape, device=dev, generator=g) ** 3 + 0.02
        return (x / x.norm(dim=-1, keepdim=True)).contiguous()
    a, b = unit((B, M, 12)), unit((B, N, 12))
    ald, bld = torch.from_numpy(al).to(dev), torch.from_numpy(bl).to(dev)
    path, plen, total = dtw_paths(a, b, ald, bld, check=True)
    ends_ok = all(tuple(path[k, int(plen[k]) - 1].tolist()) == (int(al[k]) - 1, int(bl[k]) - 1) for k in range(B))
    del path
    t = timed(lambda: dtw_paths(a, b, ald, bld), max(3, reps // 2), warm=1)
    cells = int((al.astype(np.int64) * bl.astype(np.int64)).sum())
    emit(kernel="rts_dtw_paths (ragged)", pairs=B, M_max=M, N_max=N, len_min=int(min(al.min(), bl.min())),
         len_max=int(max(M, N)), cells=cells, features="f32", seconds=t, cells_per_s=cells / t,
         workspace_bytes=workspace_bytes(nat, M, N, B), dense_output_bytes_would_be=16 * B * M * N,
         paths_end_at_last_cell=bool(ends_ok))


if __name__ == "__main__":
    main()
