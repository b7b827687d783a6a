#!/usr/bin/env python3
"""What the time map of a path costs (profiles/pathmap.md), one JSON object per line:

  kind=transfer  64 paths of about 2100 points, each carrying a table of 420 rows (the shapes of tools/bench_annot.py's
                 metric): the rts_annot_transfer launch between two events on the stream, the whole
                 AnnotationTables.transfer call (padding, upload, launch, read-back, the tuples), and the plain-Python
                 definition (tests/pathmap_model.py) over the same pairs on this machine's CPU.
  kind=dense     every frame of the same 64 paths through rts_path_map (one position per frame of column 0): the launch
                 between two events, map_frames' list form, and the model.

One warm-up run, then `repeats` timed runs of each; the device results are compared bit for bit with the model before
anything is timed.

    python tools/bench_pathmap.py [repeats=5]
"""
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def table(n_rows, step_s, seed):
    rs = np.random.RandomState(seed)
    times = np.cumsum(rs.uniform(0.5 * step_s, 1.5 * step_s, n_rows))
    return [float(t) for t in times], list(range(1, n_rows + 1))


def make_path(seed, n_frames):
    """A monotone path from (0, 0) over n_frames frames of column 0, with runs on both columns (about 1.5 points a frame)."""
    rng = random.Random(seed)
    u = v = 0
    pts = [(0, 0)]
    while u < n_frames - 1:
        step = rng.random()
        if step < 0.25:
            v += 1
        elif step < 0.5:
            u += 1
        else:
            u, v = u + 1, v + 1
        pts.append((u, v))
    return pts


def same(a, b):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes() == np.ascontiguousarray(b, dtype=np.float64).tobytes()


def main():
    import torch

    import pathmap_model as pm
    from real_time_audio_sync_amd import evaluate, pathmap
    from real_time_audio_sync_amd.annotate import AnnotationTables
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    n_pairs, n_frames, fs = 64, 1600, evaluate.FRAME_SECONDS
    paths = [make_path(100 + p, n_frames) for p in range(n_pairs)]
    points = [len(p) for p in paths]
    tab_host = table(420, 0.33, 1)                                       # 420 rows over 139 s; the paths cover 148 s
    tab = AnnotationTables([tab_host])
    dev = tab.device
    stream = torch.cuda.current_stream(dev)
    arrs = [np.asarray(p, dtype=np.int32) for p in paths]
    path_d, plen_d = pathmap.pack_paths(arrs, dev)
    pieces = [0] * n_pairs
    frames = [np.arange(n_frames, dtype=np.float64) for _ in range(n_pairs)]
    x_d = torch.from_numpy(np.stack(frames)).to(dev)

    def model_transfer():
        return [pm.transfer(p, tab_host[0], fs, 0)[0] for p in paths]

    def model_dense():
        return [pm.map_positions(p, f, 0)[0] for p, f in zip(paths, frames)]

    want_t, want_d = model_transfer(), model_dense()
    got_t, n_rows, status = tab.transfer_times(path_d, plen_d, pieces, 0)
    assert status.cpu().tolist() == [0] * n_pairs and n_rows.cpu().tolist() == [420] * n_pairs
    assert all(same(got_t[k].cpu().numpy(), want_t[k]) for k in range(n_pairs)), "the device transfer differs from the model"
    got_d = pathmap.map_frames(arrs, frames, 0)
    assert all(same(got_d[k], want_d[k]) for k in range(n_pairs)), "the device map differs from the model"
    tab.transfer(arrs, pieces, 0)                                       # the warm-up run of the wrappers

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    for rep in range(repeats):
        print(json.dumps(dict(kind="transfer", pairs=n_pairs, points_mean=float(np.mean(points)), points_max=max(points), rows=420,
                              rows_kept_first_pair=int(np.isfinite(want_t[0]).sum()),
                              launch_us=timed(lambda: tab.transfer_times(path_d, plen_d, pieces, 0)),
                              transfer_ms=wall(lambda: tab.transfer(arrs, pieces, 0)), model_ms=wall(model_transfer))), flush=True)
    for rep in range(repeats):
        print(json.dumps(dict(kind="dense", pairs=n_pairs, points_mean=float(np.mean(points)), entries_per_pair=n_frames,
                              launch_us=timed(lambda: pathmap.map_frames((path_d, plen_d), x_d, 0)),
                              map_frames_ms=wall(lambda: pathmap.map_frames(arrs, frames, 0)), model_ms=wall(model_dense))), flush=True)
    tab.close()


if __name__ == "__main__":
    main()
