#!/usr/bin/env python3
"""What the beats-and-labels feature costs and saves (profiles/annot.md), one JSON object per line:

  kind=feed    the serving shape of tools/bench_live.py (64 microphones, 1-second float32 buffers, staged mode: the
               producer's samples are already in the pinned slot) with LiveSession.annotate off and on, alternating in one
               process and one session (reset() between the segments): host time of submit() per feed, wall time per feed
               with the final sync, and device time per feed between two events on the stream.  With annotations on a
               feed enqueues one more launch (annot_live_kernel).
  kind=metric  AnnotationTables.path_errors of 64 paths of 2100 points (upload, one launch, read-back, the dicts) and the
               launch alone between two events, beside 64 sequential evaluate.AlignmentError(...).stats() calls on the
               same paths and tables on this machine's CPU; the results are compared before anything is timed.

    python tools/bench_annot.py [feeds_per_segment=120] [segments=6] [metric_repeats=5]
"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def table(n_rows, step_s, seed):
    rs = np.random.RandomState(seed)
    times = np.cumsum(rs.uniform(0.5 * step_s, 1.5 * step_s, n_rows))
    return [float(t) for t in times], list(range(1, n_rows + 1))


def bench_feed(torch, tab, n_feeds, segments):
    from real_time_audio_sync_amd import synth
    from real_time_audio_sync_amd.live import LiveSession
    B, fs = 64, 22050
    ref, _ = synth.synth_batch(2200, 1, seed=1000)
    rs = np.random.RandomState(5)
    audio = (rs.randint(-20000, 20000, size=(B, fs), dtype=np.int16).astype(np.float32) / np.float32(32768.0))
    sess = LiveSession(ref, batch=B, c=500, max_run_count=3)
    for k in range(4):                                   # fill all four staging slots once
        cv, sv = sess.staging(np.float32)
        cv[:] = fs
        sv[:B * fs] = audio.reshape(-1)
        sess.submit(np.float32)
    sess.sync()
    stream = torch.cuda.current_stream(sess.dev)
    for seg in range(segments):
        on = seg % 2 == 1
        sess.reset()
        sess.annotate(tab if on else None)

        def one():
            cv, _ = sess.staging(np.float32)
            cv[:] = fs
            sess.submit(np.float32)
        for i in range(3):
            one()
        sess.sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()
        for i in range(n_feeds):
            one()
        t_submit = time.perf_counter() - t0
        e1.record(stream)
        sess.sync()
        wall = time.perf_counter() - t0
        words = sess.beats() if on else None
        print(json.dumps(dict(kind="feed", annotate=on, streams=B, feeds=n_feeds, submit_us_per_feed=t_submit / n_feeds * 1e6,
                              wall_us_per_feed=wall / n_feeds * 1e6, device_us_per_feed=e0.elapsed_time(e1) / n_feeds * 1e3,
                              frames_consumed_total=int(sess.otw.states()[:, 8].sum()),
                              streams_with_a_beat=int(np.isfinite(words["beat"]).sum()) if on else None,
                              feeds_done=sess.poll()["feeds_done"])), flush=True)
    sess.close()


def bench_metric(torch, repeats):
    from real_time_audio_sync_amd import evaluate
    from real_time_audio_sync_amd.annotate import AnnotationTables
    n_pairs, n_points = 64, 2100
    live_t, ref_t = table(420, 0.45, 1), table(420, 0.45, 2)
    tab = AnnotationTables([live_t, ref_t])
    k = np.arange(n_points)
    paths = [np.stack([k, np.minimum(k + (k * (p % 7)) // 300, n_points - 1)], axis=1) for p in range(n_pairs)]
    tmp = tempfile.mkdtemp()
    names = []
    for name, (times, beats) in (("live.csv", live_t), ("ref.csv", ref_t)):
        names.append(os.path.join(tmp, name))
        with open(names[-1], "w") as fh:
            fh.write("".join("%r,%d\n" % (t, b) for t, b in zip(times, beats)))
    tuples = [[(int(l), int(r)) for l, r in p] for p in paths]

    def host():
        return [evaluate.AlignmentError(names[1], names[0], p).stats() for p in tuples]
    want = host()
    got = tab.path_errors(paths, [0] * n_pairs, [1] * n_pairs)
    assert got == want, "the device metric differs from AlignmentError.stats()"
    dev_paths = torch.from_numpy(np.stack(paths).astype(np.int32)).to(tab.device)
    plen = torch.full((n_pairs,), n_points, dtype=torch.int32, device=tab.device)
    p0 = torch.zeros(n_pairs, dtype=torch.int32, device=tab.device)
    p1 = torch.ones(n_pairs, dtype=torch.int32, device=tab.device)
    stream = torch.cuda.current_stream(tab.device)
    for rep in range(repeats):
        t0 = time.perf_counter()
        host()
        t_host = time.perf_counter() - t0
        t0 = time.perf_counter()
        tab.path_errors(paths, [0] * n_pairs, [1] * n_pairs)
        t_dev = time.perf_counter() - t0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        tab.path_error_counts(dev_paths, plen, p0, p1)
        e1.record(stream)
        torch.cuda.synchronize()
        print(json.dumps(dict(kind="metric", pairs=n_pairs, points=n_points, rows=420, host_stats_ms=t_host * 1e3,
                              path_errors_ms=t_dev * 1e3, launch_us=e0.elapsed_time(e1) * 1e3,
                              count_first_pair=want[0]["count"])), flush=True)
    tab.close()
    for n in names:
        os.remove(n)
    os.rmdir(tmp)


def main():
    import torch
    from real_time_audio_sync_amd.annotate import AnnotationTables
    n_feeds = int(sys.argv[1]) if len(sys.argv) > 1 else 120
    segments = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    tab = AnnotationTables([table(420, 0.5, 3)])
    bench_feed(torch, tab, n_feeds, segments)
    tab.close()
    bench_metric(torch, repeats)


if __name__ == "__main__":
    main()
