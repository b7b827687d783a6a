#!/usr/bin/env python3
"""What the tempo feature costs and saves (profiles/tempo.md), one JSON object per line:

  kind=feed    the serving shape of tools/bench_live.py and tools/bench_annot.py (64 microphones, 1-second float32 buffers,
               staged mode: the producer's samples are already in the pinned slot) with LiveSession.follow_tempo off and
               on, alternating in one process and one session (reset() between the segments): host time of submit() per
               feed, wall time per feed with the final sync, and device time per feed between two events on the stream.
               With tempo on a feed enqueues one more launch (tempo_tail_kernel, one wave per stream).
  kind=curve   tempo.tempo_curves of 64 paths of about 2100 points at K = 64 (padding, upload, one launch, read-back) and
               the launch alone between two events, beside the plain-Python model of the definition (tests/tempo_model.py)
               on the same paths on this machine's CPU; the results are compared bit for bit before anything is timed.

    python tools/bench_tempo.py [feeds_per_segment=120] [segments=6] [curve_repeats=5] [K=64]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def bench_feed(torch, n_feeds, segments, K):
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
        sess.follow_tempo(K if on else 0)

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
        words = sess.tempo() if on else None
        print(json.dumps(dict(kind="feed", follow_tempo=on, K=K if on else 0, streams=B, feeds=n_feeds,
                              submit_us_per_feed=t_submit / n_feeds * 1e6, wall_us_per_feed=wall / n_feeds * 1e6,
                              device_us_per_feed=e0.elapsed_time(e1) / n_feeds * 1e3,
                              frames_consumed_total=int(sess.otw.states()[:, 8].sum()),
                              streams_with_a_slope=int(np.isfinite(words["slope"]).sum()) if on else None,
                              feeds_done=sess.poll()["feeds_done"])), flush=True)
    sess.close()


def bench_curve(torch, repeats, K):
    import tempo_model as tm
    from real_time_audio_sync_amd import tempo
    n_paths = 64
    rs = np.random.RandomState(7)
    paths = []
    for p in range(n_paths):                             # monotone walks of 2100 +- 40 points, every tempo between 1/2 and 2
        n = 2100 + int(rs.randint(-40, 41))
        w = rs.uniform(0.2, 0.8)
        steps = np.array([(1, 0), (0, 1), (1, 1)])[rs.choice(3, size=n - 1, p=[w / 2, (1 - w) / 2, 0.5])]
        paths.append(np.concatenate([[(0, 0)], np.cumsum(steps, axis=0)]).astype(np.int32))
    top = max(int(p.max()) for p in paths) + 1

    def host():
        return [tm.curve(p.tolist(), K, 0.0, top, top) for p in paths]
    want = host()
    got = tempo.tempo_curves(paths, K)
    for (ws, wp), (gs, gp) in zip(want, got):
        assert np.array(ws).tobytes() == gs.tobytes() and np.array(wp).tobytes() == gp.tobytes(), \
            "the device curves differ from the model"
    P_max = max(len(p) for p in paths)
    host_paths = np.zeros((n_paths, P_max, 2), dtype=np.int32)
    for k, p in enumerate(paths):
        host_paths[k, :len(p)] = p
    dev_paths = torch.from_numpy(host_paths).to("cuda:0")
    plen = torch.tensor([len(p) for p in paths], dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream(dev_paths.device)
    for rep in range(repeats):
        t0 = time.perf_counter()
        host()
        t_host = time.perf_counter() - t0
        t0 = time.perf_counter()
        tempo.tempo_curves(paths, K)
        t_dev = time.perf_counter() - t0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for i in range(20):
            tempo.path_tempo(dev_paths, plen, K, 0.0, top, top)
        e1.record(stream)
        torch.cuda.synchronize()
        print(json.dumps(dict(kind="curve", paths=n_paths, points_total=int(sum(len(p) for p in paths)), K=K,
                              model_ms=t_host * 1e3, tempo_curves_ms=t_dev * 1e3, launch_us=e0.elapsed_time(e1) * 1e3 / 20,
                              finite_slopes=int(sum(np.isfinite(s).sum() for s, _ in got)))), flush=True)


def main():
    import torch
    n_feeds = int(sys.argv[1]) if len(sys.argv) > 1 else 120
    segments = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    K = int(sys.argv[4]) if len(sys.argv) > 4 else 64
    if not torch.cuda.is_available():
        raise SystemExit("bench_tempo needs a GPU: there is nothing to measure without one")
    bench_feed(torch, n_feeds, segments, K)
    bench_curve(torch, repeats, K)


if __name__ == "__main__":
    main()
