#!/usr/bin/env python3
"""What the live accompaniment costs per feed (profiles/accompany.md), one JSON object per line:

  kind=feed    64 microphones, 100 ms float32 buffers (2205 samples at 22 050 Hz), the production geometry (fft_len 4096,
               hop 2048, c = 500, a reference of 2200 frames), staged mode: the producer's samples are already in the pinned
               slot.  One session, LiveSession.accompany off and on in alternating segments of one process (reset() between
               the segments, the streams armed again after it): host time of submit() per feed, wall time per feed with the
               final sync, device time per feed between two events on the stream.  With it on a feed enqueues two more
               launches (accomp_steer_kernel, one wave per stream, and warp_run_kernel, one workgroup per stream, about 4.3
               blocks of 512 samples each at N = 1024, delta = 256) and the renderer writes the chunk into host-mapped memory.
  kind=summary the medians of the on and off segments, the spread of the off segments, and the difference.

The microphones get noise, so the trackers follow nothing in particular: the steering's status mix is reported with every on
segment.  The blocks a feed renders are set by the clock, not by the path, so the rendering does the work it would do behind
a musician.

    python tools/bench_accompany.py [feeds_per_segment=100] [segments=12]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, FS, FEED = 64, 22050, 2205


def main():
    import torch
    from real_time_audio_sync_amd import _native as nat
    from real_time_audio_sync_amd import synth
    from real_time_audio_sync_amd.live import LiveSession
    n_feeds = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    segments = int(sys.argv[2]) if len(sys.argv) > 2 else 12
    ref, _ = synth.synth_batch(2200, 1, seed=1000)
    rs = np.random.RandomState(5)
    audio = (rs.randint(-20000, 20000, size=(B, FEED), dtype=np.int16).astype(np.float32) / np.float32(32768.0))
    t = np.arange(2200 * 2048) / float(FS)
    track = (0.3 * np.sin(2 * np.pi * 220.0 * t) + 0.2 * np.sin(2 * np.pi * 331.0 * t + 1)
             + 0.02 * rs.standard_normal(len(t))).astype(np.float32)
    sess = LiveSession(ref, batch=B, c=500, max_run_count=3)
    stream = torch.cuda.current_stream(sess.dev)

    def one():
        cv, sv = sess.staging(np.float32)
        cv[:] = FEED
        sv[:B * FEED] = audio.reshape(-1)
        sess.submit(np.float32)

    for k in range(4):                                   # every staging slot touched once
        one()
    sess.sync()
    rows = []
    for seg in range(segments + 2):                      # the first two segments (one off, one on) are the warm-up
        on = seg % 2 == 1
        sess.reset()
        if on:
            sess.accompany(track, warp_N=1024, delta=256, hop_track=2048, K=64, chunk_seconds=0.25, max_anchors=1 << 12)
        else:
            sess.accompany(None)
        for i in range(45):                              # past fft_len: the trackers have path points, the clocks run
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
        row = dict(kind="feed", accompany=on, warm_up=seg < 2, streams=B, feeds=n_feeds, samples_per_feed=FEED,
                   submit_us_per_feed=t_submit / n_feeds * 1e6, wall_us_per_feed=wall / n_feeds * 1e6,
                   device_us_per_feed=e0.elapsed_time(e1) / n_feeds * 1e3, feeds_done=sess.poll()["feeds_done"])
        if on:
            a, w = sess.accompaniment()
            row.update(blocks_last_feed=int(w["blocks"].sum()), out_total_min=int(w["out_total"].min()),
                       status_counts={name: int(((w["status"] & bit) != 0).sum()) for name, bit in
                                      (("on", nat.ACC_ON), ("wait", nat.ACC_WAIT), ("free", nat.ACC_FREE), ("lo", nat.ACC_LO),
                                       ("hi", nat.ACC_HI), ("end", nat.ACC_END), ("full", nat.ACC_FULL), ("late", nat.ACC_LATE))},
                       warp_status_nonzero=int((w["warp_status"] != 0).sum()))
        print(json.dumps(row), flush=True)
        if seg >= 2:
            rows.append(row)
    sess.close()
    out = dict(kind="summary", segments_each=len(rows) // 2)
    for key in ("device_us_per_feed", "submit_us_per_feed", "wall_us_per_feed"):
        off = sorted(r[key] for r in rows if not r["accompany"])
        on = sorted(r[key] for r in rows if r["accompany"])
        out[key] = dict(off_median=float(np.median(off)), off_min=off[0], off_max=off[-1], on_median=float(np.median(on)),
                        on_min=on[0], on_max=on[-1], added_median=float(np.median(on) - np.median(off)))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
