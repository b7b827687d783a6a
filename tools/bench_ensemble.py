#!/usr/bin/env python3
"""What ensemble following costs (profiles/ensemble.md), one JSON object per line:

  kind=feed    64 streams as 16 microphones x 4 recordings of 2200 frames, 100 ms float32 buffers, staged mode (the
               samples are already in the pinned slot), annotations on, with LiveSession.follow_consensus off and on,
               alternating in one process and one session (reset() between the segments): host time of submit() per feed,
               wall time per feed with the final sync, device time per feed between two events on the stream.  With
               consensus on a feed enqueues one more launch (ensemble_fuse_kernel, one wave per microphone).
  kind=copies  the same 64 streams fed through feed(): as 64 independent microphones (64 buffers, today's path) and as 16
               microphones whose buffer EnsembleSession.feed writes four times into the staging slot, alternating: host
               time of feed() and wall time per feed.  The device does the same work either way (the chroma step runs 64
               times); the difference is what the host saves or spends on the copies.
  kind=curve   ensemble.path_consensus of 64 paths of about 2100 points in 16 groups over T = 2100 live frames (padding,
               upload, one launch) and the launch alone between two events, beside the plain-Python model of the definition
               (tests/ensemble_model.py) on this machine's CPU; the results are compared bit for bit before anything is timed.

    python tools/bench_ensemble.py [feeds_per_segment=200] [segments=10] [curve_repeats=3]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MICS, G, FS_AUDIO, FEED = 16, 4, 22050, 2205
FRAME_SECONDS = 2048 / 22050.


def recordings_and_tables(n_frames=2200):
    from real_time_audio_sync_amd import synth
    rs = np.random.RandomState(3)
    base = np.cumsum(rs.uniform(0.4, 0.6, size=int(n_frames * FRAME_SECONDS / 0.4)))
    base = base[base < n_frames * FRAME_SECONDS]
    recs = [synth.synth_ref(n_frames, seed=1000 + k) for k in range(G)]
    tables = [(list(np.sort(base * rs.uniform(0.97, 1.03))), list(range(len(base)))) for _ in range(G)]
    return recs, tables


def timed(torch, sess, n_feeds, one):
    stream = torch.cuda.current_stream(sess.dev)
    for i in range(3):
        one()
    sess.sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    t0 = time.perf_counter()
    for i in range(n_feeds):
        one()
    t_host = time.perf_counter() - t0
    e1.record(stream)
    sess.sync()
    wall = time.perf_counter() - t0
    return dict(host_us_per_feed=t_host / n_feeds * 1e6, wall_us_per_feed=wall / n_feeds * 1e6,
                device_us_per_feed=e0.elapsed_time(e1) / n_feeds * 1e3)


def bench_feed(torch, n_feeds, segments):
    from real_time_audio_sync_amd.annotate import AnnotationTables
    from real_time_audio_sync_amd.ensemble import Ensemble, EnsembleSession
    recs, tables = recordings_and_tables()
    tab = AnnotationTables(tables)
    es = EnsembleSession(recs, tab, MICS, max_dev=2.0, patience=4, c=500, max_run_count=3)
    sess, B = es.live, MICS * G
    ens = Ensemble([b // G for b in range(B)], 2.0, 4, device=sess.dev)
    rs = np.random.RandomState(5)
    audio = (rs.randint(-20000, 20000, size=(B, FEED), dtype=np.int16).astype(np.float32) / np.float32(32768.0))
    for k in range(4):                                   # fill all four staging slots once
        cv, sv = sess.staging(np.float32)
        cv[:] = FEED
        sv[:B * FEED] = audio.reshape(-1)
        sess.submit(np.float32)
    sess.sync()

    def one():
        cv, _ = sess.staging(np.float32)
        cv[:] = FEED
        sess.submit(np.float32)
    for seg in range(segments):
        on = seg % 2 == 1
        sess.reset()
        sess.sync()
        ens.reset()                                      # (reset() clears the ensemble bound at the time only)
        sess.follow_consensus(ens if on else None)
        row = timed(torch, sess, n_feeds, one)
        words = sess.consensus()
        print(json.dumps(dict(kind="feed", follow_consensus=on, streams=B, microphones=MICS, feeds=n_feeds,
                              frames_consumed_total=int(sess.otw.states()[:, 8].sum()),
                              groups_with_a_consensus=int(np.isfinite(words["consensus"]).sum()) if on else None,
                              feeds_done=sess.poll()["feeds_done"], **row)), flush=True)
    es.close()
    ens.close()
    tab.close()


def bench_copies(torch, n_feeds, segments):
    from real_time_audio_sync_amd.annotate import AnnotationTables
    from real_time_audio_sync_amd.ensemble import EnsembleSession
    recs, tables = recordings_and_tables()
    tab = AnnotationTables(tables)
    es = EnsembleSession(recs, tab, MICS, max_dev=2.0, patience=4, c=500, max_run_count=3)
    rs = np.random.RandomState(6)
    mic_audio = [(rs.randint(-20000, 20000, size=FEED, dtype=np.int16).astype(np.float32) / np.float32(32768.0))
                 for _ in range(MICS)]
    independent = [mic_audio[b // G].copy() for b in range(MICS * G)]           # 64 buffers of the caller's own
    for seg in range(segments):
        copied = seg % 2 == 1
        es.live.reset()
        es.sync()
        one = (lambda: es.feed(mic_audio)) if copied else (lambda: es.live.feed(independent))
        row = timed(torch, es.live, n_feeds, one)
        print(json.dumps(dict(kind="copies", fed_as="16 microphones x 4 copies" if copied else "64 independent buffers",
                              feeds=n_feeds, frames_consumed_total=int(es.live.otw.states()[:, 8].sum()), **row)), flush=True)
    es.close()
    tab.close()


def bench_curve(torch, repeats):
    import ensemble_model as em
    from real_time_audio_sync_amd import ensemble
    from real_time_audio_sync_amd.annotate import AnnotationTables
    n_paths, T = 64, 2100
    _, tables = recordings_and_tables()
    tab = AnnotationTables(tables)
    rs = np.random.RandomState(7)
    paths = []
    for p in range(n_paths):
        n = 2100 + int(rs.randint(-40, 41))
        w = rs.uniform(0.3, 0.7)
        steps = np.array([(1, 0), (0, 1), (1, 1)])[rs.choice(3, size=n - 1, p=[w / 2, (1 - w) / 2, 0.5])]
        paths.append(np.concatenate([[(0, 0)], np.cumsum(steps, axis=0)]).astype(np.int32))
    groups = [b // G for b in range(n_paths)]
    pieces = [b % G for b in range(n_paths)]
    ens = ensemble.Ensemble(groups, 2.0, 4, device=tab.device)

    def host():
        return em.curve([p.tolist() for p in paths], groups, tables, pieces, [0] * n_paths, T, FRAME_SECONDS, 2.0, 4)
    want = host()
    got = ensemble.path_consensus(paths, ens, tab, pieces, T)
    for w, g in zip(want, got):
        assert np.array(w, dtype=g.cpu().numpy().dtype).tobytes() == g.cpu().numpy().tobytes(), "the device curve differs from the model"
    P_max = max(len(p) for p in paths)
    host_paths = np.zeros((n_paths, P_max, 2), dtype=np.int32)
    for k, p in enumerate(paths):
        host_paths[k, :len(p)] = p
    dev_paths = torch.from_numpy(host_paths).to(tab.device)
    plen = torch.tensor([len(p) for p in paths], dtype=torch.int32, device=tab.device)
    pieces_d = torch.tensor(pieces, dtype=torch.int32, device=tab.device)
    stream = torch.cuda.current_stream(tab.device)
    for rep in range(repeats):
        t0 = time.perf_counter()
        host()
        t_host = time.perf_counter() - t0
        t0 = time.perf_counter()
        ensemble.path_consensus(paths, ens, tab, pieces, T)
        torch.cuda.synchronize()
        t_dev = time.perf_counter() - t0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for i in range(20):
            ensemble.path_consensus((dev_paths, plen), ens, tab, pieces_d, T)
        e1.record(stream)
        torch.cuda.synchronize()
        print(json.dumps(dict(kind="curve", paths=n_paths, groups=n_paths // G, T=T, points_total=int(sum(len(p) for p in paths)),
                              model_ms=t_host * 1e3, path_consensus_ms=t_dev * 1e3, launch_us=e0.elapsed_time(e1) * 1e3 / 20,
                              frames_with_a_consensus=int(np.isfinite(got[0].cpu().numpy()).sum()),
                              out_flags_set=int(got[3].sum().item()))), flush=True)
    ens.close()
    tab.close()


def main():
    import torch
    n_feeds = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    segments = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble needs a GPU: there is nothing to measure without one")
    bench_feed(torch, n_feeds, segments)
    bench_copies(torch, n_feeds, segments)
    bench_curve(torch, repeats)


if __name__ == "__main__":
    main()
