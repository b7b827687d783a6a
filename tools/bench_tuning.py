#!/usr/bin/env python3
"""What the tuning estimator costs (profiles/tuning.md), one JSON object per line, times from events on the stream, median
of `repeats`:

  kind=estimate    chroma.estimate_tuning of a 30-minute signal already on the device, end to end (the STFT in chunks of
                   `chunk_frames` frames, one accumulate per chunk, one pick, the read-back of two words), and its result.
  kind=chunk       one chunk of `chunk_frames` frames in the same run: ChromaPlan.frames(want_stft=True, want_chroma=False)
                   alone and TuningPlan.accumulate alone, with the bytes per second each moves (the STFT it writes / reads).
                   accumulate is timed twice: on the chunk just used (`warm`: 64 MiB, resident in the Infinity Cache, which
                   is how estimate_tuning meets it right behind the STFT kernel) and rotating over `rotate` different
                   chunks that together exceed that cache (`cold`).
  kind=pick        the pick launch alone.

    python tools/bench_tuning.py [minutes=30] [chunk_frames=2048] [repeats=5] [rotate=6]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(torch, stream, fn, repeats):
    """Median milliseconds of fn() between two events, after one untimed call."""
    fn()
    stream.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), [round(v, 4) for v in out]


def main():
    import torch
    import tuning_model as tm
    from real_time_audio_sync_amd import chroma
    minutes, chunk_frames, repeats, rotate = [int(v) for v in (sys.argv[1:5] + ["30", "2048", "5", "6"][len(sys.argv) - 1:])]
    plan, tuner = chroma._plan(), chroma._tuner()
    stream = torch.cuda.current_stream(plan.device)
    minute = tm.source(7.0, seconds=60.0)
    x = torch.from_numpy(np.tile(minute, minutes)).to(plan.device)
    L, H = plan.fft_len, plan.hop
    frames = plan.num_frames(x.numel(), L // 2)
    result = {}

    def estimate():
        result["r"] = chroma.estimate_tuning(x, chunk_frames=chunk_frames)
    ms, runs = timed(torch, stream, estimate, repeats)
    print(json.dumps(dict(kind="estimate", minutes=minutes, samples=x.numel(), frames=frames, chunk_frames=chunk_frames,
                          chunks=-(-frames // chunk_frames), ms=round(ms, 4), runs_ms=runs, cents=result["r"][0],
                          n_peaks=result["r"][1], stft_bytes=frames * plan.n_bins * 16)), flush=True)

    c = min(chunk_frames, frames - 1)
    chunk_bytes = c * plan.n_bins * 16
    rotate = max(1, min(rotate, (frames - 1) // c))                 # as many different chunks as the signal holds
    pieces = [x[(1 + k * c) * H - L // 2:(1 + k * c) * H - L // 2 + (c - 1) * H + L] for k in range(rotate)]
    stfts = []

    def stft_of(k):
        return plan.frames(pieces[k], pad_left=0, want_stft=True, want_chroma=False, n_frames=c)[1]
    ms_stft, runs_stft = timed(torch, stream, lambda: stft_of(0), repeats)
    for k in range(rotate):
        stfts.append(stft_of(k))
    hist = torch.zeros((1, tuner.R), dtype=torch.int64, device=plan.device)
    ms_warm, runs_warm = timed(torch, stream, lambda: tuner.accumulate(stfts[-1], None, hist), repeats)
    turn = [0]

    def cold():
        turn[0] = (turn[0] + 1) % rotate
        tuner.accumulate(stfts[turn[0]], None, hist)
    for _ in range(rotate):
        cold()
    ms_cold, runs_cold = timed(torch, stream, cold, repeats)
    tb = lambda ms: round(chunk_bytes / (ms * 1e-3) / 1e12, 4)     # noqa: E731
    print(json.dumps(dict(kind="chunk", chunk_frames=c, chunk_bytes=chunk_bytes, rotate=rotate,
                          stft_ms=round(ms_stft, 4), stft_runs_ms=runs_stft, stft_write_TBps=tb(ms_stft),
                          accumulate_warm_ms=round(ms_warm, 4), accumulate_warm_runs_ms=runs_warm, accumulate_warm_TBps=tb(ms_warm),
                          accumulate_cold_ms=round(ms_cold, 4), accumulate_cold_runs_ms=runs_cold, accumulate_cold_TBps=tb(ms_cold))),
          flush=True)
    ms_pick, runs_pick = timed(torch, stream, lambda: tuner.pick(hist), repeats)
    print(json.dumps(dict(kind="pick", S=1, R=tuner.R, W=5, ms=round(ms_pick, 4), runs_ms=runs_pick)), flush=True)


if __name__ == "__main__":
    main()
