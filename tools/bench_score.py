#!/usr/bin/env python3
"""What reference chroma from a score costs (profiles/score.md).

Two workloads, both at fft_len 4096, hop 2048, 22 050 Hz, K = 64, float64 output, normalised:
  repertoire   64 pieces of 2200 frames (204 s each), four voices of notes between 0.25 and 1 s
  long         one piece of 30 minutes (19 379 frames) with the same texture
  long, pedal  the same with one pedal note over all of it in front: the worst case for the lower end of a wave's walk
For each: rts_score_chroma (prepare and main kernel) between two events on the stream, notes and piece tables resident;
the numpy model (tests/score_model.py) for ONE 2200-frame piece on this machine's CPU; and, as the yardstick,
rts_chroma_frames over audio of the same number of frames.  The device result of the first piece is compared bit for bit with
the model before anything is timed.  One warm-up run, then `repeats` timed runs.

    python tools/bench_score.py [--repeats 5] [--out profiles/score.md] [--kernel-stats STATS.csv]
    python tools/bench_score.py --kernels-only        # the launches alone, five of each: for a kernel trace
                                                      # (rocprofv3 --kernel-trace --stats -- python tools/bench_score.py --kernels-only)
`--kernel-stats`: the kernel_stats CSV of such a trace; its split of prepare and main kernel goes into the note.
Counters, if wanted, in a run of their own; none is collected here."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FS, L, H, K = 22050, 4096, 2048, 64


def texture(n_frames, seed, pedal=False):
    """(onset, end, pitch, energy) in samples: four voices of notes of 0.25-1 s over n_frames frames, sorted by onset."""
    rng = np.random.RandomState(seed)
    total = n_frames * H
    on, end, pit = [], [], []
    if pedal:
        on.append(0), end.append(total), pit.append(36)
    for voice in range(4):
        t = 0
        while t < total:
            d = int(rng.uniform(0.25, 1.0) * FS)
            on.append(t), end.append(min(t + d, total)), pit.append(int(rng.randint(36 + 12 * voice, 48 + 12 * voice)))
            t += d
    order = np.argsort(np.array(on), kind="stable")
    return (np.array(on, dtype=np.int64)[order], np.array(end, dtype=np.int64)[order], np.array(pit, dtype=np.int32)[order],
            rng.uniform(0.2, 1.0, len(on))[order])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score.md"))
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    import torch

    import score_model as sm
    from real_time_audio_sync_amd import chroma, score
    dev = torch.device("cuda:0")
    plan = score.ScorePlan(L, H, FS, half_life_s=0.1155, K=K, device=dev)
    cplan = chroma.ChromaPlan(L, H, FS, device=dev)
    stream = torch.cuda.current_stream(dev)

    def workload(pieces):
        parts = [texture(n, seed, pedal) for n, seed, pedal in pieces]
        lens = np.array([p[0] for p in pieces], dtype=np.int32)
        nl = np.array([len(p[0]) for p in parts], dtype=np.int32)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
        args = [up(np.concatenate([p[i] for p in parts])) for i in range(4)]
        args += [up(np.concatenate([[0], np.cumsum(nl[:-1], dtype=np.int64)]).astype(np.int64)), up(nl),
                 up(np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)]).astype(np.int64)), up(lens)]
        out = torch.zeros((int(lens.sum()), 12), dtype=torch.float64, device=dev)
        ws = torch.empty((plan.workspace_bytes(int(nl.sum())),), dtype=torch.uint8, device=dev)
        audio = torch.randn((int(lens.sum()) - 1) * H + L - L // 2, dtype=torch.float32, device=dev)
        return dict(parts=parts, args=args, out=out, ws=ws, audio=audio, frames=int(lens.sum()), notes=int(nl.sum()))

    loads = {"repertoire": workload([(2200, 10 + p, False) for p in range(64)]), "long": workload([(30 * 60 * FS // H, 99, False)]),
             "long, pedal": workload([(30 * 60 * FS // H, 99, True)])}

    def run_score(w):
        plan.run(*w["args"], w["out"], True, None, None, w["ws"])

    def run_audio(w):
        cplan.frames(w["audio"], pad_left=L // 2)

    if a.kernels_only:
        for w in loads.values():
            for _ in range(5):
                run_score(w)
        torch.cuda.synchronize()
        return

    # the first piece of the repertoire against the model, bit for bit
    w = loads["repertoire"]
    on, end, pit, en = w["parts"][0]
    t0 = time.perf_counter()
    want = sm.piece_frames(plan.T, plan.CW, plan.DK, L, H, L // 2, on.tolist(), end.tolist(), pit.tolist(), en.tolist(), 2200, True)
    model_ms = (time.perf_counter() - t0) * 1e3
    run_score(w)
    torch.cuda.synchronize()
    assert w["out"][:2200].cpu().numpy().tobytes() == want.tobytes(), "the device chroma differs from the model"

    def timed(fn, w):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn(w)
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    rows = []
    for name, w in loads.items():
        run_score(w), run_audio(w)
        torch.cuda.synchronize()
        for rep in range(a.repeats):
            rows.append(dict(workload=name, frames=w["frames"], notes=w["notes"], score_us=timed(run_score, w), audio_chroma_us=timed(run_audio, w)))
            print(json.dumps(rows[-1]), flush=True)

    split = []
    if a.kernel_stats:
        with open(a.kernel_stats) as fh:
            for r in csv.DictReader(fh):
                if "score_" in r.get("Name", ""):
                    split.append((r["Name"].split("(")[0], int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))

    def span(name, key):
        v = [r[key] for r in rows if r["workload"] == name]
        return "%.1f – %.1f" % (min(v), max(v))

    with open(a.out, "w") as fh:
        fh.write("# Reference chroma from a score: what it costs\n\n")
        fh.write("`tools/bench_score.py`, one MI355X, device events round the calls, one warm-up run and %d timed runs each; fft_len 4096, "
                 "hop 2048, 22 050 Hz, K = 64, float64 output.  The first piece's device result was compared bit for bit with "
                 "tests/score_model.py first.  A note, not a gate: nothing here is asserted anywhere.\n\n" % a.repeats)
        fh.write("| workload | frames | notes | `rts_score_chroma` (µs) | `rts_chroma_frames`, audio of the same length (µs) |\n|---|---|---|---|---|\n")
        for name, w in loads.items():
            fh.write("| %s | %d | %d | %s | %s |\n" % (name, w["frames"], w["notes"], span(name, "score_us"), span(name, "audio_chroma_us")))
        fh.write("\nrepertoire: 64 pieces of 2200 frames; long: one piece of 30 minutes; long, pedal: the same with one note over all "
                 "of it in front, the worst case for the walk's lower end (the running maximum of the ends never falls, so every "
                 "wave walks the notes from the first on and leaves the ended ones out 64 at a time).  The prepare kernel is one "
                 "wave per piece and dominates a single long piece.  The event figures include "
                 "the wrapper's host work in front of the two launches.\n\n")
        fh.write("The numpy model took %.0f ms for ONE piece of 2200 frames (%d notes) on this machine's CPU; it was not run over the "
                 "whole repertoire or the 30-minute piece.\n\n" % (model_ms, len(on)))
        if split:
            fh.write("Kernel trace (`rocprofv3 --kernel-trace --stats`, a run of its own with `--kernels-only`: five calls per workload, "
                     "all workloads together):\n\n| kernel | calls | mean (µs) | min (µs) | max (µs) |\n|---|---|---|---|---|\n")
            for s in split:
                fh.write("| `%s` | %d | %.1f | %.1f | %.1f |\n" % s)
            fh.write("\n")
        else:
            fh.write("The split of prepare and main kernel was not measured (no kernel trace was given to this run).\n\n")
        fh.write("Not measured: counters of any kind, float32 output, other plans, more than 64 pieces.\n")
    plan.close(), cplan.close()


if __name__ == "__main__":
    main()
