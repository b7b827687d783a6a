#!/usr/bin/env python3
"""rts_otw_backward (csrc/otw_backward.h): what it costs on the GPU and what it gains in accuracy.  One JSON object per
line, printed and appended to profiles/otw_backward.jsonl.

  group "timing" (GPU)   BASELINE configs[2] (B = 64, c = 500, N = 2200, float32 features) on a single-reference handle
                         and on an rts_otw_create_refs handle: device time of the call from HIP events on the launch
                         stream, split into trace replay and backtrace by the events the call records itself
                         (rts_otw_backward_times); warm-up, then `reps` calls, median and min / max.  Beside it, on the
                         same inputs, the route without it: rts_otw_replay_dense into [B][2N][N] buffers, the read-back
                         and the numpy walk of tests/otw_backward_model.py, wall clock, at the largest B whose dense
                         buffers fit the device.
  group "accuracy" (CPU) forward path against backward path of the CPU oracle on the chopin 20-bar fixture through
                         evaluate.AlignmentError.

    python tools/bench_backward.py [--reps 20] [--dense-reps 20] [--cpu-only | --gpu-only]
"""
import argparse
import ctypes
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "otw_backward.jsonl")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def spread(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return dict(median=float(np.median(xs)), min=float(xs.min()), max=float(xs.max()))


# ---- group 1 ------------------------------------------------------------------------------------------------------------
def time_backward(eng, live, lens, reps, warm=3):
    """-> (total / replay / backtrace milliseconds per call, workspace bytes, the outputs of the last call)."""
    import torch
    from real_time_audio_sync_amd import _native as nat
    from real_time_audio_sync_amd.otw_batch import _np_dtype_code
    dev, B, cap = eng.device, eng.B, 3 * eng.N + 8
    need = ctypes.c_size_t()
    nat.check(nat.lib.rts_otw_backward_workspace_bytes(eng.N, eng.c, B, ctypes.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    path = torch.empty((B, cap, 2), dtype=torch.int32, device=dev)
    plen = torch.empty(B, dtype=torch.int32, device=dev)
    total = torch.empty(B, dtype=torch.float64, device=dev)
    end = torch.empty((B, 2), dtype=torch.int32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        nat.check(nat.lib.rts_otw_backward(eng._h, live.data_ptr(), _np_dtype_code(live.dtype), int(live.shape[1]),
                                           lens.data_ptr(), path.data_ptr(), plen.data_ptr(), total.data_ptr(),
                                           end.data_ptr(), None, ws.data_ptr(), ws.numel(), stream))
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    tot, rep, bt = [], [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        a, b = ctypes.c_float(), ctypes.c_float()
        nat.check(nat.lib.rts_otw_backward_times(eng._h, ctypes.byref(a), ctypes.byref(b)))
        tot.append(e0.elapsed_time(e1))
        rep.append(a.value)
        bt.append(b.value)
    n = plen.cpu().numpy()
    ph = path.cpu().numpy()
    return spread(tot), spread(rep), spread(bt), need.value, [ph[b, :n[b]].copy() for b in range(B)], total.cpu().numpy()


def dense_route(eng, B_dense, reps, warm=1):
    """rts_otw_replay_dense + read-back + numpy walk, wall clock per call in milliseconds, for streams [0, B_dense)."""
    import torch
    from otw_backward_model import backward
    ts, paths = [], None
    for i in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        acc, cost = eng.replay_dense()
        st = eng.states()
        paths = []
        for b in range(B_dense):
            m = backward(acc[b].cpu().numpy(), cost[b].cpu().numpy(), st[b][0], st[b][1], eng.c, st[b][8])
            paths.append(m["path"])
        if i >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
        del acc, cost
    return spread(ts), paths


def group_timing(reps, dense_reps):
    import torch
    from real_time_audio_sync_amd import synth
    from real_time_audio_sync_amd.otw_batch import BatchedOTW
    B, c, N, mrc = 64, 500, 2200, 3
    dev = torch.device("cuda:0")
    ref = synth.synth_ref(N, seed=1000)
    lives = [synth.synth_live(ref, seed=1001 + b) for b in range(B)]
    dense_per_stream = 2 * 2 * N * N * 8
    # ---- single reference: the new call, and the dense route on the same handle
    eng = BatchedOTW(ref, c, mrc, batch=B, dtype=torch.float32, device=dev)
    lv, ln = eng.pack(lives)
    eng.run(lv, ln)
    tot, rep, bt, ws_bytes, paths, totals = time_backward(eng, lv, ln, reps)
    free = torch.cuda.mem_get_info(dev)[0]
    B_fit = int(min(B, (free * 0.8) // dense_per_stream))
    emit(group="timing", what="rts_otw_backward", handle="rts_otw_create", B=B, c=c, N=N, features="f32", reps=reps,
         ms_call=tot, ms_replay=rep, ms_backtrace=bt, workspace_bytes=ws_bytes, bytes_per_logged_cell=8,
         dense_bytes=B * dense_per_stream, path_points_mean=float(np.mean([len(p) for p in paths])))
    if dense_reps > 0 and B_fit >= 1:
        # the handle has to hold B streams either way; the dense route walks as many as fit (all of them on this device)
        d, dpaths = dense_route(eng, B_fit, dense_reps)
        same = all(np.array_equal(paths[b], dpaths[b]) for b in range(B_fit))
        emit(group="timing", what="rts_otw_replay_dense + read-back + numpy walk", handle="rts_otw_create", B=B,
             B_walked=B_fit, c=c, N=N, features="f32", reps=dense_reps, ms_wall=d, dense_bytes=B * dense_per_stream,
             same_paths_as_rts_otw_backward=bool(same))
    eng.close()
    torch.cuda.empty_cache()
    # ---- per-stream references: ranges of different lengths (the dense replay is refused on such a handle)
    refs = [synth.synth_ref(N - 25 * (b % 8), seed=2000 + b) for b in range(B)]
    lives = [synth.synth_live(r, seed=3000 + b) for b, r in enumerate(refs)]
    eng = BatchedOTW.with_references(refs, c, mrc, dtype=torch.float32, device=dev)
    lv, ln = eng.pack(lives)
    eng.run(lv, ln)
    tot, rep, bt, ws_bytes, paths, totals = time_backward(eng, lv, ln, reps)
    emit(group="timing", what="rts_otw_backward", handle="rts_otw_create_refs", B=B, c=c, N=eng.N, features="f32",
         reps=reps, ms_call=tot, ms_replay=rep, ms_backtrace=bt, workspace_bytes=ws_bytes, bytes_per_logged_cell=8,
         path_points_mean=float(np.mean([len(p) for p in paths])))
    eng.close()


# ---- group 2 ------------------------------------------------------------------------------------------------------------
def chopin_audio():
    pieces = {}
    for fn in sorted(glob.glob(os.path.join(GOLDEN, "chopin_20b_audio.part*.npz"))):
        z = np.load(fn)
        for k in z.files:
            pieces.setdefault(k, []).append(z[k])
    return {k.replace("_lr_sum", ""): (np.concatenate(v).astype(np.float32) / np.float32(65536.0)) for k, v in pieces.items()}


def group_accuracy():
    import oracle
    from oracle import chroma_oracle
    from otw_backward_model import from_oracle
    from real_time_audio_sync_amd import evaluate
    audio = chopin_audio()
    ref_csv = os.path.join(GOLDEN, "chopin_rubinstein_20b.csv")
    live_csv = os.path.join(GOLDEN, "chopin_rachmaninoff_20b.csv")
    variants = (("OTW", oracle.OTW), ("LiveNote", oracle.LIVENOTE), ("LiveNoteV2", oracle.LIVENOTE_V2))
    feats = (("chroma", "dot", chroma_oracle.wav_to_chroma, oracle.COST_DOT),
             ("chroma_diff", "euclid", chroma_oracle.wav_to_chroma_diff, oracle.COST_EUCLID))

    def row(path):
        s = evaluate.AlignmentError(ref_csv, live_csv, [(int(l), int(r)) for l, r in path]).stats()
        return dict(points=s["count"], mean_sq_beat_error=s["squared_beat_error"] / s["count"],
                    pct_off_1_beat=s["pct_off_beats"][1], pct_off_1_s=s["pct_off_seconds"][1])
    for fname, cname, fn, cost in feats:
        ref, live = fn(audio["ref"]), fn(audio["live"])
        for vname, variant in variants:
            for c in (50, 100, 200):
                m, o = from_oracle(ref, live, c, 3, variant, cost)
                emit(group="accuracy", tracker=vname, c=c, max_run_count=3, features=fname, cost=cname, mode="insert",
                     forward=row(o.path), backward=row(m["path"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dense-reps", type=int, default=20)
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--gpu-only", action="store_true")
    args = ap.parse_args()
    if not args.cpu_only:
        group_timing(args.reps, args.dense_reps)
    if not args.gpu_only:
        group_accuracy()


if __name__ == "__main__":
    main()
