"""Device and host time of rts_otw_export / rts_otw_import beside a plain device-to-device copy of the same bytes.

    python tools/bench_snapshot.py [--streams 64] [--n-ref 2200] [--c 500] [--reps 20] [--out profiles/snapshot_bench.jsonl]

64 streams at N = 2200, c = 500 with a full history (a slow player: every stream runs into RTS_LIVE_OVERFLOW, so its
record holds 2 N frames).  Per call: HIP events round the enqueue on the current stream, the median of ``reps``; the host
time is what the call itself takes to return (it does not synchronise).  The copy is ``hipMemcpyAsync`` device to device
(torch's ``copy_``) of n * used_bytes on the same stream in the same session.  Prints one JSON line and appends it to
``--out``."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from real_time_audio_sync_amd import _native as nat, synth  # noqa: E402
from real_time_audio_sync_amd.otw_batch import BatchedOTW  # noqa: E402


def timed(fn, reps):
    """-> (median device ms, median host us) of ``fn`` over ``reps`` calls, one warm-up first."""
    fn()
    torch.cuda.synchronize()
    dev, host = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        fn()
        host.append((time.perf_counter() - t0) * 1e6)
        b.record()
        b.synchronize()
        dev.append(a.elapsed_time(b))
    return float(np.median(dev)), float(np.median(host))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--n-ref", type=int, default=2200)
    ap.add_argument("--c", type=int, default=500)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "snapshot_bench.jsonl"))
    args = ap.parse_args()
    B, N, c = args.streams, args.n_ref, args.c
    ref = synth.synth_ref(N, seed=1)
    live = synth.synth_live(ref, seed=2, lo=0.3, hi=0.4)[:, :2 * N + 64]   # slower than three rows a column: overflows
    assert live.shape[1] > 2 * N
    src = BatchedOTW(ref, c, 3, batch=B, dtype=torch.float32)
    dst = BatchedOTW(ref, c, 3, batch=B, dtype=torch.float32)
    cols = torch.from_numpy(np.ascontiguousarray(live.T)).to(torch.float32).to(src.device)
    for at in range(0, cols.shape[0], 512):
        src.push(cols[at:at + 512].unsqueeze(0).expand(B, -1, -1).contiguous())
    status_words = src.states()[:, nat.ST_STATUS]
    snap = src.export_streams(list(range(B)))
    used = snap.used_bytes()
    hist = snap.headers()[:, 5]
    assert (hist == 2 * N).all(), "the history is not full: %s (status %s)" % (sorted(set(hist)), sorted(set(status_words)))
    idx = np.arange(B, dtype=np.int32)
    desc = nat.SnapshotDesc()
    stream = src._stream()
    status = torch.zeros(B, dtype=torch.int32, device=src.device)

    def do_export():
        nat.check(nat.lib.rts_otw_export(src._h, idx.ctypes.data, B, snap.blob.data_ptr(), snap.rec_stride, ctypes.byref(desc), stream))

    cdesc = snap.c_desc()

    def do_import():
        nat.check(nat.lib.rts_otw_import(dst._h, idx.ctypes.data, B, snap.blob.data_ptr(), snap.rec_stride, ctypes.byref(cdesc),
                                         None, None, status.data_ptr(), stream))

    total = int(used.sum())
    a, b = (torch.empty(total, dtype=torch.uint8, device=src.device) for _ in range(2))
    exp_ms, exp_us = timed(do_export, args.reps)
    imp_ms, imp_us = timed(do_import, args.reps)
    assert not status.any()
    cpy_ms, cpy_us = timed(lambda: b.copy_(a), args.reps)
    out = dict(what="snapshot", streams=B, n_ref=N, c=c, reps=args.reps, rec_stride=int(snap.rec_stride),
               used_bytes_per_stream=int(used[0]), total_bytes=total, export_ms=exp_ms, import_ms=imp_ms, copy_ms=cpy_ms,
               export_over_copy=exp_ms / cpy_ms, import_over_copy=imp_ms / cpy_ms, export_host_us=exp_us, import_host_us=imp_us,
               copy_host_us=cpy_us, export_gb_s=2 * total / exp_ms / 1e6, import_gb_s=2 * total / imp_ms / 1e6,
               copy_gb_s=2 * total / cpy_ms / 1e6, device=torch.cuda.get_device_name(src.device))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
