"""bench.py's N>1 branch (BASELINE configs[3]: streams sharded 64 per GPU, no data-path collective).

  * test_bench_two_ranks_on_one_device: ALWAYS runs -- a fresh child `python -m torch.distributed.run --nproc-per-node 2
    bench.py --gpus 2 --full`, both ranks on device 0 (BENCH_SINGLE_DEVICE=1) with the report reductions over gloo
    (BENCH_DIST_BACKEND=gloo; RCCL refuses two ranks on one device).  Everything else is the driver's N>1 path: contiguous
    partition, per-rank engines, barrier / max-clock, and the parity gate over EVERY stream of EVERY rank.
  * test_bench_single_process_shards: ALWAYS runs -- `bench.py --gpus 2 --single-process --full` (shard.ShardedOTW), same line.
  * test_bench_over_rccl_on_all_devices: the same over RCCL on however many gfx950 devices the box has (skipped on a
    one-GPU box)."""
import json
import os
import socket
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _bench_line(cmd, env, timeout=900):
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def _check_sharded_line(r, n, per_gpu):
    assert r["n_gpus"] == n and r["scaling"] == "weak"
    assert r["config"]["streams_total"] == per_gpu * n and r["config"]["streams_per_gpu"] == per_gpu
    assert r["config"]["workload"].startswith("configs[3]") and "contiguous" in r["config"]["partition"]
    # every stream of every rank was checked against the C port, none differs
    assert r["parity"]["streams_checked"] == r["parity"]["streams_total"] == per_gpu * n
    assert r["parity"]["path_mismatches"] == 0 and r["value"] > 0
    assert "cpu_baseline" not in r and "secondary" not in r          # N = 1 figures by contract
    assert abs(r["value"] - r["config"]["frames_per_step"] / (r["ms_per_step"] * 1e-3)) / r["value"] < 1e-6


def test_bench_two_ranks_on_one_device():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", BENCH_SINGLE_DEVICE="1", BENCH_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "16", "--n-ref", "600", "--c", "100", "--full"]
    r = _bench_line(cmd, env)
    _check_sharded_line(r, 2, 16)
    assert "gloo" in r["config"]["launcher"]
    # the frames of the two shards add up to what one process counts for the same 32 streams
    one = _bench_line([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                       "--batch", "32", "--n-ref", "600", "--c", "100", "--full", "--no-numpy"], dict(os.environ))
    assert one["config"]["frames_per_step"] == r["config"]["frames_per_step"]
    assert one["parity"]["streams_checked"] == 32 and one["parity"]["path_mismatches"] == 0


def test_bench_single_process_shards():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = dict(os.environ, BENCH_SINGLE_DEVICE="1")
    r = _bench_line([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--single-process", "--steps", "3",
                     "--warmup", "1", "--batch", "16", "--n-ref", "600", "--c", "100", "--full"], env)
    _check_sharded_line(r, 2, 16)
    assert "ShardedOTW" in r["config"]["launcher"]


def test_bench_over_rccl_on_all_devices():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from real_time_audio_sync_amd import _native as nat
    n = nat.lib.rts_device_count()
    if n < 2:
        pytest.skip("one gfx950 device: the RCCL leg needs at least two")
    n = min(n, 6)  # the GPU box allows at most 6 processes on its cards at once
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"),
           "--gpus", str(n), "--steps", "3", "--warmup", "1", "--batch", "8", "--n-ref", "500", "--c", "100", "--full"]
    r = _bench_line(cmd, env, timeout=600)
    _check_sharded_line(r, n, 8)


def test_one_process_many_devices():
    """shard.ShardedOTW: one host process, one BatchedOTW per device, contiguous stream slices, no exchange.  Runs on
    every visible device, and always also as two slices on device 0 (which exercises the slicing, the per-handle
    device switch and two handles side by side on a one-GPU box); results must equal the oracle's."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import numpy as np
    import oracle
    from real_time_audio_sync_amd import shard, synth
    ref, lives = synth.synth_batch(400, 7, seed=77)
    lives[4] = lives[4][:, :150]
    want = []
    for live in lives:
        o = oracle.OtwOracle(ref, 100, 3)
        o.run(live)
        want.append(np.asarray(o.path))
    layouts = [[0, 0], [0, 0, 0]]
    if torch.cuda.device_count() > 1:
        layouts.append(list(range(min(torch.cuda.device_count(), 8))))
    for devices in layouts:
        eng = shard.ShardedOTW(ref, 100, 3, batch=7, devices=devices, dtype=torch.float32)
        assert [hi - lo for lo, hi in eng.slices] == [hi - lo for lo, hi in
                                                      (shard.partition(7, len(devices), r) for r in range(len(devices)))]
        packed = eng.pack(lives)
        eng.run(packed)
        eng.synchronize()
        got = eng.paths()
        assert len(got) == 7
        for b in range(7):
            assert np.array_equal(got[b], want[b]), (devices, b)
            assert np.array_equal(eng.path(b), want[b])
            assert eng.state(b)["n_path"] == len(want[b])
        eng.close()
