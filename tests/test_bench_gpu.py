"""A plain `bench.py` run: the timed headline only, and --dump-outputs writes what its last timed step computed --
every stream's path, end state and accumulated-cost bands -- equal to the C oracle on the same seeded streams."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_and_dumped_outputs(tmp_path):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import oracle
    from real_time_audio_sync_amd import shard, synth
    B, n_ref, c, mrc = 8, 400, 100, 3
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", str(B), "--n-ref", str(n_ref), "--c", str(c), "--dump-outputs", str(out)],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert r["steps"] == 3 and r["warmup"] == 1 and r["ms_per_step"] > 0 and r["unit"] == "frames/s"
    assert abs(r["value"] - r["config"]["frames_per_step"] / (r["ms_per_step"] * 1e-3)) / r["value"] < 1e-6
    assert not {"cpu_baseline", "parity", "secondary"} & set(r)          # those come with --full

    got = {f[:-4]: np.load(str(out / f)) for f in os.listdir(str(out))}
    assert set(got) == {"streams", "path_lengths", "paths", "end_state", "row_band", "col_band"}
    assert all(a.dtype == np.float64 for a in got.values()) and list(got["streams"]) == list(range(B))
    ref = synth.synth_ref(n_ref, seed=1000)                  # bench.py's own workload
    ends = np.cumsum(got["path_lengths"]).astype(int)
    frames = 0
    for b in range(B):
        o = oracle.OtwOracle(ref, c, mrc)
        frames += o.run(synth.synth_live(ref, seed=shard.stream_seed(1000, b)))
        assert np.array_equal(got["paths"][ends[b] - len(o.path):ends[b]], o.path), b
        assert got["path_lengths"][b] == got["end_state"][b, 7] == len(o.path)
        rb, cb = o.bands()
        assert np.array_equal(got["row_band"][b], rb, equal_nan=True)
        assert np.array_equal(got["col_band"][b], cb, equal_nan=True)
    assert got["end_state"][:, 8].sum() == frames == r["config"]["frames_per_step"]
