"""bench.py end to end on the GPU: a plain run prints the headline only and --dump-outputs writes
what its last timed step computed (C2, the smallest workload: 512x512 x 64 spp, ~5 ms a step)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_its_last_step(root, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--config", "C2", "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["metric"] == bench.METRIC and out["unit"] == "Msamples/s" and out["dtype"] == "f32"
    assert out["higher_is_better"] is True and out["steps"] == 2 and out["warmup"] == 1
    assert out["ms_per_step"] > 0.0
    assert out["value"] == pytest.approx(512 * 512 * 64 / out["ms_per_step"] / 1e3, rel=1e-3)
    # nothing but the headline was measured
    assert out["roofline"] is None and out["cpu_baseline"] is None and "secondary" not in out
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["accum.npy", "accum_nonfinite.npy"]
    dumped = np.load(tmp_path / "out" / "accum.npy")
    codes = np.load(tmp_path / "out" / "accum_nonfinite.npy")
    assert dumped.dtype == np.float32 and dumped.shape == (512, 512, 4)
    assert codes.dtype == np.float32 and codes.shape == (512, 512, 1)
    assert np.isfinite(dumped).all() and dumped[..., :3].max() > 0.0
    assert not codes.any()                                  # cornell_box: every sum is finite
    # the same inputs on every run: this process's run of the same path gives the same bits (every
    # step renders with ignore_history from RNG streams that move on, so the step count matters)
    c = bench.CONFIGS["C2"]
    run = bench.Run(c, c["width"], c["height"], c["spp"], 0, 1, 0, 1, "single")
    run.prime()
    for _ in range(3):
        run.step()
    mine = run.outputs()
    raw = run.pt.accum()
    run.close()
    assert np.array_equal(dumped.view(np.uint32), mine["accum"].view(np.uint32))
    assert np.array_equal(codes, mine["accum_nonfinite"])
    assert np.array_equal(dumped.view(np.uint32), raw.view(np.uint32))     # nothing was replaced
