"""bench.py's launch-mode resolution (CPU): --gpus N never silently measures fewer GPUs."""
import os
import subprocess
import sys

import pytest

import bench


def visible(n):
    return lambda: n


def test_single_default():
    assert bench.resolve_mode(1, 1, -1, visible(0)) == "single"


def test_group_when_no_launcher():
    assert bench.resolve_mode(4, 1, -1, visible(8)) == "group"
    assert bench.resolve_mode(1, 1, 1, visible(1)) == "group"      # --group 1 at N = 1


def test_torchrun_when_launched():
    assert bench.resolve_mode(8, 8, -1, visible(0)) == "torchrun"
    assert bench.resolve_mode(1, 2, -1, visible(0)) == "torchrun"


@pytest.mark.parametrize("gpus,world,group,vis", [(4, 1, -1, 2), (2, 1, 1, 1), (2, 1, 0, 8), (4, 2, -1, 8),
                                                  (1, 1, 1, 0)])
def test_refusals(gpus, world, group, vis, capsys):
    with pytest.raises(SystemExit) as e:
        bench.resolve_mode(gpus, world, group, visible(vis))
    assert e.value.code == 2
    assert "bench.py:" in capsys.readouterr().err


def test_cli_refuses_without_devices(root):
    # no GPU in this container: `--gpus 2` must exit non-zero with the reason, not report one GPU
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "2", "--cpu-baseline", "0"],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)
    assert "visible" in r.stderr
    assert r.stdout.strip() == ""


def test_headline_is_strong_scaling_by_default():
    # the metric is "1080p 1024spp, 1/2/4/8 MI355X": the fixed C3 image at every N
    args = bench.parse_args([])
    assert args.scaling == "strong" and args.config == "C3"
    c = bench.CONFIGS[args.config]
    assert (c["width"], c["height"], c["spp"]) == (1920, 1080, 1024)


def test_plain_run_is_the_default():
    # a plain run times the headline only; the roofline, CPU baselines and secondary records need --full
    args = bench.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert args.full is False and args.dump_outputs is None
    assert (args.steps, args.warmup) == (5, 2)
    args = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert args.full is True and args.dump_outputs == "out"


def test_plain_record_has_the_headline_only():
    class R:
        W, H, spp = 64, 32, 16

    cfg = {"scene": "cornell_box"}
    rec = bench.record(cfg, R(), 0.5, 400.0, 4, None, 1)
    assert rec["roofline"] is None
    assert rec["ms_per_step"] == 125.0                      # 0.5 s over 4 steps
    assert rec["value"] == round(64 * 32 * 16 * 4 / 0.5 / 1e6, 3) and rec["unit"] == "Msamples/s"
    assert rec["workload"] == bench.workload_name(cfg, 64, 32, 16)


def test_dump_outputs_whole_and_sampled(tmp_path):
    import numpy as np
    a = np.arange(40 * 30 * 4, dtype=np.float32).reshape(40, 30, 4)
    bench.dump_outputs({"accum": a}, tmp_path / "whole")
    whole = np.load(tmp_path / "whole" / "accum.npy")
    assert whole.dtype == np.float32 and np.array_equal(whole, a)
    # over the limit: a sample of whole pixels, the same on every run and in both arrays of the
    # image, within the limit in all
    b = np.arange(40 * 30, dtype=np.float32).reshape(40, 30, 1)
    limit = 1000 * 20 + 7
    for d in ("s1", "s2"):
        bench.dump_outputs({"accum": a, "accum_nonfinite": b}, tmp_path / d, limit=limit)
    s1, s2 = np.load(tmp_path / "s1" / "accum.npy"), np.load(tmp_path / "s2" / "accum.npy")
    t1 = np.load(tmp_path / "s1" / "accum_nonfinite.npy")
    assert s1.dtype == np.float32 and s1.shape == (1000, 4) and t1.shape == (1000, 1)
    assert s1.nbytes + t1.nbytes <= limit
    assert np.array_equal(s1, s2)
    px = (s1[:, 0] / 4).astype(np.int64)                    # pixel p holds 4p .. 4p + 3
    assert np.all(np.diff(px) > 0) and px[-1] < 40 * 30     # distinct pixels, in image order
    assert np.array_equal(s1, a.reshape(-1, 4)[px])
    assert np.array_equal(t1[:, 0], px)                     # the same pixels
    assert bench.DUMP_MAX_BYTES == 64 << 20


def test_finite_split_keeps_everything_but_nan_payloads():
    import numpy as np
    a = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4) - 5.0
    a[0, 1, 0] = np.nan
    a[0, 1, 3] = -np.inf
    a[1, 2, 2] = np.inf
    values, codes = bench.finite_split(a)
    assert values.dtype == np.float32 and codes.dtype == np.float32
    assert values.shape == a.shape and codes.shape == (2, 3, 1)
    assert np.isfinite(values).all() and np.isfinite(codes).all()
    want = np.zeros((2, 3, 1), dtype=np.float32)
    want[0, 1, 0] = 1 + 3 * 64                              # NaN in channel 0, -inf in channel 3
    want[1, 2, 0] = 2 * 16                                  # +inf in channel 2
    assert np.array_equal(codes, want)
    ok = np.isfinite(a)
    assert np.array_equal(values[ok].view(np.uint32), a[ok].view(np.uint32)) and not values[~ok].any()
    # and back
    c = (codes.astype(np.int64) // 4 ** np.arange(4)) % 4
    back = np.where(c == 1, np.nan, np.where(c == 2, np.inf, np.where(c == 3, -np.inf, values)))
    assert np.array_equal(back, a, equal_nan=True)


def test_gpus_below_one_exits_2(capsys):
    with pytest.raises(SystemExit) as e:
        bench.resolve_mode(0, 1, -1, visible(1))
    assert e.value.code == 2
    assert "bench.py:" in capsys.readouterr().err


def test_group_mode_timing_needs_no_torch(root):
    # --group 1: pt_group_render / pt_group_gather synchronise every device themselves, so timed()
    # brackets them without torch's barriers or events (torch may still be loaded: _native.hip()
    # imports it first to keep one HIP runtime)
    code = (
        "import sys, bench\n"
        "class R:\n"
        "    mode = 'single'\n"
        "    gather_ms = 0.0\n"
        "    def step(self): return 1.0\n"
        "e, k = bench.timed(R(), 2, 1, 0, False, use_torch=False)\n"
        "assert k == 2.0, k\n"
        "assert 'torch' not in sys.modules, 'torch imported'\n"
        "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(root), timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)
    src = (root / "bench.py").read_text()
    # every timed() call passes the process's mode-derived flag
    assert src.count("timed(") - 1 == src.count("use_torch)")
