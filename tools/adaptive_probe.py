"""Cost of adaptive sampling (pt_render_adaptive) next to the plain fused launch, same process:
  (a) tolerance 0, max_calls = 128 against render_raw(cam, 8, 128, True): the same samples, so the ratio
      is the overhead of the rounds (evaluation, compaction, one launch per call) plus the loss of the
      cost order and run-ahead; results cross-checked bit-identical;
  (b) tolerances 0.05 / 0.02 / 0.01 with min_calls = 4, max_calls = 128: wall time, mean calls per
      pixel, per-round live-lane fraction (active pixels / (64 x waves launched)) and Msamples/s of the
      adaptive rounds against the plain launch's.  (b) says nothing about quality: no error is measured.
    python tools/adaptive_probe.py [--rounds 3] [--out profiles/adaptive_probe.json]
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import pathtracercuda_amd as pa  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--spp", type=int, default=8)
ap.add_argument("--max-calls", type=int, default=128)
ap.add_argument("--out", default=str(ROOT / "profiles/adaptive_probe.json"))
a = ap.parse_args()
SPP, MAXC = a.spp, a.max_calls


def med(v):
    return round(float(np.median(v)), 3)


out = {"spp_per_call": SPP, "max_calls": MAXC, "rounds": a.rounds, "cases": {}}
for name, W, H in [("generated_scene", 1920, 1080), ("cornell_box", 512, 512)]:
    pt = pa.Pathtracer(W, H)
    cam = pt.load_scene(str(ROOT / f"scenes/{name}.scene.json"))
    st = pt.rng_state()
    npix = W * H
    plain_wall, plain_gpu, ad_wall, ad_gpu = [], [], [], []
    same = True
    for r in range(a.rounds):                      # interleaved: plain, adaptive, plain, ...
        pt.set_rng_state(st)
        t0 = time.perf_counter()
        plain_gpu.append(pt.render_raw(cam, SPP, MAXC, True))
        plain_wall.append((time.perf_counter() - t0) * 1e3)
        want = pt.accum().view(np.uint32)
        pt.set_rng_state(st)
        t0 = time.perf_counter()
        res = pt.render_adaptive(cam, SPP, 2, MAXC, 0.0)
        ad_wall.append((time.perf_counter() - t0) * 1e3)
        ad_gpu.append(res["gpu_ms"])
        same = same and np.array_equal(pt.accum().view(np.uint32), want)
    total = npix * SPP * MAXC
    case = {"image": f"{W}x{H}", "variant": pt.last_variant,
            "plain": {"wall_ms": plain_wall, "gpu_ms": plain_gpu, "Msamples_s": round(total / med(plain_wall) / 1e3, 1)},
            "tolerance_0": {"wall_ms": ad_wall, "gpu_ms": ad_gpu, "launches": res["rounds"], "bit_identical": bool(same),
                            "Msamples_s": round(total / med(ad_wall) / 1e3, 1),
                            "wall_over_plain": round(med(ad_wall) / med(plain_wall), 4)},
            "sweep": {}}
    for tol in (0.05, 0.02, 0.01):
        walls, gpus = [], []
        for r in range(a.rounds):
            pt.set_rng_state(st)
            t0 = time.perf_counter()
            res = pt.render_adaptive(cam, SPP, 4, MAXC, tol)
            walls.append((time.perf_counter() - t0) * 1e3)
            gpus.append(res["gpu_ms"])
        counts = pt.sample_counts()
        # the same render one step at a time (the steps are counted from the reset, so continuing to
        # max_calls = k runs step k alone): active pixels of every round
        pt.set_rng_state(st)
        active = [npix]
        pt.render_adaptive(cam, SPP, 4, 4, tol)
        for k in range(5, MAXC + 1):
            step = pt.render_adaptive(cam, SPP, 4, k, tol, reset=False)
            if step["rounds"] == 0:
                break
            active.append(step["samples"] // SPP)
        stepped_same = bool(np.array_equal(pt.sample_counts(), counts))
        live = [c / (64 * ((c + 63) // 64)) for c in active]
        case["sweep"][str(tol)] = {
            "wall_ms": walls, "gpu_ms": gpus, "launches": res["rounds"], "mean_calls": round(res["samples"] / SPP / npix, 3),
            "mean_spp": round(res["mean_spp"], 2), "pixels_at_max": int((counts == MAXC).sum()),
            "Msamples_s": round(res["samples"] / med(walls) / 1e3, 1),
            "Msamples_s_over_plain": round(res["samples"] / med(walls) / (total / med(plain_wall)), 4),
            "wall_over_plain": round(med(walls) / med(plain_wall), 4),
            "active_per_round": active, "live_lane_fraction_min": round(min(live), 4),
            "live_lane_fraction_mean": round(float(np.mean(live)), 5), "stepped_counts_identical": stepped_same}
    out["cases"][name] = case
    pt.close()
pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
pathlib.Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
print(json.dumps(out))
