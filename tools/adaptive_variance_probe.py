#!/usr/bin/env python3
"""Probe of the variance of an adaptive render's image: the estimate kernel's times, and the sweep behind the defaults.

Timing (part A), 1920x1080, generated_scene and cornell_box after render_adaptive(8 spp per call, min_calls 4,
max_calls 128, tolerance 0.02), three interleaved runs, hipEvent times, medians with min-max:
adaptive_variance_kernel staged and unstaged at the default min_batches and at min_batches = 255, where every pixel
with a variance walks the window; beside it, in the same session on a second context that steps a temporal
history, variance_kernel and one variance-guided iteration at s = 1 in both forms.

Quality (part B), the sweep protocol of tools/denoise_probe.py: cornell_box 256^2 and generated_scene 384x216, a
4,096-spp reference, adaptive renders at tolerance 0.05 (min_calls 4, max_calls 32) with 1-spp and with 8-spp
calls; the error = the mean squared difference after Reinhard + gamma 2.2 over the kept pixels.  A setting's
score is the geometric mean over the four renders of filtered / unfiltered.  Beside the grid: the plain a-trous
filter at its defaults on the same renders, and the best score at min_batches = 2 (no window) against the best
above it.

    python tools/adaptive_variance_probe.py [--out profiles/adaptive_variance_probe.json] [--quick]
                                            [--skip-quality] [--skip-timing]
"""
import argparse
import itertools
import json
import pathlib
import statistics
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import pathtracercuda_amd as pa  # noqa: E402
import denoise_probe as dp  # noqa: E402
import temporal_probe as tp  # noqa: E402

GRID = {"min_batches": (2, 4, 8, 16, 32), "sigma_l": (0.5, 1.0, 2.0, 4.0, 8.0, 16.0), "variance_floor": (1e-6, 1e-4)}
ADAPTIVE_QUALITY = dict(min_calls=4, max_calls=32, tolerance=0.05)
ADAPTIVE_TIMING = dict(spp=8, min_calls=4, max_calls=128, tolerance=0.02)


def geomean(xs):
    return float(np.exp(np.mean([np.log(x) for x in xs])))


def quality(quick):
    grid = {k: v[1:3] for k, v in GRID.items()} if quick else GRID
    cases, rows, plain = [], [], {}
    for scene, W, H in dp.QUALITY:
        if quick:
            W, H = W // 4, H // 4
        pt = pa.Pathtracer(W, H)
        cam = pt.load_scene(str(ROOT / "scenes" / f"{scene}.scene.json"))
        pt.render(cam, 8, True, chunks=8 if quick else 512)
        ref = pt.get_hdr_image_data()
        for spp in (1, 8):
            res = pt.render_adaptive(cam, spp, **ADAPTIVE_QUALITY)
            planes = pt.features(cam)["planes"]
            noisy = pt.get_hdr_image_data()
            counts = pt.sample_counts()
            mask = pa.denoise_keep_mask(noisy, planes[1], planes[2]) & np.isfinite(ref[..., :3]).all(-1)
            base = dp.ldr_mse(noisy, ref, mask)
            case = f"{scene}@{spp}spp"
            cases.append({"case": case, "width": W, "height": H, "kept_pixels": int(mask.sum()), "noisy_ldr_mse": base,
                          "mean_calls": float(counts.mean()), "share_at_min_calls": float((counts == 4).mean()),
                          "share_at_max_calls": float((counts == 32).mean()), "mean_spp": res["mean_spp"]})
            plain[case] = dp.ldr_mse(pt.denoise(), ref, mask) / base
            for combo in itertools.product(*grid.values()):
                kw = dict(zip(grid.keys(), combo))
                out = pt.denoise(guide="adaptive", **kw)
                rows.append(dict(kw, case=case, ldr_mse_ratio=dp.ldr_mse(out, ref, mask) / base))
        pt.close()
    table = {}
    for r in rows:
        table.setdefault(tuple(r[k] for k in grid), []).append(r)
    summary = [dict(zip(grid, combo), geomean=geomean([r["ldr_mse_ratio"] for r in rs]),
                    per_case={r["case"]: r["ldr_mse_ratio"] for r in rs}) for combo, rs in table.items()]
    best = min(summary, key=lambda s: s["geomean"])
    d, dv = pa.AVARIANCE_DEFAULTS, pa.VDENOISE_DEFAULTS
    shipped = [s for s in summary if (s["min_batches"], s["sigma_l"], s["variance_floor"]) ==
               (d["min_batches"], pa.ADENOISE_SIGMA_L, dv["variance_floor"])]
    marginals = {k: {str(v): min(s["geomean"] for s in summary if s[k] == v) for v in grid[k]} for k in grid}
    no_window = min((s for s in summary if s["min_batches"] == 2), key=lambda s: s["geomean"], default=None)
    windowed = min((s for s in summary if s["min_batches"] > 4), key=lambda s: s["geomean"], default=None)
    return {"cases": cases, "adaptive": ADAPTIVE_QUALITY, "reference_spp": 8 * (8 if quick else 512), "settings": len(summary),
            "best": best, "shipped_defaults": shipped[0] if shipped else None, "best_geomean_by_value": marginals,
            "top10": sorted(summary, key=lambda s: s["geomean"])[:10],
            "plain_atrous_at_its_defaults": {"geomean": geomean(plain.values()), "per_case": plain},
            "best_without_window_min_batches_2": no_window, "best_with_window_min_batches_above_min_calls": windowed,
            "note": "min_calls is 4, so min_batches 2 and 4 give the same variance: no pixel has fewer than 4 calls"}


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def timing(quick):
    W, H = (320, 180) if quick else (1920, 1080)
    default = pa.AVARIANCE_DEFAULTS["min_batches"]
    out = []
    for scene in ("generated_scene", "cornell_box")[:1 if quick else 2]:
        ad, mom = pa.Pathtracer(W, H), pa.Pathtracer(W, H)
        cam = ad.load_scene(str(ROOT / "scenes" / f"{scene}.scene.json"))
        mom.load_scene(str(ROOT / "scenes" / f"{scene}.scene.json"))
        res = ad.render_adaptive(cam, **dict(ADAPTIVE_TIMING, max_calls=8 if quick else 128))
        ad.features(cam)
        counts = ad.sample_counts()
        names = [f"estimate_{form}_min_batches_{mb}" for mb in (default, 255) for form in ("staged", "unstaged")]
        t = {name: [] for name in names + ["variance_kernel", "guided_s1_staged", "guided_s1_unstaged"]}
        mcam = cam

        def one_run(record):
            nonlocal mcam
            for mb in (default, 255):
                for form, staging in (("staged", 1), ("unstaged", 2)):
                    ad.denoise(guide="adaptive", min_batches=mb, iterations=1, staging=staging)
                    if record:
                        t[f"estimate_{form}_min_batches_{mb}"].append(ad.adaptive_variance_timing())
            mom.render(mcam, 1, True)
            mom.features(mcam)
            mom.temporal(frames=1, variance=True)
            if record:
                t["variance_kernel"].append(mom.temporal_moments_timing()["estimate"])
            for form, staging in (("staged", 1), ("unstaged", 2)):
                mom.denoise(source="temporal", guide="variance", iterations=1, staging=staging)
                if record:
                    t["guided_s1_" + form].append(mom.denoise_timing()["iterations"][0])
            mcam = tp.step_camera(mcam)

        one_run(False)
        one_run(False)
        for _ in range(3):
            one_run(True)
        var = ad.adaptive_variance()                  # of the last call: min_batches 255
        row = {"scene": scene, "width": W, "height": H, "runs": 3, "adaptive": dict(ADAPTIVE_TIMING), "rounds": res["rounds"],
               "mean_calls": float(counts.mean()), "share_with_a_variance": float((var >= 0).mean()),
               "young_share_at_default_min_batches": float(((counts < default) & (var >= 0)).mean()),
               "young_share_at_min_batches_255": float(((counts < 255) & (var >= 0)).mean())}
        for name, xs in t.items():
            row[name + "_ms"] = spread(xs)
        out.append(row)
        ad.close()
        mom.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "adaptive_variance_probe.json"))
    ap.add_argument("--quick", action="store_true", help="tiny sizes and grid: a rehearsal of the tool, not a measurement")
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--skip-timing", action="store_true")
    args = ap.parse_args()
    if pa.device_count() < 1:
        raise SystemExit("adaptive_variance_probe: no GPU visible")
    out = pathlib.Path(args.out)
    record = json.loads(out.read_text()) if out.exists() and (args.skip_quality or args.skip_timing) else {}
    record.update({"tool": "tools/adaptive_variance_probe.py", "quick": args.quick, "grid": {k: list(v) for k, v in GRID.items()},
                   "defaults": dict(pa.VDENOISE_DEFAULTS, sigma_l=pa.ADENOISE_SIGMA_L, **pa.AVARIANCE_DEFAULTS)})
    if not args.skip_timing:
        record["timing"] = timing(args.quick)
        print("timing done", flush=True)
    if not args.skip_quality:
        record["quality"] = quality(args.quick)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(record, indent=1) + "\n")
    print(json.dumps({k: v for k, v in record.items() if k != "quality"}, indent=1)[:8000])
    if "quality" in record:
        q = record["quality"]
        print(json.dumps({k: q[k] for k in q if k not in ("top10",)}, indent=1)[:8000])


if __name__ == "__main__":
    main()
