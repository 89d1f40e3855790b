#!/usr/bin/env python3
"""Denoiser probe: the sweep that chooses the defaults, and the timings of the new kernels.

Quality (part A).  cornell_box and generated_scene, each rendered at 1 and at 8 spp and denoised with every
combination of the grid below, against a 4096-spp render of the same scene by the same kernel.  Two
errors over the kept finite pixels (the pixels the filter may change):
  rel_mse   mean of (x - ref)^2 / (ref^2 + 0.01) over the three channels (the test's condition)
  ldr_mse   mean squared difference after the tonemap's Reinhard + gamma 2.2 (what a viewer sees; bounded,
            so a handful of fireflies does not decide it)
each as the ratio denoised / noisy.  The chosen setting minimises the geometric mean of the ldr_mse ratio
over the four cases among the settings whose rel_mse ratio is below 1 in every case.

Timing (part B), 1920x1080, three interleaved runs: the feature pass; every filter iteration with the
staged and with the unstaged form; the whole filter at the defaults beside the 1-spp progressive frame of
the same session.  All times are hipEvent times of the kernels.

    python tools/denoise_probe.py [--out profiles/denoise_probe.json] [--quick]
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

import pathtracercuda_amd as pa  # noqa: E402

GRID = {"factor": (0.5, 1.0, 2.0, 4.0, 8.0, 16.0), "sigma_plane": (0.005, 0.02, 0.1), "normal_power_log2": (3, 5, 7),
        "iterations": (3, 4, 5, 6), "demodulate": (True, False)}
QUALITY = (("cornell_box", 256, 256), ("generated_scene", 384, 216))
TIMING = (("generated_scene", 1920, 1080), ("cornell_box", 1920, 1080))


def rel_mse(img, ref, mask):
    a, r = img[..., :3][mask].astype(np.float64), ref[..., :3][mask].astype(np.float64)
    return float(np.mean((a - r) ** 2 / (r * r + 0.01)))


def ldr(img):
    c = np.maximum(img[..., :3].astype(np.float64), 0.0)
    return (c / (c + 1.0)) ** (1.0 / 2.2)


def ldr_mse(img, ref, mask):
    return float(np.mean((ldr(img)[mask] - ldr(ref)[mask]) ** 2))


def quality(quick):
    rows, cases = [], []
    grid = {k: v[:2] for k, v in GRID.items()} if quick else GRID
    for scene, W, H in QUALITY:
        if quick:
            W, H = W // 4, H // 4
        pt = pa.Pathtracer(W, H)
        cam = pt.load_scene(str(ROOT / "scenes" / f"{scene}.scene.json"))
        pt.render(cam, 8, True, chunks=8 if quick else 512)
        ref = pt.get_hdr_image_data()
        feats = pt.features(cam)
        planes = feats["planes"]
        for spp in (1, 8):
            pt.render(cam, spp, True)
            noisy = pt.get_hdr_image_data()
            mask = pa.denoise_keep_mask(noisy, planes[1], planes[2]) & np.isfinite(ref[..., :3]).all(-1)
            base = (rel_mse(noisy, ref, mask), ldr_mse(noisy, ref, mask))
            case = f"{scene}@{spp}spp"
            cases.append({"case": case, "width": W, "height": H, "kept_pixels": int(mask.sum()),
                          "noisy_rel_mse": base[0], "noisy_ldr_mse": base[1]})
            for combo in itertools.product(*grid.values()):
                kw = dict(zip(grid.keys(), combo))
                sigma = pa.auto_sigma_color(noisy, *planes, demodulate=kw["demodulate"], factor=kw["factor"])
                out = pt.denoise(iterations=kw["iterations"], sigma_color=sigma, sigma_plane=kw["sigma_plane"],
                                 normal_power_log2=kw["normal_power_log2"], demodulate=kw["demodulate"])
                rows.append(dict(kw, case=case, sigma_color=sigma, rel_mse_ratio=rel_mse(out, ref, mask) / base[0],
                                 ldr_mse_ratio=ldr_mse(out, ref, mask) / base[1]))
        pt.close()
    return cases, rows


def choose(cases, rows):
    """Per setting: the geometric means over the cases, the worst rel_mse ratio; the choice."""
    keys = list(GRID)
    table = {}
    for r in rows:
        table.setdefault(tuple(r[k] for k in keys), []).append(r)
    summary = []
    for combo, rs in table.items():
        if len(rs) != len(cases):
            continue
        summary.append(dict(zip(keys, combo), ldr_geomean=float(np.exp(np.mean([np.log(r["ldr_mse_ratio"]) for r in rs]))),
                            rel_geomean=float(np.exp(np.mean([np.log(r["rel_mse_ratio"]) for r in rs]))),
                            rel_worst=max(r["rel_mse_ratio"] for r in rs),
                            per_case={r["case"]: [r["rel_mse_ratio"], r["ldr_mse_ratio"]] for r in rs}))
    ok = [s for s in summary if s["rel_worst"] < 1.0]
    best = min(ok or summary, key=lambda s: s["ldr_geomean"])
    d = pa.DENOISE_DEFAULTS
    shipped = [s for s in summary if (s["factor"], s["sigma_plane"], s["normal_power_log2"], s["iterations"], s["demodulate"])
               == (pa.DENOISE_SIGMA_FACTOR, d["sigma_plane"], d["normal_power_log2"], d["iterations"], d["demodulate"])]
    marginals = {k: {str(v): min(s["ldr_geomean"] for s in (ok or summary) if s[k] == v) if any(s[k] == v for s in (ok or summary))
                     else None for v in GRID[k]} for k in keys}
    return {"settings": len(summary), "settings_with_rel_mse_below_1_everywhere": len(ok), "best": best,
            "shipped_defaults": shipped[0] if shipped else None, "best_ldr_geomean_by_value": marginals,
            "top10": sorted(ok or summary, key=lambda s: s["ldr_geomean"])[:10]}


def timing(quick):
    out = []
    for scene, W, H in TIMING[:1] if quick else TIMING:
        if quick:
            W, H = 320, 180
        pt = pa.Pathtracer(W, H)
        cam = pt.load_scene(str(ROOT / "scenes" / f"{scene}.scene.json"))
        pt.render(cam, 8, True)
        pt.features(cam)
        pt.denoise(iterations=6, staging=1)
        pt.denoise(iterations=6, staging=2)                       # both forms warm
        frame, feat, staged, unstaged, total = [], [], [], [], []
        for _ in range(3):
            for _k in range(4):
                frame.append(pt.render_raw(cam, 1, 1, False))
            pt.features(cam)
            pt.denoise(iterations=6, staging=1)
            t = pt.denoise_timing()
            feat.append(t["features"])
            staged.append(t["iterations"][:6])
            pt.denoise(iterations=6, staging=2)
            unstaged.append(pt.denoise_timing()["iterations"][:6])
            pt.denoise()
            t = pt.denoise_timing()
            total.append({"prepare": t["prepare"], "iterations": t["iterations"][:pa.DENOISE_DEFAULTS["iterations"]],
                          "finish": t["finish"],
                          "sum": t["prepare"] + sum(t["iterations"]) + t["finish"]})
        med = statistics.median
        out.append({"scene": scene, "width": W, "height": H, "runs": 3,
                    "progressive_1spp_frame_ms": {"median": med(frame), "all": frame},
                    "feature_pass_ms": {"median": med(feat), "all": feat},
                    "iteration_ms_staged": {"step": [1 << i for i in range(6)], "runs": staged,
                                            "median": [med(r[i] for r in staged) for i in range(6)],
                                            "note": "steps above 4 are never staged: both rows run the unstaged form there"},
                    "iteration_ms_unstaged": {"runs": unstaged, "median": [med(r[i] for r in unstaged) for i in range(6)]},
                    "filter_at_defaults_ms": {"median_sum": med(t["sum"] for t in total), "runs": total}})
        pt.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "denoise_probe.json"))
    ap.add_argument("--quick", action="store_true", help="tiny sizes and grid: a rehearsal of the tool, not a measurement")
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--rows", action="store_true", help="keep every row of the sweep in the file (large)")
    args = ap.parse_args()
    if pa.device_count() < 1:
        raise SystemExit("denoise_probe: no GPU visible")
    record = {"tool": "tools/denoise_probe.py", "quick": args.quick, "grid": {k: list(v) for k, v in GRID.items()}}
    if not args.skip_quality:
        cases, rows = quality(args.quick)
        record["cases"] = cases
        record["choice"] = choose(cases, rows)
        if args.rows:
            record["rows"] = rows
    record["timing"] = timing(args.quick)
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(record, indent=1) + "\n")
    print(json.dumps({k: record[k] for k in record if k not in ("rows",)}, indent=1)[:6000])


if __name__ == "__main__":
    main()
