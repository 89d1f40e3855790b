#!/usr/bin/env python3
"""Probe of despike, the same-surface firefly clamp: the kernel's times, and the sweep behind the defaults.

Timing (part A), 1920x1080, generated_scene and cornell_box after one 8-spp call, three interleaved runs after
two warm-up runs, hipEvent times, medians with min-max: despike_kernel alone per radius, staged and unstaged (at
the shipped rank, factor and floor), the flat pass, and beside them in the same session one a-trous iteration at
s = 1 (the automatic form).

Quality (part B), the sweep protocol of tools/denoise_probe.py: cornell_box 256^2 and generated_scene 384x216, one
call of 1 spp and one of 8 spp against a 4,096-spp reference.  Per setting of the grid and per case: the relative
MSE and the tonemapped MSE (Reinhard + gamma 2.2) over the kept pixels, as ratios to the noisy image's for the
clamp alone and to denoise()'s at its defaults for the clamp followed by denoise(); the share of the kept pixels
changed; the luminance sum retained.  The choice: among the settings whose clamp alone improves the relative MSE
in all four cases, the best geometric mean of the tonemapped MSE after the filter.  Then the shipped defaults on the
4,096-spp renders themselves: a converged image should be left essentially unchanged.

    python tools/despike_probe.py [--out profiles/despike_probe.json] [--quick] [--skip-quality] [--skip-timing]
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

GRID = {"radius": (1, 2, 3), "rank": (1, 2, 3, 4), "factor": (1.0, 2.0, 4.0, 8.0), "floor": (0.0, 0.01, 0.05, 0.2),
        "demodulate": (False, True)}
LUM = np.array([0.2126, 0.7152, 0.0722])


def geomean(xs):
    return float(np.exp(np.mean([np.log(max(x, 1e-300)) for x in xs])))


def lum_sum(img, mask):
    return float((img[..., :3][mask].astype(np.float64) @ LUM).sum())


def changed_share(a, b, mask):
    diff = (np.ascontiguousarray(a[..., :3]).view(np.uint32) != np.ascontiguousarray(b[..., :3]).view(np.uint32)).any(-1)
    return float((diff & mask).sum() / max(int(mask.sum()), 1))


def settings_of(kw):
    """The grid leaves min_neighbors to the default rule: 3, raised to rank."""
    return dict(kw, min_neighbors=max(pa.DESPIKE_DEFAULTS["min_neighbors"], kw["rank"]))


def quality(quick):
    grid = {k: v[1:3] if len(v) > 2 else v for k, v in GRID.items()} if quick else GRID
    cases, rows, converged = [], [], []
    for scene, W, H in dp.QUALITY:
        if quick:
            W, H = W // 4, H // 4
        pt = pa.Pathtracer(W, H)
        cam = pt.load_scene(str(ROOT / "scenes" / f"{scene}.scene.json"))
        pt.render(cam, 8, True, chunks=8 if quick else 512)
        ref = pt.get_hdr_image_data()
        planes = pt.features(cam)["planes"]
        # a converged render: the shipped defaults should leave it essentially as it is
        mask = pa.denoise_keep_mask(ref, planes[1], planes[2])
        out = pt.despike()
        converged.append({"scene": scene, "width": W, "height": H, "spp": 8 * (8 if quick else 512), "kept_pixels": int(mask.sum()),
                          "count": pt.despike_count(), "changed_share_of_kept": changed_share(out, ref, mask),
                          "luminance_retained": lum_sum(out, mask) / lum_sum(ref, mask),
                          "rel_mse_against_itself": dp.rel_mse(out, ref, mask), "ldr_mse_against_itself": dp.ldr_mse(out, ref, mask)})
        for spp in (1, 8):
            pt.render(cam, spp, True)
            planes = pt.features(cam)["planes"]
            noisy = pt.get_hdr_image_data()
            mask = pa.denoise_keep_mask(noisy, planes[1], planes[2]) & np.isfinite(ref[..., :3]).all(-1)
            plain = pt.denoise()
            base = {"rel": dp.rel_mse(noisy, ref, mask), "ldr": dp.ldr_mse(noisy, ref, mask),
                    "rel_filtered": dp.rel_mse(plain, ref, mask), "ldr_filtered": dp.ldr_mse(plain, ref, mask)}
            case = f"{scene}@{spp}spp"
            cases.append(dict(base, case=case, width=W, height=H, kept_pixels=int(mask.sum()),
                              median_luminance=float(np.median(noisy[..., :3][mask].astype(np.float64) @ LUM))))
            total = lum_sum(noisy, mask)
            for combo in itertools.product(*grid.values()):
                kw = dict(zip(grid.keys(), combo))
                out = pt.despike(same_primitive=True, **settings_of(kw))
                count = pt.despike_count()
                both = pt.denoise(source="despiked")
                rows.append(dict(kw, case=case, count=count, changed_share_of_kept=changed_share(out, noisy, mask),
                                 luminance_retained=lum_sum(out, mask) / total if total else 1.0,
                                 rel_ratio=dp.rel_mse(out, ref, mask) / base["rel"],
                                 ldr_ratio=dp.ldr_mse(out, ref, mask) / base["ldr"],
                                 rel_ratio_filtered=dp.rel_mse(both, ref, mask) / base["rel_filtered"],
                                 ldr_ratio_filtered=dp.ldr_mse(both, ref, mask) / base["ldr_filtered"]))
        pt.close()
    table = {}
    for r in rows:
        table.setdefault(tuple(r[k] for k in grid), []).append(r)
    summary = []
    for combo, rs in table.items():
        summary.append(dict(zip(grid, combo), ldr_filtered_geomean=geomean([r["ldr_ratio_filtered"] for r in rs]),
                            rel_filtered_geomean=geomean([r["rel_ratio_filtered"] for r in rs]),
                            rel_geomean=geomean([r["rel_ratio"] for r in rs]), ldr_geomean=geomean([r["ldr_ratio"] for r in rs]),
                            improves_rel_in_every_case=all(r["rel_ratio"] < 1.0 for r in rs),
                            worst_rel_ratio=max(r["rel_ratio"] for r in rs),
                            least_luminance_retained=min(r["luminance_retained"] for r in rs),
                            most_changed_share=max(r["changed_share_of_kept"] for r in rs),
                            per_case={r["case"]: {k: r[k] for k in ("count", "changed_share_of_kept", "luminance_retained", "rel_ratio",
                                                                    "ldr_ratio", "rel_ratio_filtered", "ldr_ratio_filtered")} for r in rs}))
    eligible = [s for s in summary if s["improves_rel_in_every_case"]]
    best = min(eligible, key=lambda s: s["ldr_filtered_geomean"]) if eligible else None
    d = pa.DESPIKE_DEFAULTS
    shipped = [s for s in summary if all(s[k] == d[k] for k in grid)]
    marginals = {k: {str(v): min((s["ldr_filtered_geomean"] for s in eligible if s[k] == v), default=None) for v in grid[k]} for k in grid}
    return {"cases": cases, "reference_spp": 8 * (8 if quick else 512), "settings": len(summary), "eligible_settings": len(eligible),
            "rule": "best ldr_filtered_geomean among the settings with rel_ratio < 1 in every case",
            "fixed": {"same_primitive": True, "sigma_plane": d["sigma_plane"], "normal_cos_min": d["normal_cos_min"],
                      "min_neighbors": "max(3, rank)"},
            "best": best, "shipped_defaults": shipped[0] if shipped else None, "best_eligible_geomean_by_value": marginals,
            "top10_eligible": sorted(eligible, key=lambda s: s["ldr_filtered_geomean"])[:10],
            "top5_by_rel_geomean": sorted(summary, key=lambda s: s["rel_geomean"])[:5],
            "shipped_defaults_on_converged_renders": converged}


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def timing(quick):
    W, H = (320, 180) if quick else (1920, 1080)
    out = []
    for scene in ("generated_scene", "cornell_box")[:1 if quick else 2]:
        pt = pa.Pathtracer(W, H)
        cam = pt.load_scene(str(ROOT / "scenes" / f"{scene}.scene.json"))
        pt.render(cam, 8, True)
        pt.features(cam)
        names = [f"despike_radius_{r}_{form}" for r in (1, 2, 3) for form in ("staged", "unstaged")]
        t = {name: [] for name in names + ["prepare", "atrous_s1"]}
        counts = {}

        def one_run(record):
            for r in (1, 2, 3):
                for form, staging in (("staged", 1), ("unstaged", 2)):
                    pt.despike(radius=r, staging=staging)
                    ms = pt.despike_timing()
                    counts[r] = pt.despike_count()
                    if record:
                        t[f"despike_radius_{r}_{form}"].append(ms["despike"])
                        t["prepare"].append(ms["prepare"])
            pt.denoise(iterations=1, sigma_color=1.0)
            if record:
                t["atrous_s1"].append(pt.denoise_timing()["iterations"][0])

        one_run(False)
        one_run(False)
        for _ in range(3):
            one_run(True)
        row = {"scene": scene, "width": W, "height": H, "runs": 3, "spp": 8, "count_by_radius": counts}
        for name, xs in t.items():
            row[name + "_ms"] = spread(xs)
        row["faster_form_by_radius"] = {str(r): min(("staged", "unstaged"), key=lambda f: row[f"despike_radius_{r}_{f}_ms"]["median"])
                                        for r in (1, 2, 3)}
        out.append(row)
        pt.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "despike_probe.json"))
    ap.add_argument("--quick", action="store_true", help="tiny sizes and grid: a rehearsal of the tool, not a measurement")
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--skip-timing", action="store_true")
    args = ap.parse_args()
    if pa.device_count() < 1:
        raise SystemExit("despike_probe: no GPU visible")
    out = pathlib.Path(args.out)
    record = json.loads(out.read_text()) if out.exists() and (args.skip_quality or args.skip_timing) else {}
    record.update({"tool": "tools/despike_probe.py", "quick": args.quick, "grid": {k: list(v) for k, v in GRID.items()},
                   "defaults": dict(pa.DESPIKE_DEFAULTS)})
    if not args.skip_timing:
        record["timing"] = timing(args.quick)
        print("timing done", flush=True)
    if not args.skip_quality:
        record["quality"] = quality(args.quick)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(record, indent=1) + "\n")
    print(json.dumps({k: v for k, v in record.items() if k != "quality"}, indent=1)[:6000])
    if "quality" in record:
        q = record["quality"]
        print(json.dumps({k: q[k] for k in q if k not in ("top10_eligible",)}, indent=1)[:9000])


if __name__ == "__main__":
    main()
