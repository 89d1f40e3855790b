#!/usr/bin/env python3
"""Probe of the per-pixel variance and the variance-guided filter: kernel times, and the sweep behind the defaults.

Timing (part A), 1920x1080, generated_scene and cornell_box, a moving camera, three interleaved runs of three
frames, hipEvent times, medians: the moments step and the variance estimate (pt_temporal_moments), every
iteration of the variance-guided filter staged (s <= 4) and unstaged, and beside them in the same session
pt_temporal's kernel and the plain a-trous iterations in both forms.  Two contexts render the same frames: a
plain temporal step would take the moments from under the other.

Quality (part B), the protocol of tools/temporal_probe.py: its orbits of cornell_box 128^2 and generated_scene
192x108, 48 frames rendered alone at 1 spp, a 1024-spp reference per frame, the error = the mean squared
difference after Reinhard + gamma 2.2 over the hit, finite pixels.  The temporal step runs at its shipped
defaults; the grid below is run over the kept frames.  A setting's score is the mean over the frames from the
seventeenth on of (temporal, then variance-guided) / raw; the chosen setting minimises the geometric mean of the
two scenes' scores.  The per-frame table at the shipped defaults has the rows raw, temporal, temporal then
a-trous, temporal then variance-guided.

    python tools/svgf_probe.py [--out profiles/svgf_probe.json] [--quick] [--skip-quality] [--skip-timing]
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
import temporal_probe as tp  # noqa: E402

GRID = {"sigma_l": (0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0), "variance_floor": (1e-8, 1e-6, 1e-4), "iterations": (3, 4, 5, 6)}
MIN_TEMPORAL = (2, 4, 8)


def moments_frames(seq, min_temporal):
    """Per frame of an orbit: (temporal image, variance), the temporal step at its shipped defaults."""
    out, hist, prev = [], None, None
    for cam, noisy, planes, ref, mask in seq:
        image, *hist, var = pa.temporal_moments_image(noisy, *planes, cam, hist, prev, min_temporal=min_temporal)
        prev = cam
        out.append((image, var))
    return out


def quality(quick):
    frames, settled = (6, 2) if quick else (tp.FRAMES, tp.SETTLED)
    grid = {k: v[1:3] for k, v in GRID.items()} if quick else GRID
    mts = MIN_TEMPORAL[:2] if quick else MIN_TEMPORAL
    seqs = {}
    for scene, W, H in tp.QUALITY:
        if quick:
            W, H = W // 2, H // 2
        seqs[scene] = tp.orbit(scene, W, H, frames, 8 if quick else tp.REF_CHUNKS)
    raw = {scene: [tp.ldr_mse(f[1], f[3], f[4]) for f in seq] for scene, seq in seqs.items()}
    table = []
    for mt in mts:
        temporal = {scene: moments_frames(seq, mt) for scene, seq in seqs.items()}
        for combo in itertools.product(*grid.values()):
            kw = dict(zip(grid.keys(), combo))
            scores = {}
            for scene, seq in seqs.items():
                ratios = []
                for k in range(settled, frames):
                    image, var = temporal[scene][k]
                    out = pa.denoise_variance_image(image, *seq[k][2], var, **kw)
                    ratios.append(tp.ldr_mse(out, seq[k][3], seq[k][4]) / raw[scene][k])
                scores[scene] = float(np.mean(ratios))
            table.append(dict(kw, min_temporal=mt, scores=scores,
                              geomean=float(np.exp(np.mean([np.log(s) for s in scores.values()])))))
        print(f"min_temporal {mt} done", flush=True)
    best = min(table, key=lambda r: r["geomean"])
    d, dv = pa.VDENOISE_DEFAULTS, pa.VARIANCE_DEFAULTS
    shipped = [r for r in table if all(r[k] == d[k] for k in GRID) and r["min_temporal"] == dv["min_temporal"]]
    keys = dict(grid, min_temporal=mts)
    marginals = {k: {str(v): min(r["geomean"] for r in table if r[k] == v) for v in keys[k]} for k in keys}
    series, means = {}, {}
    for scene, seq in seqs.items():
        rows = tp.run(seq, with_filter=True)                      # raw, temporal, temporal + a-trous at their defaults
        for k, (image, var) in enumerate(moments_frames(seq, dv["min_temporal"])):
            guided = pa.denoise_variance_image(image, *seq[k][2], var)
            rows[k]["temporal_variance_guided"] = tp.ldr_mse(guided, seq[k][3], seq[k][4])
            rows[k]["kept_variance_mean"] = float(var[var >= 0].mean()) if (var >= 0).any() else None
        series[scene] = rows
        means[scene] = {name: float(np.mean([r[name] for r in rows[settled:]]))
                        for name in ("raw", "temporal", "temporal_atrous", "temporal_variance_guided")}
    cases = [{"scene": scene, "width": seq[0][1].shape[1], "height": seq[0][1].shape[0], "frames": frames,
              "reference_spp": 8 * (8 if quick else tp.REF_CHUNKS)} for scene, seq in seqs.items()]
    return {"cases": cases, "settled_from_frame": settled, "temporal_step": pa.TEMPORAL_DEFAULTS, "settings": len(table),
            "best": best, "shipped_defaults": shipped[0] if shipped else None, "best_geomean_by_value": marginals,
            "top10": sorted(table, key=lambda r: r["geomean"])[:10], "mean_mse_frames_settled_on_at_shipped_defaults": means,
            "per_frame_at_shipped_defaults": series}


def timing(quick):
    W, H = (320, 180) if quick else (1920, 1080)
    its = 5
    out = []
    for scene in ("generated_scene", "cornell_box")[:1 if quick else 2]:
        plain, mom = pa.Pathtracer(W, H), pa.Pathtracer(W, H)
        cam = plain.load_scene(str(ROOT / "scenes" / f"{scene}.scene.json"))
        mom.load_scene(str(ROOT / "scenes" / f"{scene}.scene.json"))
        t = {"temporal_kernel": [], "moments_step": [], "variance_estimate": [],
             "atrous_staged": [[] for _ in range(its)], "atrous_unstaged": [[] for _ in range(its)],
             "guided_staged": [[] for _ in range(its)], "guided_unstaged": [[] for _ in range(its)]}
        young = []

        def frame(record):
            for p in (plain, mom):
                p.render(cam, 1, True)
                p.features(cam)
            plain.temporal(frames=1)
            mom.temporal(frames=1, variance=True)
            ms = mom.temporal_moments_timing()
            if record:
                t["temporal_kernel"].append(plain.temporal_timing())
                t["moments_step"].append(ms["step"])
                t["variance_estimate"].append(ms["estimate"])
                n = mom.history_lengths()
                young.append(float(((n >= 1) & (n < pa.VARIANCE_DEFAULTS["min_temporal"])).mean()))
            for name, staging in (("staged", 1), ("unstaged", 2)):
                plain.denoise(source="temporal", iterations=its, sigma_color=0.5, staging=staging)
                a = plain.denoise_timing()["iterations"]
                mom.denoise(source="temporal", guide="variance", iterations=its, staging=staging)
                g = mom.denoise_timing()["iterations"]
                if record:
                    for i in range(its):
                        t["atrous_" + name][i].append(a[i])
                        t["guided_" + name][i].append(g[i])

        for _ in range(2):                                        # everything warm, and a history to reproject
            frame(False)
            cam = tp.step_camera(cam)
        for _ in range(3):
            for _k in range(3):
                frame(True)
                cam = tp.step_camera(cam)
        med = statistics.median
        row = {"scene": scene, "width": W, "height": H, "runs": 3, "launches_per_run": 3,
               "young_pixel_share_per_frame": young}
        for name in ("temporal_kernel", "moments_step", "variance_estimate"):
            row[name + "_ms"] = {"median": med(t[name]), "all": t[name]}
        for name in ("atrous_staged", "atrous_unstaged", "guided_staged", "guided_unstaged"):
            row[name + "_ms_by_step"] = {str(1 << i): {"median": med(t[name][i]), "all": t[name][i]} for i in range(its)}
        row["note"] = "staged = staging 1: the steps 1, 2, 4 run the LDS form, 8 and 16 are unstaged in both columns"
        out.append(row)
        plain.close()
        mom.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "svgf_probe.json"))
    ap.add_argument("--quick", action="store_true", help="tiny sizes and grid: a rehearsal of the tool, not a measurement")
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--skip-timing", action="store_true")
    args = ap.parse_args()
    if pa.device_count() < 1:
        raise SystemExit("svgf_probe: no GPU visible")
    out = pathlib.Path(args.out)
    record = json.loads(out.read_text()) if out.exists() and (args.skip_quality or args.skip_timing) else {}
    record.update({"tool": "tools/svgf_probe.py", "quick": args.quick, "grid": dict({k: list(v) for k, v in GRID.items()},
                                                                                     min_temporal=list(MIN_TEMPORAL)),
                   "defaults": dict(pa.VDENOISE_DEFAULTS, **pa.VARIANCE_DEFAULTS)})
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
        print(json.dumps({k: q[k] for k in ("best", "shipped_defaults", "best_geomean_by_value",
                                            "mean_mse_frames_settled_on_at_shipped_defaults")}, indent=1))


if __name__ == "__main__":
    main()
