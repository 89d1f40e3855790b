#!/usr/bin/env python3
"""Probe of the feedback of the filtered colour into the temporal history: the kernel's time, and the sweep
behind PT_VFEEDBACK_DEFAULT_LEVEL.  The protocol is tools/svgf_probe.py's.

Timing (part A), 1920x1080, generated_scene and cornell_box, a moving camera, three interleaved runs of three
frames after two warm ones, hipEvent times, medians: the feedback kernel, and beside it in the same session the
moments step, the variance estimate and the guided iterations of the same call.  The feedback kernel's
compulsory traffic is 32 B read + 16 B written per pixel; the bandwidth it reaches is reported against that.

Quality (part B): the 48-frame orbits of tools/temporal_probe.py (cornell_box 128^2, generated_scene 192x108, each
frame alone at 1 spp, a 1024-spp reference per frame, the error = the mean squared difference after Reinhard +
gamma 2.2 over the hit, finite pixels).  With feedback a frame's history depends on the filter of the frame before,
so every setting runs its own chain through pt_temporal_moments_image and pt_denoise_variance_feedback_image
(level 0: pt_denoise_variance_image, no feedback).  Grid: level 0 / 1 / 2 / 3, sigma_l 0.25 .. 16 in factors of
2, alpha_min 0.02 / 0.05 / 0.1 / 0.2; 5 iterations, variance_floor 1e-4, everything else at the shipped defaults.
A setting's score is the mean over the frames from the seventeenth on of filtered / raw; the geometric mean of the
two scenes' scores ranks the settings.  Flicker: the mean over frames 18-48 of the mean squared difference
between the tonemapped error images (output minus reference at the same camera) of consecutive frames, over the
pixels in both masks.  Recorded, not asserted.

    python tools/feedback_probe.py [--out profiles/feedback_probe.json] [--quick] [--skip-quality] [--skip-timing]
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

GRID = {"level": (0, 1, 2, 3), "sigma_l": (0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0), "alpha_min": (0.02, 0.05, 0.1, 0.2)}
ITERATIONS, VARIANCE_FLOOR = 5, 1e-4
TRAFFIC_BYTES = 48                          # per pixel: the texel and h0 read, h0 written


def chain(seq, level, sigma_l, alpha_min):
    """One setting's own chain over an orbit.  Per frame: (temporal image, filtered image)."""
    out, hist, prev = [], None, None
    for cam, noisy, planes, ref, mask in seq:
        image, h0, h1, h2, h3, var = pa.temporal_moments_image(noisy, *planes, cam, hist, prev, alpha_min=alpha_min)
        kw = dict(iterations=ITERATIONS, sigma_l=sigma_l, variance_floor=VARIANCE_FLOOR)
        if level:
            filtered, h0 = pa.denoise_variance_feedback_image(image, *planes, var, h0, level=level, **kw)
        else:
            filtered = pa.denoise_variance_image(image, *planes, var, **kw)
        hist, prev = (h0, h1, h2, h3), cam
        out.append((image, filtered))
    return out


def flicker(seq, images, first):
    """Mean over the frames from index `first` on of the MSE between consecutive tonemapped error images."""
    vals = []
    for k in range(first, len(seq)):
        both = seq[k][4] & seq[k - 1][4]
        e1 = tp.ldr(images[k])[both] - tp.ldr(seq[k][3])[both]
        e0 = tp.ldr(images[k - 1])[both] - tp.ldr(seq[k - 1][3])[both]
        vals.append(float(np.mean((e1 - e0) ** 2)))
    return float(np.mean(vals))


def quality(quick):
    frames, settled = (6, 2) if quick else (tp.FRAMES, tp.SETTLED)
    grid = {k: v[:2] for k, v in GRID.items()} if quick else GRID
    seqs = {}
    for scene, W, H in tp.QUALITY:
        if quick:
            W, H = W // 2, H // 2
        seqs[scene] = tp.orbit(scene, W, H, frames, 8 if quick else tp.REF_CHUNKS)
    raw = {scene: [tp.ldr_mse(f[1], f[3], f[4]) for f in seq] for scene, seq in seqs.items()}
    table = []
    for combo in itertools.product(*grid.values()):
        kw = dict(zip(grid.keys(), combo))
        scores, flick = {}, {}
        for scene, seq in seqs.items():
            imgs = chain(seq, **kw)
            errs = [tp.ldr_mse(f, seq[k][3], seq[k][4]) for k, (_, f) in enumerate(imgs)]
            scores[scene] = float(np.mean([errs[k] / raw[scene][k] for k in range(settled, frames)]))
            flick[scene] = flicker(seq, [f for _, f in imgs], settled + 1)
        table.append(dict(kw, scores=scores, flicker=flick,
                          geomean=float(np.exp(np.mean([np.log(s) for s in scores.values()])))))
        print(".", end="", flush=True)
    print(flush=True)
    fed = [r for r in table if r["level"] >= 1]
    unfed = [r for r in table if r["level"] == 0]
    best_fed, best_unfed = min(fed, key=lambda r: r["geomean"]), min(unfed, key=lambda r: r["geomean"])
    d, dt = pa.VDENOISE_DEFAULTS, pa.TEMPORAL_DEFAULTS

    def at_shipped(level):
        rows = [r for r in table if r["level"] == level and r["sigma_l"] == d["sigma_l"] and r["alpha_min"] == dt["alpha_min"]]
        return rows[0] if rows else None

    marginals = {k: {str(v): min(r["geomean"] for r in table if r[k] == v) for v in grid[k]} for k in grid}
    by_level_sigma = {str(L): {str(s): min(r["geomean"] for r in table if r["level"] == L and r["sigma_l"] == s)
                               for s in grid["sigma_l"]} for L in grid["level"]}
    series = {}
    for scene, seq in seqs.items():
        rows = tp.run(seq, with_filter=True)                      # raw, temporal, temporal + a-trous at their defaults
        plain = chain(seq, 0, d["sigma_l"], dt["alpha_min"])
        chosen = chain(seq, best_fed["level"], best_fed["sigma_l"], best_fed["alpha_min"])
        for k in range(frames):
            rows[k]["temporal_variance_guided"] = tp.ldr_mse(plain[k][1], seq[k][3], seq[k][4])
            rows[k]["fed_temporal"] = tp.ldr_mse(chosen[k][0], seq[k][3], seq[k][4])
            rows[k]["temporal_variance_guided_fed_back"] = tp.ldr_mse(chosen[k][1], seq[k][3], seq[k][4])
        series[scene] = {"rows": rows,
                         "flicker": {"temporal_variance_guided": flicker(seq, [f for _, f in plain], settled + 1),
                                     "temporal_variance_guided_fed_back": flicker(seq, [f for _, f in chosen], settled + 1)}}
    cases = [{"scene": scene, "width": seq[0][1].shape[1], "height": seq[0][1].shape[0], "frames": frames,
              "reference_spp": 8 * (8 if quick else tp.REF_CHUNKS)} for scene, seq in seqs.items()]
    return {"cases": cases, "settled_from_frame": settled, "iterations": ITERATIONS, "variance_floor": VARIANCE_FLOOR,
            "settings": len(table), "best_fed": best_fed, "best_unfed": best_unfed, "shipped_unfed": at_shipped(0),
            "fed_at_shipped_parameters_by_level": {str(L): at_shipped(L) for L in grid["level"] if L},
            "best_geomean_by_value": marginals, "best_geomean_by_level_and_sigma_l": by_level_sigma,
            "top10": sorted(table, key=lambda r: r["geomean"])[:10], "table": table,
            "per_frame_unfed_at_shipped_defaults_and_fed_at_best_fed": series}


def timing(quick):
    W, H = (320, 180) if quick else (1920, 1080)
    its = ITERATIONS
    level = pa.VFEEDBACK_DEFAULTS["level"]
    out = []
    for scene in ("generated_scene", "cornell_box")[:1 if quick else 2]:
        pt = pa.Pathtracer(W, H)
        cam = pt.load_scene(str(ROOT / "scenes" / f"{scene}.scene.json"))
        t = {"moments_step": [], "variance_estimate": [], "feedback": [], "guided": [[] for _ in range(its)]}

        def frame(record):
            pt.render(cam, 1, True)
            pt.features(cam)
            pt.temporal(frames=1, variance=True)
            pt.denoise(source="temporal", guide="variance", iterations=its, feedback=level)
            if record:
                ms = pt.temporal_moments_timing()
                t["moments_step"].append(ms["step"])
                t["variance_estimate"].append(ms["estimate"])
                t["feedback"].append(pt.feedback_timing())
                g = pt.denoise_timing()["iterations"]
                for i in range(its):
                    t["guided"][i].append(g[i])

        for _ in range(2):                                        # everything warm, and a history to reproject
            frame(False)
            cam = tp.step_camera(cam)
        for _ in range(3):
            for _k in range(3):
                frame(True)
                cam = tp.step_camera(cam)

        def summary(v):
            return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}

        row = {"scene": scene, "width": W, "height": H, "runs": 3, "launches_per_run": 3, "level": level}
        for name in ("moments_step", "variance_estimate", "feedback"):
            row[name + "_ms"] = summary(t[name])
        row["guided_ms_by_step"] = {str(1 << i): summary(t["guided"][i]) for i in range(its)}
        fb = row["feedback_ms"]
        row["feedback_compulsory_bytes"] = TRAFFIC_BYTES * W * H
        row["feedback_GBps"] = {k: TRAFFIC_BYTES * W * H / (fb[k] * 1e-3) / 1e9 for k in ("median", "max", "min")}
        row["note"] = "staging 0: the steps 1 and 2 run the LDS form; GB/s at the median, the slowest and the fastest launch"
        out.append(row)
        pt.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "feedback_probe.json"))
    ap.add_argument("--quick", action="store_true", help="tiny sizes and grid: a rehearsal of the tool, not a measurement")
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--skip-timing", action="store_true")
    args = ap.parse_args()
    if pa.device_count() < 1:
        raise SystemExit("feedback_probe: no GPU visible")
    out = pathlib.Path(args.out)
    record = json.loads(out.read_text()) if out.exists() and (args.skip_quality or args.skip_timing) else {}
    record.update({"tool": "tools/feedback_probe.py", "quick": args.quick, "grid": {k: list(v) for k, v in GRID.items()},
                   "defaults": dict(pa.VDENOISE_DEFAULTS, **pa.VARIANCE_DEFAULTS, **pa.VFEEDBACK_DEFAULTS)})
    out.parent.mkdir(parents=True, exist_ok=True)
    if not args.skip_timing:
        record["timing"] = timing(args.quick)
        print("timing done", flush=True)
        out.write_text(json.dumps(record, indent=1) + "\n")
    if not args.skip_quality:
        record["quality"] = quality(args.quick)
    out.write_text(json.dumps(record, indent=1) + "\n")
    print(json.dumps({k: v for k, v in record.items() if k != "quality"}, indent=1)[:6000])
    if "quality" in record:
        q = record["quality"]
        print(json.dumps({k: q[k] for k in ("best_fed", "best_unfed", "shipped_unfed", "fed_at_shipped_parameters_by_level",
                                            "best_geomean_by_value", "best_geomean_by_level_and_sigma_l")}, indent=1))


if __name__ == "__main__":
    main()
