#!/usr/bin/env python3
"""Temporal reprojection probe: the sweep that chooses the defaults, and the kernel's time.

Quality (part A).  cornell_box and generated_scene at small sizes, an orbit of the camera (a step to the right
and a turn to the left per frame), every frame rendered alone at 1 spp (ignore_history = True) with its
feature planes, and a 1024-spp render at the same camera as the reference.  The frames are kept on the host
and every setting of the grid is run over them with pt_temporal_image, so all settings see the same
samples.  Per frame, the error is the mean squared difference after the tonemap's Reinhard + gamma 2.2 over
the hit, finite pixels, for the raw frame, the temporal image, and the temporal image filtered by the a-trous
denoiser at its defaults.  A setting's score is the mean over the frames from the seventeenth on of temporal / raw,
and the chosen setting minimises the geometric mean of the two scenes' scores.

Timing (part B), 1920x1080, three interleaved runs, hipEvent times of the kernels: the temporal kernel (with
a history, the camera moving), an unstaged a-trous iteration at s = 1, the feature pass and the 1-spp frame
of the same session.  The temporal kernel's compulsory traffic is 64 B read + 64 B written per pixel.

    python tools/temporal_probe.py [--out profiles/temporal_probe.json] [--quick]
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

GRID = {"alpha_min": (0.02, 0.05, 0.1, 0.2), "max_history": (8, 16, 32, 64), "sigma_plane": (0.005, 0.02, 0.1, 0.3),
        "normal_cos_min": (0.0, 0.5, 0.9, 0.99)}
QUALITY = (("cornell_box", 128, 128), ("generated_scene", 192, 108))
FRAMES, SETTLED, REF_CHUNKS = 48, 16, 128
STEP = (0.012, 0.0, 0.0, -0.0024)         # translate right / up / back, yaw per frame


def ldr(img):
    c = np.maximum(img[..., :3].astype(np.float64), 0.0)
    return (c / (c + 1.0)) ** (1.0 / 2.2)


def ldr_mse(img, ref, mask):
    return float(np.mean((ldr(img)[mask] - ldr(ref)[mask]) ** 2))


def step_camera(cam):
    cam = pa.PtCamera.from_buffer_copy(cam)
    pa.camera_translate(cam, *STEP[:3])
    pa.camera_rotate(cam, 0.0, STEP[3])
    return cam


def ok_mask(color, planes):
    fl = np.ascontiguousarray(planes[2][..., 3]).view(np.uint32)
    fin = np.isfinite(color[..., :3]).all(-1) & np.isfinite(planes[1][..., :3]).all(-1) & np.isfinite(planes[2][..., :3]).all(-1)
    return ((fl & 1) != 0) & fin


def orbit(scene, W, H, frames, ref_chunks):
    """[(camera, 1-spp image, planes, reference, mask)] along the orbit."""
    pt = pa.Pathtracer(W, H)
    cam = pt.load_scene(str(ROOT / "scenes" / f"{scene}.scene.json"))
    out = []
    for _ in range(frames):
        pt.render(cam, 8, True, chunks=ref_chunks)
        ref = pt.get_hdr_image_data()
        pt.render(cam, 1, True)
        noisy = pt.get_hdr_image_data()
        planes = pt.features(cam)["planes"]
        out.append((cam, noisy, planes, ref, ok_mask(noisy, planes) & np.isfinite(ref[..., :3]).all(-1)))
        cam = step_camera(cam)
    pt.close()
    return out


def run(seq, with_filter=False, **kw):
    """Per frame: (raw, temporal[, temporal + a-trous, raw + a-trous]) errors and the mean history length."""
    rows, hist, prev = [], None, None
    for cam, noisy, planes, ref, mask in seq:
        image, *hist = pa.temporal_image(noisy, *planes, cam, hist, prev, **kw)
        prev = cam
        row = {"raw": ldr_mse(noisy, ref, mask), "temporal": ldr_mse(image, ref, mask),
               "mean_history": float(image[..., 3][mask].mean())}
        if with_filter:
            row["temporal_atrous"] = ldr_mse(pa.denoise_image(image, *planes), ref, mask)
            row["raw_atrous"] = ldr_mse(pa.denoise_image(noisy, *planes), ref, mask)
        rows.append(row)
    return rows


def score(rows, settled):
    return float(np.mean([r["temporal"] / r["raw"] for r in rows[settled:]]))


def quality(quick):
    frames, settled = (6, 2) if quick else (FRAMES, SETTLED)
    grid = {k: v[:2] for k, v in GRID.items()} if quick else GRID
    seqs = {}
    for scene, W, H in QUALITY:
        if quick:
            W, H = W // 2, H // 2
        seqs[scene] = orbit(scene, W, H, frames, 8 if quick else REF_CHUNKS)
    table = []
    for combo in itertools.product(*grid.values()):
        kw = dict(zip(grid.keys(), combo))
        scores = {scene: score(run(seq, **kw), settled) for scene, seq in seqs.items()}
        print(".", end="", flush=True)
        table.append(dict(kw, scores=scores, geomean=float(np.exp(np.mean([np.log(s) for s in scores.values()])))))
    best = min(table, key=lambda r: r["geomean"])
    d = pa.TEMPORAL_DEFAULTS
    shipped = [r for r in table if all(r[k] == d[k] for k in GRID)]
    marginals = {k: {str(v): min(r["geomean"] for r in table if r[k] == v) for v in grid[k]} for k in grid}
    series = {scene: run(seq, with_filter=True) for scene, seq in seqs.items()}         # at the shipped defaults
    cases = [{"scene": scene, "width": seq[0][1].shape[1], "height": seq[0][1].shape[0], "frames": frames,
              "reference_spp": 8 * (8 if quick else REF_CHUNKS), "hit_finite_pixels": [int(f[4].sum()) for f in seq]}
             for scene, seq in seqs.items()]
    return {"cases": cases, "orbit_step": {"translate": STEP[:3], "yaw": STEP[3]}, "settled_from_frame": settled,
            "settings": len(table), "best": best, "shipped_defaults": shipped[0] if shipped else None,
            "best_geomean_by_value": marginals, "top10": sorted(table, key=lambda r: r["geomean"])[:10],
            "per_frame_at_shipped_defaults": series}


def timing(quick):
    W, H = (320, 180) if quick else (1920, 1080)
    out = []
    for scene in ("generated_scene", "cornell_box")[:1 if quick else 2]:
        pt = pa.Pathtracer(W, H)
        cam = pt.load_scene(str(ROOT / "scenes" / f"{scene}.scene.json"))
        pt.render(cam, 1, True)
        pt.features(cam)
        pt.temporal(frames=1)
        pt.denoise(iterations=1, staging=2)                       # everything warm
        frame, feat, temporal, atrous, lengths = [], [], [], [], []
        for _ in range(3):
            for _k in range(3):
                cam = step_camera(cam)
                frame.append(pt.render_raw(cam, 1, 1, True))
                pt.features(cam)
                pt.temporal(frames=1)
                temporal.append(pt.temporal_timing())
                pt.denoise(iterations=1, staging=2)
                t = pt.denoise_timing()
                feat.append(t["features"])
                atrous.append(t["iterations"][0])
            lengths.append(float(pt.history_lengths().mean()))
        med = statistics.median
        npix = W * H
        tm = med(temporal)
        out.append({"scene": scene, "width": W, "height": H, "runs": 3, "launches_per_run": 3,
                    "progressive_1spp_frame_ms": {"median": med(frame), "all": frame},
                    "feature_pass_ms": {"median": med(feat), "all": feat},
                    "atrous_iteration_s1_unstaged_ms": {"median": med(atrous), "all": atrous},
                    "temporal_kernel_ms": {"median": tm, "all": temporal},
                    "mean_history_length_after_each_run": lengths,
                    "compulsory_bytes_per_pixel": 128, "tap_bytes_per_pixel_at_most": 192,
                    "compulsory_GB_per_s_at_median": 128 * npix / (tm * 1e-3) / 1e9 if tm > 0 else None})
        pt.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "temporal_probe.json"))
    ap.add_argument("--quick", action="store_true", help="tiny sizes and grid: a rehearsal of the tool, not a measurement")
    ap.add_argument("--skip-quality", action="store_true")
    args = ap.parse_args()
    if pa.device_count() < 1:
        raise SystemExit("temporal_probe: no GPU visible")
    record = {"tool": "tools/temporal_probe.py", "quick": args.quick, "grid": {k: list(v) for k, v in GRID.items()},
              "defaults": pa.TEMPORAL_DEFAULTS}
    if not args.skip_quality:
        record["quality"] = quality(args.quick)
        print("quality done", flush=True)
    record["timing"] = timing(args.quick)
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(record, indent=1) + "\n")
    print(json.dumps(record, indent=1)[:5000])


if __name__ == "__main__":
    main()
