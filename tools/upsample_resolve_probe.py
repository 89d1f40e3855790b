#!/usr/bin/env python3
"""Probe of the guided upsampling onto supersampled planes (pt_upsample_resolve, rule 9 of include/pt_hip.h): the
kernel's time staged and unstaged beside the parent's upsample_kernel at the S-times size (what a user runs today
before averaging on the host) and beside the time of the rule's minimal traffic, the whole frame beside
tools/upsample_probe.py's two frames, and the quality at equal camera paths beside the one-sample guided result and
bilinear resampling.

Every measurement runs in a process of its own (this script again with --worker), the configurations interleaved in
rounds, and is reported as the median [min, max] over the processes.

Timing: 1920 x 1080 from 960 x 540, S = 2 and 3, cornell_box and generated_scene, after one 1-spp call at the low
size.  A worker makes the contexts, warms up twice and takes the median hipEvent time of seven calls.
  resolve  upsample_resolve_kernel and the flat pass, staging 1 and 2
  parent   upsample_kernel (pt_upsample, staged) onto the S W x S H context
  frame    wall clock of one frame, stream-synchronised: resolve = render 1 spp at the low size + features at the low
           size + features at S W x S H + denoise() at the low size + pt_upsample_resolve; low and full as
           tools/upsample_probe.py has them (one-sample upsampling; the full-resolution frame)
Minimal traffic, every byte once: the three S-times planes (48 S^2 B per output pixel), the output (16 B) and the
packed low texels (48 B per low pixel); for the parent's kernel 64 B per S-times pixel and the same low texels.  At the
6.3 TB/s a float4 copy achieves on this device.

Quality: 960 x 540 from 480 x 270 at 4 spp, the low image raw and after denoise() at its defaults, against a 1,024-spp
reference at 960 x 540.  Tonemapped MSE (Reinhard + gamma 2.2) as ratios to the raw 1-spp full-resolution frame's, over
all pixels and over the edge pixels (the 2 x 2 sub-pixel ids of the S = 2 planes are not all equal).

    python tools/upsample_resolve_probe.py [--out profiles/upsample_resolve_probe.json] [--quick] [--skip-quality] [--skip-timing]
"""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import pathtracercuda_amd as pa  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
SCENES = ("cornell_box", "generated_scene")
FULL, LOW = (1920, 1080), (960, 540)
FACTORS = (2, 3)


def scene_path(name):
    return str(ROOT / "scenes" / f"{name}.scene.json")


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": len(xs)}


def contexts(scene, *sizes):
    pts = [pa.Pathtracer(*s) for s in sizes]
    cam = None
    for p in pts:
        cam = p.load_scene(scene_path(scene))
    return pts, cam


def worker(a):
    N = pa._native
    lib, ref = N.hip(), N.C.byref
    full, low, S = (a.width, a.height), (a.low_width, a.low_height), a.factor
    big = (S * full[0], S * full[1])

    def features(p, cam):
        N.check_ctx(lib.pt_render_features(p._ctx, ref(cam)), p._ctx)

    if a.worker in ("resolve", "parent"):
        (hi, lo, ss), cam = contexts(a.scene, full, low, big)
        lo.render(cam, 1, True)
        features(lo, cam)
        features(ss, cam)
        us = pa.upsample_params(staging=a.staging)
        target = hi if a.worker == "resolve" else ss
        times = []
        for k in range(9):
            if a.worker == "resolve":
                rc = lib.pt_upsample_resolve(hi._ctx, ss._ctx, lo._ctx, N.PT_UPSAMPLE_ACCUM, 1, S, ref(us))
            else:
                rc = lib.pt_upsample(ss._ctx, lo._ctx, N.PT_UPSAMPLE_ACCUM, 1, ref(us))
            N.check_ctx(rc, target._ctx)
            if k >= 2:
                times.append(target.upsample_timing())
        out = {"upsample_us": 1e3 * statistics.median(t["upsample"] for t in times),
               "prepare_us": 1e3 * statistics.median(t["prepare"] for t in times), "counts": target.upsample_counts()}
    else:
        dn, us = pa.denoise_params(sigma_color=1.0), pa.upsample_params()
        if a.worker == "frame_resolve":
            (hi, lo, ss), cam = contexts(a.scene, full, low, big)
        elif a.worker == "frame_low":
            (hi, lo), cam = contexts(a.scene, full, low)
        else:
            (hi,), cam = contexts(a.scene, full)
            lo = hi
        times = []
        for k in range(9):
            t0 = time.perf_counter()
            lo.render(cam, 1, True)
            features(lo, cam)
            if a.worker == "frame_low":
                features(hi, cam)
            if a.worker == "frame_resolve":
                features(ss, cam)
            N.check_ctx(lib.pt_denoise(lo._ctx, 1, ref(dn)), lo._ctx)
            if a.worker == "frame_low":
                N.check_ctx(lib.pt_upsample(hi._ctx, lo._ctx, N.PT_UPSAMPLE_DENOISED, 1, ref(us)), hi._ctx)
            if a.worker == "frame_resolve":
                N.check_ctx(lib.pt_upsample_resolve(hi._ctx, ss._ctx, lo._ctx, N.PT_UPSAMPLE_DENOISED, 1, S, ref(us)), hi._ctx)
            if k >= 2:
                times.append(1e3 * (time.perf_counter() - t0))
        out = {"frame_ms": statistics.median(times)}
    print("RESULT " + json.dumps(out))


def run_worker(kind, scene, full, low, factor=2, staging=0):
    cmd = [sys.executable, __file__, "--worker", kind, "--scene", scene, "--width", str(full[0]), "--height", str(full[1]),
           "--low-width", str(low[0]), "--low-height", str(low[1]), "--factor", str(factor), "--staging", str(staging)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(f"worker {cmd} failed with {r.returncode}:\n{r.stdout}\n{r.stderr}")
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])


def timing(quick):
    full, low = ((480, 270), (240, 135)) if quick else (FULL, LOW)
    reps = 1 if quick else 3
    rows = []
    for scene in SCENES:
        for S in FACTORS:
            kinds = {"staged": ("resolve", 1), "unstaged": ("resolve", 2), "parent_at_s_times": ("parent", 1),
                     "frame_resolve": ("frame_resolve", 0), "frame_low": ("frame_low", 0), "frame_full": ("frame_full", 0)}
            got = {k: [] for k in kinds}
            for _ in range(reps):                       # interleaved: one of each per round
                for name, (kind, staging) in kinds.items():
                    got[name].append(run_worker(kind, scene, full, low, S, staging))
            nout, nlo = full[0] * full[1], low[0] * low[1]
            minimal = {"resolve": (48 * S * S + 16) * nout + 48 * nlo, "parent_at_s_times": 64 * S * S * nout + 48 * nlo}
            row = {"scene": scene, "output": list(full), "low": list(low), "factor": S, "minimal_bytes": minimal,
                   "minimal_us_at_6.3_TB_per_s": {k: 1e6 * v / HBM_BYTES_PER_S for k, v in minimal.items()},
                   "counts": got["staged"][0]["counts"]}
            for form in ("staged", "unstaged", "parent_at_s_times"):
                row[f"{form}_upsample_us"] = spread([g["upsample_us"] for g in got[form]])
                row[f"{form}_prepare_us"] = spread([g["prepare_us"] for g in got[form]])
                least = row["minimal_us_at_6.3_TB_per_s"]["parent_at_s_times" if form == "parent_at_s_times" else "resolve"]
                row[f"{form}_achieved_fraction"] = least / row[f"{form}_upsample_us"]["median"]
            for name in ("frame_resolve", "frame_low", "frame_full"):
                row[f"{name}_ms"] = spread([g["frame_ms"] for g in got[name]])
            row["frame_resolve_over_full"] = row["frame_resolve_ms"]["median"] / row["frame_full_ms"]["median"]
            row["frame_resolve_over_low"] = row["frame_resolve_ms"]["median"] / row["frame_low_ms"]["median"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def ldr(img):
    x = np.maximum(np.nan_to_num(img[..., :3].astype(np.float64), nan=0.0, posinf=1e30), 0.0)
    return (x / (1.0 + x)) ** (1.0 / 2.2)


def quality(quick):
    import upsample_model as um
    full, low = ((240, 136), (120, 68)) if quick else ((960, 540), (480, 270))
    rows = []
    for scene in SCENES:
        (hi, lo), cam = contexts(scene, full, low)
        hi.render(cam, 8, True, chunks=4 if quick else 128)
        ref = ldr(hi.get_hdr_image_data())
        hi.render(cam, 1, True)
        raw = hi.get_hdr_image_data()
        hi.features(cam)
        lo.render(cam, 4, True)
        lo.features(cam)
        low_raw = lo.get_hdr_image_data()
        low_filtered = lo.denoise()
        images = {"guided_of_denoised_low": hi.upsample(lo, source="denoised"), "bilinear_of_denoised_low": um.bilinear(low_filtered, *full),
                  "guided_of_raw_low": hi.upsample(lo, source="accum"), "bilinear_of_raw_low": um.bilinear(low_raw, *full)}
        edge = None
        counts = {}
        for S in FACTORS:
            ss = pa.Pathtracer(S * full[0], S * full[1])
            ss.load_scene(scene_path(scene))
            ids = ss.features(cam)["primitive"].reshape(full[1], S, full[0], S)
            if edge is None:
                edge = (ids != ids[:, :1, :, :1]).any(axis=(1, 3))
            images[f"resolved_s{S}_of_denoised_low"] = hi.upsample(lo, planes=ss, source="denoised")
            images[f"resolved_s{S}_of_raw_low"] = hi.upsample(lo, planes=ss, source="accum")
            counts[f"s{S}"] = hi.upsample_counts()
            ss.close()
        err = {k: (ldr(v) - ref) ** 2 for k, v in images.items()}
        base_err = (ldr(raw) - ref) ** 2
        base = float(base_err.mean())
        row = {"scene": scene, "output": list(full), "low": list(low), "low_spp": 4, "reference_spp": 8 * (4 if quick else 128),
               "raw_full_1spp_ldr_mse": base, "edge_pixels": int(edge.sum()), "edge_fraction": float(edge.mean()),
               "ratios_to_raw_full": {k: float(e.mean()) / base for k, e in err.items()},
               "edge_pixels_ldr_mse": {k: float(e[edge].mean()) for k, e in err.items()},
               "other_pixels_ldr_mse": {k: float(e[~edge].mean()) for k, e in err.items()},
               "share_of_the_error_on_edge_pixels": {k: float(e[edge].sum() / e.sum()) for k, e in err.items()},
               "counts": counts}
        rows.append(row)
        print(json.dumps(row), flush=True)
        hi.close()
        lo.close()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "upsample_resolve_probe.json"))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--worker", choices=("resolve", "parent", "frame_resolve", "frame_low", "frame_full"))
    ap.add_argument("--scene", default="cornell_box")
    ap.add_argument("--width", type=int, default=FULL[0])
    ap.add_argument("--height", type=int, default=FULL[1])
    ap.add_argument("--low-width", type=int, default=LOW[0])
    ap.add_argument("--low-height", type=int, default=LOW[1])
    ap.add_argument("--factor", type=int, default=2)
    ap.add_argument("--staging", type=int, default=0)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    record = {"device": "MI355X", "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S, "defaults": pa.UPSAMPLE_DEFAULTS}
    if not a.skip_timing:
        record["timing"] = timing(a.quick)
    if not a.skip_quality:
        record["quality"] = quality(a.quick)
    pathlib.Path(a.out).write_text(json.dumps(record, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    sys.exit(main())
