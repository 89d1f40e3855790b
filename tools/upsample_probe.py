#!/usr/bin/env python3
"""Probe of the guided upsampling (pt_upsample, rule 8 of include/pt_hip.h): the kernels' times staged and unstaged
beside the time of the rule's minimal traffic, the whole frame against the full-resolution frame, and the quality at
equal rays beside bilinear and nearest resampling.

Every measurement runs in a process of its own (this script again with --worker), the configurations interleaved,
and is reported as the median [min, max] over the processes.

Timing: 1920 x 1080 from 960 x 540 and from 640 x 360, cornell_box and generated_scene, after one 1-spp call at the
low size.  A worker makes the contexts, warms up twice and takes the median hipEvent time of seven calls.
  kernel   upsample_kernel and the flat pass, staging 1 and 2
  frame    wall clock of one frame, stream-synchronised: this tree = render 1 spp at the low size + features at both
           sizes + denoise() at the low size + upsample; full = render 1 spp + features + denoise() at 1920 x 1080
           (what the parent commit offers)
The minimal traffic of upsample_kernel is every byte once: 3 high planes and the output (64 B per high pixel) and the
packed low texels (48 B per low pixel), at the 6.3 TB/s a float4 copy achieves on this device.

Quality: cornell_box and generated_scene at 960 x 540 from 480 x 270, at equal rays: the low image at 4 spp, the full
image at 1 spp, each with denoise() at its defaults, against a 1,024-spp reference at 960 x 540.  Tonemapped MSE
(Reinhard + gamma 2.2) over all pixels, as ratios to the raw 1-spp full-resolution frame's; beside them bilinear and
nearest resampling of the same filtered low image; and a small sweep of sigma_plane, the normal power and the flags.

    python tools/upsample_probe.py [--out profiles/upsample_probe.json] [--quick] [--skip-quality] [--skip-timing]
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
FULL = (1920, 1080)
LOWS = ((960, 540), (640, 360))


def scene_path(name):
    return str(ROOT / "scenes" / f"{name}.scene.json")


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": len(xs)}


def make_pair(scene, full, low):
    hi, lo = pa.Pathtracer(*full), pa.Pathtracer(*low)
    cam = hi.load_scene(scene_path(scene))
    lo.load_scene(scene_path(scene))
    return hi, lo, cam


def worker(a):
    full, low = (a.width, a.height), (a.low_width, a.low_height)
    if a.worker == "kernel":
        hi, lo, cam = make_pair(a.scene, full, low)
        lo.render(cam, 1, True)
        N = pa._native
        for p in (hi, lo):
            N.check_ctx(N.hip().pt_render_features(p._ctx, N.C.byref(cam)), p._ctx)
        us = pa.upsample_params(staging=a.staging)
        times = []
        for k in range(9):
            N.check_ctx(N.hip().pt_upsample(hi._ctx, lo._ctx, N.PT_UPSAMPLE_ACCUM, 1, N.C.byref(us)), hi._ctx)
            if k >= 2:
                times.append(hi.upsample_timing())
        out = {"upsample_us": 1e3 * statistics.median(t["upsample"] for t in times),
               "prepare_us": 1e3 * statistics.median(t["prepare"] for t in times), "counts": hi.upsample_counts()}
    else:
        # one frame by the C ABI's calls alone (every one of them synchronises its stream): no read-back in the time
        N = pa._native
        lib, ref = N.hip(), N.C.byref
        dn, us = pa.denoise_params(sigma_color=1.0), pa.upsample_params()
        if a.worker == "frame_low":
            hi, lo, cam = make_pair(a.scene, full, low)
        else:
            hi = lo = pa.Pathtracer(*full)
            cam = hi.load_scene(scene_path(a.scene))
        times = []
        for k in range(9):
            t0 = time.perf_counter()
            lo.render(cam, 1, True)
            N.check_ctx(lib.pt_render_features(lo._ctx, ref(cam)), lo._ctx)
            if a.worker == "frame_low":
                N.check_ctx(lib.pt_render_features(hi._ctx, ref(cam)), hi._ctx)
            N.check_ctx(lib.pt_denoise(lo._ctx, 1, ref(dn)), lo._ctx)
            if a.worker == "frame_low":
                N.check_ctx(lib.pt_upsample(hi._ctx, lo._ctx, N.PT_UPSAMPLE_DENOISED, 1, ref(us)), hi._ctx)
            if k >= 2:
                times.append(1e3 * (time.perf_counter() - t0))
        out = {"frame_ms": statistics.median(times)}
    print("RESULT " + json.dumps(out))


def run_worker(kind, scene, full, low, staging=0):
    cmd = [sys.executable, __file__, "--worker", kind, "--scene", scene, "--width", str(full[0]), "--height", str(full[1]),
           "--low-width", str(low[0]), "--low-height", str(low[1]), "--staging", str(staging)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(f"worker {cmd} failed with {r.returncode}:\n{r.stdout}\n{r.stderr}")
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])


def timing(quick):
    full = (480, 270) if quick else FULL
    lows = ((240, 135),) if quick else LOWS
    reps = 1 if quick else 3
    rows = []
    for scene in SCENES:
        for low in lows:
            got = {"staged": [], "unstaged": [], "frame_low": [], "frame_full": []}
            for _ in range(reps):                       # interleaved: one of each per round
                got["staged"].append(run_worker("kernel", scene, full, low, 1))
                got["unstaged"].append(run_worker("kernel", scene, full, low, 2))
                got["frame_low"].append(run_worker("frame_low", scene, full, low))
                got["frame_full"].append(run_worker("frame_full", scene, full, low))
            nhi, nlo = full[0] * full[1], low[0] * low[1]
            minimal_bytes = 64 * nhi + 48 * nlo
            minimal_us = 1e6 * minimal_bytes / HBM_BYTES_PER_S
            row = {"scene": scene, "high": list(full), "low": list(low), "minimal_bytes": minimal_bytes,
                   "minimal_us_at_6.3_TB_per_s": minimal_us, "counts": got["staged"][0]["counts"]}
            for form in ("staged", "unstaged"):
                row[f"{form}_upsample_us"] = spread([g["upsample_us"] for g in got[form]])
                row[f"{form}_achieved_fraction"] = minimal_us / row[f"{form}_upsample_us"]["median"]
            row["prepare_us"] = spread([g["prepare_us"] for g in got["staged"] + got["unstaged"]])
            row["frame_low_ms"] = spread([g["frame_ms"] for g in got["frame_low"]])
            row["frame_full_ms"] = spread([g["frame_ms"] for g in got["frame_full"]])
            row["frame_ratio"] = row["frame_low_ms"]["median"] / row["frame_full_ms"]["median"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def ldr(img):
    x = np.maximum(np.nan_to_num(img[..., :3].astype(np.float64), nan=0.0, posinf=1e30), 0.0)
    return (x / (1.0 + x)) ** (1.0 / 2.2)


def ldr_mse(img, ref):
    return float(((ldr(img) - ldr(ref)) ** 2).mean())


def quality(quick):
    import upsample_model as um
    full, low = ((240, 136), (120, 68)) if quick else ((960, 540), (480, 270))
    rows = []
    for scene in SCENES:
        hi, lo, cam = make_pair(scene, full, low)
        hi.render(cam, 8, True, chunks=4 if quick else 128)
        ref = hi.get_hdr_image_data()
        hi.render(cam, 1, True)
        raw = hi.get_hdr_image_data()
        hi.features(cam)
        full_filtered = hi.denoise()
        lo.render(cam, 4, True)
        lo.features(cam)
        low_raw = lo.get_hdr_image_data()
        low_filtered = lo.denoise()
        base = ldr_mse(raw, ref)
        row = {"scene": scene, "high": list(full), "low": list(low), "reference_spp": 8 * (4 if quick else 128),
               "raw_full_1spp_ldr_mse": base, "ratios_to_raw_full": {
                   "full_1spp_denoised": ldr_mse(full_filtered, ref) / base,
                   "guided_of_denoised_low_4spp": ldr_mse(hi.upsample(lo, source="denoised"), ref) / base,
                   "bilinear_of_denoised_low_4spp": ldr_mse(um.bilinear(low_filtered, *full), ref) / base,
                   "nearest_of_denoised_low_4spp": ldr_mse(um.nearest(low_filtered, *full), ref) / base,
                   "guided_of_raw_low_4spp": ldr_mse(hi.upsample(lo, source="accum"), ref) / base,
                   "bilinear_of_raw_low_4spp": ldr_mse(um.bilinear(low_raw, *full), ref) / base},
               "counts_at_defaults": hi.upsample_counts(), "sweep": []}
        for sigma_plane in (0.005, 0.05, 0.3):
            for power in (0, 3, 7):
                for demodulate, same_primitive in ((True, True), (True, False), (False, True)):
                    out = hi.upsample(lo, source="denoised", sigma_plane=sigma_plane, normal_power_log2=power,
                                      demodulate=demodulate, same_primitive=same_primitive)
                    row["sweep"].append({"sigma_plane": sigma_plane, "normal_power_log2": power, "demodulate": demodulate,
                                         "same_primitive": same_primitive, "ratio_to_raw_full": ldr_mse(out, ref) / base,
                                         "counts": hi.upsample_counts()})
        row["best_of_sweep"] = min(row["sweep"], key=lambda r: r["ratio_to_raw_full"])
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "sweep"}), flush=True)
        hi.close()
        lo.close()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "upsample_probe.json"))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--worker", choices=("kernel", "frame_low", "frame_full"))
    ap.add_argument("--scene", default="cornell_box")
    ap.add_argument("--width", type=int, default=FULL[0])
    ap.add_argument("--height", type=int, default=FULL[1])
    ap.add_argument("--low-width", type=int, default=LOWS[0][0])
    ap.add_argument("--low-height", type=int, default=LOWS[0][1])
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
