#!/usr/bin/env python3
"""Moving objects in the temporal passes (rule 7 of include/pt_hip.h): what the two motion kernels cost against the
two kernels they stand beside, and what keeping the history of a moving object is worth.

Timing (part A), tools/temporal_probe.py's protocol: 1920x1080, hipEvent times of the kernels, three interleaved
runs of three launches, medians.  On generated_scene and cornell_box:
  existing     temporal_kernel and temporal_moments_kernel, the camera stepping, of the tree given by --parent (the
               parent commit's build, tools/snap_rev.sh) and of this tree
  moved_all    temporal_motion_kernel and temporal_moments_motion_kernel after load_scene_moved of a file in which
               every object is shifted (two files, loaded in turn), the camera stepping
  moved_none   the same kernels after load_scene_moved of the unchanged file (an identity table)
Every measurement runs in a fresh child process (this script with --child), so the two builds never share one.

Quality (part B): section 5.9's orbit, 1-spp frames, with one object moving a step per frame; a 1024-spp render of
every frame's scene and camera as the reference; tonemapped (Reinhard + gamma 2.2) MSE over the hit, finite pixels
of the whole image and of the moving object, relative to the raw frame's, for
  motion       load_scene_moved, temporal() at the defaults
  restarted    load_scene every frame, which is what a scene change did before: the history ends, so the image is
               the raw frame
  camera_only  the history kept by hand through pt_temporal_image at the defaults: rule 3 on a scene that moved

    python tools/motion_probe.py [--parent _snap/parent] [--out profiles/motion_probe.json] [--quick]
"""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parents[1]
SCENES = ("generated_scene", "cornell_box")
STEP = (0.012, 0.0, 0.0, -0.0024)         # temporal_probe's orbit: translate right / up / back, yaw per frame
QUALITY = (("cornell_box", 128, 128, 6), ("generated_scene", 192, 108, None))
FRAMES, SETTLED, REF_CHUNKS = 24, 8, 128


def scene_variant(scene, out_dir, name, shift):
    """The scene file with every object (shift = a number) or one object (shift = (index, vector)) displaced, written
    to out_dir with its texture paths made absolute; returns the path."""
    d = json.loads((ROOT / "scenes" / f"{scene}.scene.json").read_text())
    for k, o in enumerate(d["objects"]):
        tex = o["material"].get("texture", "")
        if tex and (ROOT / "scenes" / tex).exists():
            o["material"]["texture"] = str(ROOT / "scenes" / tex)
        if isinstance(shift, tuple):
            if k == shift[0]:
                o["position"] = [p + s for p, s in zip(o["position"], shift[1])]
        else:
            o["position"] = [o["position"][0] + shift, o["position"][1], o["position"][2]]
    if d.get("skybox") and (ROOT / "scenes" / d["skybox"]).exists():
        d["skybox"] = str(ROOT / "scenes" / d["skybox"])
    out_dir.mkdir(parents=True, exist_ok=True)
    path = out_dir / f"{scene}_{name}.scene.json"
    path.write_text(json.dumps(d))
    return str(path)


# ---- a child: one mode on one tree -------------------------------------------------------------------
def child(tree, mode, quick, tmp):
    sys.path.insert(0, str(tree))
    import pathtracercuda_amd as pa

    def step_camera(cam):
        cam = pa.PtCamera.from_buffer_copy(cam)
        pa.camera_translate(cam, *STEP[:3])
        pa.camera_rotate(cam, 0.0, STEP[3])
        return cam

    W, H = (320, 180) if quick else (1920, 1080)
    out = {}
    for scene in SCENES:
        pt = pa.Pathtracer(W, H)
        files = [scene_variant(scene, tmp, "a", 0.0), scene_variant(scene, tmp, "b", 0.01 if mode == "moved_all" else 0.0)]
        cam = pt.load_scene(files[0])
        times = {"temporal": [], "moments": []}
        for variance in (False, True):
            pt.render(cam, 1, True)
            pt.features(cam)
            pt.temporal(frames=1, variance=variance, reset=True)              # warm, and a history to reproject
            used, lengths = [], []
            for k in range(3):
                cam = step_camera(cam)
                if mode != "existing":
                    pt.load_scene_moved(files[(k + 1) % 2])
                    assert pt.holds_motion()
                pt.render(cam, 1, True)
                pt.features(cam)
                pt.temporal(frames=1, variance=variance)
                used.append(bool(pt.history_used))
                times["moments" if variance else "temporal"].append(
                    pt.temporal_moments_timing()["step"] if variance else pt.temporal_timing())
                lengths.append(float(pt.history_lengths().mean()))
            assert all(used), (scene, mode, used)
            if mode != "existing":
                pt.load_scene(files[0])
        out[scene] = dict(times, mean_history_length=lengths[-1])
        pt.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_child(tree, mode, quick, tmp):
    cmd = [sys.executable, str(pathlib.Path(__file__).resolve()), "--child", "--tree", str(tree), "--mode", mode, "--tmp", str(tmp)]
    r = subprocess.run(cmd + (["--quick"] if quick else []), capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"motion_probe: child {mode} on {tree} ended with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def timing(parent, quick, tmp):
    plans = [("parent_existing", parent, "existing"), ("existing", ROOT, "existing"), ("moved_all", ROOT, "moved_all"),
             ("moved_none", ROOT, "moved_none")]
    if parent is None:
        plans = plans[1:]
    raw = {name: {s: {"temporal": [], "moments": []} for s in SCENES} for name, _, _ in plans}
    for _ in range(3):                                        # interleaved: every plan once per run
        for name, tree, mode in plans:
            res = run_child(tree, mode, quick, tmp)
            print(name, {s: [round(t, 4) for t in res[s]["temporal"]] for s in SCENES}, flush=True)
            for s in SCENES:
                for kern in ("temporal", "moments"):
                    raw[name][s][kern] += res[s][kern]
    med = statistics.median
    out = []
    for s in SCENES:
        row = {"scene": s, "width": 320 if quick else 1920, "height": 180 if quick else 1080, "runs": 3, "launches_per_run": 3}
        for name, _, _ in plans:
            for kern in ("temporal", "moments"):
                row[f"{name}_{kern}_ms"] = {"median": med(raw[name][s][kern]), "all": raw[name][s][kern]}
        base = "parent_existing" if parent is not None else "existing"
        for kern in ("temporal", "moments"):
            b = row[f"{base}_{kern}_ms"]["median"]
            row[f"ratios_{kern}_against_{base}"] = {name: row[f"{name}_{kern}_ms"]["median"] / b for name, _, _ in plans}
        out.append(row)
    return out


# ---- quality ----------------------------------------------------------------------------------------
def quality(quick, tmp):
    import numpy as np
    sys.path.insert(0, str(ROOT))
    import pathtracercuda_amd as pa

    def ldr(img):
        c = np.maximum(img[..., :3].astype(np.float64), 0.0)
        return (c / (c + 1.0)) ** (1.0 / 2.2)

    def mse(img, ref, mask):
        return float(np.mean((ldr(img)[mask] - ldr(ref)[mask]) ** 2))

    frames, settled = (6, 2) if quick else (FRAMES, SETTLED)
    out = []
    for scene, W, H, mover in QUALITY:
        if quick:
            W, H = W // 2, H // 2
        objs = json.loads((ROOT / "scenes" / f"{scene}.scene.json").read_text())["objects"]
        if mover is None:                                     # the largest object but the ground
            sizes = [float(np.prod(o["scale"])) for o in objs]
            mover = int(np.argsort(sizes)[-2])
        step = (0.02, 0.0, 0.01)
        pm, pp = pa.Pathtracer(W, H), pa.Pathtracer(W, H)
        cam, hist, prev = None, None, None
        rows = []
        for k in range(frames):
            path = scene_variant(scene, tmp, f"q{k}", (mover, tuple(s * k for s in step)))
            c = pm.load_scene_moved(path)
            pp.load_scene(path)
            if cam is None:
                cam = c
            pp.render(cam, 8, True, chunks=8 if quick else REF_CHUNKS)
            ref = pp.get_hdr_image_data()
            for p in (pm, pp):
                p.render(cam, 1, True)
            noisy = pp.get_hdr_image_data()
            planes = pp.features(cam)["planes"]
            pm.features(cam)
            moved = pm.temporal()
            assert pm.history_used == (k > 0)
            by_camera = pa.temporal_image(noisy, *planes, cam, hist, prev)
            hist, prev = by_camera[1:], pa.PtCamera.from_buffer_copy(cam)
            fl = np.ascontiguousarray(planes[2][..., 3]).view(np.uint32)
            ok = ((fl & 1) != 0) & np.isfinite(noisy[..., :3]).all(-1) & np.isfinite(planes[1][..., :3]).all(-1) & \
                np.isfinite(planes[2][..., :3]).all(-1) & np.isfinite(ref[..., :3]).all(-1)
            table = pm.motion_table()
            row = {"pixels": int(ok.sum())}
            on = None
            if table is not None:
                ident = np.zeros((3, 4), np.float32)
                ident[0, 0] = ident[1, 1] = ident[2, 2] = 1
                prim = np.flatnonzero((table[0] != ident).any(axis=(1, 2)))
                on = ok & np.isin(np.ascontiguousarray(planes[0][..., 3]).view(np.uint32), prim.astype(np.uint32))
                row["pixels_of_the_moving_object"] = int(on.sum())
            for name, img in (("raw_and_restarted", noisy), ("motion", moved), ("camera_only", by_camera[0])):
                row[name] = mse(img, ref, ok)
                if on is not None and on.sum():
                    row[name + "_on_object"] = mse(img, ref, on)
            row["mean_history_motion"] = float(moved[..., 3][ok].mean())
            row["mean_history_camera_only"] = float(by_camera[0][..., 3][ok].mean())
            if on is not None and on.sum():
                row["mean_history_motion_on_object"] = float(moved[..., 3][on].mean())
                row["mean_history_camera_only_on_object"] = float(by_camera[0][..., 3][on].mean())
            rows.append(row)
            cam = pa.PtCamera.from_buffer_copy(cam)
            pa.camera_translate(cam, *STEP[:3])
            pa.camera_rotate(cam, 0.0, STEP[3])
        late = [r for r in rows[settled:]]

        def ratio(name, suffix=""):
            vals = [r[name + suffix] / r["raw_and_restarted" + suffix] for r in late if name + suffix in r]
            return float(np.mean(vals)) if vals else None

        out.append({"scene": scene, "width": W, "height": H, "frames": frames, "settled_from_frame": settled,
                    "moving_object": mover, "step_per_frame": step, "reference_spp": 8 * (8 if quick else REF_CHUNKS),
                    "mean_ratio_to_raw": {"motion": ratio("motion"), "restarted": 1.0, "camera_only": ratio("camera_only")},
                    "mean_ratio_to_raw_on_object": {"motion": ratio("motion", "_on_object"), "restarted": 1.0,
                                                    "camera_only": ratio("camera_only", "_on_object")},
                    "per_frame": rows})
        pm.close()
        pp.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "motion_probe.json"))
    ap.add_argument("--parent", default=None, help="a tree with the parent commit's build (tools/snap_rev.sh), e.g. _snap/parent")
    ap.add_argument("--quick", action="store_true", help="tiny sizes: a rehearsal of the tool, not a measurement")
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--tmp", default=str(pathlib.Path(tempfile.gettempdir()) / "motion_probe_scenes"),
                    help="where the displaced scene files are written")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=str(ROOT), help=argparse.SUPPRESS)
    ap.add_argument("--mode", default="existing", help=argparse.SUPPRESS)
    args = ap.parse_args()
    tmp = pathlib.Path(args.tmp)
    if args.child:
        child(pathlib.Path(args.tree).resolve(), args.mode, args.quick, tmp)
        return
    parent = pathlib.Path(args.parent).resolve() if args.parent else None
    record = {"tool": "tools/motion_probe.py", "quick": args.quick, "parent_tree": args.parent}
    record["timing"] = timing(parent, args.quick, tmp)
    print("timing done", flush=True)
    if not args.skip_quality:
        record["quality"] = quality(args.quick, tmp)
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(record, indent=1) + "\n")
    print(json.dumps({k: v for k, v in record.items() if k != "quality"}, indent=1)[:6000])
    for q in record.get("quality", []):
        print(q["scene"], q["mean_ratio_to_raw"], q["mean_ratio_to_raw_on_object"])


if __name__ == "__main__":
    main()
