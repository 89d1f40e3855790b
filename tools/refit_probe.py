#!/usr/bin/env python3
"""What a move costs, and what a refitted tree costs the tracer -> profiles/refit_probe.json.

  python tools/refit_probe.py [--rounds 3] [--out profiles/refit_probe.json]

Every measurement runs in a process of its own (this script starts itself with `one ...`), in three interleaved rounds;
the report gives the median and the range of each.

move      one pt_move_primitives of 1, 100 and all primitives of generated_scene and of the benchmark's 100k-object
          scene (generated as bench.py generates it), onto the poses they have (the cost does not depend on where a
          box goes): wall clock of the call, the host packing, the one host-to-device copy and the kernels
          (pt_read_refit_timing), and what is left: the checks, the launches and the 32-byte read-back.
objects   the same through Pathtracer.move_objects, whose host work grows with the whole scene (the class refits its
          own tree and fills a full motion table), against load_scene_moved of a file with the same poses.
rebuild   what the same poses cost without the refit: the host's SAH build (pth_scene_timing) and pt_set_scene_moved
          with the full table.
trace     the step time of a 1920 x 1080 frame of generated_scene at 8 samples per pixel after a tenth of the objects
          moved by 0.1, 1 and 10 times their size: on the refitted tree, then on the tree rebuild_scene() makes of the
          same poses.
"""
import argparse
import ctypes as C
import json
import pathlib
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def scene_file(name):
    if name == "stress_100k":
        import bench
        return bench.scene_path("stress_100k")
    return str(ROOT / "scenes" / f"{name}.scene.json")


def element_boxes(scene, prims):
    objs, aabbs = scene.objects()
    n = scene.object_count
    where = {}
    for i in range(n):
        where.setdefault(bytes(objs[i]), []).append(i)
    return np.array([aabbs[where[bytes(prims[e])].pop(0)] for e in range(n)], dtype=np.float32)


def one_move(name, count):
    import pathtracercuda_amd as pa
    from pathtracercuda_amd import _native as N
    lib, fp, up = N.hip(), C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    path = scene_file(name)
    pt = pa.Pathtracer(64, 64)
    pt.load_scene(path)
    scene = pa.Scene(path, 64, 64)
    nodes, prims = scene.bvh()
    n = scene.object_count
    boxes = element_boxes(scene, prims)
    N.check_ctx(lib.pt_set_primitive_boxes(pt._ctx, boxes.ctypes.data_as(fp)), pt._ctx)
    count = n if count <= 0 else min(count, n)
    index = np.sort(np.random.default_rng(7).choice(n, size=count, replace=False)).astype(np.uint32)
    sub = (pa.PtHittable * count)(*[prims[int(j)] for j in index])
    sb = np.ascontiguousarray(boxes[index])
    rows = np.ascontiguousarray(np.tile(np.eye(3, 4, dtype=np.float32), (count, 1, 1)))
    walls, kernels, packs, copies = [], [], [], []
    ms = (C.c_float * 3)()
    for rep in range(6):                     # the first call allocates the staging buffer and the table
        t0 = time.perf_counter()
        rc = lib.pt_move_primitives(pt._ctx, count, index.ctypes.data_as(up), sub, sb.ctypes.data_as(fp), rows.ctypes.data_as(fp),
                                    index.ctypes.data_as(up))
        t1 = time.perf_counter()
        N.check_ctx(rc, pt._ctx)
        N.check_ctx(lib.pt_read_refit_timing(pt._ctx, ms), pt._ctx)
        if rep:
            walls.append(1e3 * (t1 - t0))
            kernels.append(float(ms[0]))
            packs.append(float(ms[1]))
            copies.append(float(ms[2]))
    k = int(np.argsort(walls)[len(walls) // 2])
    return {"objects": n, "moved": count, "wall_ms": walls[k], "pack_ms": packs[k], "copy_ms": copies[k], "kernels_ms": kernels[k],
            "checks_launches_readback_ms": walls[k] - packs[k] - copies[k] - kernels[k]}


def one_objects(name, count):
    """What a user calls: Pathtracer.move_objects, whose host work (the class's own refit of its tree, the full motion
    table, the Python arrays) grows with the whole scene, against load_scene_moved of a file with the same poses."""
    import pathtracercuda_amd as pa
    path = scene_file(name)
    pt = pa.Pathtracer(64, 64)
    pt.load_scene(path)
    pos, rot, scale = pt.object_transforms()
    n = len(pos)
    count = n if count <= 0 else min(count, n)
    which = np.sort(np.random.default_rng(7).choice(n, size=count, replace=False))
    walls = []
    for rep in range(4):
        t0 = time.perf_counter()
        pt.move_objects(which, pos[which], rot[which], scale[which])
        walls.append(1e3 * (time.perf_counter() - t0))
    t0 = time.perf_counter()
    pt.load_scene_moved(path)
    loaded = 1e3 * (time.perf_counter() - t0)
    return {"objects": n, "moved": count, "move_objects_wall_ms": statistics.median(walls[1:]), "load_scene_moved_wall_ms": loaded}


def one_rebuild(name):
    import pathtracercuda_amd as pa
    from pathtracercuda_amd import _native as N
    lib, fp, up = N.hip(), C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    path = scene_file(name)
    pt = pa.Pathtracer(64, 64)
    pt.load_scene(path)
    builds, sets = [], []
    for rep in range(3):
        scene = pa.Scene(path, 64, 64)      # parse and SAH build, as every frame's load does
        nodes, prims = scene.bvh()
        n = scene.object_count
        rows = np.ascontiguousarray(np.tile(np.eye(3, 4, dtype=np.float32), (n, 1, 1)))
        prev = np.arange(n, dtype=np.uint32)
        t0 = time.perf_counter()
        rc = lib.pt_set_scene_moved(pt._ctx, nodes, scene.node_count, prims, n, rows.ctypes.data_as(fp), prev.ctypes.data_as(up))
        t1 = time.perf_counter()
        N.check_ctx(rc, pt._ctx)
        builds.append(scene.timing()["bvh_ms"])
        sets.append(1e3 * (t1 - t0))
    return {"objects": n, "sah_build_ms": statistics.median(builds), "set_scene_moved_ms": statistics.median(sets),
            "total_ms": statistics.median(builds) + statistics.median(sets)}


def one_trace(factor):
    import pathtracercuda_amd as pa
    pt = pa.Pathtracer(1920, 1080)
    cam = pt.load_scene(scene_file("generated_scene"))
    pos, rot, scale = pt.object_transforms()
    n = len(pos)
    rng = np.random.default_rng(11)
    which = np.sort(rng.choice(n, size=max(1, n // 10), replace=False))
    step = rng.uniform(-1.0, 1.0, (len(which), 3)).astype(np.float32) * np.abs(scale[which]).max(axis=1, keepdims=True) * np.float32(factor)

    def step_ms():
        out = []
        for _ in range(4):
            pt.render(cam, 8, True)
            out.append(pt.get_timing())
        return statistics.median(out[1:])

    base = step_ms()
    pt.move_objects(which, pos[which] + step, rot[which], scale[which])
    refitted = step_ms()
    pt.rebuild_scene()
    rebuilt = step_ms()
    return {"factor": factor, "moved": int(len(which)), "objects": int(n), "before_ms": base, "refitted_ms": refitted, "rebuilt_ms": rebuilt}


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "refit_probe.json"))
    ap.add_argument("one", nargs="*")
    a = ap.parse_args()
    if a.one:
        kind = a.one[1]
        r = one_move(a.one[2], int(a.one[3])) if kind == "move" else one_objects(a.one[2], int(a.one[3])) if kind == "objects" else one_rebuild(a.one[2]) if kind == "rebuild" else one_trace(float(a.one[2]))
        print("RESULT " + json.dumps(r))
        return
    jobs = [("move", s, str(c)) for s in ("generated_scene", "stress_100k") for c in (1, 100, 0)]
    jobs += [("objects", s, str(c)) for s in ("generated_scene", "stress_100k") for c in (1, 0)]
    jobs += [("rebuild", s) for s in ("generated_scene", "stress_100k")] + [("trace", f) for f in ("0.1", "1", "10")]
    got = {j: [] for j in jobs}
    for _ in range(a.rounds):
        for j in jobs:                       # interleaved: every job once per round
            run = subprocess.run([sys.executable, __file__, "one", *j], capture_output=True, text=True, timeout=600)
            line = [l for l in run.stdout.splitlines() if l.startswith("RESULT ")]
            if run.returncode != 0 or not line:
                raise SystemExit(f"{j}: rc {run.returncode}\n{run.stderr[-2000:]}")
            got[j].append(json.loads(line[-1][7:]))
            print("ROUND", json.dumps({"job": list(j), "result": got[j][-1]}), flush=True)
    report = []
    for j, rs in got.items():
        entry = {"job": list(j), "rounds": len(rs)}
        for key in rs[0]:
            vals = [r[key] for r in rs]
            entry[key] = vals[0] if key in ("objects", "moved", "factor") else spread(vals)
        report.append(entry)
    pathlib.Path(a.out).write_text(json.dumps({"tool": "tools/refit_probe.py", "results": report}, indent=1) + "\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
