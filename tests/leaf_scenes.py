"""Directed scenes for the leaf tests' cube and quadric paths (tests/test_leaf_forms.py,
tests/test_gpu_leaf_forms.py), and numpy helpers that show a scene holds what it claims.

The cube test has two forms (pathtracercuda_amd/csrc/pt_leaf_forms.h): the reference's loop, which the
kernel runs, and a min/max form behind one wave-uniform guard that falls back to the loop for the whole
wave when a lane's local ray leaves the guard (a zero, denormal, huge or NaN direction component, a
non-finite origin, a NaN t_max).  Each scene here drives one side of that guard, or the boundary
between the two, through cubes that
share leaves with the other shapes.  All are meant for 48 x 32 pixels.

A camera with fovy = 0 sends every primary ray exactly along its viewing direction (tan 0 = 0, so
horizontal = vertical = 0): looking down a world axis at an unrotated cube, the local direction has
two components that are exactly 0, whatever the pixel's jitter.  The paths still differ per pixel
from the first bounce on (each pixel has its own random stream).
"""
from __future__ import annotations

import pathlib

import numpy as np

import kat
from ref_scenes import M, _write, cam, drop_unset_uv_textures

W, H = 48, 32
F32 = np.float32
SPHERE, CYLINDER, DISK, CONE, PARABOLOID, QUAD, CUBE = range(7)
QUADRICS = (SPHERE, CYLINDER, CONE, PARABOLOID)
T_MIN = 0.001


def _floor():
    return kat.obj("QUAD", pos=(0.0, -1.5, 0.0), scale=(8.0, 1.0, 8.0), mat=M("LAMBERT", base=(0.6, 0.6, 0.6)))


def _neighbours():
    """Other shapes around the cube, so its leaf and the bounce rays meet every family."""
    return [_floor(),
            kat.obj("SPHERE", pos=(2.2, 0.0, 2.5), scale=(0.7, 0.7, 0.7), mat=M("GGX", rough=0.3, metal=1.0)),
            kat.obj("CYLINDER", pos=(-2.2, -0.5, -2.0), scale=(0.5, 1.0, 0.5), mat=M(base=(0.9, 0.3, 0.3), rough=0.4))]


def cube_axis(tmp, axis):
    """An unrotated unit cube seen exactly along world x or z (fovy 0): two local direction components
    are exactly 0 on every primary ray, so 1 / d is +-inf and the slab distances are +-inf.  Along y the
    camera's basis is undefined (it looks along its up vector), so the cube is turned instead -- 90
    degrees about x, whose cosine is -4.4e-8 in float32: components near 1e-8, inside the guard, with
    reciprocals above 1e7."""
    cube = kat.obj("CUBE", rot=(90.0, 0.0, 0.0) if axis == "y" else (0.0, 0.0, 0.0),
                   mat=M(base=(0.3, 0.5, 0.9), rough=0.4, metal=0.2))
    eye = {"x": ((6.0, 0.25, 0.125), (0.0, 0.25, 0.125)), "y": ((0.25, 0.125, 6.0), (0.25, 0.125, 0.0)),
           "z": ((0.25, 0.125, 6.0), (0.25, 0.125, 0.0))}[axis]
    return _write(tmp, f"leaf_cube_axis_{axis}", [cube] + _neighbours(), cam(eye[0], eye[1], 0.0))


def cube_face_plane(tmp):
    """The camera on the plane of the cube's face x = 1, looking along -z with fovy 0: the local origin's
    x is exactly 1 and the direction's x exactly 0, so (1 - o.x) * (1 / d.x) = 0 * inf = NaN, which the
    reference's selects skip."""
    cube = kat.obj("CUBE", mat=M(base=(0.9, 0.6, 0.2), rough=0.4, metal=0.2))
    return _write(tmp, "leaf_cube_face_plane", [cube] + _neighbours(), cam((1.0, 0.125, 6.0), (1.0, 0.125, 0.0), 0.0))


def cube_inside(tmp):
    """The camera inside an unrotated cube: every primary ray leaves lo = tMin, and the hit is at tMin
    itself (AABB::intersect's entry distance), so a path creeps forward 0.001 per bounce."""
    glow = (0.15, 0.2, 0.25)
    objs = [kat.obj("CUBE", scale=(2.0, 2.0, 2.0), mat=M(rough=0.4, metal=0.3, emissive=glow)),
            kat.obj("SPHERE", pos=(0.6, 0.7, 0.3), scale=(0.1, 0.1, 0.1), mat=M("LAMBERT", emissive=(8.0, 7.0, 6.0))),
            kat.obj("CUBE", pos=(-0.8, -0.5, 0.6), rot=(10.0, 30.0, 0.0), scale=(0.2, 0.2, 0.2), mat=M(base=(0.9, 0.3, 0.3)))]
    return _write(tmp, "leaf_cube_inside", objs, cam((0.1, 0.8, 0.1), (1.0, 0.9, 0.6), 80.0))


def cubes_scaled(tmp):
    """Cubes under rotations about all three axes and scales from 1e-3 to 1e3: local direction
    components and origins from 1e-3 to 1e3 times the world's."""
    objs = [kat.obj("CUBE", pos=(-2.5, 0.0, 0.0), rot=(12.0, 34.0, 56.0), scale=(1.0, 0.3, 0.6), mat=M("LAMBERT", base=(0.9, 0.9, 0.2))),
            kat.obj("CUBE", pos=(0.0, 0.0, 0.0), rot=(-65.0, 5.0, 130.0), scale=(1e-3, 0.8, 0.8), mat=M("GGX", rough=0.1, metal=1.0)),
            kat.obj("CUBE", pos=(2.5, 0.0, 0.0), rot=(33.0, 47.0, 71.0), scale=(0.7, 1e-3, 0.9), mat=M(base=(0.3, 0.9, 0.3))),
            kat.obj("CUBE", pos=(0.0, -1003.0, 0.0), rot=(0.0, 20.0, 0.0), scale=(1e3, 1e3, 1e3), mat=M(rough=0.6)),
            kat.obj("CUBE", pos=(0.0, 2.0, -1.0), rot=(45.0, 45.0, 45.0), scale=(0.4, 0.4, 1e-3), mat=M(base=(0.3, 0.3, 0.9))),
            kat.obj("CUBE", pos=(0.0, 0.0, -60.0), rot=(10.0, 20.0, 30.0), scale=(1e3, 30.0, 1e-3), mat=M("LAMBERT", base=(0.5, 0.5, 0.7)))]
    return _write(tmp, "leaf_cubes_scaled", objs, cam((0.0, 1.0, 9.0), (0.0, 0.0, 0.0), 50.0))


def cube_edges(tmp):
    """Cubes 1e-4 wide seen from 120 away along all three axes (the construction of ref_scenes.rim): in
    local space the origin and the products d * t are near 1.2e6, where a float's step is 1/8, so hit
    points and slab distances sit on a 1/8 grid: rays exactly along edges and through corners, where
    the per-axis entry distances tie."""
    mats = [M("LAMBERT", base=(0.9, 0.2, 0.2), emissive=(0.5, 0.1, 0.1)), M("LAMBERT", base=(0.2, 0.9, 0.2), emissive=(0.1, 0.5, 0.1)),
            M("LAMBERT", base=(0.2, 0.2, 0.9), emissive=(0.1, 0.1, 0.5))]
    objs = [kat.obj("CUBE", pos=(x, 0.0, 0.0), scale=(1e-4, 1e-4, 1e-4), mat=m) for x, m in zip((-3e-4, 0.0, 3e-4), mats)]
    return _write(tmp, "leaf_cube_edges", objs, cam((120.0, 120.0, 120.0), (0.0, 0.0, 0.0), 2.2e-4))


def cube_leaf4(tmp):
    """Four small cubes close together and far from the rest: one BVH leaf of four cubes, so a lane runs
    the cube path four times in a row with a falling t_max."""
    red, blue = M("LAMBERT", base=(0.9, 0.1, 0.1)), M("GGX", base=(0.1, 0.1, 0.9), rough=0.3, metal=1.0)
    green, grey = M("LAMBERT", base=(0.1, 0.9, 0.1)), M(rough=0.5)
    objs = [_floor(),
            kat.obj("SPHERE", pos=(3.0, 0.0, -2.0), mat=M(rough=0.3, metal=0.5)),
            kat.obj("CYLINDER", pos=(-3.0, -0.5, -2.0), scale=(0.5, 1.0, 0.5), mat=grey),
            kat.obj("QUAD", pos=(0.0, 1.0, -4.0), rot=(90.0, 0.0, 0.0), scale=(2.0, 1.0, 1.0), mat=green),
            kat.obj("CUBE", pos=(-0.3, 0.0, 2.0), rot=(0.0, 15.0, 0.0), scale=(0.25, 0.25, 0.25), mat=red),
            kat.obj("CUBE", pos=(0.3, 0.0, 2.0), rot=(20.0, 0.0, 0.0), scale=(0.25, 0.25, 0.25), mat=blue),
            kat.obj("CUBE", pos=(-0.3, 0.0, 2.6), scale=(0.25, 0.25, 0.25), mat=green),
            kat.obj("CUBE", pos=(0.3, 0.0, 2.6), rot=(0.0, 0.0, 30.0), scale=(0.25, 0.25, 0.25), mat=grey)]
    return _write(tmp, "leaf_cube_leaf4", objs, cam((0.0, 1.5, 7.0), (0.0, 0.0, 2.0), 40.0))


def all_quadrics(tmp):
    """All four quadric shapes beside planes and cubes: two groups of four (sphere, quad, cube, cylinder
    and cone, disk, cube, paraboloid), each close together and far from the other, so each is one leaf
    in which a wave runs all three family paths."""
    a, b = (-2.0, 0.0, 0.0), (2.0, 0.0, 0.0)
    objs = [kat.obj("SPHERE", pos=(a[0] - 0.5, 0.0, 0.0), scale=(0.4, 0.4, 0.4), mat=M("GGX", rough=0.3, metal=1.0)),
            kat.obj("QUAD", pos=(a[0], -0.45, 0.2), scale=(0.9, 1.0, 0.9), mat=M("LAMBERT", base=(0.7, 0.7, 0.3))),
            kat.obj("CUBE", pos=(a[0] + 0.5, -0.1, 0.0), rot=(0.0, 25.0, 0.0), scale=(0.3, 0.3, 0.3), mat=M(base=(0.3, 0.5, 0.9))),
            kat.obj("CYLINDER", pos=(a[0], 0.0, -0.6), rot=(15.0, 0.0, 20.0), scale=(0.25, 0.5, 0.25), mat=M(base=(0.9, 0.3, 0.3), rough=0.4)),
            kat.obj("CONE", pos=(b[0] - 0.5, 0.0, 0.0), rot=(10.0, 0.0, 15.0), scale=(0.4, 0.4, 0.4), mat=M(base=(0.3, 0.9, 0.3))),
            kat.obj("DISK", pos=(b[0], -0.45, 0.2), scale=(0.9, 1.0, 0.9), mat=M(rough=0.2, metal=0.7)),
            kat.obj("CUBE", pos=(b[0] + 0.5, -0.1, 0.0), rot=(30.0, 0.0, 10.0), scale=(0.3, 0.3, 0.3), mat=M("LAMBERT", base=(0.9, 0.9, 0.2))),
            kat.obj("PARABOLOID", pos=(b[0], 0.2, -0.6), rot=(0.0, 33.0, 160.0), scale=(0.4, 0.6, 0.4), mat=M(base=(0.3, 0.3, 0.9)))]
    return _write(tmp, "leaf_all_quadrics", objs, cam((0.0, 1.2, 6.0), (0.0, -0.1, 0.0), 50.0))


LEAF_SCENES = {
    "cube_axis_x": lambda tmp: cube_axis(tmp, "x"),
    "cube_axis_y": lambda tmp: cube_axis(tmp, "y"),
    "cube_axis_z": lambda tmp: cube_axis(tmp, "z"),
    "cube_face_plane": cube_face_plane,
    "cube_inside": cube_inside,
    "cubes_scaled": cubes_scaled,
    "cube_edges": cube_edges,
    "cube_leaf4": cube_leaf4,
    "all_quadrics": all_quadrics,
}
ZERO_COMPONENT = ("cube_axis_x", "cube_axis_z", "cube_face_plane")     # claim: exact zeros in the local direction
CUBE_PRIMARY = tuple(LEAF_SCENES)                                      # claim: some primary hit is a cube


def leaf_scene(tmp: pathlib.Path, name: str) -> pathlib.Path:
    """The named scene, written into tmp, in the form every layer is given."""
    return drop_unset_uv_textures(LEAF_SCENES[name](tmp))


# ---- what a scene holds --------------------------------------------------------------------------
def camera_rays(camera):
    """Origin and per-pixel unit directions (H x W x 3, float32) of the rays through the pixel centres,
    formed as the renderers form them: normalize((llc + u * horizontal) + v * vertical)."""
    o = np.array(camera.origin, dtype=F32)
    llc, hor, ver = (np.array(getattr(camera, k), dtype=F32) for k in ("lowerLeftCorner", "horizontal", "vertical"))
    u = ((np.arange(W, dtype=F32) + F32(0.5)) / F32(W))[None, :, None]
    v = ((np.arange(H, dtype=F32) + F32(0.5)) / F32(H))[:, None, None]
    d = (llc + u * hor) + v * ver
    l2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return o, (d * (F32(1.0) / np.sqrt(l2))[..., None]).astype(F32)


def to_local(rows, o, d):
    """World ray -> object space with the 3 x 4 inverse rows, in float32 in the kernel's order."""
    r = np.array(rows, dtype=F32).reshape(3, 4)
    lo = np.array([((o[0] * r[k, 0] + o[1] * r[k, 1]) + o[2] * r[k, 2]) + r[k, 3] for k in range(3)], dtype=F32)
    ld = np.stack([(d[..., 0] * r[k, 0] + d[..., 1] * r[k, 1]) + d[..., 2] * r[k, 2] for k in range(3)], axis=-1)
    return lo, ld.astype(F32)


def _hit_distance(kind, o, d):
    """Hit distance per pixel (inf = miss) of one primitive for local rays, in float64: enough to name
    the primary hit of a pixel-centre ray."""
    o = o.astype(np.float64)
    d = d.astype(np.float64)
    big = np.float64(3.402823466e38)
    with np.errstate(all="ignore"):
        if kind in (DISK, QUAD):
            t = -o[1] / d[..., 1]
            hx, hz = o[0] + d[..., 0] * t, o[2] + d[..., 2] * t
            ok = (d[..., 1] != 0) & (t > T_MIN)
            ok &= ((np.abs(hx) <= 1) & (np.abs(hz) <= 1)) if kind == QUAD else (hx * hx + hz * hz < 1)
            return np.where(ok, t, np.inf)
        if kind == CUBE:
            lo = np.full(d.shape[:-1], T_MIN)
            hi = np.full(d.shape[:-1], big)
            for a in range(3):
                inv = 1.0 / d[..., a]
                t0, t1 = (-1.0 - o[a]) * inv, (1.0 - o[a]) * inv
                t0, t1 = np.where(inv < 0, t1, t0), np.where(inv < 0, t0, t1)
                lo = np.where(t0 > lo, t0, lo)
                hi = np.where(t1 < hi, t1, hi)
            return np.where(hi <= lo, np.inf, lo)
        B = {SPHERE: 1.0, CONE: -1.0}.get(kind, 0.0)
        Hc = -1.0 if kind == PARABOLOID else 0.0
        J = -1.0 if kind in (SPHERE, CYLINDER) else 0.0
        a = d[..., 0] ** 2 + B * d[..., 1] ** 2 + d[..., 2] ** 2
        b = 2 * o[0] * d[..., 0] + 2 * B * o[1] * d[..., 1] + 2 * o[2] * d[..., 2] + Hc * d[..., 1]
        c = o[0] ** 2 + B * o[1] ** 2 + o[2] ** 2 + Hc * o[1] + J
        disc = b * b - 4 * a * c
        rt = np.sqrt(np.where(disc < 0, 0.0, disc))
        q = np.where(b < 0, -0.5 * (b - rt), -0.5 * (b + rt))
        x0, x1 = q / a, c / q
        t0, t1 = np.minimum(x0, x1), np.maximum(x0, x1)
        if kind == SPHERE:
            return np.where((disc >= 0) & (t1 > T_MIN), np.where(t0 > T_MIN, t0, t1), np.inf)
        v0 = (t0 > T_MIN) & (np.abs(d[..., 1] * t0 + o[1]) <= 1)
        v1 = (t1 > T_MIN) & (np.abs(d[..., 1] * t1 + o[1]) <= 1)
        return np.where((disc >= 0) & (v0 | v1), np.where(v0, t0, t1), np.inf)


def scene_facts(osc):
    """From an oracle scene (BVH-order primitives, camera): per pixel the type of the primary hit (-1 =
    sky) and whether some cube's local direction has a component that is exactly zero."""
    o, d = camera_rays(osc.camera)
    best = np.full((H, W), np.inf)
    kind_at = np.full((H, W), -1)
    zero = np.zeros((H, W), dtype=bool)
    for i in range(osc.prim_count):
        p = osc.prims[i]
        lo, ld = to_local(p.rows, o, d)
        if p.type == CUBE:
            zero |= (ld == 0).any(-1)
        t = _hit_distance(int(p.type), lo, ld)
        closer = t < best
        best = np.where(closer, t, best)
        kind_at = np.where(closer, int(p.type), kind_at)
    return kind_at, zero


def leaf_types(osc):
    """The primitive types of every BVH leaf, as tuples."""
    out = []
    for i in range(osc.node_count):
        n = osc.nodes[i]
        count = n.primitiveCountAxis >> 16
        if count:
            out.append(tuple(int(osc.prims[n.offset + k].type) for k in range(count)))
    return out
