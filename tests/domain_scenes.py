"""Scenes over the whole accepted input range (DESIGN.md §3 "Input domain"), for tests/test_domain.py
and tests/test_gpu_domain.py: a scene file the loader reads without error, whose values are finite
float32, and whose BVH the reference builds.  What arithmetic makes of such values -- overflowing
emission, NaN throughput, position == look_at -- is inside the domain.  One input is refused by
name instead of rendered: an object whose inverse transform is not finite (a zero scale,
refused_by_loader); the reference's source and the oracle are still compared on such scenes.

The kernel drops range guards on the strength of arguments written in comments (sqrt_dom,
normalize_dom, rcp_fast, the select forms of acos and atan2, the slab test without early returns).
tools/fp_exhaustive.hip proves each fast function on its stated domain; the scenes here ask whether
the call sites stay inside it.  Each directed builder names the comment it attacks.  All directed
scenes are meant for 48 x 32 pixels, the random ones for 32 x 24.

The comparison rule for float buffers is same_bits_or_both_nan: on x86 the sign of a NaN produced by
an operation depends on the operand order the compiler picked, so the reference's source and the
oracle disagree on it (0x7fc00000 against 0xffc00000, seen with zero scales); "the same bits" is
only defined for words that are not NaN.  RNG states and tonemapped bytes stay strictly equal.
"""
from __future__ import annotations

import collections
import math
import pathlib

import numpy as np

import kat
from ref_scenes import CHECKER, H, M, W, _write, cam, drop_unset_uv_textures

RW, RH = 32, 24                                   # the random scenes' resolution


# ---- the comparison rule ------------------------------------------------------------------------
def same_bits_or_both_nan(a, b, what, seed=None, path=None):
    """Every 32-bit word equal, or both NaN.  On a mismatch the message names the first differing
    pixel with both values, and for a random scene the seed and the scene's path."""
    fa, fb = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert fa.shape == fb.shape, f"{what}: shapes {fa.shape} vs {fb.shape}"
    ua, ub = fa.view(np.uint32), fb.view(np.uint32)
    bad = (ua != ub) & ~(np.isnan(fa) & np.isnan(fb))
    if bad.any():
        d = np.argwhere(bad)
        at = tuple(int(i) for i in (d[0][:2] if fa.ndim >= 2 else d[0]))
        where = f"; seed {seed}" if seed is not None else ""
        where += f"; scene {path}" if path is not None else ""
        raise AssertionError(f"{what}: {len(d)} words differ (NaN == NaN); first at pixel (row, x) = {at}: "
                             f"{fa[at]} [{' '.join(f'{w:#010x}' for w in np.atleast_1d(ua[at]))}] vs "
                             f"{fb[at]} [{' '.join(f'{w:#010x}' for w in np.atleast_1d(ub[at]))}]{where}")


def nan_signs_differ(a, b) -> int:
    """Words that are NaN in both buffers with different bits: why the rule above exists."""
    fa, fb = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return int((np.isnan(fa) & np.isnan(fb) & (fa.view(np.uint32) != fb.view(np.uint32))).sum())


# ---- helpers ------------------------------------------------------------------------------------
def fl(v):
    return tuple(float(x) for x in v)


def Mf(mtype="LAMBERT_GGX", base=(0.8, 0.8, 0.8), rough=0.5, metal=0.0, emissive=(0.0, 0.0, 0.0), texture=""):
    # the loader reads roughness and metalness only from JSON floats: an integer would be ignored
    return M(mtype, base=fl(base), rough=float(rough), metal=float(metal), emissive=fl(emissive), texture=texture)


def obj(kind, pos=(0.0, 0.0, 0.0), rot=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0), mat=None):
    return kat.obj(kind, pos=fl(pos), rot=fl(rot), scale=fl(scale), mat=mat)


FLOOR = dict(pos=(0.0, -1.0, 0.0), scale=(6.0, 1.0, 6.0))
STD_CAM = ((0.0, 0.5, 5.0), (0.0, 0.0, 0.0), 40.0)


def floor(mat=None):
    return obj("QUAD", mat=mat or Mf("LAMBERT", base=(0.6, 0.6, 0.6)), **FLOOR)


def still_life():
    """Ordinary objects for the scenes whose edge is the camera or the sky."""
    return [floor(Mf(rough=0.3, metal=0.5)),
            obj("SPHERE", pos=(-1.2, 0.0, 0.0), mat=Mf("GGX", base=(0.9, 0.6, 0.2), rough=0.3, metal=1.0)),
            obj("CUBE", pos=(1.2, -0.5, 0.0), rot=(0.0, 30.0, 0.0), scale=(0.5, 0.5, 0.5), mat=Mf(base=(0.2, 0.6, 0.9))),
            obj("CYLINDER", pos=(0.0, -0.5, -1.5), scale=(0.4, 0.5, 0.4), mat=Mf("LAMBERT", base=(0.9, 0.3, 0.3)))]


def write_rgbe_raw(path: pathlib.Path, data: np.ndarray) -> pathlib.Path:
    """Flat RGBE scanlines from h x w x 4 bytes as they are (any exponent byte, 255 included)."""
    h, w, _ = data.shape
    assert not ((data[:, 0, 0] == 2) & (data[:, 0, 1] == 2)).any()      # not the RLE marker
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n" + f"-Y {h} +X {w}\n".encode())
        f.write(np.ascontiguousarray(data, dtype=np.uint8).tobytes())
    return path


# ---- roughness above 1 --------------------------------------------------------------------------
def rough_normal(tmp, rough, mtype="LAMBERT_GGX", name=None):
    """pt_dev_path.h specular_ggx, "the first operand, NdotV^2 (1 - a2) + a2 with a2 in [0, 1], is NaN or
    >= 1e-10 (sqrt_dom)".  Nothing keeps a2 = roughness^4 in [0, 1]: the loader clamps roughness only
    from below.  With NdotV = |V.z| + 1e-5 > 1 the operand is negative once a2 (1 - NdotV^2) < -NdotV^2,
    i.e. for a2 > ~50001 (roughness > 14.953) within acos(1 - 1e-5 + 1 / (2 a2)) of normal incidence:
    0.12 degrees at roughness 16, 0.26 at 64.  The reference takes sqrtf of it: NaN.  A quad seen along
    its normal from (1e-3, 5, 1e-3) with fovy 0.2 degrees keeps every ray inside that cone.
    Roughness 14 (a2 = 38416) is the twin below the bound: no NaN."""
    objs = [obj("QUAD", scale=(2.5, 1.0, 2.5), mat=Mf(mtype, rough=rough, metal=0.5))]
    return _write(tmp, name or f"rough_normal_{rough:g}", objs, cam((1e-3, 5.0, 1e-3), (0.0, 0.0, 0.0), 0.2))


def ggx_rough_normal(tmp):
    """The same operand under pure GGX.  Its direction always comes from the VNDF lobe, and at normal
    incidence with a = roughness^2 >= 224 the sampled half vector is stretched by a into the surface
    plane, so the mirrored direction points below the surface (dir.z < 0) and the sample is dropped
    before specular_ggx runs.  A sample survives only when the unstretched half vector lies within
    ~1/a of the normal: a fraction ~1/a^2 of the samples (2e-5 at roughness 15, 6e-8 at 64), against
    every cosine-lobe sample of LAMBERT_GGX.  So the lobe can reach the negative operand, rarely: a
    search over roughness 15 to 32, fovy 0.05 to 0.2 degrees and camera offsets of 1e-4 to 1.2e-3 found
    one NaN pixel of 1536 in the reference's output in 21 of 216 configurations and none in the rest.
    Roughness 17 with fovy 0.05 degrees had it at nine of twelve offsets; this scene uses the middle
    one (tests/test_domain.py asserts the NaN is there)."""
    objs = [obj("QUAD", scale=(2.5, 1.0, 2.5), mat=Mf("GGX", rough=GGX_ROUGH[0], metal=0.5))]
    dx = GGX_ROUGH[1]
    return _write(tmp, "ggx_rough_normal", objs, cam((dx, 5.0, 1e-4), (0.0, 0.0, 0.0), GGX_ROUGH[2]))


GGX_ROUGH = (17.0, 5e-4, 0.05)       # roughness, camera x offset, fovy: see ggx_rough_normal


def rough_spheres(tmp, rough):
    """The same operand, vndf_pdf's root and vndf_sample_rsc's `a * V` at ordinary angles: roughness 2
    (a2 = 16) and 1e10 (a = 1e20, a2 = inf: inf - inf and 0 * inf in d_ggx and the two roots)."""
    objs = [floor(Mf(rough=rough, metal=0.2)),
            obj("SPHERE", pos=(0.0, 0.0, 0.0), mat=Mf("LAMBERT_GGX", base=(0.8, 0.5, 0.3), rough=rough, metal=0.5)),
            obj("SPHERE", pos=(-1.6, -0.4, 0.8), scale=(0.6, 0.6, 0.6), mat=Mf("GGX", rough=rough, metal=1.0))]
    return _write(tmp, f"rough_spheres_{rough:g}", objs, cam(*STD_CAM))


# ---- metalness and base colour outside [0, 1] ---------------------------------------------------
def metal_out(tmp):
    """shade(): F0 = lerp(0.04, base, metal) and the diffuse weight 1 - metal with metalness -1 and 3:
    negative attenuation, negative throughput, negative pixels.  No guard was removed on the
    strength of metalness in [0, 1]; this pins that none may be."""
    objs = [floor(Mf(rough=0.4, metal=-1.0)),
            obj("SPHERE", pos=(-1.1, 0.0, 0.0), mat=Mf("LAMBERT_GGX", base=(0.8, 0.5, 0.3), rough=0.4, metal=3.0)),
            obj("SPHERE", pos=(1.1, 0.0, 0.0), mat=Mf("GGX", base=(0.3, 0.5, 0.8), rough=0.3, metal=-1.0)),
            obj("CUBE", pos=(0.0, -0.6, 1.5), scale=(0.4, 0.4, 0.4), mat=Mf("GGX", rough=0.5, metal=3.0))]
    return _write(tmp, "metal_out", objs, cam(*STD_CAM))


def base_out(tmp):
    """shade(): `is_zero(att)`, the throughput product and the emission sum with base colour
    (-0.5, 2, 1e20) and (5, 5, 5) with emission (1e38, 1e38, -1e38): sums overflow to +-inf,
    inf - inf and 0 * inf follow."""
    objs = [floor(Mf(base=(-0.5, 2.0, 1e20), rough=0.5, metal=0.3)),
            obj("SPHERE", pos=(-1.1, 0.0, 0.0), mat=Mf("LAMBERT", base=(5.0, 5.0, 5.0), emissive=(1e38, 1e38, -1e38))),
            obj("SPHERE", pos=(1.1, 0.0, 0.0), mat=Mf("GGX", base=(-0.5, 2.0, 1e20), rough=0.3, metal=1.0)),
            obj("CYLINDER", pos=(0.0, -0.5, 1.5), scale=(0.3, 0.5, 0.3), mat=Mf("LAMBERT", base=(-0.5, 2.0, 1e20)))]
    return _write(tmp, "base_out", objs, cam(*STD_CAM))


# ---- degenerate transforms ----------------------------------------------------------------------
ZERO_SCALES = {"SPHERE": (0.0, 1.0, 1.0), "CUBE": (0.0, 0.0, 0.0), "CYLINDER": (1.0, 0.0, 1.0), "QUAD": (0.0, 1.0, 1.0),
               "CONE": (1.0, 1.0, 0.0), "PARABOLOID": (0.0, 1.0, 0.0), "DISK": (1.0, 1.0, 0.0)}


def scale_zero(tmp, shape):
    """REFUSED by the loader and by pt_set_scene (refused_by_loader below); the reference's source and
    the oracle still render it, and the CPU tests compare the two.  A zero scale: the inverse transform's rows hold inf and NaN, so the local ray, the roots and the
    hit distance are NaN, and `t <= tMin || t > tMax` accepts a NaN t.  Attacks quadric_roots' `disc <
    0`, prim_hit_rec's range tests, the slab tests' "both bounds are monotone and never NaN"
    (pt_dev_scene.h node_test_fast, pt_dev_walk.h slab_lo_x) once t_max is NaN, `rose = tMax > tLeaf`
    and normalize_dom(lp) on a "point on the unit sphere" that is NaN.  An ordinary floor and sphere
    share the BVH with the degenerate shape."""
    objs = [obj(shape, pos=(0.0, 0.2, 0.0), rot=(10.0, 20.0, 30.0), scale=ZERO_SCALES[shape],
                mat=Mf(base=(0.8, 0.5, 0.3), rough=0.4, metal=0.3)),
            floor(), obj("SPHERE", pos=(1.5, -0.5, 0.5), scale=(0.5, 0.5, 0.5), mat=Mf("GGX", rough=0.3, metal=1.0))]
    return _write(tmp, f"scale_zero_{shape}", objs, cam(*STD_CAM))


def scale_neg(tmp):
    """Mirrored cone, cube and paraboloid (negative scales): the normal's transform and the
    `dot(d, n) < 0` flip in surface_of under a transform of negative determinant."""
    objs = [floor(),
            obj("CONE", pos=(-1.5, 0.0, 0.0), rot=(15.0, 0.0, 10.0), scale=(-1.0, 1.0, 1.0), mat=Mf(rough=0.4, metal=0.3)),
            obj("CUBE", pos=(0.0, -0.4, 0.5), rot=(0.0, 25.0, 0.0), scale=(0.5, -0.5, 0.5), mat=Mf("GGX", rough=0.3, metal=1.0)),
            obj("PARABOLOID", pos=(1.5, 0.0, 0.0), rot=(0.0, 0.0, 160.0), scale=(-0.7, -1.0, -0.7),
                mat=Mf(base=(0.3, 0.8, 0.4), rough=0.5))]
    return _write(tmp, "scale_neg", objs, cam(*STD_CAM))


def scale_extreme(tmp):
    """Scales 1e-6 and 1e6, positions +-1e6, a rotation of 1e6 degrees: rcp_rn's and sqrt_rn's range
    guards in the intersection (disc up to ~1e24, q / a with a ~1e-12), the wave-uniform rcp_fast guard
    of traverse_cb_phase, the u, v of a hit 1e6 away in tex2d."""
    objs = [obj("QUAD", pos=(0.0, -1.0, 0.0), scale=(1e6, 1.0, 1e6), mat=Mf(rough=0.5, texture=CHECKER)),
            obj("SPHERE", pos=(0.0, 0.0, 0.0), scale=(1e-6, 1e-6, 1e-6), mat=Mf("GGX", rough=0.3, metal=1.0)),
            obj("SPHERE", pos=(1e6, 0.0, -1e6), scale=(1e6, 1e6, 1e6), mat=Mf(base=(0.8, 0.4, 0.4), rough=0.4)),
            obj("CYLINDER", pos=(-1e6, 0.0, -1e6), rot=(0.0, 0.0, 1e6), scale=(1e6, 1e6, 1e-6), mat=Mf("LAMBERT")),
            obj("CUBE", pos=(0.8, -0.5, 0.0), rot=(1e6, 1e6, 1e6), scale=(0.5, 0.5, 0.5), mat=Mf(base=(0.3, 0.5, 0.9))),
            obj("CONE", pos=(-0.8, 0.0, 0.0), scale=(0.5, 1.0, 1e-6), mat=Mf(rough=0.3, metal=0.6))]
    return _write(tmp, "scale_extreme", objs, cam(*STD_CAM))


def tangent_edge(tmp):
    """tangent_frame: "N unit, |up . N| < 0.999 or up = x: |up x N|^2 >= 0.001" (normalize_dom).
    Quads whose normals have |N.z| just below, at and above 0.999, and exactly 1."""
    tilt = math.degrees(math.acos(0.999))
    objs = [obj("QUAD", pos=(x, 0.0, -1.0), rot=(90.0, 0.0, 0.0 + t), scale=(0.45, 1.0, 0.8),
                mat=Mf(base=(0.8, 0.6, 0.4), rough=0.4, metal=0.4))
            for x, t in ((-1.5, tilt * 1.0001), (-0.5, tilt), (0.5, tilt * 0.9999), (1.5, 0.0))]
    return _write(tmp, "tangent_edge", [floor()] + objs, cam((0.0, 0.3, 4.0), (0.0, 0.0, 0.0), 45.0))


# ---- camera -------------------------------------------------------------------------------------
def cam_lookat_eq(tmp):
    """camera_ray's normalize and traverse_cb_phase's reciprocals on a camera whose position equals
    look_at: normalize(0) in the Camera constructor, every ray NaN."""
    return _write(tmp, "cam_lookat_eq", still_life(), cam((0.0, 0.5, 5.0), (0.0, 0.5, 5.0), 40.0))


def cam_along_up(tmp):
    """Looking straight down the up vector: cross(up, backward) = 0 in the Camera constructor, so right
    and up are NaN and every ray direction is NaN: NaN into rcp_fast, the slab selects, acos_sel and
    atan2_sel of the sky lookup.  (The tangent frame's own precondition, pt_math.h normalize_dom "the
    cross product of the up vector with a unit normal at least 0.001 away from it", is attacked with
    finite values by tangent_edge.)"""
    return _write(tmp, "cam_along_up", still_life(), cam((0.0, 5.0, 0.0), (0.0, 0.0, 0.0), 40.0))


FOVYS = (1e-4, 1e-6, 179.9, 180.0, -60.0)


def fovy(tmp, deg):
    """The camera's tan(fovy / 2): 1e-4 and 1e-6 degrees (every ray the same up to rounding, llc +
    u * horizontal cancels), 179.9 and 180 (tan ~1146 and ~-2.3e7 in float32), -60 (a mirrored image)."""
    return _write(tmp, f"fovy_{deg:g}", still_life(), cam(STD_CAM[0], STD_CAM[1], deg))


def cam_on_surface(tmp):
    """The camera on the floor quad's plane and on a sphere's surface: t = -o.y / d.y = +-0 against
    tMin, the sphere's `t0 > tMin ? t0 : t1` with t0 ~ 0 (the far-root rise of repair_pending)."""
    objs = still_life() + [obj("SPHERE", pos=(0.0, 0.0, 4.0), mat=Mf(rough=0.3, metal=0.5))]
    return _write(tmp, "cam_on_surface", objs, cam((0.0, -1.0, 3.0), (0.0, -0.5, 0.0), 60.0))


# ---- textures -----------------------------------------------------------------------------------
def sky_bright(tmp):
    """A sky whose texels carry the largest RGBE exponent (byte 255: 255 * 2^119 = 1.7e38): one sample
    is finite, the sum of a call's samples is inf, throughput 0 * inf and inf - inf follow in the
    next bounce's products.  Every fourth column is black, so lookups blend 1.7e38 with 0."""
    data = np.zeros((8, 16, 4), dtype=np.uint8)
    data[...] = (255, 128, 1, 255)
    data[:, ::4] = (0, 0, 0, 0)
    write_rgbe_raw(tmp / "sky_bright.hdr", data)
    objs = [floor(Mf(base=(0.0, 1.0, 0.5), rough=0.3, metal=1.0)),
            obj("SPHERE", mat=Mf("LAMBERT", base=(1.0, 0.0, 0.5)))]
    return kat.write_scene(tmp / "sky_bright.json", objs, cam(*STD_CAM), str(tmp / "sky_bright.hdr"))


def sky_1x1(tmp):
    """tex2d's wrap and clamp with width = height = 1: i0 in [-1, 0], i1 in [0, 1], both rows 0."""
    kat.write_rgbe(tmp / "sky_1x1.hdr", np.array([[[0.7, 0.9, 1.3]]]))
    return kat.write_scene(tmp / "sky_1x1.json", still_life(), cam(*STD_CAM), str(tmp / "sky_1x1.hdr"))


def hdr_texture(tmp):
    """An .hdr file as a material texture: taps above 1 (up to ~60) into pow_(., 2.2), base colours in
    the thousands."""
    kat.write_rgbe(tmp / "bright_tex.hdr", 20.0 * kat.sky_test_texture(32, 16))
    t = str(tmp / "bright_tex.hdr")
    objs = [floor(Mf(rough=0.4, metal=0.2, texture=t)),
            obj("SPHERE", pos=(-1.0, 0.0, 0.0), rot=(20.0, 40.0, 0.0), mat=Mf("LAMBERT", texture=t)),
            obj("CYLINDER", pos=(1.0, -0.3, 0.0), scale=(0.5, 0.7, 0.5), mat=Mf("GGX", rough=0.4, metal=1.0, texture=t)),
            obj("DISK", pos=(0.0, -0.2, 1.5), rot=(60.0, 0.0, 0.0), scale=(0.6, 1.0, 0.6), mat=Mf(rough=0.3, texture=t))]
    return _write(tmp, "hdr_texture", objs, cam(*STD_CAM))


# ---- one of each in one BVH ---------------------------------------------------------------------
def domain_combined(tmp):
    """One object of every accepted directed scene above in one BVH (14 primitives, several leaves),
    for the sweep over the kernel variants: the node-at-a-time walks (node_test_fast), the one-pass and
    the resumable child-box walks all meet roughness above 15 and 1e10 (NaN throughput), negative and
    huge colours, mirrored and extreme transforms next to ordinary neighbours.  (Zero scales are
    refused by the loader, so none is here.)"""
    kat.write_rgbe(tmp / "bright_tex.hdr", 20.0 * kat.sky_test_texture(32, 16))
    t = str(tmp / "bright_tex.hdr")
    objs = [floor(Mf(rough=16.0, metal=0.5)),
            obj("SPHERE", pos=(-3.0, 0.0, 0.0), mat=Mf(rough=1e10, metal=0.5)),
            obj("SPHERE", pos=(-1.5, 0.0, 0.0), scale=(0.6, 0.6, 0.6), mat=Mf("GGX", rough=2.0, metal=1.0)),
            obj("SPHERE", pos=(0.0, 0.0, 0.0), scale=(0.6, 0.6, 0.6), mat=Mf(rough=0.4, metal=3.0)),
            obj("CUBE", pos=(1.5, -0.5, 0.0), scale=(0.5, 0.5, 0.5), mat=Mf("GGX", rough=0.3, metal=-1.0)),
            obj("CYLINDER", pos=(3.0, -0.5, 0.0), scale=(0.4, 0.5, 0.4), mat=Mf("LAMBERT", base=(-0.5, 2.0, 1e20))),
            obj("SPHERE", pos=(-3.0, 1.5, -2.0), scale=(0.5, 0.5, 0.5),
                mat=Mf("LAMBERT", base=(5.0, 5.0, 5.0), emissive=(1e38, 1e38, -1e38))),
            obj("CONE", pos=(1.5, 0.0, 2.0), scale=(-0.5, 0.5, 0.5), mat=Mf(rough=0.4, metal=0.3)),
            obj("PARABOLOID", pos=(3.0, 0.0, 2.0), rot=(0.0, 0.0, 160.0), scale=(-0.5, -0.7, -0.5), mat=Mf(rough=0.5)),
            obj("SPHERE", pos=(0.5, -0.9, 3.0), scale=(1e-6, 1e-6, 1e-6), mat=Mf("GGX", rough=0.3, metal=1.0)),
            obj("SPHERE", pos=(1e6, 0.0, -1e6), scale=(1e6, 1e6, 1e6), mat=Mf(base=(0.8, 0.4, 0.4), rough=0.4)),
            obj("CUBE", pos=(-0.8, -0.6, 3.0), rot=(1e6, 1e6, 1e6), scale=(0.3, 0.3, 0.3), mat=Mf(base=(0.3, 0.5, 0.9))),
            obj("QUAD", pos=(0.0, 0.5, -3.0), rot=(90.0, 0.0, math.degrees(math.acos(0.999))), scale=(2.0, 1.0, 1.0),
                mat=Mf(rough=0.4, metal=0.4, texture=t)),
            obj("DISK", pos=(2.0, -0.8, 3.0), scale=(0.5, 1.0, 0.5), mat=Mf(rough=0.3, texture=CHECKER))]
    return _write(tmp, "domain_combined", objs, cam((0.5, 1.5, 8.0), (0.0, 0.3, 0.0), 50.0))


ALL_SHAPES = ["SPHERE", "CYLINDER", "DISK", "CONE", "PARABOLOID", "QUAD", "CUBE"]

DIRECTED = {
    "rough_normal_16": lambda tmp: rough_normal(tmp, 16.0),
    "rough_normal_64": lambda tmp: rough_normal(tmp, 64.0),
    "rough_normal_14": lambda tmp: rough_normal(tmp, 14.0),
    "ggx_rough_normal": ggx_rough_normal,
    "rough_spheres_2": lambda tmp: rough_spheres(tmp, 2.0),
    "rough_spheres_1e10": lambda tmp: rough_spheres(tmp, 1e10),
    "metal_out": metal_out,
    "base_out": base_out,
}
for _s in ALL_SHAPES:
    DIRECTED[f"scale_zero_{_s}"] = (lambda tmp, s=_s: scale_zero(tmp, s))
DIRECTED.update(scale_neg=scale_neg, scale_extreme=scale_extreme, tangent_edge=tangent_edge, cam_lookat_eq=cam_lookat_eq,
                cam_along_up=cam_along_up)
for _f in FOVYS:
    DIRECTED[f"fovy_{_f:g}"] = (lambda tmp, f=_f: fovy(tmp, f))
DIRECTED.update(cam_on_surface=cam_on_surface, sky_bright=sky_bright, sky_1x1=sky_1x1, hdr_texture=hdr_texture,
                domain_combined=domain_combined)

ROUGH_NAN = ("rough_normal_16", "rough_normal_64", "ggx_rough_normal", "rough_spheres_1e10")   # NaN from roughness alone
ZERO_SCALE = tuple(f"scale_zero_{s}" for s in ALL_SHAPES)


def refused_by_loader(path):
    """Index of the first object the loader refuses, or None.  The rule: the inverse
    transform must be finite, i.e. 1 / s must be a finite float32 for every scale component s the
    shape uses -- |s| > 2^-128 -- where a disk's and a quad's y scale is overridden and unused."""
    import json
    with np.errstate(all="ignore"):
        for i, o in enumerate(json.loads(pathlib.Path(path).read_text()).get("objects", [])):
            sc = [np.float32(v) for v in o.get("scale", [1.0, 1.0, 1.0])]
            used = (sc[0], sc[2]) if o.get("type") in ("DISK", "QUAD") else sc
            if not all(np.isfinite(np.float32(1.0) / v) for v in used):
                return i
    return None


def without_refused_objects(path):
    """The scene without the objects the loader refuses, written next to it, or None when no object is
    left: what remains of a refused random scene still goes through the kernel."""
    import json
    path = pathlib.Path(path)
    j = json.loads(path.read_text())
    keep = []
    for o in j["objects"]:
        j1 = dict(j, objects=[o])
        probe = path.with_name(path.stem + ".probe.json")
        probe.write_text(json.dumps(j1))
        if refused_by_loader(probe) is None:
            keep.append(o)
    if not keep:
        return None
    out = path.with_name(path.stem + ".accepted.json")
    out.write_text(json.dumps(dict(j, objects=keep)))
    return out


def directed_scene(tmp: pathlib.Path, name: str) -> pathlib.Path:
    """The named directed scene, written into tmp, in the form every layer is given."""
    return drop_unset_uv_textures(DIRECTED[name](tmp))


# ---- seeded random scenes -----------------------------------------------------------------------
# Each field is an edge value with the stated probability, else ordinary.
POOL = {
    "count": (1, 2, 3, 4, 5, 8, 9, 17),                       # around the leaf size 4
    "scale": ((0.0, -1.0, 1e-6, 1e3, -0.0), 0.3, (0.2, 2.0)),
    "position": ((0.0, 1e4, -1e4, 1e-30), 0.1, (-3.0, 3.0)),
    "rotation": ((0.0, 90.0, 180.0, 360.0, 1e6, -90.0), 0.3, (-180.0, 180.0)),
    "base": ((0.0, 1.0, -0.5, 4.0, 1e20), 0.2, (0.05, 0.95)),
    "roughness": ((0.0, 0.04, 1.0, 2.0, 16.0, 64.0, 1e10, -1.0), 0.3, (0.05, 1.0)),
    "metalness": ((0.0, 1.0, -1.0, 3.0), 0.3, (0.0, 1.0)),
    "emission": ((1.0, 1e38, -1.0, 1e-40), 0.1, (0.0, 0.0)),
    "fovy": ((1e-4, 179.9, 0.2), 0.15, (20.0, 90.0)),
}
TEXTURE_P = 0.2
SEEDS_CPU = range(256)
SEEDS_GPU = range(128)


def random_scene(tmp: pathlib.Path, seed: int, draws: collections.Counter = None) -> pathlib.Path:
    """The seed's scene, written into tmp.  `draws` counts which edge value of which field was drawn,
    keyed (field, repr(value))."""
    rng = np.random.default_rng(seed)
    draws = draws if draws is not None else collections.Counter()

    def field(name):
        edges, p, (lo, hi) = POOL[name]
        if rng.random() < p:
            v = float(edges[int(rng.integers(len(edges)))])
            draws[(name, repr(v))] += 1
            return v
        return float(np.float32(rng.uniform(lo, hi)))

    def vec(name):
        return tuple(field(name) for _ in range(3))

    n = int(POOL["count"][int(rng.integers(len(POOL["count"])))])
    draws[("count", repr(n))] += 1
    objs = []
    for _ in range(n):
        shape = ALL_SHAPES[int(rng.integers(7))]
        mtype = ("LAMBERT", "GGX", "LAMBERT_GGX")[int(rng.integers(3))]
        mat = Mf(mtype, base=vec("base"), rough=field("roughness"), metal=field("metalness"), emissive=vec("emission"),
                 texture=CHECKER if rng.random() < TEXTURE_P else "")
        objs.append(obj(shape, pos=vec("position"), rot=vec("rotation"), scale=vec("scale"), mat=mat))
    pos = (rng.uniform(-4.0, 4.0), rng.uniform(-1.0, 4.0), rng.uniform(2.0, 7.0))
    look = tuple(rng.uniform(-0.5, 0.5, 3))
    path = _write(tmp, f"random_{seed}", objs, cam(pos, look, field("fovy")))
    return drop_unset_uv_textures(path)


def every_edge_value():
    """(field, repr(value)) of every edge value of the pool."""
    keys = [("count", repr(n)) for n in POOL["count"]]
    for name, spec in POOL.items():
        if name != "count":
            keys += [(name, repr(float(v))) for v in spec[0]]
    return keys
