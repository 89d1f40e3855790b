"""Edge scenes for the comparison with the reference's own source (tests/test_ref_source.py,
tests/test_gpu_ref_source.py): the places where an intersection routine, a transform, the BVH or a
material can go wrong without the shipped scenes noticing.

Each builder writes one JSON scene into a directory with the helpers of tests/kat.py and returns
its path.  Every scene uses the synthetic sky of kat.py, and scenes/checker.png where it needs a
texture.  All are meant for 48 x 32 pixels.
"""
from __future__ import annotations

import copy
import json
import pathlib

import kat

ROOT = pathlib.Path(__file__).resolve().parents[1]
CHECKER = str(ROOT / "scenes" / "checker.png")
W, H = 48, 32

UV_UNSET = ("CONE", "PARABOLOID", "CUBE")     # hitCone, hitParaboloid, hitBox leave u, v unset


def M(mtype="LAMBERT_GGX", base=(0.8, 0.8, 0.8), rough=0.5, metal=0.0, emissive=(0.0, 0.0, 0.0), texture=""):
    m = kat.material(mtype, base=base, rough=rough, metal=metal, emissive=emissive)
    m["texture"] = texture
    return m


def cam(position, look_at, fovy):
    return {"position": [float(x) for x in position], "look_at": [float(x) for x in look_at], "fovy": float(fovy)}


def shifted(objects, d):
    out = copy.deepcopy(objects)
    for o in out:
        o["position"] = [p + q for p, q in zip(o["position"], d)]
    return out


def _write(tmp: pathlib.Path, name: str, objects, camera) -> pathlib.Path:
    sky = tmp / "edge_sky.hdr"
    if not sky.exists():
        kat.write_rgbe(sky, kat.sky_test_texture())
    return kat.write_scene(tmp / f"{name}.json", objects, camera, str(sky))


def drop_unset_uv_textures(path: pathlib.Path, out_dir: pathlib.Path = None) -> pathlib.Path:
    """Copy of the scene with the texture taken off every cone, paraboloid and cube: the reference
    leaves u and v unset for these (Hittable.inl hitCone, hitParaboloid, hitBox), so a texture on one
    reads indeterminate values in its code.  Texture and sky paths are made absolute, so the copy
    works from any directory; it is written next to the scene, or into out_dir.  Every scene, shipped
    ones included, goes through this before it reaches the reference's code."""
    path = pathlib.Path(path)
    j = json.loads(path.read_text())

    def absolute(p):
        if p and not pathlib.Path(p).is_absolute() and (path.parent / p).exists():
            return str(path.parent / p)
        return p

    for o in j.get("objects", []):
        m = o.get("material", {})
        if isinstance(m.get("texture"), str):
            m["texture"] = "" if o.get("type") in UV_UNSET else absolute(m["texture"])
    if isinstance(j.get("skybox"), str):
        j["skybox"] = absolute(j["skybox"])
    out = (out_dir or path.parent) / (path.name.replace(".json", "") + ".nouv.json")
    out.write_text(json.dumps(j))
    return out


# ---- inside: the camera sits inside the shape ---------------------------------------------------
# Far roots (t0 <= tMin < t1), back faces through setFaceNormal, the `t0 > tMin ? t0 : t1` and
# `hitPointValid0 ? t0 : t1` choices.  The shape glows faintly and a small lamp sits inside it, so every
# bounce adds light and the closed shapes are not black.  (From inside, the cube's AABB::intersect
# returns t = tMin, so a path there creeps forward 0.001 per bounce: the reference's behaviour.)
def inside(tmp, shape):
    glow = (0.15, 0.2, 0.25)
    lamp = kat.obj("SPHERE", pos=(0.6, 0.7, 0.3), scale=(0.1, 0.1, 0.1), mat=M("LAMBERT", emissive=(8.0, 7.0, 6.0)))
    if shape in ("DISK", "QUAD"):
        # inside the slab |y| <= 0.01 that bounds a flat shape, looking nearly along it
        objs = [kat.obj(shape, scale=(3.0, 1.0, 3.0), mat=M(rough=0.3, metal=0.5, emissive=glow)), lamp]
        return _write(tmp, f"inside_{shape}", objs, cam((0.1, 0.005, 0.2), (1.0, 0.3, 0.4), 70.0))
    objs = [kat.obj(shape, scale=(2.0, 2.0, 2.0), rot=(0.0, 20.0, 0.0), mat=M(rough=0.4, metal=0.3, emissive=glow)), lamp]
    return _write(tmp, f"inside_{shape}", objs, cam((0.1, 0.8, 0.1), (1.0, 0.9, 0.6), 80.0))


# ---- axis: degenerate directions ----------------------------------------------------------------
def axis(tmp, shape):
    if shape in ("DISK", "QUAD"):
        # edge-on: local dir.y near 0 on every ray, both signs, t = -o.y / d.y large
        objs = [kat.obj(shape, scale=(2.0, 1.0, 2.0), mat=M(rough=0.3)),
                kat.obj("SPHERE", pos=(0.0, -1.5, 0.0), mat=M("LAMBERT", base=(0.7, 0.2, 0.2)))]
        return _write(tmp, f"axis_{shape}", objs, cam((0.0, 1e-3, 5.0), (0.0, 1e-3, 0.0), 25.0))
    # the shape's local y axis lies along world z; the camera looks down it from 1e-3 off axis, so the
    # quadratic's `a` is near 0 and q / a is large
    objs = [kat.obj(shape, rot=(90.0, 0.0, 0.0), mat=M(rough=0.3, metal=0.2)),
            kat.obj("QUAD", pos=(0.0, -1.2, 0.0), scale=(4.0, 1.0, 4.0), mat=M("LAMBERT", base=(0.3, 0.6, 0.3)))]
    return _write(tmp, f"axis_{shape}", objs, cam((1e-3, 0.0, 5.0), (1e-3, 0.0, 0.0), 30.0))


# ---- transforms ---------------------------------------------------------------------------------
def transform_objects(c=(0.0, 0.0, 0.0)):
    """All seven shapes: rotations about all three axes at once at angles that are no multiple of 90
    degrees, non-uniform scales from 1e-3 to 1e3, a disk and a quad whose y scale is not 1 (the
    constructor overrides it)."""
    objs = [
        kat.obj("SPHERE", pos=(-3.0, 0.0, 0.0), rot=(33.0, 47.0, 71.0), scale=(1.5, 0.7, 1.1), mat=M(base=(0.9, 0.3, 0.3))),
        kat.obj("CYLINDER", pos=(0.0, 0.0, -2.0), rot=(-21.0, 64.0, 38.0), scale=(1e-3, 1.0, 0.8), mat=M("GGX", rough=0.3, metal=1.0)),
        kat.obj("CONE", pos=(3.0, 0.0, 0.0), rot=(17.0, -53.0, 29.0), scale=(0.9, 1.3, 0.6), mat=M(base=(0.3, 0.9, 0.3))),
        kat.obj("PARABOLOID", pos=(0.0, 2.0, 0.0), rot=(101.0, 13.0, -77.0), scale=(0.7, 1.2, 0.9), mat=M(base=(0.3, 0.3, 0.9))),
        kat.obj("CUBE", pos=(-2.0, -2.0, 1.0), rot=(12.0, 34.0, 56.0), scale=(1.0, 0.3, 0.6), mat=M("LAMBERT", base=(0.9, 0.9, 0.2))),
        kat.obj("DISK", pos=(2.0, -2.0, 0.0), rot=(40.0, -15.0, 25.0), scale=(1.2, 7.0, 0.8), mat=M(rough=0.2, metal=0.7)),
        kat.obj("QUAD", pos=(0.0, -3.0, 0.0), rot=(5.0, 10.0, -8.0), scale=(1e3, 0.25, 1e3), mat=M(rough=0.6)),
        kat.obj("SPHERE", pos=(0.0, 0.0, -50.0), rot=(10.0, 20.0, 30.0), scale=(1e3, 30.0, 1e-3), mat=M("LAMBERT", base=(0.5, 0.5, 0.7))),
        kat.obj("CUBE", pos=(1.0, 1.0, 2.0), rot=(-65.0, 5.0, 130.0), scale=(1e-3, 0.5, 0.5), mat=M("GGX", rough=0.1, metal=1.0)),
    ]
    return shifted(objs, c)


def transforms(tmp):
    c = (1e4, 0.0, 0.0)                         # 1e4 from the origin
    return _write(tmp, "transforms", transform_objects(c), cam((c[0], 1.0, 9.0), c, 50.0))


# ---- ties ---------------------------------------------------------------------------------------
def tie_objects():
    red, blue = M("LAMBERT", base=(0.9, 0.1, 0.1)), M("GGX", base=(0.1, 0.1, 0.9), rough=0.3, metal=1.0)
    green, grey = M("LAMBERT", base=(0.1, 0.9, 0.1)), M(rough=0.5)
    return [
        # coplanar, coincident quads and disks with different materials: the later one never wins
        kat.obj("QUAD", scale=(2.5, 1.0, 2.5), mat=red),
        kat.obj("QUAD", scale=(2.5, 1.0, 2.5), mat=blue),
        kat.obj("DISK", pos=(-1.5, 0.5, 0.0), mat=green),
        kat.obj("DISK", pos=(-1.5, 0.5, 0.0), mat=blue),
        # a cube whose top face coincides with a quad
        kat.obj("CUBE", pos=(1.5, 0.5, 0.0), scale=(0.5, 0.5, 0.5), mat=grey),
        kat.obj("QUAD", pos=(1.5, 1.0, 0.0), scale=(0.5, 1.0, 0.5), mat=green),
        # two spheres touching in one point
        kat.obj("SPHERE", pos=(-0.5, 1.5, -1.0), scale=(0.5, 0.5, 0.5), mat=grey),
        kat.obj("SPHERE", pos=(0.5, 1.5, -1.0), scale=(0.5, 0.5, 0.5), mat=blue),
        # two surfaces 5e-4 apart, below tMin = 0.001: a bounce off the lower one skips the upper one
        kat.obj("QUAD", pos=(0.0, 0.3, 1.5), scale=(0.7, 1.0, 0.7), mat=grey),
        kat.obj("QUAD", pos=(0.0, 0.3005, 1.5), scale=(0.7, 1.0, 0.7), mat=red),
        # four primitives close together and far from the rest: one BVH leaf of four
        kat.obj("SPHERE", pos=(-2.2, 0.2, 2.0), scale=(0.1, 0.1, 0.1), mat=green),
        kat.obj("CYLINDER", pos=(-2.0, 0.2, 2.0), scale=(0.1, 0.1, 0.1), mat=red),
        kat.obj("CONE", pos=(-2.2, 0.2, 2.2), scale=(0.1, 0.1, 0.1), mat=blue),
        kat.obj("PARABOLOID", pos=(-2.0, 0.2, 2.2), scale=(0.1, 0.1, 0.1), mat=grey),
    ]


def ties(tmp):
    # the camera's target lies on the cube's upper front edge (the normal rule's `>` ties)
    return _write(tmp, "ties", tie_objects(), cam((0.0, 2.5, 6.0), (1.5, 1.0, 0.5), 45.0))


# ---- rim: hits exactly on a boundary -------------------------------------------------------------
def rim(tmp):
    """The disk ends at `x*x + z*z >= 1.0f` and the quad at `fabsf(x) > 1.0f`: the two differ from their
    neighbours `>` and `>=` only for a hit exactly on the rim, which a jittered ray all but never
    produces.  Both shapes are 1e-4 wide and seen from 120 away along all three axes, so in local space
    the origin's x and z and the products d * t are all near 1.2e6, where a float's step is 1/8; their
    sum is exact, so every hit point lies on a 1/8 grid, and a few per cent of the hits on the disk land
    exactly on (+-1, 0) or (0, +-1), and of those on the quad exactly on an edge.  (The y scale stays 1:
    the boxes keep a y extent the traversal can resolve at that distance.)  A cube of the same size
    stands beside them: hits exactly on a cube edge, where the normal rule's `>` comparisons tie.  And
    the far wall of a cylinder of radius 1 and height 1e-4 crosses the frame, seen through its open
    top: there the local height is on the 1/8 grid and lands exactly on the limit `<= 1.0f`."""
    objs = [kat.obj("DISK", scale=(1e-4, 1.0, 1e-4), mat=M("LAMBERT", base=(0.9, 0.2, 0.2), emissive=(0.5, 0.1, 0.1))),
            kat.obj("QUAD", pos=(3e-4, 0.0, 0.0), scale=(1e-4, 1.0, 1e-4),
                    mat=M("LAMBERT", base=(0.2, 0.9, 0.2), emissive=(0.1, 0.5, 0.1))),
            kat.obj("CUBE", pos=(-3e-4, 0.0, 0.0), scale=(1e-4, 1e-4, 1e-4),
                    mat=M("LAMBERT", base=(0.2, 0.2, 0.9), emissive=(0.1, 0.1, 0.5))),
            kat.obj("CYLINDER", pos=(1.0006, 0.0, 0.0), scale=(1.0, 1e-4, 1.0),
                    mat=M("LAMBERT", base=(0.9, 0.9, 0.2), emissive=(0.4, 0.4, 0.1)))]
    return _write(tmp, "rim", objs, cam((120.0, 120.0, 120.0), (1.5e-4, 0.0, 0.0), 2.2e-4))


# ---- materials ----------------------------------------------------------------------------------
def material_objects():
    mats = [
        M("GGX", rough=0.0, metal=1.0),                       # roughness 0, clamped to 0.04
        M("GGX", rough=1.0, metal=1.0),
        M("GGX", base=(0.9, 0.6, 0.2), rough=0.4, metal=0.0),
        M("GGX", base=(0.9, 0.6, 0.2), rough=0.4, metal=0.5),
        M("GGX", base=(0.9, 0.6, 0.2), rough=0.4, metal=1.0),
        M("LAMBERT_GGX", base=(0.2, 0.6, 0.9), rough=0.4, metal=0.0),
        M("LAMBERT_GGX", base=(0.2, 0.6, 0.9), rough=0.4, metal=0.5),
        M("LAMBERT_GGX", base=(0.2, 0.6, 0.9), rough=0.4, metal=1.0),
        M("LAMBERT", base=(0.0, 0.0, 0.0)),                   # attenuation == 0 ends the path
        M("LAMBERT_GGX", base=(0.0, 0.0, 0.0), rough=0.0, metal=1.0),
        M("LAMBERT", base=(0.0, 0.0, 0.0), emissive=(3.0, 2.0, 1.0)),   # emissive, base colour 0
        M("LAMBERT_GGX", rough=1.0, metal=0.0),
    ]
    objs = [kat.obj("QUAD", scale=(100.0, 1.0, 100.0), mat=M("LAMBERT_GGX", rough=0.2, metal=0.5))]
    for i, m in enumerate(mats):
        objs.append(kat.obj("SPHERE", pos=(-4.4 + 0.8 * i, 0.38, 0.3 * (i % 3)), scale=(0.38, 0.38, 0.38), mat=m))
    return objs


def materials(tmp):
    return _write(tmp, "materials", material_objects(), cam((0.0, 1.6, 6.5), (0.0, 0.3, 0.0), 60.0))


def materials_grazing(tmp):
    # the LAMBERT_GGX floor seen at a grazing angle with the sky on
    return _write(tmp, "materials_grazing", material_objects(), cam((0.0, 0.02, 6.5), (0.0, 0.0, 0.0), 60.0))


# ---- textured -----------------------------------------------------------------------------------
def textured(tmp):
    """Textures on every shape.  SPHERE, CYLINDER, DISK and QUAD have u, v mappings in the reference;
    CONE, PARABOLOID and CUBE do not, and lose their texture in drop_unset_uv_textures()."""
    t = dict(texture=CHECKER)
    objs = [
        kat.obj("QUAD", pos=(0.0, -1.0, 0.0), rot=(0.0, 30.0, 0.0), scale=(6.0, 1.0, 6.0), mat=M(rough=0.5, **t)),
        kat.obj("SPHERE", pos=(-2.5, 0.0, 0.0), rot=(20.0, 40.0, 60.0), scale=(1.0, 0.8, 1.0), mat=M("LAMBERT", **t)),
        kat.obj("CYLINDER", pos=(0.0, 0.0, 0.0), rot=(15.0, 25.0, -35.0), scale=(0.7, 1.0, 0.7), mat=M("GGX", rough=0.4, metal=1.0, **t)),
        kat.obj("DISK", pos=(2.5, 0.0, 0.0), rot=(70.0, 10.0, 20.0), scale=(1.0, 1.0, 0.8), mat=M(rough=0.3, metal=0.5, **t)),
        kat.obj("CONE", pos=(-1.5, 0.0, 2.0), rot=(10.0, 0.0, 15.0), scale=(0.5, 0.5, 0.5), mat=M(**t)),
        kat.obj("PARABOLOID", pos=(0.5, -0.5, 2.0), rot=(0.0, 33.0, -20.0), scale=(0.5, 0.8, 0.5), mat=M(**t)),
        kat.obj("CUBE", pos=(2.0, -0.5, 2.0), rot=(0.0, 25.0, 0.0), scale=(0.5, 0.5, 0.5), mat=M("LAMBERT", **t)),
    ]
    return _write(tmp, "textured", objs, cam((0.0, 2.0, 7.0), (0.0, -0.2, 0.0), 50.0))


# ---- everything in one BVH ----------------------------------------------------------------------
def combined(tmp):
    """All seven shapes under general transforms, the ties and the material set in one BVH."""
    objs = tie_objects() + shifted(material_objects()[1:], (0.0, 0.0, 3.0)) + transform_objects((0.0, 4.0, -4.0))
    return _write(tmp, "combined", objs, cam((0.5, 3.0, 9.0), (0.0, 1.2, 0.0), 60.0))


ALL_SHAPES = ["SPHERE", "CYLINDER", "DISK", "CONE", "PARABOLOID", "QUAD", "CUBE"]

EDGE_SCENES = {}
for _s in ALL_SHAPES:
    EDGE_SCENES[f"inside_{_s}"] = (lambda tmp, s=_s: inside(tmp, s))
for _s in ("CYLINDER", "CONE", "PARABOLOID", "DISK", "QUAD"):
    EDGE_SCENES[f"axis_{_s}"] = (lambda tmp, s=_s: axis(tmp, s))
EDGE_SCENES.update(transforms=transforms, ties=ties, rim=rim, materials=materials, materials_grazing=materials_grazing,
                   textured=textured, combined=combined)


def edge_scene(tmp: pathlib.Path, name: str) -> pathlib.Path:
    """The named edge scene, written into tmp, in the form every layer is given (see
    drop_unset_uv_textures)."""
    return drop_unset_uv_textures(EDGE_SCENES[name](tmp))
