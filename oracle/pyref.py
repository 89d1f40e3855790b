"""ctypes driver for the reference's own source compiled for the host (oracle/_ref/libptref.so,
built by `make -C oracle ref` from oracle/ref_wrap.cpp).  TEST INFRASTRUCTURE ONLY.

Where pyoracle.py drives a restatement of the reference, this drives the reference's code itself:
CpuHittable's constructor, BVH::build, Camera, hitBVH, getColor, traceKernel, tonemap.  Scene files are
parsed by pyoracle.parse_scene, so both receive the same float32 inputs.  The library is built where
a checkout of the reference is present and is loaded as it stands elsewhere.
"""
from __future__ import annotations

import ctypes as C
import os
import pathlib
from typing import Optional

import numpy as np

from . import pyoracle as po

HERE = pathlib.Path(__file__).resolve().parent
LIB_PATH = HERE / "_ref" / "libptref.so"

# The reference leaves u and v unset in hitCone, hitParaboloid and hitBox (Hittable.inl:237-297,
# 331-358), so a texture on one of these reads indeterminate coordinates there.
UV_UNSET_TYPES = (po.SHAPES.index("CONE"), po.SHAPES.index("PARABOLOID"), po.SHAPES.index("CUBE"))


def reference_tree() -> Optional[pathlib.Path]:
    """The checkout `make` builds from: $REF, or `reference` next to this repository."""
    root = pathlib.Path(os.environ.get("REF") or HERE.parent.parent / "reference")
    return root if (root / "PathtracerCUDA" / "src" / "pathtracer" / "kernels" / "trace.cu").exists() else None


def available() -> bool:
    return LIB_PATH.exists()


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise RuntimeError(f"{LIB_PATH} missing: run `make -C oracle ref REF=<reference checkout>`")
        po.lib()                                   # liboracle.so first: libptref.so takes its symbols from it
        L = C.CDLL(str(LIB_PATH))
        f, u32, vp = C.c_float, C.c_uint32, C.c_void_p
        P = C.POINTER
        L.ref_sizeof.restype = u32
        L.ref_sizeof.argtypes = [C.c_int]
        L.ref_scene_create.restype = vp
        L.ref_scene_create.argtypes = [u32, P(u32), P(f), P(f), P(f), P(u32), P(f), P(f), P(f), P(f), P(u32)]
        L.ref_scene_free.argtypes = [vp]
        L.ref_scene_node_count.restype = u32
        L.ref_scene_node_count.argtypes = [vp]
        L.ref_scene_validate.restype = C.c_int
        L.ref_scene_validate.argtypes = [vp]
        L.ref_scene_depth.restype = u32
        L.ref_scene_depth.argtypes = [vp]
        L.ref_scene_objects.argtypes = [vp, vp, P(f)]
        L.ref_scene_bvh.argtypes = [vp, vp, vp, P(f)]
        L.ref_scene_set_textures.argtypes = [vp, u32, P(po.Texture), u32]
        L.ref_camera_make.argtypes = [P(f), P(f), P(f), f, f, vp]
        L.ref_camera_rotate.argtypes = [vp, f, f, f]
        L.ref_camera_translate.argtypes = [vp, f, f, f]
        L.ref_init_rand_state.argtypes = [u32, u32, vp]
        L.ref_render.argtypes = [vp, vp, u32, u32, P(f), vp, u32, C.c_int, u32]
        L.ref_tonemap.argtypes = [P(f), u32, u32, u32, P(C.c_uint8)]
        for which in range(7):
            if which != 2:                         # CpuHittable never crosses the ABI
                assert L.ref_sizeof(which) == po.lib().or_sizeof(which), f"layout {which} differs from the oracle's"
        _lib = L
    return _lib


def drop_unset_uv_textures(si: po.SceneInputs) -> po.SceneInputs:
    """Take the texture off every cone, paraboloid and cube, in place: the reference never sets their
    u, v.  What the oracle and the kernel do for a textured one stays covered by their own tests."""
    for i, t in enumerate(si.types):
        if t in UV_UNSET_TYPES:
            si.texture_handles[i] = 0
    return si


def _f32(rows) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(rows, dtype=np.float32).reshape(-1))


def _u32(vals) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(vals, dtype=np.uint32))


def make_camera(position, look_at, fovy_radians: float, aspect: float, up=(0.0, 1.0, 0.0)) -> po.Camera:
    cam = po.Camera()
    lib().ref_camera_make(po.f3(position), po.f3(look_at), po.f3(up), fovy_radians, aspect, C.byref(cam))
    return cam


def camera_rotate(cam: po.Camera, pitch: float, yaw: float, roll: float = 0.0) -> po.Camera:
    lib().ref_camera_rotate(C.byref(cam), pitch, yaw, roll)
    return cam


def camera_translate(cam: po.Camera, x: float, y: float, z: float) -> po.Camera:
    lib().ref_camera_translate(C.byref(cam), x, y, z)
    return cam


class RefScene:
    """A scene built by the reference's constructors and BVH::build(count, elements, 4)."""

    def __init__(self, si: po.SceneInputs, width: int, height: int) -> None:
        L = lib()
        for i, t in enumerate(si.types):
            if t in UV_UNSET_TYPES and si.texture_handles[i] != 0:
                raise ValueError("textured cone, paraboloid or cube: the reference reads unset u, v there "
                                 "(drop_unset_uv_textures)")
        self.inputs = si
        self.count = len(si)
        self._h = None
        self.node_count = 0
        if self.count:
            arrs = [_u32(si.types), _f32(si.positions), _f32(si.rotations), _f32(si.scales), _u32(si.material_types),
                    _f32(si.base_colors), _f32(si.emissives), _f32(si.roughness), _f32(si.metalness),
                    _u32(si.texture_handles)]
            ptrs = [a.ctypes.data_as(C.POINTER(C.c_uint32 if a.dtype == np.uint32 else C.c_float)) for a in arrs]
            self._h = C.c_void_p(L.ref_scene_create(self.count, *ptrs))
            self.node_count = int(L.ref_scene_node_count(self._h))
            self._tex = (po.Texture * max(1, len(si.textures)))()
            for i, t in enumerate(si.textures):
                self._tex[i].width, self._tex[i].height, self._tex[i].texels = t.shape[1], t.shape[0], po.fptr(t)
            L.ref_scene_set_textures(self._h, len(si.textures), self._tex, si.skybox)
        self.camera = make_camera(si.camera_position, si.camera_look_at, si.camera_fovy, po.aspect_of(width, height))

    def __del__(self) -> None:
        if getattr(self, "_h", None):
            lib().ref_scene_free(self._h)
            self._h = None

    def validate(self) -> bool:
        return bool(lib().ref_scene_validate(self._h))

    def depth(self) -> int:
        return int(lib().ref_scene_depth(self._h))

    def objects(self):
        """(count x 96 bytes, count x 6 float32) in file order: hittables and their boxes."""
        h = np.zeros((self.count, 96), dtype=np.uint8)
        a = np.zeros((self.count, 6), dtype=np.float32)
        lib().ref_scene_objects(self._h, h.ctypes.data, po.fptr(a))
        return h, a

    def bvh(self):
        """(nodes x 32 bytes, count x 96 bytes, count x 6 float32): the nodes, and the hittables and
        boxes in the order the build left them."""
        n = np.zeros((self.node_count, 32), dtype=np.uint8)
        h = np.zeros((self.count, 96), dtype=np.uint8)
        a = np.zeros((self.count, 6), dtype=np.float32)
        lib().ref_scene_bvh(self._h, n.ctypes.data, h.ctypes.data, po.fptr(a))
        return n, h, a


def load_scene(path: os.PathLike, width: int, height: int) -> RefScene:
    """Parse with pyoracle.parse_scene, drop the textures the reference cannot address, build."""
    return RefScene(drop_unset_uv_textures(po.parse_scene(path)), width, height)


class RefRenderer:
    """The per-pixel state of the reference's Pathtracer: accumulation buffer, curandState, frame
    counter.  render() is one Pathtracer::render call."""

    def __init__(self, scene: RefScene, width: int, height: int) -> None:
        self.scene = scene
        self.width, self.height = width, height
        self.accum = np.zeros((height, width, 4), dtype=np.float32)
        self.rng = np.zeros((height, width, 6), dtype=np.uint32)
        lib().ref_init_rand_state(width, height, self.rng.ctypes.data)
        self.frames = 0

    def render(self, camera: po.Camera, spp: int, ignore_history: bool) -> None:
        if ignore_history:
            self.frames = 0
        if self.scene.count and spp:
            lib().ref_render(self.scene._h, C.byref(camera), self.width, self.height, po.fptr(self.accum),
                             self.rng.ctypes.data, spp, int(bool(ignore_history)), self.frames)
        self.frames += 1

    def rng_array(self) -> np.ndarray:
        return self.rng

    def tonemap(self, frames: Optional[int] = None) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        lib().ref_tonemap(po.fptr(self.accum), self.width, self.height, self.frames if frames is None else frames,
                          out.ctypes.data_as(C.POINTER(C.c_uint8)))
        return out
