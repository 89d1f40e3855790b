"""MI355X-native path tracer with the capabilities of DoerriesT/PathtracerCUDA's hot path.

Python mirror of the reference's host interface (PathtracerCUDA/src/pathtracer/Pathtracer.h:12-68,
SceneLoader.h, Camera.h) over the native libraries:

    pt = Pathtracer(width, height)            # Pathtracer(w, h)            Pathtracer.cpp:30
    cam = pt.load_scene("scene.json")         # loadScene(pt, params)        SceneLoader.cpp:124
    pt.render(cam, 8, ignore_history=True)    # render(camera, spp, ignore)  Pathtracer.cpp:162
    ms = pt.get_timing()                      # getTiming()                  Pathtracer.cpp:229
    hdr = pt.get_hdr_image_data()             # getHDRImageData()            Pathtracer.cpp:299
    rgba8 = pt.get_image_data()               # getImageData()               Pathtracer.cpp:317

All rendering runs in hand-written HIP kernels for gfx950 (libpt_hip.so); scene loading, the SAH
BVH and frame accounting run in host C++ (libpt_host.so).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Sequence

import numpy as np

from . import _native as N
from ._native import PathtracerError, PtBvhNode, PtCamera, PtHittable, PtRenderStats, device_count

__all__ = ["Pathtracer", "Scene", "make_camera", "camera_rotate", "camera_translate", "radians", "device_count", "PathtracerError", "PtCamera",
           "PtBvhNode", "PtHittable", "write_png", "write_hdr", "HITTABLE_TYPES", "MATERIAL_TYPES", "denoise_image",
           "denoise_params", "auto_sigma_color", "denoise_keep_mask", "DENOISE_DEFAULTS", "DENOISE_SIGMA_FACTOR",
           "temporal_params", "temporal_image", "TEMPORAL_DEFAULTS", "variance_params", "vdenoise_params",
           "temporal_moments_image", "denoise_variance_image", "VARIANCE_DEFAULTS", "VDENOISE_DEFAULTS",
           "vfeedback_params", "denoise_variance_feedback_image", "VFEEDBACK_DEFAULTS", "adaptive_variance_params",
           "adaptive_variance_image", "AVARIANCE_DEFAULTS", "ADENOISE_SIGMA_L", "despike_params", "despike_image",
           "DESPIKE_DEFAULTS", "upsample_params", "upsample_image", "upsample_resolve_image", "UPSAMPLE_DEFAULTS", "UPSAMPLE_SOURCES", "motion_table", "refit_boxes", "temporal_motion_image", "temporal_moments_motion_image", "NO_PREVIOUS"]

HITTABLE_TYPES = ["SPHERE", "CYLINDER", "DISK", "CONE", "PARABOLOID", "QUAD", "CUBE"]   # Hittable.h:9-12
MATERIAL_TYPES = ["LAMBERT", "GGX", "LAMBERT_GGX"]                                     # Material.h:9-12


def _f3(v: Sequence[float]):
    return (C.c_float * 3)(*[float(np.float32(x)) for x in v])


def radians(degrees: float) -> float:
    """SceneLoader.cpp:193-196 (float arithmetic)."""
    return float(N.host().pth_radians(float(degrees)))


def make_camera(position, look_at, up=(0.0, 1.0, 0.0), fovy_radians: float = 1.0471976, aspect: float = 1.0) -> PtCamera:
    """Camera ctor (Camera.inl:4-23)."""
    cam = PtCamera()
    N.check_host(N.host().pth_camera_make(_f3(position), _f3(look_at), _f3(up), float(fovy_radians), float(aspect),
                                          C.byref(cam)))
    return cam


def camera_rotate(camera: PtCamera, pitch: float, yaw: float, roll: float = 0.0) -> PtCamera:
    """Camera::rotate (Camera.inl:30-45), in place; returns the camera."""
    N.check_host(N.host().pth_camera_rotate(C.byref(camera), float(pitch), float(yaw), float(roll)))
    return camera


def camera_translate(camera: PtCamera, x: float, y: float, z: float) -> PtCamera:
    """Camera::translate (Camera.inl:47-51), in place; returns the camera."""
    N.check_host(N.host().pth_camera_translate(C.byref(camera), float(x), float(y), float(z)))
    return camera


def write_png(path: str, rgba: np.ndarray, flip: bool = True) -> None:
    a = np.ascontiguousarray(rgba, dtype=np.uint8)
    h, w = a.shape[:2]
    N.check_host(N.host().pth_write_png(os.fsencode(path), w, h, a.ctypes.data_as(C.POINTER(C.c_uint8)), int(flip)))


def write_hdr(path: str, rgba: np.ndarray, flip: bool = True) -> None:
    a = np.ascontiguousarray(rgba, dtype=np.float32)
    h, w = a.shape[:2]
    N.check_host(N.host().pth_write_hdr(os.fsencode(path), w, h, a.ctypes.data_as(C.POINTER(C.c_float)), int(flip)))


# Defaults of the denoiser, chosen by the sweep of tools/denoise_probe.py (profiles/denoise_probe.json;
# argued in DESIGN.md §5.7).  sigma_color=None means DENOISE_SIGMA_FACTOR x the median luminance of the
# kept pixels' (demodulated) colour, computed on the host.
DENOISE_DEFAULTS = {"iterations": 5, "sigma_plane": 0.005, "normal_power_log2": 3, "demodulate": True,
                    "same_primitive": False}
DENOISE_SIGMA_FACTOR = 4.0


def _refuse(what: str) -> "PathtracerError":
    return PathtracerError(N.PT_ERR_ARG, what)


def denoise_params(iterations: int = 5, sigma_color: float = 1.0, sigma_plane: Optional[float] = None,
                   normal_power_log2: Optional[int] = None, demodulate: Optional[bool] = None,
                   same_primitive: Optional[bool] = None, staging: int = 0) -> "N.PtDenoiseParams":
    """pt_denoise_params from keyword arguments, refused here (PT_ERR_ARG naming the field) before any
    device call when a value is outside the accepted range of include/pt_hip.h."""
    d = DENOISE_DEFAULTS
    sigma_plane = d["sigma_plane"] if sigma_plane is None else sigma_plane
    normal_power_log2 = d["normal_power_log2"] if normal_power_log2 is None else normal_power_log2
    demodulate = d["demodulate"] if demodulate is None else demodulate
    same_primitive = d["same_primitive"] if same_primitive is None else same_primitive
    if int(iterations) != iterations or not 1 <= int(iterations) <= 8:
        raise _refuse(f"denoise: iterations must be 1..8, not {iterations!r}")
    sc, sp = np.float32(sigma_color), np.float32(sigma_plane)
    if not (sc > 0 and np.isfinite(sc)):
        raise _refuse(f"denoise: sigma_color must be > 0 and finite, not {sigma_color!r}")
    if not (sp >= np.float32(1e-6) and np.isfinite(sp)):
        raise _refuse(f"denoise: sigma_plane must be >= 1e-6 and finite, not {sigma_plane!r}")
    if int(normal_power_log2) != normal_power_log2 or not 0 <= int(normal_power_log2) <= 7:
        raise _refuse(f"denoise: normal_power_log2 must be 0..7, not {normal_power_log2!r}")
    if staging not in (0, 1, 2):
        raise _refuse(f"denoise: staging must be 0, 1 or 2, not {staging!r}")
    flags = (N.PT_DENOISE_DEMODULATE if demodulate else 0) | (N.PT_DENOISE_SAME_PRIMITIVE if same_primitive else 0)
    return N.PtDenoiseParams(int(iterations), float(sc), float(sp), int(normal_power_log2), flags, int(staging))


def denoise_keep_mask(color: np.ndarray, plane1: np.ndarray, plane2: np.ndarray) -> np.ndarray:
    """keep of the filter rule: HIT, not EMISSIVE, and colour, normal and position finite."""
    fl = np.ascontiguousarray(plane2[..., 3]).view(np.uint32)
    fin = np.isfinite(color[..., :3]).all(-1) & np.isfinite(plane1[..., :3]).all(-1) & np.isfinite(plane2[..., :3]).all(-1)
    return ((fl & N.PT_FEATURE_HIT) != 0) & ((fl & N.PT_FEATURE_EMISSIVE) == 0) & fin


def auto_sigma_color(color: np.ndarray, plane0: np.ndarray, plane1: np.ndarray, plane2: np.ndarray,
                     demodulate: bool = True, factor: Optional[float] = None) -> float:
    """The automatic sigma_color: `factor` (default DENOISE_SIGMA_FACTOR) x the median luminance of the kept
    pixels' colour, divided by max(albedo, 1/64) first when demodulating.  1.0 when nothing is kept or the
    median is not positive.  A host-side statistic: the device rule needs no reduction."""
    keep = denoise_keep_mask(color, plane1, plane2)
    if not keep.any():
        return 1.0
    c = color[..., :3][keep].astype(np.float32)
    if demodulate:
        c = c / np.maximum(plane0[..., :3][keep].astype(np.float32), np.float32(1.0 / 64.0))
    lum = c @ np.array([0.2126, 0.7152, 0.0722], dtype=np.float32)
    med = float(np.median(lum))
    f = DENOISE_SIGMA_FACTOR if factor is None else float(factor)
    return f * med if med > 0 and np.isfinite(med) else 1.0


def _image4(name: str, a, shape=None) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 4 or a.shape[0] == 0 or a.shape[1] == 0:
        raise _refuse(f"denoise_image: {name} must be height x width x 4 float32, not shape {a.shape}")
    if shape is not None and a.shape != shape:
        raise _refuse(f"denoise_image: {name} has shape {a.shape}, color has {shape}")
    return a


def denoise_image(color, plane0, plane1, plane2, iterations: int = 5, sigma_color: Optional[float] = None,
                  sigma_plane: Optional[float] = None, normal_power_log2: Optional[int] = None,
                  demodulate: Optional[bool] = None, same_primitive: Optional[bool] = None, staging: int = 0,
                  device: int = 0) -> np.ndarray:
    """pt_denoise_image: the a-trous filter of include/pt_hip.h on host arrays (height x width x 4 float32:
    the colour and the three feature planes of Pathtracer.features()["planes"]), without a Pathtracer --
    for a frame gathered from several GPUs, or any image with such planes.  Returns height x width x 4."""
    c = _image4("color", color)
    planes = [_image4(f"plane{k}", p, c.shape) for k, p in enumerate((plane0, plane1, plane2))]
    demod = DENOISE_DEFAULTS["demodulate"] if demodulate is None else demodulate
    if sigma_color is None:
        sigma_color = auto_sigma_color(c, *planes, demodulate=demod)
    params = denoise_params(iterations, sigma_color, sigma_plane, normal_power_log2, demod, same_primitive, staging)
    out = np.zeros_like(c)
    fp = C.POINTER(C.c_float)
    rc = N.hip().pt_denoise_image(int(device), c.shape[1], c.shape[0], c.ctypes.data_as(fp), planes[0].ctypes.data_as(fp),
                                  planes[1].ctypes.data_as(fp), planes[2].ctypes.data_as(fp), C.byref(params),
                                  out.ctypes.data_as(fp))
    N.check_ctx(rc, None)
    return out


# Defaults of the temporal pass, chosen by the sweep of tools/temporal_probe.py (profiles/temporal_probe.json;
# argued in DESIGN.md §5.9).
TEMPORAL_DEFAULTS = {"alpha_min": 0.02, "max_history": 64, "sigma_plane": 0.3, "normal_cos_min": 0.0,
                     "demodulate": True, "same_primitive": False}


def temporal_params(alpha_min: Optional[float] = None, max_history: Optional[int] = None,
                    sigma_plane: Optional[float] = None, normal_cos_min: Optional[float] = None,
                    demodulate: Optional[bool] = None, same_primitive: Optional[bool] = None) -> "N.PtTemporalParams":
    """pt_temporal_params from keyword arguments, refused here (PT_ERR_ARG naming the field) before any
    device call when a value is outside the accepted range of include/pt_hip.h."""
    d = TEMPORAL_DEFAULTS
    alpha_min = d["alpha_min"] if alpha_min is None else alpha_min
    max_history = d["max_history"] if max_history is None else max_history
    sigma_plane = d["sigma_plane"] if sigma_plane is None else sigma_plane
    normal_cos_min = d["normal_cos_min"] if normal_cos_min is None else normal_cos_min
    demodulate = d["demodulate"] if demodulate is None else demodulate
    same_primitive = d["same_primitive"] if same_primitive is None else same_primitive
    am, sp, nc = np.float32(alpha_min), np.float32(sigma_plane), np.float32(normal_cos_min)
    if not 0 <= am <= 1:
        raise _refuse(f"temporal: alpha_min must be 0..1, not {alpha_min!r}")
    if isinstance(max_history, float) and not np.isfinite(max_history):
        raise _refuse(f"temporal: max_history must be 1..65535, not {max_history!r}")
    if int(max_history) != max_history or not 1 <= int(max_history) <= 65535:
        raise _refuse(f"temporal: max_history must be 1..65535, not {max_history!r}")
    if not (sp >= np.float32(1e-6) and np.isfinite(sp)):
        raise _refuse(f"temporal: sigma_plane must be >= 1e-6 and finite, not {sigma_plane!r}")
    if not -1 <= nc <= 1:
        raise _refuse(f"temporal: normal_cos_min must be -1..1, not {normal_cos_min!r}")
    flags = (N.PT_TEMPORAL_DEMODULATE if demodulate else 0) | (N.PT_TEMPORAL_SAME_PRIMITIVE if same_primitive else 0)
    return N.PtTemporalParams(float(am), int(max_history), float(sp), float(nc), flags)


def temporal_image(color, plane0, plane1, plane2, cur_camera: PtCamera, history=None, prev_camera: Optional[PtCamera] = None,
                   alpha_min: Optional[float] = None, max_history: Optional[int] = None, sigma_plane: Optional[float] = None,
                   normal_cos_min: Optional[float] = None, demodulate: Optional[bool] = None,
                   same_primitive: Optional[bool] = None, device: int = 0):
    """pt_temporal_image: one step of the temporal rule of include/pt_hip.h on host arrays (height x width x 4
    float32), without a Pathtracer.  `history` = the (h0, h1, h2) an earlier step returned, with that step's
    camera as `prev_camera`, or None.  Returns (image, h0, h1, h2)."""
    params = temporal_params(alpha_min, max_history, sigma_plane, normal_cos_min, demodulate, same_primitive)
    c = _image4("color", color)
    arrays = [c] + [_image4(f"plane{k}", p, c.shape) for k, p in enumerate((plane0, plane1, plane2))]
    fp = C.POINTER(C.c_float)
    null = C.cast(None, fp)
    if history is not None:
        if prev_camera is None:
            raise _refuse("temporal_image: history is given without prev_camera")
        hist = [_image4(f"history[{k}]", h, c.shape) for k, h in enumerate(history)]
        if len(hist) != 3:
            raise _refuse("temporal_image: history must be (h0, h1, h2)")
        hp = [h.ctypes.data_as(fp) for h in hist]
    else:
        hp = [null, null, null]
    outs = [np.zeros_like(c) for _ in range(4)]
    rc = N.hip().pt_temporal_image(int(device), c.shape[1], c.shape[0], *[a.ctypes.data_as(fp) for a in arrays],
                                   C.byref(cur_camera), *hp, C.byref(prev_camera) if prev_camera is not None else None,
                                   C.byref(params), *[o.ctypes.data_as(fp) for o in outs])
    N.check_ctx(rc, None)
    return tuple(outs)


NO_PREVIOUS = 0xffffffff     # prev_index / previous-object entry of something that was not in the earlier scene


def motion_table(prev_objects, cur_objects):
    """pth_motion_table: rule 7's per-object maps (include/pt_hip.h, include/pt_host.h) from two equally long
    sequences of PtHittable -- object i as it was and as it is.  Pure CPU.  Returns (rows, valid): count x 3 x 4
    float32 and count bool; an entry that is not valid (a word of its map is not finite) must get NO_PREVIOUS as its
    prev_index."""
    prev, cur = list(prev_objects), list(cur_objects)
    if len(prev) != len(cur):
        raise _refuse(f"motion_table: {len(prev)} previous objects and {len(cur)} current ones")
    n = len(cur)
    rows = np.zeros((n, 3, 4), dtype=np.float32)
    valid = np.zeros(n, dtype=np.uint32)
    if n:
        N.check_host(N.host().pth_motion_table((PtHittable * n)(*prev), (PtHittable * n)(*cur), n,
                                               rows.ctypes.data_as(C.POINTER(C.c_float)),
                                               valid.ctypes.data_as(C.POINTER(C.c_uint32))))
    return rows, valid != 0


def refit_boxes(nodes, boxes):
    """pth_refit_boxes: rule 10 of include/pt_hip.h on the host.  nodes: a sequence of PtBvhNode (or a ctypes array of
    them); boxes: prim_count x 6 float32 (min xyz, max xyz).  Returns a new PtBvhNode array: every node reachable from
    the root with its box refitted, every other word as it was.  Pure CPU."""
    src = list(nodes)
    if not src:
        raise _refuse("refit_boxes: nodes is empty")
    b = np.ascontiguousarray(boxes, dtype=np.float32)
    if b.ndim != 2 or b.shape[1] != 6 or b.shape[0] == 0:
        raise _refuse(f"refit_boxes: boxes must be prim_count x 6, not {b.shape}")
    out = (PtBvhNode * len(src))(*[PtBvhNode.from_buffer_copy(n) for n in src])
    N.check_host(N.host().pth_refit_boxes(out, len(src), b.ctypes.data_as(C.POINTER(C.c_float)), b.shape[0]))
    return out


def _motion_arrays(what: str, motion_rows, prev_index):
    rows = np.ascontiguousarray(motion_rows, dtype=np.float32)
    prev = np.ascontiguousarray(prev_index, dtype=np.uint32)
    if rows.ndim < 1 or rows.size != 12 * prev.size or prev.ndim != 1:
        raise _refuse(f"{what}: motion_rows must be count x 3 x 4 and prev_index count, not {rows.shape} and {prev.shape}")
    return rows, prev


def temporal_motion_image(color, plane0, plane1, plane2, cur_camera: PtCamera, motion_rows, prev_index, history=None,
                          prev_camera: Optional[PtCamera] = None, alpha_min: Optional[float] = None,
                          max_history: Optional[int] = None, sigma_plane: Optional[float] = None,
                          normal_cos_min: Optional[float] = None, demodulate: Optional[bool] = None,
                          same_primitive: Optional[bool] = None, device: int = 0):
    """pt_temporal_motion_image: temporal_image() under rule 7 of include/pt_hip.h.  motion_rows (count x 3 x 4
    float32) and prev_index (count uint32, NO_PREVIOUS = take no history) have one entry per primitive of the scene
    the planes were made from: the map to, and the index in, the scene `history` was made from.  Returns (image, h0,
    h1, h2); the new history is of the current scene."""
    params = temporal_params(alpha_min, max_history, sigma_plane, normal_cos_min, demodulate, same_primitive)
    rows, prev = _motion_arrays("temporal_motion_image", motion_rows, prev_index)
    c = _image4("color", color)
    arrays = [c] + [_image4(f"plane{k}", p, c.shape) for k, p in enumerate((plane0, plane1, plane2))]
    fp = C.POINTER(C.c_float)
    null = C.cast(None, fp)
    if history is not None:
        if prev_camera is None:
            raise _refuse("temporal_motion_image: history is given without prev_camera")
        hist = [_image4(f"history[{k}]", h, c.shape) for k, h in enumerate(history)]
        if len(hist) != 3:
            raise _refuse("temporal_motion_image: history must be (h0, h1, h2)")
        hp = [h.ctypes.data_as(fp) for h in hist]
    else:
        hp = [null, null, null]
    outs = [np.zeros_like(c) for _ in range(4)]
    rc = N.hip().pt_temporal_motion_image(int(device), c.shape[1], c.shape[0], *[a.ctypes.data_as(fp) for a in arrays],
                                          C.byref(cur_camera), *hp,
                                          C.byref(prev_camera) if prev_camera is not None else None, C.byref(params),
                                          *[o.ctypes.data_as(fp) for o in outs], int(prev.size), rows.ctypes.data_as(fp),
                                          prev.ctypes.data_as(C.POINTER(C.c_uint32)))
    N.check_ctx(rc, None)
    return tuple(outs)


def temporal_moments_motion_image(color, plane0, plane1, plane2, cur_camera: PtCamera, motion_rows, prev_index,
                                  history=None, prev_camera: Optional[PtCamera] = None, alpha_min: Optional[float] = None,
                                  max_history: Optional[int] = None, sigma_plane: Optional[float] = None,
                                  normal_cos_min: Optional[float] = None, demodulate: Optional[bool] = None,
                                  same_primitive: Optional[bool] = None, min_temporal: Optional[int] = None,
                                  device: int = 0):
    """pt_temporal_moments_motion_image: temporal_moments_image() under rule 7 (see temporal_motion_image).
    Returns (image, h0, h1, h2, h3, variance)."""
    params = temporal_params(alpha_min, max_history, sigma_plane, normal_cos_min, demodulate, same_primitive)
    vparams = variance_params(min_temporal)
    rows, prev = _motion_arrays("temporal_moments_motion_image", motion_rows, prev_index)
    c = _image4("color", color)
    arrays = [c] + [_image4(f"plane{k}", p, c.shape) for k, p in enumerate((plane0, plane1, plane2))]
    fp = C.POINTER(C.c_float)
    null = C.cast(None, fp)
    if history is not None:
        if prev_camera is None:
            raise _refuse("temporal_moments_motion_image: history is given without prev_camera")
        hist = [_image4(f"history[{k}]", h, c.shape) for k, h in enumerate(history)]
        if len(hist) != 4:
            raise _refuse("temporal_moments_motion_image: history must be (h0, h1, h2, h3)")
        hp = [h.ctypes.data_as(fp) for h in hist]
    else:
        hp = [null, null, null, null]
    outs = [np.zeros_like(c) for _ in range(5)] + [np.zeros(c.shape[:2], dtype=np.float32)]
    rc = N.hip().pt_temporal_moments_motion_image(int(device), c.shape[1], c.shape[0],
                                                  *[a.ctypes.data_as(fp) for a in arrays], C.byref(cur_camera), *hp,
                                                  C.byref(prev_camera) if prev_camera is not None else None,
                                                  C.byref(params), C.byref(vparams), *[o.ctypes.data_as(fp) for o in outs],
                                                  int(prev.size), rows.ctypes.data_as(fp),
                                                  prev.ctypes.data_as(C.POINTER(C.c_uint32)))
    N.check_ctx(rc, None)
    return tuple(outs)


# Defaults of the variance estimate and the variance-guided filter (PT_VARIANCE_DEFAULT_*, PT_VDENOISE_DEFAULT_*
# of include/pt_hip.h), chosen by the sweep of tools/svgf_probe.py (profiles/svgf_probe.json).
VARIANCE_DEFAULTS = {"min_temporal": 4}
VDENOISE_DEFAULTS = {"iterations": 5, "sigma_l": 16.0, "variance_floor": 1e-4, "sigma_plane": 0.005,
                     "normal_power_log2": 3, "demodulate": True, "same_primitive": False}


def variance_params(min_temporal: Optional[int] = None) -> "N.PtVarianceParams":
    """pt_variance_params, refused here (PT_ERR_ARG naming the field) when out of range."""
    min_temporal = VARIANCE_DEFAULTS["min_temporal"] if min_temporal is None else min_temporal
    if isinstance(min_temporal, float) and not np.isfinite(min_temporal):
        raise _refuse(f"temporal: min_temporal must be 1..255, not {min_temporal!r}")
    if int(min_temporal) != min_temporal or not 1 <= int(min_temporal) <= 255:
        raise _refuse(f"temporal: min_temporal must be 1..255, not {min_temporal!r}")
    return N.PtVarianceParams(int(min_temporal))


def vdenoise_params(iterations: Optional[int] = None, sigma_l: Optional[float] = None,
                    variance_floor: Optional[float] = None, sigma_plane: Optional[float] = None,
                    normal_power_log2: Optional[int] = None, demodulate: Optional[bool] = None,
                    same_primitive: Optional[bool] = None, staging: int = 0) -> "N.PtVDenoiseParams":
    """pt_vdenoise_params from keyword arguments, refused here (PT_ERR_ARG naming the field) before any
    device call when a value is outside the accepted range of include/pt_hip.h."""
    d = VDENOISE_DEFAULTS
    iterations = d["iterations"] if iterations is None else iterations
    sigma_l = d["sigma_l"] if sigma_l is None else sigma_l
    variance_floor = d["variance_floor"] if variance_floor is None else variance_floor
    sigma_plane = d["sigma_plane"] if sigma_plane is None else sigma_plane
    normal_power_log2 = d["normal_power_log2"] if normal_power_log2 is None else normal_power_log2
    demodulate = d["demodulate"] if demodulate is None else demodulate
    same_primitive = d["same_primitive"] if same_primitive is None else same_primitive
    if int(iterations) != iterations or not 1 <= int(iterations) <= 8:
        raise _refuse(f"denoise: iterations must be 1..8, not {iterations!r}")
    sl, vf, sp = np.float32(sigma_l), np.float32(variance_floor), np.float32(sigma_plane)
    if not (sl > 0 and sl <= np.float32(2.0 ** 20)):
        raise _refuse(f"denoise: sigma_l must be in (0, 2^20], not {sigma_l!r}")
    if not (vf > 0 and np.isfinite(vf)):
        raise _refuse(f"denoise: variance_floor must be > 0 and finite, not {variance_floor!r}")
    if not (sp >= np.float32(1e-6) and np.isfinite(sp)):
        raise _refuse(f"denoise: sigma_plane must be >= 1e-6 and finite, not {sigma_plane!r}")
    if int(normal_power_log2) != normal_power_log2 or not 0 <= int(normal_power_log2) <= 7:
        raise _refuse(f"denoise: normal_power_log2 must be 0..7, not {normal_power_log2!r}")
    if staging not in (0, 1, 2):
        raise _refuse(f"denoise: staging must be 0, 1 or 2, not {staging!r}")
    flags = (N.PT_DENOISE_DEMODULATE if demodulate else 0) | (N.PT_DENOISE_SAME_PRIMITIVE if same_primitive else 0)
    return N.PtVDenoiseParams(int(iterations), float(sl), float(vf), float(sp), int(normal_power_log2), flags, int(staging))


def _image1(name: str, a, shape) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.shape != shape[:2]:
        raise _refuse(f"denoise_variance_image: {name} has shape {a.shape}, color has {shape}")
    return a


def temporal_moments_image(color, plane0, plane1, plane2, cur_camera: PtCamera, history=None,
                           prev_camera: Optional[PtCamera] = None, alpha_min: Optional[float] = None,
                           max_history: Optional[int] = None, sigma_plane: Optional[float] = None,
                           normal_cos_min: Optional[float] = None, demodulate: Optional[bool] = None,
                           same_primitive: Optional[bool] = None, min_temporal: Optional[int] = None, device: int = 0):
    """pt_temporal_moments_image: temporal_image() with the moments plane and the variance estimate.
    `history` = the (h0, h1, h2, h3) an earlier step returned, or None.  Returns (image, h0, h1, h2, h3,
    variance); variance is height x width float32, -1 where the pixel is not a finite hit."""
    params = temporal_params(alpha_min, max_history, sigma_plane, normal_cos_min, demodulate, same_primitive)
    vparams = variance_params(min_temporal)
    c = _image4("color", color)
    arrays = [c] + [_image4(f"plane{k}", p, c.shape) for k, p in enumerate((plane0, plane1, plane2))]
    fp = C.POINTER(C.c_float)
    null = C.cast(None, fp)
    if history is not None:
        if prev_camera is None:
            raise _refuse("temporal_moments_image: history is given without prev_camera")
        hist = [_image4(f"history[{k}]", h, c.shape) for k, h in enumerate(history)]
        if len(hist) != 4:
            raise _refuse("temporal_moments_image: history must be (h0, h1, h2, h3)")
        hp = [h.ctypes.data_as(fp) for h in hist]
    else:
        hp = [null, null, null, null]
    outs = [np.zeros_like(c) for _ in range(5)] + [np.zeros(c.shape[:2], dtype=np.float32)]
    rc = N.hip().pt_temporal_moments_image(int(device), c.shape[1], c.shape[0], *[a.ctypes.data_as(fp) for a in arrays],
                                           C.byref(cur_camera), *hp,
                                           C.byref(prev_camera) if prev_camera is not None else None, C.byref(params),
                                           C.byref(vparams), *[o.ctypes.data_as(fp) for o in outs])
    N.check_ctx(rc, None)
    return tuple(outs)


def denoise_variance_image(color, plane0, plane1, plane2, variance, iterations: Optional[int] = None,
                           sigma_l: Optional[float] = None, variance_floor: Optional[float] = None,
                           sigma_plane: Optional[float] = None, normal_power_log2: Optional[int] = None,
                           demodulate: Optional[bool] = None, same_primitive: Optional[bool] = None, staging: int = 0,
                           device: int = 0) -> np.ndarray:
    """pt_denoise_variance_image: the variance-guided a-trous filter of include/pt_hip.h on host arrays, without
    a Pathtracer.  `variance` is height x width float32, of the luminance of the (demodulated, when demodulating)
    colour, from any source; a pixel whose variance is negative or not finite passes through."""
    params = vdenoise_params(iterations, sigma_l, variance_floor, sigma_plane, normal_power_log2, demodulate,
                             same_primitive, staging)
    c = _image4("color", color)
    planes = [_image4(f"plane{k}", p, c.shape) for k, p in enumerate((plane0, plane1, plane2))]
    var = _image1("variance", variance, c.shape)
    out = np.zeros_like(c)
    fp = C.POINTER(C.c_float)
    rc = N.hip().pt_denoise_variance_image(int(device), c.shape[1], c.shape[0], c.ctypes.data_as(fp),
                                           *[p.ctypes.data_as(fp) for p in planes], var.ctypes.data_as(fp),
                                           C.byref(params), out.ctypes.data_as(fp))
    N.check_ctx(rc, None)
    return out


# Default of the feedback of the filtered colour into the history (PT_VFEEDBACK_DEFAULT_LEVEL of
# include/pt_hip.h).  The feedback itself is off unless asked for (denoise(feedback=L)).
VFEEDBACK_DEFAULTS = {"level": 3}


def vfeedback_params(level: Optional[int] = None, iterations: Optional[int] = None) -> "N.PtVFeedbackParams":
    """pt_vfeedback_params, refused here (PT_ERR_ARG naming the field) unless 1 <= level <= iterations
    (iterations=None: the filter's default; the device checks against the parameters it is given)."""
    level = VFEEDBACK_DEFAULTS["level"] if level is None else level
    iterations = VDENOISE_DEFAULTS["iterations"] if iterations is None else iterations
    if isinstance(level, float) and not np.isfinite(level):
        raise _refuse(f"denoise: feedback level must be 1..iterations, not {level!r}")
    if int(level) != level or not 1 <= int(level) <= int(iterations):
        raise _refuse(f"denoise: feedback level must be 1..iterations ({iterations}), not {level!r}")
    return N.PtVFeedbackParams(int(level))


def denoise_variance_feedback_image(color, plane0, plane1, plane2, variance, hist0, level: Optional[int] = None,
                                    iterations: Optional[int] = None, sigma_l: Optional[float] = None,
                                    variance_floor: Optional[float] = None, sigma_plane: Optional[float] = None,
                                    normal_power_log2: Optional[int] = None, demodulate: Optional[bool] = None,
                                    same_primitive: Optional[bool] = None, staging: int = 0, device: int = 0):
    """pt_denoise_variance_feedback_image: denoise_variance_image() with the feedback of include/pt_hip.h on host
    arrays.  `hist0` = the h0 a temporal_moments_image() step returned for the same frame; the output of
    iteration level - 1 replaces its colours where the pixel is kept and the colour finite.  Returns (out, hist0):
    out is denoise_variance_image()'s result word for word, hist0 goes into the next step's history."""
    params = vdenoise_params(iterations, sigma_l, variance_floor, sigma_plane, normal_power_log2, demodulate,
                             same_primitive, staging)
    fb = vfeedback_params(level, params.iterations)
    c = _image4("color", color)
    planes = [_image4(f"plane{k}", p, c.shape) for k, p in enumerate((plane0, plane1, plane2))]
    var = _image1("variance", variance, c.shape)
    h0 = _image4("hist0", hist0, c.shape)
    out, out_h0 = np.zeros_like(c), np.zeros_like(c)
    fp = C.POINTER(C.c_float)
    rc = N.hip().pt_denoise_variance_feedback_image(int(device), c.shape[1], c.shape[0], c.ctypes.data_as(fp),
                                                    *[p.ctypes.data_as(fp) for p in planes], var.ctypes.data_as(fp),
                                                    h0.ctypes.data_as(fp), C.byref(params), C.byref(fb),
                                                    out.ctypes.data_as(fp), out_h0.ctypes.data_as(fp))
    N.check_ctx(rc, None)
    return out, out_h0


# Defaults of the variance of an adaptive render's image (PT_AVARIANCE_DEFAULT_* of include/pt_hip.h; DESIGN.md
# §5.12): sigma_plane, normal_cos_min and the flags are the temporal pass's, whose same-surface window this is.
# min_batches and ADENOISE_SIGMA_L, the filter's sigma_l for this source, are the minimiser of the sweep of
# tools/adaptive_variance_probe.py (profiles/adaptive_variance_probe.json); the filter's other defaults are
# VDENOISE_DEFAULTS.
ADENOISE_SIGMA_L = 2.0
AVARIANCE_DEFAULTS = {"min_batches": 32, "sigma_plane": 0.3, "normal_cos_min": 0.0, "demodulate": True,
                      "same_primitive": False}


def adaptive_variance_params(min_batches: Optional[int] = None, sigma_plane: Optional[float] = None,
                             normal_cos_min: Optional[float] = None, demodulate: Optional[bool] = None,
                             same_primitive: Optional[bool] = None) -> "N.PtAdaptiveVarianceParams":
    """pt_adaptive_variance_params from keyword arguments, refused here (PT_ERR_ARG naming the field) before any
    device call when a value is outside the accepted range of include/pt_hip.h."""
    d = AVARIANCE_DEFAULTS
    min_batches = d["min_batches"] if min_batches is None else min_batches
    sigma_plane = d["sigma_plane"] if sigma_plane is None else sigma_plane
    normal_cos_min = d["normal_cos_min"] if normal_cos_min is None else normal_cos_min
    demodulate = d["demodulate"] if demodulate is None else demodulate
    same_primitive = d["same_primitive"] if same_primitive is None else same_primitive
    if isinstance(min_batches, float) and not np.isfinite(min_batches):
        raise _refuse(f"denoise: min_batches must be 2..255, not {min_batches!r}")
    if int(min_batches) != min_batches or not 2 <= int(min_batches) <= 255:
        raise _refuse(f"denoise: min_batches must be 2..255, not {min_batches!r}")
    sp, nc = np.float32(sigma_plane), np.float32(normal_cos_min)
    if not (sp >= np.float32(1e-6) and np.isfinite(sp)):
        raise _refuse(f"denoise: variance sigma_plane must be >= 1e-6 and finite, not {sigma_plane!r}")
    if not -1 <= nc <= 1:
        raise _refuse(f"denoise: normal_cos_min must be -1..1, not {normal_cos_min!r}")
    flags = (N.PT_DENOISE_DEMODULATE if demodulate else 0) | (N.PT_DENOISE_SAME_PRIMITIVE if same_primitive else 0)
    return N.PtAdaptiveVarianceParams(int(min_batches), float(sp), float(nc), flags)


def adaptive_variance_image(color, plane0, plane1, plane2, moments, min_batches: Optional[int] = None,
                            sigma_plane: Optional[float] = None, normal_cos_min: Optional[float] = None,
                            demodulate: Optional[bool] = None, same_primitive: Optional[bool] = None, staging: int = 0,
                            device: int = 0) -> np.ndarray:
    """pt_adaptive_variance_image: the variance of an adaptive render's image (rule 5 of include/pt_hip.h) on host
    arrays, without a Pathtracer -- for a frame gathered from several GPUs.  `color` is the accumulation divided by
    every pixel's own count (get_hdr_image_data() after render_adaptive), the planes are features()["planes"],
    `moments` is Pathtracer.moments() (height x width x 3).  Returns height x width float32, -1 where the rule
    gives none; denoise_variance_image() takes it."""
    params = adaptive_variance_params(min_batches, sigma_plane, normal_cos_min, demodulate, same_primitive)
    if staging not in (0, 1, 2):
        raise _refuse(f"denoise: staging must be 0, 1 or 2, not {staging!r}")
    c = _image4("color", color)
    planes = [_image4(f"plane{k}", p, c.shape) for k, p in enumerate((plane0, plane1, plane2))]
    mom = np.ascontiguousarray(moments, dtype=np.float32)
    if mom.shape != c.shape[:2] + (3,):
        raise _refuse(f"adaptive_variance_image: moments has shape {mom.shape}, color has {c.shape}")
    out = np.zeros(c.shape[:2], dtype=np.float32)
    fp = C.POINTER(C.c_float)
    rc = N.hip().pt_adaptive_variance_image(int(device), c.shape[1], c.shape[0], c.ctypes.data_as(fp),
                                            *[p.ctypes.data_as(fp) for p in planes], mom.ctypes.data_as(fp),
                                            C.byref(params), int(staging), out.ctypes.data_as(fp))
    N.check_ctx(rc, None)
    return out


# Defaults of despike, the same-surface firefly clamp (PT_DESPIKE_DEFAULT_* of include/pt_hip.h): radius, rank, factor,
# floor and the flags are the choice of the sweep of tools/despike_probe.py (profiles/despike_probe.json; DESIGN.md
# §5.13 says what they cost in energy); sigma_plane and normal_cos_min are the temporal pass's.
DESPIKE_DEFAULTS = {"radius": 1, "rank": 2, "factor": 4.0, "floor": 0.2, "min_neighbors": 3, "sigma_plane": 0.3,
                    "normal_cos_min": 0.0, "demodulate": False, "same_primitive": True}


def despike_params(radius: Optional[int] = None, rank: Optional[int] = None, factor: Optional[float] = None,
                   floor: Optional[float] = None, min_neighbors: Optional[int] = None, sigma_plane: Optional[float] = None,
                   normal_cos_min: Optional[float] = None, demodulate: Optional[bool] = None,
                   same_primitive: Optional[bool] = None, staging: int = 0) -> "N.PtDespikeParams":
    """pt_despike_params from keyword arguments, refused here (PT_ERR_ARG naming the field) before any device call
    when a value is outside the accepted range of include/pt_hip.h.  min_neighbors=None: the default, raised to
    `rank` and lowered to the window's size where the default lies outside them."""
    d = DESPIKE_DEFAULTS
    radius = d["radius"] if radius is None else radius
    rank = d["rank"] if rank is None else rank
    factor = d["factor"] if factor is None else factor
    floor = d["floor"] if floor is None else floor
    sigma_plane = d["sigma_plane"] if sigma_plane is None else sigma_plane
    normal_cos_min = d["normal_cos_min"] if normal_cos_min is None else normal_cos_min
    demodulate = d["demodulate"] if demodulate is None else demodulate
    same_primitive = d["same_primitive"] if same_primitive is None else same_primitive

    def integer(name, v, lo, hi, what):
        if isinstance(v, float) and not np.isfinite(v) or int(v) != v or not lo <= int(v) <= hi:
            raise _refuse(f"despike: {name} must be {what}, not {v!r}")
        return int(v)

    radius = integer("radius", radius, 1, 3, "1..3")
    rank = integer("rank", rank, 1, 4, "1..4")
    taps = (2 * radius + 1) ** 2 - 1
    if min_neighbors is None:
        min_neighbors = min(max(d["min_neighbors"], rank), taps)
    min_neighbors = integer("min_neighbors", min_neighbors, rank, taps, f"rank..(2 radius + 1)^2 - 1 = {rank}..{taps}")
    fa, fo, sp, nc = (np.float32(v) for v in (factor, floor, sigma_plane, normal_cos_min))
    if not (fa >= 1 and np.isfinite(fa)):
        raise _refuse(f"despike: factor must be >= 1 and finite, not {factor!r}")
    if not (fo >= 0 and np.isfinite(fo)):
        raise _refuse(f"despike: floor must be >= 0 and finite, not {floor!r}")
    if not (sp >= np.float32(1e-6) and np.isfinite(sp)):
        raise _refuse(f"despike: sigma_plane must be >= 1e-6 and finite, not {sigma_plane!r}")
    if not -1 <= nc <= 1:
        raise _refuse(f"despike: normal_cos_min must be -1..1, not {normal_cos_min!r}")
    if staging not in (0, 1, 2):
        raise _refuse(f"despike: staging must be 0, 1 or 2, not {staging!r}")
    flags = (N.PT_DENOISE_DEMODULATE if demodulate else 0) | (N.PT_DENOISE_SAME_PRIMITIVE if same_primitive else 0)
    return N.PtDespikeParams(radius, rank, float(fa), float(fo), min_neighbors, float(sp), float(nc), flags, int(staging))


def despike_image(color, plane0, plane1, plane2, radius: Optional[int] = None, rank: Optional[int] = None,
                  factor: Optional[float] = None, floor: Optional[float] = None, min_neighbors: Optional[int] = None,
                  sigma_plane: Optional[float] = None, normal_cos_min: Optional[float] = None,
                  demodulate: Optional[bool] = None, same_primitive: Optional[bool] = None, staging: int = 0,
                  device: int = 0, return_count: bool = False):
    """pt_despike_image: despike (rule 6 of include/pt_hip.h) on host arrays (height x width x 4 float32: the colour
    and the three feature planes), without a Pathtracer -- for a frame gathered from several GPUs, and ahead of the
    other *_image forms.  Returns height x width x 4, or (image, number of spikes) with return_count."""
    params = despike_params(radius, rank, factor, floor, min_neighbors, sigma_plane, normal_cos_min, demodulate,
                            same_primitive, staging)
    c = _image4("color", color)
    planes = [_image4(f"plane{k}", p, c.shape) for k, p in enumerate((plane0, plane1, plane2))]
    out = np.zeros_like(c)
    count = C.c_uint32(0)
    fp = C.POINTER(C.c_float)
    rc = N.hip().pt_despike_image(int(device), c.shape[1], c.shape[0], c.ctypes.data_as(fp),
                                  *[p.ctypes.data_as(fp) for p in planes], C.byref(params), out.ctypes.data_as(fp),
                                  C.byref(count))
    N.check_ctx(rc, None)
    return (out, int(count.value)) if return_count else out


# Defaults of the guided upsampling (PT_UPSAMPLE_DEFAULT_* of include/pt_hip.h): sigma_plane and the
# normal power are the a-trous filter's, and both flags are set.
UPSAMPLE_DEFAULTS = {"sigma_plane": 0.005, "normal_power_log2": 3, "demodulate": True, "same_primitive": True}
# upsample(source=...): the image of the low-resolution Pathtracer that is taken (PT_UPSAMPLE_* of include/pt_hip.h)
UPSAMPLE_SOURCES = {"accum": N.PT_UPSAMPLE_ACCUM, "denoised": N.PT_UPSAMPLE_DENOISED, "temporal": N.PT_UPSAMPLE_TEMPORAL,
                    "despiked": N.PT_UPSAMPLE_DESPIKED}


def upsample_params(sigma_plane: Optional[float] = None, normal_power_log2: Optional[int] = None,
                    demodulate: Optional[bool] = None, same_primitive: Optional[bool] = None,
                    staging: int = 0) -> "N.PtUpsampleParams":
    """pt_upsample_params from keyword arguments, refused here (PT_ERR_ARG naming the field) before any device call
    when a value is outside the accepted range of include/pt_hip.h."""
    d = UPSAMPLE_DEFAULTS
    sigma_plane = d["sigma_plane"] if sigma_plane is None else sigma_plane
    normal_power_log2 = d["normal_power_log2"] if normal_power_log2 is None else normal_power_log2
    demodulate = d["demodulate"] if demodulate is None else demodulate
    same_primitive = d["same_primitive"] if same_primitive is None else same_primitive
    sp = np.float32(sigma_plane)
    if not (sp >= np.float32(1e-6) and np.isfinite(sp)):
        raise _refuse(f"upsample: sigma_plane must be >= 1e-6 and finite, not {sigma_plane!r}")
    n = normal_power_log2
    if isinstance(n, float) and not np.isfinite(n) or int(n) != n or not 0 <= int(n) <= 7:
        raise _refuse(f"upsample: normal_power_log2 must be 0..7, not {normal_power_log2!r}")
    if staging not in (0, 1, 2):
        raise _refuse(f"upsample: staging must be 0, 1 or 2, not {staging!r}")
    flags = (N.PT_DENOISE_DEMODULATE if demodulate else 0) | (N.PT_DENOISE_SAME_PRIMITIVE if same_primitive else 0)
    return N.PtUpsampleParams(float(sp), int(n), flags, int(staging))


def upsample_image(color, lo_plane0, lo_plane1, lo_plane2, hi_plane0, hi_plane1, hi_plane2,
                   sigma_plane: Optional[float] = None, normal_power_log2: Optional[int] = None,
                   demodulate: Optional[bool] = None, same_primitive: Optional[bool] = None, staging: int = 0,
                   device: int = 0, return_counts: bool = False):
    """pt_upsample_image: the guided upsampling (rule 8 of include/pt_hip.h) on host arrays, without a Pathtracer:
    the colour and the three feature planes of a low image (h x w x 4 float32) and the three planes of the full frame
    (H x W x 4, w <= W and h <= H).  Returns H x W x 4, or (image, (pixels that needed the wider ring, pixels that took
    the nearest low pixel)) with return_counts."""
    params = upsample_params(sigma_plane, normal_power_log2, demodulate, same_primitive, staging)
    c = _image4("color", color)
    lows = [_image4(f"lo_plane{k}", p, c.shape) for k, p in enumerate((lo_plane0, lo_plane1, lo_plane2))]
    h0 = _image4("hi_plane0", hi_plane0)
    highs = [h0] + [_image4(f"hi_plane{k + 1}", p, h0.shape) for k, p in enumerate((hi_plane1, hi_plane2))]
    if c.shape[0] > h0.shape[0] or c.shape[1] > h0.shape[1]:
        raise _refuse(f"upsample_image: the low image {c.shape[:2]} is larger than the high planes {h0.shape[:2]}")
    out = np.zeros_like(h0)
    counts = (C.c_uint32 * 2)()
    fp = C.POINTER(C.c_float)
    rc = N.hip().pt_upsample_image(int(device), c.shape[1], c.shape[0], c.ctypes.data_as(fp),
                                   *[p.ctypes.data_as(fp) for p in lows], h0.shape[1], h0.shape[0],
                                   *[p.ctypes.data_as(fp) for p in highs], C.byref(params), out.ctypes.data_as(fp), counts)
    N.check_ctx(rc, None)
    return (out, (int(counts[0]), int(counts[1]))) if return_counts else out


def upsample_resolve_image(color, lo_plane0, lo_plane1, lo_plane2, ss_plane0, ss_plane1, ss_plane2, factor: int,
                           sigma_plane: Optional[float] = None, normal_power_log2: Optional[int] = None,
                           demodulate: Optional[bool] = None, same_primitive: Optional[bool] = None, staging: int = 0,
                           device: int = 0, return_counts: bool = False):
    """pt_upsample_resolve_image: the guided upsampling onto supersampled planes (rule 9 of include/pt_hip.h) on host
    arrays, without a Pathtracer: the colour and the three feature planes of a low image (h x w x 4 float32) and the
    three planes of a frame `factor` (2, 3 or 4) times the output in width and height (S H x S W x 4, w <= W and
    h <= H).  Returns H x W x 4, every pixel the mean of rule 8's result at its S x S samples, or (image, (sub-pixels
    that needed the wider ring, sub-pixels that took the nearest low pixel)) with return_counts."""
    params = upsample_params(sigma_plane, normal_power_log2, demodulate, same_primitive, staging)
    if isinstance(factor, bool) or not isinstance(factor, (int, np.integer)) or not 2 <= int(factor) <= 4:
        raise _refuse(f"upsample_resolve_image: factor must be 2, 3 or 4, not {factor!r}")
    S = int(factor)
    c = _image4("color", color)
    lows = [_image4(f"lo_plane{k}", p, c.shape) for k, p in enumerate((lo_plane0, lo_plane1, lo_plane2))]
    h0 = _image4("ss_plane0", ss_plane0)
    highs = [h0] + [_image4(f"ss_plane{k + 1}", p, h0.shape) for k, p in enumerate((ss_plane1, ss_plane2))]
    if h0.shape[0] % S or h0.shape[1] % S:
        raise _refuse(f"upsample_resolve_image: factor {S} does not divide the planes {h0.shape[:2]}")
    H, W = h0.shape[0] // S, h0.shape[1] // S
    if c.shape[0] > H or c.shape[1] > W:
        raise _refuse(f"upsample_resolve_image: the low image {c.shape[:2]} is larger than the output {(H, W)}")
    out = np.zeros((H, W, 4), dtype=np.float32)
    counts = (C.c_uint32 * 2)()
    fp = C.POINTER(C.c_float)
    rc = N.hip().pt_upsample_resolve_image(int(device), c.shape[1], c.shape[0], c.ctypes.data_as(fp),
                                           *[p.ctypes.data_as(fp) for p in lows], h0.shape[1], h0.shape[0],
                                           *[p.ctypes.data_as(fp) for p in highs], S, C.byref(params),
                                           out.ctypes.data_as(fp), counts)
    N.check_ctx(rc, None)
    return (out, (int(counts[0]), int(counts[1]))) if return_counts else out


class Scene:
    """A parsed scene file (no GPU): objects in file order, the SAH BVH, camera, textures."""

    def __init__(self, path: str, width: int, height: int) -> None:
        self._h = C.c_void_p()
        N.check_host(N.host().pth_scene_load(os.fsencode(str(path)), int(width), int(height), C.byref(self._h)))
        self.path = str(path)

    def __del__(self) -> None:
        h = getattr(self, "_h", None)
        if h:
            N.host().pth_scene_free(h)
            self._h = None

    def timing(self) -> Dict[str, float]:
        """Host wall time of the load: {"parse_ms": JSON + transforms, "bvh_ms": SAH build}."""
        a, b = C.c_double(), C.c_double()
        N.check_host(N.host().pth_scene_timing(self._h, C.byref(a), C.byref(b)))
        return {"parse_ms": a.value, "bvh_ms": b.value}

    @property
    def object_count(self) -> int:
        return int(N.host().pth_scene_object_count(self._h))

    @property
    def node_count(self) -> int:
        return int(N.host().pth_scene_node_count(self._h))

    @property
    def bvh_depth(self) -> int:
        return int(N.host().pth_scene_bvh_depth(self._h))

    def objects(self):
        n = self.object_count
        objs = (PtHittable * max(1, n))()
        aabbs = np.zeros((n, 6), dtype=np.float32)
        N.check_host(N.host().pth_scene_objects(self._h, objs, aabbs.ctypes.data_as(C.POINTER(C.c_float))))
        return objs, aabbs

    def bvh(self):
        nodes = (PtBvhNode * max(1, self.node_count))()
        prims = (PtHittable * max(1, self.object_count))()
        N.check_host(N.host().pth_scene_bvh(self._h, nodes, prims))
        return nodes, prims

    def camera(self) -> PtCamera:
        cam = PtCamera()
        N.check_host(N.host().pth_scene_camera(self._h, C.byref(cam)))
        return cam

    @property
    def skybox(self) -> int:
        return int(N.host().pth_scene_skybox(self._h))

    def textures(self):
        out = []
        for handle in range(1, int(N.host().pth_scene_texture_count(self._h)) + 1):
            w, h = C.c_uint32(), C.c_uint32()
            N.check_host(N.host().pth_scene_texture_info(self._h, handle, C.byref(w), C.byref(h)))
            t = np.zeros((h.value, w.value, 4), dtype=np.float32)
            N.check_host(N.host().pth_scene_texture_data(self._h, handle, t.ctypes.data_as(C.POINTER(C.c_float))))
            out.append(t)
        return out


class Pathtracer:
    """The reference's Pathtracer on one MI355X, on a row-band tile of the image, or on several GPUs.

    Tiles: the image is cut into bands of `band_rows` rows and this object renders the bands
    b = row_offset + k * row_stride (band_rows = 1: rows y = row_offset + k * row_stride).
    `devices=[...]` spans several GPUs of this process (pt_group_*, RCCL gather; 8-row bands unless
    `band_rows` says otherwise, as the C++ constructor and the CLI): the image calls (accum,
    get_hdr_image_data, get_image_data, tonemap, rng_state) then cover the full image, the tuning
    knobs apply to every device, and the per-context diagnostics raise PathtracerError.
    """

    def __init__(self, width: int, height: int, device: int = 0, row_offset: int = 0, row_stride: int = 1,
                 band_rows: Optional[int] = None, devices: Optional[Sequence[int]] = None) -> None:
        self._r = C.c_void_p()
        if band_rows is None:
            band_rows = 8 if devices is not None else 1
        if devices is not None:
            devs = (C.c_int * len(devices))(*[int(d) for d in devices])
            N.check_host(N.host().pth_renderer_create_group(int(width), int(height), len(devices), devs, int(band_rows),
                                                            C.byref(self._r)))
        else:
            N.check_host(N.host().pth_renderer_create_banded(int(width), int(height), int(device), int(band_rows),
                                                             int(row_offset), int(row_stride), C.byref(self._r)))
        self.width, self.height = int(width), int(height)
        self.device = int(device)
        self.row_offset, self.row_stride, self.band_rows = int(row_offset), int(row_stride), int(band_rows)
        self.devices = list(devices) if devices is not None else None
        self.rows = int(N.host().pth_renderer_local_rows(self._r))
        self._ctx = N.host().pth_renderer_context(self._r)
        self._group = N.host().pth_renderer_group(self._r)

    # --- device groups ------------------------------------------------------------------------
    def _contexts(self):
        """Every device context: the group's, or this object's one."""
        if not self._group:
            return [self._ctx]
        return [N.hip().pt_group_context(self._group, i) for i in range(int(N.hip().pt_group_size(self._group)))]

    def _single(self, what: str) -> None:
        if self._group:
            raise PathtracerError(N.PT_ERR_STATE, f"{what}: per-context call, not available on a device group "
                                                  f"(use pt_group_context(i) through the C ABI)")

    def _group_rows(self):
        """Per device of a group: (context, its local rows' global row indices)."""
        out = []
        n = len(self.devices)
        shift = self.band_rows.bit_length() - 1
        for i, c in enumerate(self._contexts()):
            rows = int(N.hip().pt_local_rows(c))
            ly = np.arange(rows, dtype=np.int64)
            out.append((c, ((i + (ly >> shift) * n) << shift) + (ly & (self.band_rows - 1))))
        return out

    def close(self) -> None:
        if getattr(self, "_r", None):
            N.host().pth_renderer_destroy(self._r)
            self._r = None

    def __del__(self) -> None:
        self.close()

    def __enter__(self) -> "Pathtracer":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    # --- reference API --------------------------------------------------------------------------
    def load_scene(self, path: str) -> PtCamera:
        cam = PtCamera()
        N.check_host(N.host().pth_renderer_load_scene(self._r, os.fsencode(str(path)), C.byref(cam)))
        return cam

    def load_scene_moved(self, path: str, previous: Optional[Sequence[int]] = None) -> PtCamera:
        """load_scene() for a file whose objects moved since the last load, keeping the temporal history
        (pth_renderer_load_scene_moved; rule 7 of include/pt_hip.h): the next temporal() reprojects every pixel
        through its object's motion.  previous[k] = the index object k of the file had in the last scene's file, or
        NO_PREVIOUS for a new object; None: object k was object k (the counts must then match).  Per frame:
        load_scene_moved(f_k), render(cam, 1, True), features(cam), temporal(variance=True),
        denoise(source="temporal", guide="variance").  One move per temporal step: a second move before the next
        temporal() ends the history.  Single device only."""
        self._single("load_scene_moved")
        cam = PtCamera()
        prev = None
        if previous is not None:
            prev = np.ascontiguousarray([int(v) for v in previous], dtype=np.uint32)
            n = int(Scene(str(path), self.width, self.height).object_count)
            if prev.size != n:
                raise _refuse(f"load_scene_moved: previous has {prev.size} entries, the scene {n} objects")
        N.check_host(N.host().pth_renderer_load_scene_moved(
            self._r, os.fsencode(str(path)), prev.ctypes.data_as(C.POINTER(C.c_uint32)) if prev is not None else None,
            C.byref(cam)))
        return cam

    def move_objects(self, indices, position, rotation, scale) -> None:
        """Move objects without a rebuild (pth_renderer_move_objects; pt_move_primitives, rule 10 of include/pt_hip.h).
        indices: n distinct object indices in the scene file's order; position, rotation (radians), scale: n x 3, the
        new transforms (type and material stay).  An upload of the n records and a refit of the existing tree on the
        device (only the upload scales with n: the refit and the motion table run over the whole scene); the temporal history is kept as load_scene_moved keeps it.  Per frame: move_objects(...),
        render(cam, 1, True), features(cam), temporal(...).  The tree is afterwards not the one a fresh build would
        make: renders equal the oracle walking bvh(); rebuild_scene() returns to the build's tree.  Single device
        only."""
        self._single("move_objects")
        idx = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        if idx.size == 0:
            raise _refuse("move_objects: indices is empty")
        if (idx < 0).any() or (idx > 0xFFFFFFFE).any():
            raise _refuse("move_objects: indices must be object indices")
        arrays = []
        for name, a in (("position", position), ("rotation", rotation), ("scale", scale)):
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != (idx.size, 3):
                raise _refuse(f"move_objects: {name} must be {idx.size} x 3, not {a.shape}")
            arrays.append(a)
        idx = idx.astype(np.uint32)
        fp = C.POINTER(C.c_float)
        N.check_host(N.host().pth_renderer_move_objects(self._r, idx.size, idx.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                        *[a.ctypes.data_as(fp) for a in arrays]))

    def object_transforms(self):
        """(position, rotation, scale), each count x 3 float32: the transforms the current objects were made with, in
        the scene file's order (rotation in radians)."""
        n = int(N.host().pth_renderer_object_transforms(self._r, None, None, None))
        out = [np.zeros((n, 3), dtype=np.float32) for _ in range(3)]
        if n:
            N.host().pth_renderer_object_transforms(self._r, *[a.ctypes.data_as(C.POINTER(C.c_float)) for a in out])
        return tuple(out)

    def rebuild_scene(self) -> None:
        """A fresh SAH build of the current objects with the temporal history kept (pth_renderer_rebuild_scene): for
        when a tree refitted by move_objects has grown slow.  Counts as the one move of its temporal step."""
        self._single("rebuild_scene")
        N.check_host(N.host().pth_renderer_rebuild_scene(self._r))

    def refit_timing(self) -> float:
        """hipEvent milliseconds of the last move_objects' kernels (pt_read_refit_timing)."""
        self._single("refit_timing")
        ms = C.c_float()
        N.check_host(N.host().pth_renderer_refit_timing(self._r, C.byref(ms)))
        return float(ms.value)

    def bvh(self):
        """(nodes, prims): the tree this object holds as PtBvhNode and PtHittable arrays -- the device's tree, after
        move_objects the refitted one."""
        nn, np_ = C.c_uint32(), C.c_uint32()
        N.check_host(N.host().pth_renderer_bvh(self._r, None, None, C.byref(nn), C.byref(np_)))
        nodes, prims = (PtBvhNode * max(1, nn.value))(), (PtHittable * max(1, np_.value))()
        N.check_host(N.host().pth_renderer_bvh(self._r, nodes, prims, None, None))
        return nodes, prims

    def holds_motion(self) -> bool:
        """Whether a motion table is held for the next temporal step (pt_holds_motion): from a load_scene_moved over a
        held history until the next temporal(), load_scene, texture or other sky."""
        self._single("holds_motion")
        return bool(N.hip().pt_holds_motion(self._ctx))

    def motion_table(self):
        """The per-primitive table of the last load_scene_moved (rows: count x 3 x 4 float32, prev_index: count
        uint32, in the current BVH's primitive order), or None when the last scene call was not a move."""
        rows, prev = C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)()
        n = int(N.host().pth_renderer_motion_table(self._r, C.byref(rows), C.byref(prev)))
        if n == 0:
            return None
        return (np.ctypeslib.as_array(rows, shape=(n, 3, 4)).copy(), np.ctypeslib.as_array(prev, shape=(n,)).copy())

    def render(self, camera: PtCamera, spp: int, ignore_history: bool, chunks: int = 1) -> None:
        """`chunks` x render(camera, spp, ignore_history and first) in one kernel launch."""
        N.check_host(N.host().pth_renderer_render(self._r, C.byref(camera), int(spp), int(chunks), int(bool(ignore_history))))

    # --- adaptive sampling (pt_render_adaptive, pt_hip.h) -----------------------------------------
    def render_adaptive(self, camera: PtCamera, spp: int, min_calls: int, max_calls: int, tolerance: float,
                        floor: float = 0.01, reset: bool = True) -> Dict[str, float]:
        """Render calls of `spp` samples per pixel until the standard error of a pixel's per-call
        luminance is below tolerance x (|mean| + floor): at least `min_calls`, at most `max_calls`
        calls.  A pixel stopped after n calls holds what n render(camera, spp, ...) calls leave.
        Afterwards get_hdr_image_data() / get_image_data() divide every pixel by its own n; see also
        moments(), sample_counts(), noise_map().  reset=False continues the previous adaptive render.
        Returns {"rounds", "samples", "gpu_ms", "mean_spp"}."""
        self._single("render_adaptive")
        ap = N.PtAdaptiveParams(int(spp), int(min_calls), int(max_calls), float(tolerance), float(floor), int(bool(reset)))
        res = N.PtAdaptiveResult()
        N.check_host(N.host().pth_renderer_render_adaptive(self._r, C.byref(camera), C.byref(ap), C.byref(res)))
        npix = max(1, self.rows * self.width)
        return {"rounds": int(res.rounds), "samples": int(res.samples), "gpu_ms": float(res.gpu_ms),
                "mean_spp": int(res.samples) / npix}

    @property
    def adaptive(self) -> bool:
        """The buffer holds an adaptive render (pixels with different numbers of calls): until the next render
        writes it.  While it is true, moments() and the image calls succeed, whatever scene, texture or RNG
        state was set since."""
        return bool(N.host().pth_renderer_adaptive(self._r))

    def moments(self) -> np.ndarray:
        """Per-pixel luminance moments of the last adaptive render: rows x width x 3 float32 (m1, m2,
        and n as uint32 bits -- sample_counts() gives it as integers)."""
        self._single("moments")
        out = np.zeros((self.rows, self.width, 3), dtype=np.float32)
        N.check_ctx(N.hip().pt_read_moments(self._ctx, out.ctypes.data_as(C.POINTER(C.c_float))), self._ctx)
        return out

    def sample_counts(self) -> np.ndarray:
        """render() calls folded into each pixel by the last adaptive render (rows x width uint32)."""
        return np.ascontiguousarray(self.moments()[..., 2]).view(np.uint32)

    def noise_map(self) -> np.ndarray:
        """Relative standard error of each pixel's mean per-call luminance (rows x width float32):
        sqrt(max(m2 - m1^2 / n, 0) / (n (n - 1))) / |m1 / n|; 0 where the mean is 0, NaN where the
        pixel is not finite or has fewer than 2 calls."""
        m = self.moments()
        n = self.sample_counts().astype(np.float32)
        with np.errstate(all="ignore"):
            mean = m[..., 0] / n
            se = np.sqrt(np.maximum(m[..., 1] - m[..., 0] * mean, 0) / (n * (n - 1)))
            out = np.where(mean == 0, np.float32(0), se / np.abs(mean)).astype(np.float32)
        out[n < 2] = np.nan
        return out

    # --- first-hit features and the denoiser (pt_render_features, pt_denoise; pt_hip.h) -------------
    def features(self, camera: PtCamera) -> Dict[str, np.ndarray]:
        """Trace each pixel's first-sample ray and return its closest hit (rows x width arrays): "albedo"
        (x 3), "primitive" (uint32, 0xffffffff on a miss), "normal" (x 3, turned against the ray),
        "depth" (the hit distance), "position" (x 3), "hit" and "emissive" (bool), and "planes": the three
        raw float4 planes as denoise_image() takes them.  Touches nothing of the render state."""
        self._single("features")
        N.check_ctx(N.hip().pt_render_features(self._ctx, C.byref(camera)), self._ctx)
        planes = []
        for k in range(3):
            p = np.zeros((self.rows, self.width, 4), dtype=np.float32)
            N.check_ctx(N.hip().pt_read_features(self._ctx, k, p.ctypes.data_as(C.POINTER(C.c_float))), self._ctx)
            planes.append(p)
        flags = np.ascontiguousarray(planes[2][..., 3]).view(np.uint32)
        self._planes = planes
        return {"albedo": planes[0][..., :3].copy(), "primitive": np.ascontiguousarray(planes[0][..., 3]).view(np.uint32),
                "normal": planes[1][..., :3].copy(), "depth": planes[1][..., 3].copy(),
                "position": planes[2][..., :3].copy(), "hit": (flags & N.PT_FEATURE_HIT) != 0,
                "emissive": (flags & N.PT_FEATURE_EMISSIVE) != 0, "planes": planes}

    def denoise(self, iterations: int = 5, sigma_color: Optional[float] = None, sigma_plane: Optional[float] = None,
                normal_power_log2: Optional[int] = None, demodulate: Optional[bool] = None,
                same_primitive: Optional[bool] = None, staging: int = 0, frames: Optional[int] = None,
                source: str = "accumulation", guide: str = "color", sigma_l: Optional[float] = None,
                variance_floor: Optional[float] = None, feedback: int = 0, min_batches: Optional[int] = None,
                normal_cos_min: Optional[float] = None, window_sigma_plane: Optional[float] = None) -> np.ndarray:
        """Filter the image with the edge-avoiding a-trous denoiser (include/pt_hip.h), guided by the
        planes of the last features(camera) call; returns rows x width x 4 float32 in
        get_hdr_image_data()'s units and leaves the accumulation as it is.  sigma_color=None: a factor times
        the median luminance of the kept pixels (auto_sigma_color).  `frames`: the divisor of the
        accumulation (default: the frame counter; an adaptive render divides every pixel by its own count).
        source="temporal": the image of the last temporal() is filtered instead (pt_denoise_temporal), guided
        by the planes it was made from; the automatic sigma is then of that image.
        guide="variance" (with source="temporal", after temporal(variance=True)): the colour weight follows the
        per-pixel variance of that step instead of one sigma_color (pt_denoise_variance); sigma_l is in
        standard deviations of the luminance, variance_floor keeps the weight defined where the variance is 0.
        feedback=L (1..iterations; only with source="temporal", guide="variance"): the same result, and the output
        of iteration L - 1 becomes the colour of the held history, which the next temporal(variance=True)
        reprojects (pt_denoise_variance_feedback).  0: no feedback.
        guide="adaptive" (with source="accumulation", after render_adaptive and features): the same filter, its
        variance made from the adaptive render's own per-pixel moments (pt_denoise_adaptive; adaptive_variance()
        returns it).  A pixel with fewer than `min_batches` calls takes the larger of its own estimate and the
        spread of its 7 x 7 same-surface window, whose plane and normal tests take `window_sigma_plane` and
        `normal_cos_min`; sigma_l (default ADENOISE_SIGMA_L), variance_floor and the rest are the filter's as with
        guide="variance".
        source="despiked": the plain filter on the image the last despike() left (pt_denoise_despiked); only with
        guide="color" and without feedback.
        Arguments out of range raise before any device call."""
        self._single("denoise")
        if source not in ("accumulation", "temporal", "despiked"):
            raise _refuse(f"denoise: source must be 'accumulation', 'temporal' or 'despiked', not {source!r}")
        if source == "despiked":
            if guide != "color":
                raise _refuse("denoise: source='despiked' needs guide='color' (the moments of the variance-guided "
                              "filters describe the unclamped colour)")
            if feedback != 0:
                raise _refuse("denoise: feedback is not used with source='despiked' (there is no temporal history to feed)")
            if frames is not None:
                raise _refuse("denoise: frames is not used with source='despiked' (despike() has divided already)")
        if guide not in ("color", "variance", "adaptive"):
            raise _refuse(f"denoise: guide must be 'color', 'variance' or 'adaptive', not {guide!r}")
        if guide == "adaptive":
            if source != "accumulation":
                raise _refuse("denoise: guide='adaptive' needs source='accumulation' (the variance is of the adaptive "
                              "render's own moments)")
            if sigma_color is not None:
                raise _refuse("denoise: sigma_color is not used with guide='adaptive' (give sigma_l)")
            if feedback != 0:
                raise _refuse("denoise: feedback is not used with guide='adaptive' (there is no temporal history to feed)")
            if frames is not None:
                raise _refuse("denoise: frames is not used with guide='adaptive' (every pixel is divided by its own count)")
            vparams = vdenoise_params(iterations, ADENOISE_SIGMA_L if sigma_l is None else sigma_l, variance_floor,
                                      sigma_plane, normal_power_log2, demodulate, same_primitive, staging)
            aparams = adaptive_variance_params(min_batches, window_sigma_plane, normal_cos_min,
                                               bool(vparams.flags & N.PT_DENOISE_DEMODULATE), same_primitive)
            N.check_ctx(N.hip().pt_denoise_adaptive(self._ctx, C.byref(aparams), C.byref(vparams)), self._ctx)
            return self.denoised()
        if min_batches is not None or normal_cos_min is not None or window_sigma_plane is not None:
            raise _refuse("denoise: min_batches, normal_cos_min and window_sigma_plane are given without guide='adaptive'")
        if feedback != 0 and (source != "temporal" or guide != "variance"):
            raise _refuse("denoise: feedback needs source='temporal' and guide='variance' (it feeds the temporal history)")
        if guide == "variance":
            if source != "temporal":
                raise _refuse("denoise: guide='variance' needs source='temporal' (the variance is the temporal history's)")
            if sigma_color is not None:
                raise _refuse("denoise: sigma_color is not used with guide='variance' (give sigma_l)")
            vparams = vdenoise_params(iterations, sigma_l, variance_floor, sigma_plane, normal_power_log2, demodulate,
                                      same_primitive, staging)
            if feedback != 0:
                fb = vfeedback_params(feedback, vparams.iterations)
                N.check_ctx(N.hip().pt_denoise_variance_feedback(self._ctx, C.byref(vparams), C.byref(fb)), self._ctx)
                return self.denoised()
            N.check_ctx(N.hip().pt_denoise_variance(self._ctx, C.byref(vparams)), self._ctx)
            return self.denoised()
        if sigma_l is not None or variance_floor is not None:
            raise _refuse("denoise: sigma_l and variance_floor are given without guide='variance'")
        demod = DENOISE_DEFAULTS["demodulate"] if demodulate is None else demodulate
        params = denoise_params(iterations, 1.0 if sigma_color is None else sigma_color, sigma_plane, normal_power_log2,
                                demod, same_primitive, staging)
        if source == "temporal":
            if sigma_color is None:
                planes = getattr(self, "_planes", None)
                if planes is None:
                    raise PathtracerError(N.PT_ERR_STATE, "denoise: no feature planes (call features(camera) first)")
                params.sigma_color = auto_sigma_color(self.temporal_image(), *planes, demodulate=demod)
            N.check_ctx(N.hip().pt_denoise_temporal(self._ctx, C.byref(params)), self._ctx)
            return self.denoised()
        if source == "despiked":
            if sigma_color is None:
                planes = getattr(self, "_planes", None)
                if planes is None:
                    raise PathtracerError(N.PT_ERR_STATE, "denoise: no feature planes (call features(camera) first)")
                params.sigma_color = auto_sigma_color(self.despiked(), *planes, demodulate=demod)
            N.check_ctx(N.hip().pt_denoise_despiked(self._ctx, C.byref(params)), self._ctx)
            return self.denoised()
        f = self.frames if frames is None else int(frames)
        if sigma_color is None:
            planes = getattr(self, "_planes", None)
            if planes is None:
                raise PathtracerError(N.PT_ERR_STATE, "denoise: no feature planes (call features(camera) first)")
            if N.hip().pt_holds_adaptive(self._ctx):
                # the image pt_denoise filters (pt_read_adaptive_hdr's arithmetic), never an earlier denoised one
                color = self.accum() / np.maximum(self.sample_counts(), 1).astype(np.float32)[..., None]
            else:
                color = self.accum() * (np.float32(1.0) / np.float32(max(f, 1)))
            params.sigma_color = auto_sigma_color(color, *planes, demodulate=demod)
        N.check_ctx(N.hip().pt_denoise(self._ctx, f, C.byref(params)), self._ctx)
        return self.denoised()

    # --- despike, the same-surface firefly clamp (pt_despike; rule 6 of pt_hip.h) ---------------------
    def despike(self, radius: Optional[int] = None, rank: Optional[int] = None, factor: Optional[float] = None,
                floor: Optional[float] = None, min_neighbors: Optional[int] = None, sigma_plane: Optional[float] = None,
                normal_cos_min: Optional[float] = None, demodulate: Optional[bool] = None,
                same_primitive: Optional[bool] = None, staging: int = 0, frames: Optional[int] = None) -> np.ndarray:
        """Clamp the fireflies of the image (include/pt_hip.h, rule 6): a pixel whose luminance is above `factor`
        times the `rank`-th largest of its same-surface neighbours within `radius`, plus `floor`, is scaled down to
        that limit; every other pixel keeps its words.  Guided by the planes of the last features(camera) call;
        returns rows x width x 4 float32 in get_hdr_image_data()'s units and leaves the accumulation as it is.
        denoise(source="despiked") filters the result; despike_count() tells how many pixels were clamped.
        Arguments out of range raise before any device call."""
        self._single("despike")
        params = despike_params(radius, rank, factor, floor, min_neighbors, sigma_plane, normal_cos_min, demodulate,
                                same_primitive, staging)
        f = self.frames if frames is None else int(frames)
        if not 0 <= f <= 0xffffffff:
            raise _refuse(f"despike: frames must be 0..2^32 - 1, not {frames!r}")
        N.check_ctx(N.hip().pt_despike(self._ctx, f, C.byref(params)), self._ctx)
        return self.despiked()

    def despiked(self) -> np.ndarray:
        """The held despiked image again (pt_read_despiked): until a render, features(), or a scene, texture or sky
        change."""
        self._single("despiked")
        out = np.zeros((self.rows, self.width, 4), dtype=np.float32)
        N.check_ctx(N.hip().pt_read_despiked(self._ctx, out.ctypes.data_as(C.POINTER(C.c_float))), self._ctx)
        return out

    def tonemap_despiked(self) -> np.ndarray:
        """The held despiked image through the tonemap (RGBA8, rows x width)."""
        self._single("tonemap_despiked")
        out = np.zeros((self.rows, self.width, 4), dtype=np.uint8)
        N.check_ctx(N.hip().pt_tonemap_despiked(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint8))), self._ctx)
        return out

    def despike_count(self) -> int:
        """The number of pixels the last despike() clamped (pt_read_despike_count)."""
        self._single("despike_count")
        n = C.c_uint32(0)
        N.check_ctx(N.hip().pt_read_despike_count(self._ctx, C.byref(n)), self._ctx)
        return int(n.value)

    def despike_timing(self) -> Dict[str, float]:
        """Kernel times of the last despike() in ms (hipEvents): {"prepare", "despike"}."""
        self._single("despike_timing")
        ms = (C.c_float * 2)()
        N.check_ctx(N.hip().pt_read_despike_timing(self._ctx, ms), self._ctx)
        return {"prepare": float(ms[0]), "despike": float(ms[1])}

    # --- guided upsampling of a low-resolution render (pt_upsample; rule 8 of pt_hip.h) ----------------
    def upsample(self, lo: "Pathtracer", source: str = "accum", frames: Optional[int] = None,
                 sigma_plane: Optional[float] = None, normal_power_log2: Optional[int] = None,
                 demodulate: Optional[bool] = None, same_primitive: Optional[bool] = None, staging: int = 0,
                 planes: Optional["Pathtracer"] = None) -> np.ndarray:
        """Reconstruct this Pathtracer's frame from the image of `lo`, a Pathtracer of the same scene and camera at a
        lower resolution (include/pt_hip.h, rule 8): every pixel takes the demodulated colour of the low pixels around
        it that lie on its surface, times its own albedo.  Both need the planes of a features(camera) call; this one
        needs no render.  source: "accum" (lo's render, over `frames`, default lo.frames), "denoised", "temporal" or
        "despiked" (what lo holds).  Returns rows x width x 4 float32 and leaves both render states as they are.
        planes: a Pathtracer of the same scene and camera at exactly 2, 3 or 4 times this one's width and height that
        has had features(camera); every pixel is then the mean of the result at its S x S first-hit samples, which
        antialiases the silhouettes (rule 9, pt_upsample_resolve), and this Pathtracer needs no features of its own.
        Arguments out of range raise before any device call."""
        self._single("upsample")
        params = upsample_params(sigma_plane, normal_power_log2, demodulate, same_primitive, staging)
        if source not in UPSAMPLE_SOURCES:
            raise _refuse(f"upsample: source must be 'accum', 'denoised', 'temporal' or 'despiked', not {source!r}")
        if not isinstance(lo, Pathtracer):
            raise _refuse(f"upsample: lo must be a Pathtracer, not {type(lo).__name__}")
        lo._single("upsample")
        if frames is not None and source != "accum":
            raise _refuse(f"upsample: frames is not used with source={source!r} (the held image has been divided already)")
        f = lo.frames if frames is None else int(frames)
        if not 0 <= f <= 0xffffffff:
            raise _refuse(f"upsample: frames must be 0..2^32 - 1, not {frames!r}")
        if planes is not None:
            if not isinstance(planes, Pathtracer):
                raise _refuse(f"upsample: planes must be a Pathtracer, not {type(planes).__name__}")
            planes._single("upsample")
            factor = planes.width // self.width       # (anything but exactly 2..4 times this frame is refused by name)
            N.check_ctx(N.hip().pt_upsample_resolve(self._ctx, planes._ctx, lo._ctx, UPSAMPLE_SOURCES[source], f, factor,
                                                    C.byref(params)), self._ctx)
            return self.upsampled()
        N.check_ctx(N.hip().pt_upsample(self._ctx, lo._ctx, UPSAMPLE_SOURCES[source], f, C.byref(params)), self._ctx)
        return self.upsampled()

    def upsampled(self) -> np.ndarray:
        """The held upsampled image again (pt_read_upsampled): until the next upsample() begins."""
        self._single("upsampled")
        out = np.zeros((self.rows, self.width, 4), dtype=np.float32)
        N.check_ctx(N.hip().pt_read_upsampled(self._ctx, out.ctypes.data_as(C.POINTER(C.c_float))), self._ctx)
        return out

    def tonemap_upsampled(self) -> np.ndarray:
        """The held upsampled image through the tonemap (RGBA8, rows x width)."""
        self._single("tonemap_upsampled")
        out = np.zeros((self.rows, self.width, 4), dtype=np.uint8)
        N.check_ctx(N.hip().pt_tonemap_upsampled(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint8))), self._ctx)
        return out

    def upsample_counts(self) -> Dict[str, int]:
        """Of the last upsample(): {"wide": guided pixels that needed the second ring, "nearest": guided pixels no tap
        of either ring served, which took the nearest low pixel} (pt_read_upsample_counts).  After upsample(lo,
        planes=...) both count first-hit samples, up to S * S per pixel."""
        self._single("upsample_counts")
        n = (C.c_uint32 * 2)()
        N.check_ctx(N.hip().pt_read_upsample_counts(self._ctx, n), self._ctx)
        return {"wide": int(n[0]), "nearest": int(n[1])}

    def upsample_timing(self) -> Dict[str, float]:
        """Kernel times of the last upsample() in ms (hipEvents): {"prepare", "upsample"}."""
        self._single("upsample_timing")
        ms = (C.c_float * 2)()
        N.check_ctx(N.hip().pt_read_upsample_timing(self._ctx, ms), self._ctx)
        return {"prepare": float(ms[0]), "upsample": float(ms[1])}

    def adaptive_variance(self) -> np.ndarray:
        """The per-pixel variance the last denoise(guide="adaptive") made (pt_read_adaptive_variance): rows x width
        float32, of the luminance of the (demodulated) colour; -1 where the pixel is not a finite, non-emissive
        hit or has fewer than two calls.  Held until a render writes the accumulation or features() runs."""
        self._single("adaptive_variance")
        out = np.zeros((self.rows, self.width), dtype=np.float32)
        N.check_ctx(N.hip().pt_read_adaptive_variance(self._ctx, out.ctypes.data_as(C.POINTER(C.c_float))), self._ctx)
        return out

    def adaptive_variance_timing(self) -> float:
        """Kernel time of the window estimate of the last denoise(guide="adaptive") in ms (hipEvents)."""
        self._single("adaptive_variance_timing")
        ms = C.c_float(0.0)
        N.check_ctx(N.hip().pt_read_adaptive_variance_timing(self._ctx, C.byref(ms)), self._ctx)
        return float(ms.value)

    def denoised(self) -> np.ndarray:
        """The last denoise()'s result again (pt_read_denoised)."""
        self._single("denoised")
        out = np.zeros((self.rows, self.width, 4), dtype=np.float32)
        N.check_ctx(N.hip().pt_read_denoised(self._ctx, out.ctypes.data_as(C.POINTER(C.c_float))), self._ctx)
        return out

    def tonemap_denoised(self) -> np.ndarray:
        """The last denoise()'s result through the tonemap (RGBA8, rows x width)."""
        self._single("tonemap_denoised")
        out = np.zeros((self.rows, self.width, 4), dtype=np.uint8)
        N.check_ctx(N.hip().pt_tonemap_denoised(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint8))), self._ctx)
        return out

    def denoise_timing(self) -> Dict[str, object]:
        """Kernel times of the last features() and denoise() in ms: {"features", "prepare", "iterations", "finish"}."""
        self._single("denoise_timing")
        ms = (C.c_float * 10)()
        fm = C.c_float(0.0)
        N.check_ctx(N.hip().pt_read_denoise_timing(self._ctx, ms), self._ctx)
        N.check_ctx(N.hip().pt_read_features_timing(self._ctx, C.byref(fm)), self._ctx)
        return {"features": float(fm.value), "prepare": float(ms[0]), "iterations": [float(x) for x in ms[1:9]],
                "finish": float(ms[9])}

    # --- temporal reprojection (pt_temporal; pt_hip.h) ---------------------------------------------
    def temporal(self, alpha_min: Optional[float] = None, max_history: Optional[int] = None,
                 sigma_plane: Optional[float] = None, normal_cos_min: Optional[float] = None, demodulate: Optional[bool] = None,
                 same_primitive: Optional[bool] = None, reset: bool = False, frames: Optional[int] = None,
                 variance: bool = False, min_temporal: Optional[int] = None) -> np.ndarray:
        """One step of temporal accumulation (include/pt_hip.h): the result of the previous temporal() is
        reprojected into the camera of the last features(camera) through its planes, rejected where it is no
        longer the same surface, and the current image blended in.  Call order per frame:
        render(cam, spp, True), features(cam), temporal().  Returns the image, rows x width x 4 float32 in
        get_hdr_image_data()'s units with w = the history length; `history_used` tells whether a previous
        history was held (none after reset=True, a scene load, a texture or another sky).  Touches nothing of
        the render state.  Arguments out of range raise before any device call.
        variance=True (pt_temporal_moments): the same image word for word, and luminance moments are carried in
        the history and a per-pixel variance estimated from them (temporal_variance(); min_temporal = the
        history length from which the temporal estimate is trusted); a history left by a step without
        variance is not used."""
        self._single("temporal")
        params = temporal_params(alpha_min, max_history, sigma_plane, normal_cos_min, demodulate, same_primitive)
        f = self.frames if frames is None else int(frames)
        used = C.c_int(0)
        if variance:
            vparams = variance_params(min_temporal)
            N.check_ctx(N.hip().pt_temporal_moments(self._ctx, f, C.byref(params), C.byref(vparams), int(bool(reset)),
                                                    C.byref(used)), self._ctx)
        else:
            if min_temporal is not None:
                raise _refuse("temporal: min_temporal is given without variance=True")
            N.check_ctx(N.hip().pt_temporal(self._ctx, f, C.byref(params), int(bool(reset)), C.byref(used)), self._ctx)
        self.history_used = bool(used.value)
        return self.temporal_image()

    def temporal_variance(self) -> np.ndarray:
        """The per-pixel variance of the last temporal(variance=True) (pt_read_temporal_variance): rows x width
        float32, of the luminance of the (demodulated) colour; -1 where the pixel is not a finite hit."""
        self._single("temporal_variance")
        out = np.zeros((self.rows, self.width), dtype=np.float32)
        N.check_ctx(N.hip().pt_read_temporal_variance(self._ctx, out.ctypes.data_as(C.POINTER(C.c_float))), self._ctx)
        return out

    def temporal_moments_timing(self) -> Dict[str, float]:
        """Kernel times of the last temporal(variance=True) in ms (hipEvents): {"step", "estimate"}."""
        self._single("temporal_moments_timing")
        ms = (C.c_float * 2)()
        N.check_ctx(N.hip().pt_read_temporal_moments_timing(self._ctx, ms), self._ctx)
        return {"step": float(ms[0]), "estimate": float(ms[1])}

    def temporal_history(self):
        """The held history (pt_read_temporal_history): (h0, h1, h2, h3), rows x width x 4 float32 each -- (I, n),
        (N, id), (P, t), (m1, m2, v, 0) -- as temporal_moments_image() takes it; h3 is None while the history has
        no moments.  After denoise(feedback=L) h0 holds the fed colours."""
        self._single("temporal_history")
        fp = C.POINTER(C.c_float)
        planes = []
        for k in range(3):
            p = np.zeros((self.rows, self.width, 4), dtype=np.float32)
            N.check_ctx(N.hip().pt_read_temporal_history(self._ctx, k, p.ctypes.data_as(fp)), self._ctx)
            planes.append(p)
        p = np.zeros((self.rows, self.width, 4), dtype=np.float32)
        rc = N.hip().pt_read_temporal_history(self._ctx, 3, p.ctypes.data_as(fp))
        if rc == N.PT_ERR_ARG:
            planes.append(None)
        else:
            N.check_ctx(rc, self._ctx)
            planes.append(p)
        return tuple(planes)

    def feedback_timing(self) -> float:
        """Kernel time of the feedback of the last denoise(feedback=L) in ms (hipEvents)."""
        self._single("feedback_timing")
        ms = C.c_float(0.0)
        N.check_ctx(N.hip().pt_read_feedback_timing(self._ctx, C.byref(ms)), self._ctx)
        return float(ms.value)

    def temporal_image(self) -> np.ndarray:
        """The last temporal()'s image again (pt_read_temporal)."""
        self._single("temporal_image")
        out = np.zeros((self.rows, self.width, 4), dtype=np.float32)
        N.check_ctx(N.hip().pt_read_temporal(self._ctx, out.ctypes.data_as(C.POINTER(C.c_float))), self._ctx)
        return out

    def history_lengths(self) -> np.ndarray:
        """The history length n of every pixel after the last temporal() (rows x width float32; 0 = not a
        finite hit, 1 = this frame alone)."""
        return self.temporal_image()[..., 3].copy()

    def tonemap_temporal(self) -> np.ndarray:
        """The last temporal()'s image through the tonemap (RGBA8, rows x width)."""
        self._single("tonemap_temporal")
        out = np.zeros((self.rows, self.width, 4), dtype=np.uint8)
        N.check_ctx(N.hip().pt_tonemap_temporal(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint8))), self._ctx)
        return out

    def temporal_timing(self) -> float:
        """Kernel time of the last temporal() in ms (hipEvents)."""
        self._single("temporal_timing")
        ms = C.c_float(0.0)
        N.check_ctx(N.hip().pt_read_temporal_timing(self._ctx, C.byref(ms)), self._ctx)
        return float(ms.value)

    def get_timing(self) -> float:
        return float(N.host().pth_renderer_timing(self._r))

    @property
    def frames(self) -> int:
        return int(N.host().pth_renderer_frames(self._r))

    def get_hdr_image_data(self) -> np.ndarray:
        p = N.host().pth_renderer_hdr(self._r)
        if not p:
            N.check_host(N.PT_ERR_HIP)
        return np.ctypeslib.as_array(p, shape=(self.rows, self.width, 4)).copy()

    def get_image_data(self) -> np.ndarray:
        p = N.host().pth_renderer_image(self._r)
        if not p:
            N.check_host(N.PT_ERR_HIP)
        return np.ctypeslib.as_array(p, shape=(self.rows, self.width, 4)).copy()

    # --- device-layer access (C ABI of pt_hip.h) ------------------------------------------------
    def accum(self) -> np.ndarray:
        """Raw accumulation sums (rows x width x 4 float32); the gathered full image for a group."""
        out = np.zeros((self.rows, self.width, 4), dtype=np.float32)
        if self._group:
            N.check_group(N.hip().pt_group_read_accum(self._group, out.ctypes.data_as(C.POINTER(C.c_float))), self._group)
        else:
            N.check_ctx(N.hip().pt_read_accum(self._ctx, out.ctypes.data_as(C.POINTER(C.c_float))), self._ctx)
        return out

    def gather(self) -> float:
        """Group only: RCCL gather of every device's rows to devices[0]; returns its wall time in ms."""
        ms = C.c_float(0.0)
        N.check_group(N.hip().pt_group_gather(self._group, C.byref(ms)), self._group)
        return float(ms.value)

    def rng_state(self) -> np.ndarray:
        out = np.zeros((self.rows, self.width, 6), dtype=np.uint32)
        if self._group:
            for c, gy in self._group_rows():
                part = np.zeros((gy.size, self.width, 6), dtype=np.uint32)
                N.check_ctx(N.hip().pt_read_rng(c, part.ctypes.data_as(C.POINTER(C.c_uint32))), c)
                out[gy] = part
            return out
        N.check_ctx(N.hip().pt_read_rng(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint32))), self._ctx)
        return out

    def set_rng_state(self, state: np.ndarray) -> None:
        s = np.ascontiguousarray(state, dtype=np.uint32)
        if s.shape != (self.rows, self.width, 6):
            raise PathtracerError(N.PT_ERR_ARG, f"set_rng_state: shape {s.shape}, expected {(self.rows, self.width, 6)}")
        if self._group:
            for c, gy in self._group_rows():
                part = np.ascontiguousarray(s[gy])
                N.check_ctx(N.hip().pt_write_rng(c, part.ctypes.data_as(C.POINTER(C.c_uint32))), c)
            return
        N.check_ctx(N.hip().pt_write_rng(self._ctx, s.ctypes.data_as(C.POINTER(C.c_uint32))), self._ctx)

    def render_raw(self, camera: PtCamera, spp: int, chunks: int, ignore_history: bool) -> float:
        """Device-layer launch without frame accounting; returns the kernel time in ms (a group: every
        device concurrently, the slowest device's time; the next image read gathers again)."""
        ms = C.c_float(0.0)
        if self._group:
            N.check_group(N.hip().pt_group_render(self._group, C.byref(camera), int(spp), int(chunks),
                                                  int(bool(ignore_history)), C.byref(ms)), self._group)
            return float(ms.value)
        N.check_ctx(N.hip().pt_render(self._ctx, C.byref(camera), int(spp), int(chunks), int(bool(ignore_history)),
                                      C.byref(ms)), self._ctx)
        return float(ms.value)

    def render_instrumented(self, camera: PtCamera, spp: int, chunks: int, ignore_history: bool) -> Dict[str, int]:
        self._single("render_instrumented")
        ms = C.c_float(0.0)
        st = PtRenderStats()
        N.check_ctx(N.hip().pt_render_instrumented(self._ctx, C.byref(camera), int(spp), int(chunks),
                                                   int(bool(ignore_history)), C.byref(ms), C.byref(st)), self._ctx)
        d = {name: int(getattr(st, name)) for name, _ in PtRenderStats._fields_}
        d["ms"] = float(ms.value)
        return d

    def set_kernel_variant(self, variant: int) -> None:
        """pt_set_kernel_variant on every device context."""
        for c in self._contexts():
            N.check_ctx(N.hip().pt_set_kernel_variant(c, int(variant)), c)

    def set_occupancy(self, workgroups_per_cu: int) -> None:
        """Persistent grids hold at most this many 4-wave workgroups per CU (waves per SIMD); 0 = all
        that fit (pt_set_occupancy).  A measurement knob: results are identical."""
        for c in self._contexts():
            N.check_ctx(N.hip().pt_set_occupancy(c, int(workgroups_per_cu)), c)

    def set_issue_priority(self, mode: int, level3: int = 0, level2: int = 0, level1: int = 0) -> None:
        """Issue priority by cost-order position (pt_set_issue_priority): mode 0 automatic, 1 off,
        2 explicit (positions < level3 at priority 3, < level2 at 2, < level1 at 1).  Results are
        identical."""
        for c in self._contexts():
            N.check_ctx(N.hip().pt_set_issue_priority(c, int(mode), int(level3), int(level2), int(level1)), c)

    def set_schedule(self, mode: int) -> None:
        """0 = cost-sorted tile dispatch (default), 1 = row-major (pt_set_schedule), every device."""
        for c in self._contexts():
            N.check_ctx(N.hip().pt_set_schedule(c, int(mode)), c)

    def set_strip_units(self, mode: int) -> None:
        """pt_set_strip_units on every device context (0 automatic, 1 off, K >= 2 always K tiles per unit)."""
        for c in self._contexts():
            N.check_ctx(N.hip().pt_set_strip_units(c, int(mode)), c)

    def set_run_ahead(self, mode: int) -> None:
        """Run-ahead across render() calls (pt_set_run_ahead): 0 automatic, 1 off, 2 always make a
        stash, 3 make stashes but never use them (diagnostic).  Results are the reference's for every
        setting."""
        for c in self._contexts():
            N.check_ctx(N.hip().pt_set_run_ahead(c, int(mode)), c)

    def set_cold_start(self, prepass_spp: int = 0, priority: bool = True) -> None:
        """Cold-start scheduling (pt_set_cold_start): cost pre-pass spp (0 = default) and issue
        priority on the pre-pass's order.  Results are identical for every setting."""
        for c in self._contexts():
            N.check_ctx(N.hip().pt_set_cold_start(c, int(prepass_spp), int(bool(priority))), c)

    def set_rise_repair(self, enabled: bool) -> None:
        """Test knob (pt_set_rise_repair): False skips the rebuild of the pending far children after a
        leaf raised t_max, so results are NOT the reference's on such rays (negative control)."""
        for c in self._contexts():
            N.check_ctx(N.hip().pt_set_rise_repair(c, int(bool(enabled))), c)

    def set_zero_quadric_consts(self, shape_type: int) -> None:
        """Test knob (pt_set_zero_quadric_consts): the next scene upload replaces the quadric constants of
        every primitive of this shape type (-1 = none): zeros for a quadric (results are NOT the reference's),
        NaN for a disk, quad or cube (never read: results unchanged)."""
        for c in self._contexts():
            N.check_ctx(N.hip().pt_set_zero_quadric_consts(c, int(shape_type)), c)

    def set_sample_groups(self, mode: int) -> None:
        """Speculative sample groups (pt_set_sample_groups): 0 = automatic, 1 = off, G >= 2 = always G."""
        for c in self._contexts():
            N.check_ctx(N.hip().pt_set_sample_groups(c, int(mode)), c)

    @property
    def last_sample_groups(self) -> int:
        """Groups of the last launch (a device group: the largest over its devices)."""
        return max(int(N.hip().pt_last_sample_groups(c)) for c in self._contexts())

    @property
    def last_variant(self) -> int:
        """Trace-kernel variant of the last launch's main pass (a device group: device 0's)."""
        return int(N.hip().pt_last_variant(self._contexts()[0]))

    @property
    def last_launch(self) -> Dict[str, int]:
        """The last trace launch (pt_last_launch): dynamic LDS bytes of a workgroup, what it staged
        in LDS (0 nothing, 1 records or nodes, 2 primitives too), waves per workgroup, workgroups."""
        self._single("last_launch")
        out = (C.c_uint32 * 4)()
        N.check_ctx(N.hip().pt_last_launch(self._ctx, out), self._ctx)
        return {"lds_bytes": int(out[0]), "staged": int(out[1]), "waves_per_group": int(out[2]), "groups": int(out[3])}

    def set_patch_rounds(self, rounds: int) -> None:
        for c in self._contexts():
            N.check_ctx(N.hip().pt_set_patch_rounds(c, int(rounds)), c)

    def set_group_lookback(self, far: int = 64, near: int = 16) -> None:
        """Sample groups: a second phase also stops on a junction with its first phase `far` or
        `near` samples back (0 = off).  Scheduling only (pt_set_group_lookback)."""
        for c in self._contexts():
            N.check_ctx(N.hip().pt_set_group_lookback(c, int(far), int(near)), c)

    def group_fold_word(self, word: int) -> np.ndarray:
        """Diagnostics: a plane of the grouped launch's fold state (pt_read_group_fold); words 19 /
        20 / 21 = the guess statistics (float32): draw pairs per sample, odd-length fraction, variance."""
        self._single("group_fold_word")
        out = np.zeros((self.rows, self.width), dtype=np.uint32)
        N.check_ctx(N.hip().pt_read_group_fold(self._ctx, int(word), out.ctypes.data_as(C.POINTER(C.c_uint32))), self._ctx)
        return out.view(np.float32) if word >= 19 else out

    def group_stats(self) -> Dict[str, object]:
        """How the last grouped launch went: groups, patch rounds, dead-end pixels after each fold."""
        self._single("group_stats")
        out = (C.c_uint32 * 10)()
        N.check_ctx(N.hip().pt_read_group_stats(self._ctx, out), self._ctx)
        v = list(out)
        return {"groups": v[0], "patch_rounds": v[1], "dead_ends": v[2:2 + v[1] + 1] if v[0] else []}

    def group_log_counts(self) -> np.ndarray:
        """Samples each (tile, item) of the last grouped launch logged: (tiles, 2 * groups - 1, 64), tiles
        in dispatch (cost) order; item 0 = group 0, items 2g - 1 and 2g = group g at its guess and one
        draw pair later."""
        self._single("group_log_counts")
        g = 2 * self.last_sample_groups - 1
        tiles = ((self.width + 7) // 8) * ((self.rows + 7) // 8)
        out = np.zeros((tiles, g, 64), dtype=np.uint32)
        N.check_ctx(N.hip().pt_read_group_log_counts(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size),
                    self._ctx)
        return out

    def tile_costs(self) -> np.ndarray:
        """Shader-clock cycles of each 8x8 tile in the last launch (tiles_y x tiles_x)."""
        self._single("tile_costs")
        tx, ty = (self.width + 7) // 8, (self.rows + 7) // 8
        out = np.zeros(tx * ty, dtype=np.uint32)
        N.check_ctx(N.hip().pt_read_tile_costs(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint32)), tx * ty), self._ctx)
        return out.reshape(ty, tx)

    def tile_idle(self) -> np.ndarray:
        """Per tile of the last instrumented launch: mean lane cycles spent done while the tile ran
        (tiles_y x tiles_x; divide by tile_costs() for the idle-lane fraction)."""
        self._single("tile_idle")
        tx, ty = (self.width + 7) // 8, (self.rows + 7) // 8
        out = np.zeros(tx * ty, dtype=np.uint32)
        N.check_ctx(N.hip().pt_read_tile_idle(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint32)), tx * ty), self._ctx)
        return out.reshape(ty, tx)

    def set_tile_trace(self, enabled: bool) -> None:
        """Instrumented launches also record per tile the start cycle and hardware ids of the wave
        that ran it (diagnostics)."""
        for c in self._contexts():
            N.check_ctx(N.hip().pt_set_tile_trace(c, int(bool(enabled))), c)

    def tile_trace(self) -> np.ndarray:
        """Last traced launch: (tiles_y x tiles_x x 2) u32 -- start cycle (low 32 bits) and
        XCC_ID << 16 | HW_ID (bits 0-15) of the wave that ran each tile."""
        self._single("tile_trace")
        tx, ty = (self.width + 7) // 8, (self.rows + 7) // 8
        out = np.zeros(2 * tx * ty, dtype=np.uint32)
        N.check_ctx(N.hip().pt_read_tile_trace(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint32)), 2 * tx * ty),
                    self._ctx)
        return out.reshape(ty, tx, 2)

    def copy_accum_to_device(self, dst_ptr: int, nbytes: int) -> None:
        self._single("copy_accum_to_device")
        N.check_ctx(N.hip().pt_copy_accum_device(self._ctx, C.c_void_p(int(dst_ptr)), int(nbytes)), self._ctx)

    def tonemap_device(self, dst_ptr: int, nbytes: int, frames: Optional[int] = None) -> None:
        """Tonemap into a device buffer (RGBA8, rows x width) -- the pixel-buffer path of render()."""
        self._single("tonemap_device")
        f = self.frames if frames is None else int(frames)
        N.check_ctx(N.hip().pt_tonemap_device(self._ctx, f, C.c_void_p(int(dst_ptr)), int(nbytes)), self._ctx)

    def tonemap(self, frames: Optional[int] = None) -> np.ndarray:
        out = np.zeros((self.rows, self.width, 4), dtype=np.uint8)
        f = self.frames if frames is None else int(frames)
        if self._group:
            N.check_group(N.hip().pt_group_tonemap(self._group, f, out.ctypes.data_as(C.POINTER(C.c_uint8))), self._group)
            return out
        N.check_ctx(N.hip().pt_tonemap(self._ctx, f, out.ctypes.data_as(C.POINTER(C.c_uint8))), self._ctx)
        return out
