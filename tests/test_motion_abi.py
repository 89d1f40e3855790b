"""The C ABI and the Python arguments of the temporal passes across moved objects (rule 7 of include/pt_hip.h:
pt_set_scene_moved, pt_holds_motion and the two _motion_image forms; pth_renderer_load_scene_moved and pth_motion_table
of include/pt_host.h): the symbols are declared, exported and bound with the signatures the headers state, and every
refusal that can be reached without a device comes before any device call."""
import ctypes as C
import re

import numpy as np
import pytest

import pathtracercuda_amd as pa
from pathtracercuda_amd import _native as N

SYMBOLS = ("pt_set_scene_moved", "pt_holds_motion", "pt_temporal_motion_image", "pt_temporal_moments_motion_image")
HOST_SYMBOLS = ("pth_renderer_load_scene_moved", "pth_renderer_holds_motion", "pth_renderer_motion_table", "pth_motion_table")
P = C.POINTER
fp, up = P(C.c_float), P(C.c_uint32)
nan = float("nan")
BAD_TEMPORAL = ((dict(alpha_min=1.5), "alpha_min"), (dict(alpha_min=nan), "alpha_min"), (dict(max_history=0), "max_history"),
                (dict(sigma_plane=0.0), "sigma_plane"), (dict(sigma_plane=nan), "sigma_plane"),
                (dict(normal_cos_min=2.0), "normal_cos_min"), (dict(flags=4), "flags"))


def tparams(**over):
    v = dict(alpha_min=0.1, max_history=6, sigma_plane=0.05, normal_cos_min=0.9, flags=3)
    v.update(over)
    return N.PtTemporalParams(v["alpha_min"], v["max_history"], v["sigma_plane"], v["normal_cos_min"], v["flags"])


def test_symbols_are_declared_exported_and_bound(root):
    text = (root / "include" / "pt_hip.h").read_text()
    lib = N.hip()
    for name in SYMBOLS:
        assert re.search(rf"PT_API int {name}\(", text), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in N._HIP_SYMBOLS and getattr(lib, name).argtypes == N._HIP_SYMBOLS[name][1]
    assert N._HIP_SYMBOLS["pt_set_scene_moved"][1] == N._HIP_SYMBOLS["pt_set_scene"][1] + [fp, up]
    assert N._HIP_SYMBOLS["pt_holds_motion"][1] == [C.c_void_p]
    # the image forms take the arguments of the forms they follow, then prim_count, motion_rows, prev_index
    for name, base in (("pt_temporal_motion_image", "pt_temporal_image"),
                       ("pt_temporal_moments_motion_image", "pt_temporal_moments_image")):
        assert N._HIP_SYMBOLS[name][1] == N._HIP_SYMBOLS[base][1] + [C.c_uint32, fp, up]
        decl = re.search(rf"PT_API int {name}\((.*?)\);", text, re.S).group(1)
        base_decl = re.search(rf"PT_API int {base}\((.*?)\);", text, re.S).group(1)
        norm = lambda s: re.sub(r"\s+", " ", s).strip()
        assert norm(decl) == norm(base_decl) + ", uint32_t prim_count, const float *motion_rows, const uint32_t *prev_index"
    # no existing function's signature changed
    assert len(N._HIP_SYMBOLS["pt_temporal"][1]) == 5 and len(N._HIP_SYMBOLS["pt_temporal_moments"][1]) == 6
    assert len(N._HIP_SYMBOLS["pt_set_scene"][1]) == 5
    host_text = (root / "include" / "pt_host.h").read_text()
    for name in HOST_SYMBOLS:
        assert re.search(rf"{name}\(", host_text) and hasattr(N.host(), name) and name in N._HOST_SYMBOLS
    assert N._HOST_SYMBOLS["pth_renderer_load_scene_moved"][1] == [C.c_void_p, C.c_char_p, up, P(N.PtCamera)]
    assert N._HOST_SYMBOLS["pth_motion_table"][1] == [P(N.PtHittable), P(N.PtHittable), C.c_uint32, fp, up]
    for name in ("motion_table", "temporal_motion_image", "temporal_moments_motion_image", "NO_PREVIOUS"):
        assert name in pa.__all__
    for name in ("load_scene_moved", "holds_motion", "motion_table"):
        assert callable(getattr(pa.Pathtracer, name))
    assert pa.NO_PREVIOUS == 0xffffffff
    # the header says what the rule does not cover
    rule = text[text.index("Moving objects in the temporal passes"):text.index("PT_API int pt_set_scene_moved(")]
    for phrase in ("Not covered", "device groups", "command-line", "OTHER surfaces", "Nothing checks that", "not normalised"):
        assert phrase in rule, phrase


def test_set_scene_moved_without_a_context():
    lib = N.hip()
    rows = (C.c_float * 12)()
    prev = (C.c_uint32 * 1)()
    node, prim = N.PtBvhNode(), N.PtHittable()
    assert lib.pt_set_scene_moved(None, C.byref(node), 1, C.byref(prim), 1, rows, prev) == N.PT_ERR_ARG
    assert lib.pt_holds_motion(None) == 0                  # a question, never an error


def image_args(hist=True, table=True, params=None, width=4, height=4, count=2, moments=False):
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, fp)
    cam = N.PtCamera()
    rows = (C.c_float * 24)()
    prev = (C.c_uint32 * 2)()
    h = [ptr if hist else None] * (4 if moments else 3)
    args = [0, width, height, ptr, ptr, ptr, ptr, C.byref(cam), *h, C.byref(cam), C.byref(params or tparams())]
    if moments:
        args += [C.byref(N.PtVarianceParams(4))]
    args += [ptr] * (6 if moments else 4)
    args += [count, C.cast(rows, fp) if table else None, C.cast(prev, up) if table else None]
    return args, buf


@pytest.mark.parametrize("moments", (False, True), ids=("plain", "moments"))
def test_the_image_forms_refuse_before_touching_a_device(moments):
    lib = N.hip()
    call = lib.pt_temporal_moments_motion_image if moments else lib.pt_temporal_motion_image

    def refused(word, **kw):
        args, buf = image_args(moments=moments, **kw)
        assert call(*args) == N.PT_ERR_ARG, kw
        msg = lib.pt_last_error(None).decode()
        assert word in msg and msg.startswith("pt_temporal_moments_motion_image" if moments else "pt_temporal_motion_image"), msg
        assert not any(buf)                                # a refused call changes nothing

    for over, field in BAD_TEMPORAL:
        refused(field, params=tparams(**over))
    refused("motion_rows or prev_index is null", table=False)
    refused("prim_count", count=0)
    refused("prim_count", count=1 << 26)
    refused("width", width=0)
    args, _ = image_args(moments=moments)
    args[3] = None                                         # the colour
    assert call(*args) == N.PT_ERR_ARG and "null" in lib.pt_last_error(None).decode()
    args, _ = image_args(moments=moments)
    args[9] = None                                         # hist1 without hist0's companions
    assert call(*args) == N.PT_ERR_ARG and "hist0 is given without" in lib.pt_last_error(None).decode()
    if moments:
        args, _ = image_args(moments=True)
        args[14] = C.byref(N.PtVarianceParams(0))
        assert call(*args) == N.PT_ERR_ARG and "min_temporal" in lib.pt_last_error(None).decode()


def refused(word, call, *args, **kw):
    with pytest.raises(pa.PathtracerError) as e:
        call(*args, **kw)
    assert e.value.code == N.PT_ERR_ARG and word in str(e.value), str(e.value)


@pytest.mark.parametrize("call", (pa.temporal_motion_image, pa.temporal_moments_motion_image), ids=("plain", "moments"))
def test_python_arguments_are_refused_by_name(call):
    img = np.zeros((4, 4, 4), dtype=np.float32)
    cam = N.PtCamera()
    rows, prev = np.zeros((2, 3, 4), np.float32), np.zeros(2, np.uint32)
    refused("alpha_min", call, img, img, img, img, cam, rows, prev, alpha_min=2.0)
    refused("max_history", call, img, img, img, img, cam, rows, prev, max_history=0)
    refused("plane1", call, img, img, img[:2], img, cam, rows, prev)
    refused("motion_rows must be", call, img, img, img, img, cam, rows[:1], prev)
    refused("motion_rows must be", call, img, img, img, img, cam, rows, prev.reshape(2, 1))
    refused("without prev_camera", call, img, img, img, img, cam, rows, prev, history=(img, img, img, img))
    refused("history must be", call, img, img, img, img, cam, rows, prev, history=(img,) * 5, prev_camera=cam)
    if call is pa.temporal_moments_motion_image:
        refused("min_temporal", call, img, img, img, img, cam, rows, prev, min_temporal=0)
