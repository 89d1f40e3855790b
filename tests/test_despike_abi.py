"""The C ABI and the Python arguments of despike, the same-surface firefly clamp (pt_despike and its kin,
include/pt_hip.h): the symbols are declared, exported and bound, the parameter struct has the layout the header
states, and every refusal by field name comes before any device call -- so all of this answers on a machine
without a GPU."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import pathtracercuda_amd as pa
from pathtracercuda_amd import _native as N

SYMBOLS = ("pt_despike", "pt_holds_despiked", "pt_read_despiked", "pt_tonemap_despiked", "pt_read_despike_count", "pt_read_despike_timing",
           "pt_denoise_despiked", "pt_despike_image")
HOST_SYMBOLS = ("pth_renderer_despike", "pth_renderer_despike_count")
nan, inf = float("nan"), float("inf")
FIELDS = ("radius", "rank", "factor", "floor", "min_neighbors", "sigma_plane", "normal_cos_min", "flags", "staging")
GOOD = dict(radius=2, rank=2, factor=2.0, floor=0.05, min_neighbors=3, sigma_plane=0.3, normal_cos_min=0.0, flags=2, staging=0)
# every field below, above and (for the floats) at NaN and infinity; min_neighbors against rank and the window
BAD = ((dict(radius=0), "radius"), (dict(radius=4), "radius"), (dict(rank=0), "rank"), (dict(rank=5), "rank"),
       (dict(factor=0.5), "factor"), (dict(factor=nan), "factor"), (dict(factor=inf), "factor"),
       (dict(floor=-0.1), "floor"), (dict(floor=nan), "floor"), (dict(floor=inf), "floor"),
       (dict(min_neighbors=1), "min_neighbors"), (dict(min_neighbors=25), "min_neighbors"),
       (dict(radius=1, min_neighbors=9), "min_neighbors"), (dict(rank=4, min_neighbors=3), "min_neighbors"),
       (dict(sigma_plane=1e-7), "sigma_plane"), (dict(sigma_plane=nan), "sigma_plane"), (dict(sigma_plane=inf), "sigma_plane"),
       (dict(normal_cos_min=1.5), "normal_cos_min"), (dict(normal_cos_min=-1.5), "normal_cos_min"),
       (dict(normal_cos_min=nan), "normal_cos_min"), (dict(flags=4), "flags"), (dict(staging=3), "staging"))


def struct(**over):
    v = dict(GOOD, **over)
    return N.PtDespikeParams(*[v[f] for f in FIELDS])


def test_symbols_are_declared_exported_and_bound(root):
    text = (root / "include" / "pt_hip.h").read_text()
    lib = N.hip()
    for name in SYMBOLS:
        assert re.search(rf"PT_API int {name}\(", text), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in N._HIP_SYMBOLS and getattr(lib, name).argtypes == N._HIP_SYMBOLS[name][1]
    P = C.POINTER
    assert N._HIP_SYMBOLS["pt_despike"][1] == [C.c_void_p, C.c_uint32, P(N.PtDespikeParams)]
    assert N._HIP_SYMBOLS["pt_denoise_despiked"][1] == [C.c_void_p, P(N.PtDenoiseParams)]
    assert N._HIP_SYMBOLS["pt_read_despike_count"][1] == [C.c_void_p, P(C.c_uint32)]
    assert len(N._HIP_SYMBOLS["pt_despike_image"][1]) == 10
    host_text = (root / "include" / "pt_host.h").read_text()
    for name in HOST_SYMBOLS:
        assert re.search(rf"{name}\(", host_text) and hasattr(N.host(), name) and name in N._HOST_SYMBOLS
    for name in ("despike_params", "despike_image", "DESPIKE_DEFAULTS"):
        assert name in pa.__all__
    for name in ("despike", "despiked", "despike_count", "despike_timing", "tonemap_despiked"):
        assert callable(getattr(pa.Pathtracer, name))


def test_struct_layout_and_defaults(root):
    S = N.PtDespikeParams
    assert C.sizeof(S) == 36
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [(f, 4 * k) for k, f in enumerate(FIELDS)]
    text = (root / "include" / "pt_hip.h").read_text()
    block = text[text.index("typedef struct pt_despike_params"):text.index("} pt_despike_params;")]
    assert re.findall(r"^\s+(?:uint32_t|float) (\w+);", block, re.M) == list(FIELDS)

    def macro(name):
        return float(re.search(rf"#define PT_DESPIKE_DEFAULT_{name} ([0-9.e-]+)[fu]?$", text, re.M).group(1))

    d = pa.DESPIKE_DEFAULTS
    for key in ("radius", "rank", "factor", "floor", "min_neighbors", "sigma_plane", "normal_cos_min"):
        assert macro(key.upper()) == d[key], key
    flags = (1 if d["demodulate"] else 0) | (2 if d["same_primitive"] else 0)
    assert macro("FLAGS") == flags
    p = pa.despike_params()
    assert [getattr(p, f) for f in ("radius", "rank", "min_neighbors", "flags", "staging")] == \
        [d["radius"], d["rank"], d["min_neighbors"], flags, 0]
    assert (np.float32(p.factor), np.float32(p.floor)) == (np.float32(d["factor"]), np.float32(d["floor"]))


def test_the_image_form_refuses_by_field_name_before_touching_a_device():
    lib = N.hip()
    fp = C.POINTER(C.c_float)
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, fp)
    count = C.c_uint32(77)
    for over, field in BAD:
        params = struct(**over)
        rc = lib.pt_despike_image(0, 4, 4, ptr, ptr, ptr, ptr, C.byref(params), ptr, C.byref(count))
        assert rc == N.PT_ERR_ARG and field in lib.pt_last_error(None).decode(), (over, rc)
    good = struct()
    assert lib.pt_despike_image(0, 4, 4, ptr, ptr, ptr, None, C.byref(good), ptr, C.byref(count)) == N.PT_ERR_ARG
    assert "null" in lib.pt_last_error(None).decode()
    assert lib.pt_despike_image(0, 4, 4, ptr, ptr, ptr, ptr, None, ptr, C.byref(count)) == N.PT_ERR_ARG
    assert lib.pt_despike_image(0, 0, 4, ptr, ptr, ptr, ptr, C.byref(good), ptr, C.byref(count)) == N.PT_ERR_ARG
    assert "width" in lib.pt_last_error(None).decode()
    assert count.value == 77 and not any(buf)              # a refused call changes nothing
    assert lib.pt_holds_despiked(None) == 0                # a question, never an error
    for name in ("pt_despike", "pt_denoise_despiked"):     # without a context there is nothing to refuse by name
        assert getattr(lib, name)(None, *([0] if name == "pt_despike" else []), None) == N.PT_ERR_ARG


def refused(word, call, *args, **kw):
    with pytest.raises(pa.PathtracerError) as e:
        call(*args, **kw)
    assert e.value.code == N.PT_ERR_ARG and word in str(e.value), str(e.value)


PY_BAD = ((dict(radius=0), "radius"), (dict(radius=4), "radius"), (dict(radius=1.5), "radius"), (dict(radius=nan), "radius"),
          (dict(rank=0), "rank"), (dict(rank=5), "rank"), (dict(rank=nan), "rank"),
          (dict(factor=0.99), "factor"), (dict(factor=nan), "factor"), (dict(factor=inf), "factor"),
          (dict(floor=-1e-9), "floor"), (dict(floor=nan), "floor"), (dict(floor=inf), "floor"),
          (dict(min_neighbors=1), "min_neighbors"), (dict(min_neighbors=25), "min_neighbors"),
          (dict(min_neighbors=2.5), "min_neighbors"), (dict(min_neighbors=nan), "min_neighbors"),
          (dict(radius=1, min_neighbors=9), "min_neighbors"),
          (dict(sigma_plane=0.0), "sigma_plane"), (dict(sigma_plane=nan), "sigma_plane"), (dict(sigma_plane=inf), "sigma_plane"),
          (dict(normal_cos_min=2.0), "normal_cos_min"), (dict(normal_cos_min=nan), "normal_cos_min"),
          (dict(staging=3), "staging"), (dict(staging=-1), "staging"))


def test_python_parameters_are_refused_by_name():
    for kw, word in PY_BAD:
        refused(word, pa.despike_params, **kw)
    p = pa.despike_params(radius=3, rank=4, factor=1.0, floor=0.0, min_neighbors=48, sigma_plane=1e-6, normal_cos_min=-1.0,
                          demodulate=True, same_primitive=False, staging=2)
    assert (p.radius, p.rank, p.min_neighbors, p.flags, p.staging) == (3, 4, 48, 1, 2)
    # the default min_neighbors follows rank and the window
    assert pa.despike_params(rank=4).min_neighbors == 4
    assert pa.despike_params(radius=1, rank=1).min_neighbors == 3
    img = np.zeros((4, 4, 4), dtype=np.float32)
    for kw, word in PY_BAD:
        refused(word, pa.despike_image, img, img, img, img, **kw)
    refused("plane1", pa.despike_image, img, img, img[:2], img)
    refused("color", pa.despike_image, np.zeros((4, 4), np.float32), img, img, img)


def test_the_methods_refuse_their_arguments_before_any_device_call():
    # an object with no renderer behind it: any native call through it would fail otherwise than with PT_ERR_ARG
    pt = pa.Pathtracer.__new__(pa.Pathtracer)
    pt._group, pt._r, pt._ctx = None, None, None
    for kw, word in PY_BAD:
        refused(word, pt.despike, **kw)
    refused("guide", pt.denoise, source="despiked", guide="variance")
    refused("guide", pt.denoise, source="despiked", guide="adaptive")
    refused("feedback", pt.denoise, source="despiked", feedback=2)
    refused("frames", pt.denoise, source="despiked", frames=2)
    refused("iterations", pt.denoise, source="despiked", iterations=9)
    refused("sigma_color", pt.denoise, source="despiked", sigma_color=0.0)
    refused("sigma_l", pt.denoise, source="despiked", sigma_l=2.0)
    refused("source", pt.denoise, source="clamped")


def test_the_cli_lists_the_option_and_refuses_it_with_the_adaptive_guide():
    run = subprocess.run([str(N.CLI), "-help"], capture_output=True, text=True, timeout=60)
    assert re.search(r"^-despike\s", run.stdout, re.M), run.stdout
    run = subprocess.run([str(N.CLI), "-despike", "-adaptive", "0.1", "-denoise", "-denoise_guide", "adaptive", "x.json"],
                         capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "Invalid input for -despike" in run.stdout and "USAGE" in run.stdout, run.stdout
