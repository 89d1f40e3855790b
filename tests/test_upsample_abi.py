"""The C ABI and the Python arguments of the guided upsampling (pt_upsample and its kin, include/pt_hip.h): the symbols
are declared, exported and bound, the parameter struct has the layout the header states, and every refusal by field
name comes before any device call -- so all of this answers on a machine without a GPU."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import pathtracercuda_amd as pa
from pathtracercuda_amd import _native as N

SYMBOLS = ("pt_upsample", "pt_holds_upsampled", "pt_read_upsampled", "pt_tonemap_upsampled", "pt_read_upsample_counts",
           "pt_read_upsample_timing", "pt_upsample_image")
HOST_SYMBOLS = ("pth_renderer_upsample", "pth_renderer_upsample_counts")
nan, inf = float("nan"), float("inf")
FIELDS = ("sigma_plane", "normal_power_log2", "flags", "staging")
GOOD = dict(sigma_plane=0.005, normal_power_log2=3, flags=3, staging=0)
BAD = ((dict(sigma_plane=1e-7), "sigma_plane"), (dict(sigma_plane=nan), "sigma_plane"), (dict(sigma_plane=inf), "sigma_plane"),
       (dict(sigma_plane=-1.0), "sigma_plane"), (dict(normal_power_log2=8), "normal_power_log2"), (dict(flags=4), "flags"),
       (dict(staging=3), "staging"))


def struct(**over):
    v = dict(GOOD, **over)
    return N.PtUpsampleParams(*[v[f] for f in FIELDS])


def test_symbols_are_declared_exported_and_bound(root):
    text = (root / "include" / "pt_hip.h").read_text()
    lib = N.hip()
    for name in SYMBOLS:
        assert re.search(rf"PT_API int {name}\(", text), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in N._HIP_SYMBOLS and getattr(lib, name).argtypes == N._HIP_SYMBOLS[name][1]
    P = C.POINTER
    assert N._HIP_SYMBOLS["pt_upsample"][1] == [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, P(N.PtUpsampleParams)]
    assert N._HIP_SYMBOLS["pt_read_upsample_counts"][1] == [C.c_void_p, P(C.c_uint32)]
    assert len(N._HIP_SYMBOLS["pt_upsample_image"][1]) == 15
    host_text = (root / "include" / "pt_host.h").read_text()
    for name in HOST_SYMBOLS:
        assert re.search(rf"{name}\(", host_text) and hasattr(N.host(), name) and name in N._HOST_SYMBOLS
    for name in ("upsample_params", "upsample_image", "UPSAMPLE_DEFAULTS", "UPSAMPLE_SOURCES"):
        assert name in pa.__all__
    for name in ("upsample", "upsampled", "upsample_counts", "upsample_timing", "tonemap_upsampled"):
        assert callable(getattr(pa.Pathtracer, name))
    for word, value in (("ACCUM", 0), ("DENOISED", 1), ("TEMPORAL", 2), ("DESPIKED", 3)):
        assert re.search(rf"#define PT_UPSAMPLE_{word} {value}u$", text, re.M) and getattr(N, f"PT_UPSAMPLE_{word}") == value
        assert pa.UPSAMPLE_SOURCES[word.lower()] == value


def test_struct_layout_and_defaults(root):
    S = N.PtUpsampleParams
    assert C.sizeof(S) == 16
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [(f, 4 * k) for k, f in enumerate(FIELDS)]
    text = (root / "include" / "pt_hip.h").read_text()
    block = text[text.index("typedef struct pt_upsample_params"):text.index("} pt_upsample_params;")]
    assert re.findall(r"^\s+(?:uint32_t|float) (\w+);", block, re.M) == list(FIELDS)

    def macro(prefix, name):
        return float(re.search(rf"#define PT_{prefix}_DEFAULT_{name} ([0-9.e-]+)[fu]?$", text, re.M).group(1))

    d = pa.UPSAMPLE_DEFAULTS
    for key in ("sigma_plane", "normal_power_log2"):
        assert macro("UPSAMPLE", key.upper()) == d[key] == macro("DENOISE", key.upper()), key   # the filter's shipped values
    flags = (1 if d["demodulate"] else 0) | (2 if d["same_primitive"] else 0)
    assert macro("UPSAMPLE", "FLAGS") == flags == 3
    p = pa.upsample_params()
    assert (p.normal_power_log2, p.flags, p.staging) == (d["normal_power_log2"], 3, 0)
    assert np.float32(p.sigma_plane) == np.float32(d["sigma_plane"])


def test_the_image_form_refuses_by_field_name_before_touching_a_device():
    lib = N.hip()
    fp = C.POINTER(C.c_float)
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, fp)
    counts = (C.c_uint32 * 2)(77, 78)

    def call(params, lw=2, lh=2, hw=4, hh=4, last=ptr):
        return lib.pt_upsample_image(0, lw, lh, ptr, ptr, ptr, ptr, hw, hh, ptr, ptr, last, params, ptr, counts)

    for over, field in BAD:
        params = struct(**over)
        rc = call(C.byref(params))
        assert rc == N.PT_ERR_ARG and field in lib.pt_last_error(None).decode(), (over, rc)
    good = struct()
    assert call(C.byref(good), last=None) == N.PT_ERR_ARG and "null" in lib.pt_last_error(None).decode()
    assert call(None) == N.PT_ERR_ARG
    assert call(C.byref(good), lw=0) == N.PT_ERR_ARG and "width" in lib.pt_last_error(None).decode()
    assert call(C.byref(good), hh=0) == N.PT_ERR_ARG and "width" in lib.pt_last_error(None).decode()
    assert call(C.byref(good), lw=5) == N.PT_ERR_ARG and "larger" in lib.pt_last_error(None).decode()
    assert call(C.byref(good), lh=5) == N.PT_ERR_ARG and "larger" in lib.pt_last_error(None).decode()
    assert list(counts) == [77, 78] and not any(buf)       # a refused call changes nothing
    assert lib.pt_holds_upsampled(None) == 0               # a question, never an error
    assert lib.pt_upsample(None, None, 0, 1, C.byref(good)) == N.PT_ERR_ARG
    for name in ("pt_read_upsampled", "pt_tonemap_upsampled", "pt_read_upsample_counts", "pt_read_upsample_timing"):
        assert getattr(lib, name)(None, None) == N.PT_ERR_ARG


def refused(word, call, *args, **kw):
    with pytest.raises(pa.PathtracerError) as e:
        call(*args, **kw)
    assert e.value.code == N.PT_ERR_ARG and word in str(e.value), str(e.value)


PY_BAD = ((dict(sigma_plane=0.0), "sigma_plane"), (dict(sigma_plane=nan), "sigma_plane"), (dict(sigma_plane=inf), "sigma_plane"),
          (dict(normal_power_log2=8), "normal_power_log2"), (dict(normal_power_log2=-1), "normal_power_log2"),
          (dict(normal_power_log2=1.5), "normal_power_log2"), (dict(normal_power_log2=nan), "normal_power_log2"),
          (dict(staging=3), "staging"), (dict(staging=-1), "staging"))


def test_python_parameters_are_refused_by_name():
    for kw, word in PY_BAD:
        refused(word, pa.upsample_params, **kw)
    p = pa.upsample_params(sigma_plane=1e-6, normal_power_log2=7, demodulate=False, same_primitive=True, staging=2)
    assert (p.normal_power_log2, p.flags, p.staging) == (7, 2, 2)
    assert pa.upsample_params(demodulate=True, same_primitive=False).flags == 1
    lo, hi = np.zeros((2, 2, 4), dtype=np.float32), np.zeros((4, 4, 4), dtype=np.float32)
    for kw, word in PY_BAD:
        refused(word, pa.upsample_image, lo, lo, lo, lo, hi, hi, hi, **kw)
    refused("lo_plane1", pa.upsample_image, lo, lo, lo[:1], lo, hi, hi, hi)
    refused("hi_plane2", pa.upsample_image, lo, lo, lo, lo, hi, hi, hi[:2])
    refused("color", pa.upsample_image, np.zeros((2, 2), np.float32), lo, lo, lo, hi, hi, hi)
    refused("larger", pa.upsample_image, hi, hi, hi, hi, lo, lo, lo)


def test_the_method_refuses_its_arguments_before_any_device_call():
    # objects with no renderer behind them: any native call through them would fail otherwise than with PT_ERR_ARG
    pt, lo = pa.Pathtracer.__new__(pa.Pathtracer), pa.Pathtracer.__new__(pa.Pathtracer)
    for o in (pt, lo):
        o._group, o._r, o._ctx = None, None, None
    for kw, word in PY_BAD:
        refused(word, pt.upsample, lo, **kw)
    refused("source", pt.upsample, lo, source="filtered")
    refused("lo must be", pt.upsample, None)
    refused("frames", pt.upsample, lo, source="denoised", frames=2)
    refused("frames", pt.upsample, lo, frames=-1)


def test_the_cli_lists_the_option_and_refuses_what_it_cannot_serve():
    run = subprocess.run([str(N.CLI), "-help"], capture_output=True, text=True, timeout=60)
    assert re.search(r"^-upsample K\s", run.stdout, re.M), run.stdout
    for k in ("1", "5", "x", "2.5"):
        run = subprocess.run([str(N.CLI), "-upsample", k, "x.json"], capture_output=True, text=True, timeout=60)
        assert run.returncode == 0 and "Invalid input for -upsample" in run.stdout and "USAGE" in run.stdout, run.stdout
    run = subprocess.run([str(N.CLI), "-upsample", "2", "-adaptive", "0.1", "-denoise", "-denoise_guide", "adaptive", "x.json"],
                         capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "Invalid input for -upsample! (not with -denoise_guide adaptive)" in run.stdout, run.stdout
