"""The C ABI and the Python arguments of the guided upsampling onto supersampled planes (pt_upsample_resolve,
pt_upsample_resolve_image, include/pt_hip.h): the symbols are declared, exported and bound, the parameter struct is
pt_upsample's, and every refusal by name comes before any device call -- so all of this answers on a machine without
a GPU."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import pathtracercuda_amd as pa
from pathtracercuda_amd import _native as N

SYMBOLS = ("pt_upsample_resolve", "pt_upsample_resolve_image")
FIELDS = ("sigma_plane", "normal_power_log2", "flags", "staging")
GOOD = dict(sigma_plane=0.005, normal_power_log2=3, flags=3, staging=0)
nan, inf = float("nan"), float("inf")
BAD = ((dict(sigma_plane=1e-7), "sigma_plane"), (dict(sigma_plane=nan), "sigma_plane"), (dict(sigma_plane=inf), "sigma_plane"),
       (dict(normal_power_log2=8), "normal_power_log2"), (dict(flags=4), "flags"), (dict(staging=3), "staging"))


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
    assert N._HIP_SYMBOLS["pt_upsample_resolve"][1] == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                        P(N.PtUpsampleParams)]
    image = N._HIP_SYMBOLS["pt_upsample_resolve_image"][1]
    assert len(image) == 16 and image[12] == C.c_uint32 and image[13] == P(N.PtUpsampleParams)
    # the declaration's parameters, in the header's order
    decl = re.search(r"PT_API int pt_upsample_resolve\(([^;]*)\);", text).group(1)
    assert [re.sub(r".*[ *]", "", a.strip()) for a in decl.split(",")] == ["hi", "planes", "lo", "source", "frames", "factor",
                                                                          "params"]
    host_text = (root / "include" / "pt_host.h").read_text()
    assert re.search(r"pth_renderer_upsample_resolve\(", host_text)
    assert hasattr(N.host(), "pth_renderer_upsample_resolve") and "pth_renderer_upsample_resolve" in N._HOST_SYMBOLS
    assert "upsample_resolve_image" in pa.__all__ and callable(pa.upsample_resolve_image)
    assert re.search(r"void upsample\(Pathtracer& lo, Pathtracer& planes, const UpsampleOptions& options\);",
                     (root / "include" / "pathtracer_amd.hpp").read_text())


def test_the_struct_is_pt_upsamples_and_rule_9_is_stated(root):
    S = N.PtUpsampleParams
    assert C.sizeof(S) == 16
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [(f, 4 * k) for k, f in enumerate(FIELDS)]
    text = (root / "include" / "pt_hip.h").read_text()
    assert text.count("typedef struct pt_upsample_params") == 1      # no second parameter struct
    assert re.search(r"^ \* 9\. ", text, re.M) and "tests/upsample_resolve_model.py restates it" in text


def test_the_image_form_refuses_by_name_before_touching_a_device():
    lib = N.hip()
    fp = C.POINTER(C.c_float)
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, fp)
    counts = (C.c_uint32 * 2)(77, 78)

    def call(params, lw=2, lh=2, sw=8, sh=8, factor=2, last=ptr):
        return lib.pt_upsample_resolve_image(0, lw, lh, ptr, ptr, ptr, ptr, sw, sh, ptr, ptr, last, factor, params, ptr, counts)

    def said(word):
        return word in lib.pt_last_error(None).decode()

    for over, field in BAD:
        params = struct(**over)
        assert call(C.byref(params)) == N.PT_ERR_ARG and said(field), over
    good = struct()
    assert call(None) == N.PT_ERR_ARG
    assert call(C.byref(good), last=None) == N.PT_ERR_ARG and said("null")
    for factor in (0, 1, 5, 0xffffffff):
        assert call(C.byref(good), factor=factor) == N.PT_ERR_ARG and said("factor must be 2, 3 or 4"), factor
    assert call(C.byref(good), sw=9) == N.PT_ERR_ARG and said("does not divide")
    assert call(C.byref(good), sh=7, factor=3) == N.PT_ERR_ARG and said("does not divide")
    assert call(C.byref(good), lw=0) == N.PT_ERR_ARG and said("width")
    assert call(C.byref(good), sw=0) == N.PT_ERR_ARG and said("width")
    assert call(C.byref(good), lw=5) == N.PT_ERR_ARG and said("larger")      # the output is 4 x 4
    assert call(C.byref(good), lh=3, sh=4) == N.PT_ERR_ARG and said("larger")
    assert list(counts) == [77, 78] and not any(buf)       # a refused call changes nothing
    assert lib.pt_upsample_resolve(None, None, None, 0, 1, 2, C.byref(good)) == N.PT_ERR_ARG


def refused(word, call, *args, **kw):
    with pytest.raises(pa.PathtracerError) as e:
        call(*args, **kw)
    assert e.value.code == N.PT_ERR_ARG and word in str(e.value), str(e.value)


def test_python_arguments_are_refused_by_name():
    lo, ss = np.zeros((2, 2, 4), dtype=np.float32), np.zeros((8, 8, 4), dtype=np.float32)
    for kw, word in ((dict(sigma_plane=0.0), "sigma_plane"), (dict(normal_power_log2=8), "normal_power_log2"),
                     (dict(staging=3), "staging")):
        refused(word, pa.upsample_resolve_image, lo, lo, lo, lo, ss, ss, ss, 2, **kw)
    for factor in (1, 5, 2.0, True, None):
        refused("factor", pa.upsample_resolve_image, lo, lo, lo, lo, ss, ss, ss, factor)
    refused("does not divide", pa.upsample_resolve_image, lo, lo, lo, lo, ss, ss, ss, 3)
    refused("lo_plane1", pa.upsample_resolve_image, lo, lo, lo[:1], lo, ss, ss, ss, 2)
    refused("ss_plane2", pa.upsample_resolve_image, lo, lo, lo, lo, ss, ss, ss[:2], 2)
    refused("larger", pa.upsample_resolve_image, ss, ss, ss, ss, ss, ss, ss, 2)
    # the method: objects with no renderer behind them, so any native call through them would fail otherwise
    pt, low = pa.Pathtracer.__new__(pa.Pathtracer), pa.Pathtracer.__new__(pa.Pathtracer)
    for o in (pt, low):
        o._group, o._r, o._ctx = None, None, None
    refused("planes must be", pt.upsample, low, planes=7, frames=1)
    refused("staging", pt.upsample, low, planes=low, staging=3)
    refused("source", pt.upsample, low, planes=low, source="filtered")


def test_the_cli_lists_the_option_and_refuses_what_it_cannot_serve():
    run = subprocess.run([str(N.CLI), "-help"], capture_output=True, text=True, timeout=60)
    assert re.search(r"^-upsample_aa S\s", run.stdout, re.M), run.stdout
    for s in ("1", "5", "x", "2.5"):
        run = subprocess.run([str(N.CLI), "-upsample", "2", "-upsample_aa", s, "x.json"], capture_output=True, text=True, timeout=60)
        assert run.returncode == 0 and "Invalid input for -upsample_aa! (a factor of 2..4)" in run.stdout and "USAGE" in run.stdout
    run = subprocess.run([str(N.CLI), "-upsample_aa", "2", "x.json"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "Invalid input for -upsample_aa! (needs -upsample K)" in run.stdout, run.stdout
    # it carries -upsample's refusals
    run = subprocess.run([str(N.CLI), "-upsample", "2", "-upsample_aa", "2", "-adaptive", "0.1", "-denoise", "-denoise_guide",
                          "adaptive", "x.json"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "Invalid input for -upsample! (not with -denoise_guide adaptive)" in run.stdout, run.stdout
    run = subprocess.run([str(N.CLI), "-upsample", "7", "-upsample_aa", "2", "x.json"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "Invalid input for -upsample! (a factor of 2..4)" in run.stdout, run.stdout
