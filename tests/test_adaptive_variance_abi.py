"""The C ABI and the Python arguments of the variance of an adaptive render's image (pt_denoise_adaptive and its
kin, include/pt_hip.h): the symbols are declared, exported and bound, the parameter struct has the layout the
header states, and every refusal by field name comes before any device call -- so all of this answers on a
machine without a GPU."""
import ctypes as C
import re

import pytest

import pathtracercuda_amd as pa
from pathtracercuda_amd import _native as N

SYMBOLS = ("pt_denoise_adaptive", "pt_read_adaptive_variance", "pt_read_adaptive_variance_timing",
           "pt_adaptive_variance_image")
HOST_SYMBOLS = ("pth_renderer_denoise_adaptive", "pth_renderer_adaptive_variance")
A = N.PtAdaptiveVarianceParams
nan, inf = float("nan"), float("inf")
BAD = ((A(1, 0.3, 0.0, 1), "min_batches"), (A(0, 0.3, 0.0, 1), "min_batches"), (A(256, 0.3, 0.0, 1), "min_batches"),
       (A(8, 1e-7, 0.0, 1), "sigma_plane"), (A(8, 0.0, 0.0, 1), "sigma_plane"), (A(8, inf, 0.0, 1), "sigma_plane"),
       (A(8, nan, 0.0, 1), "sigma_plane"), (A(8, 0.3, 1.5, 1), "normal_cos_min"), (A(8, 0.3, -1.5, 1), "normal_cos_min"),
       (A(8, 0.3, nan, 1), "normal_cos_min"), (A(8, 0.3, 0.0, 4), "flags"))


def test_symbols_are_declared_exported_and_bound(root):
    text = (root / "include" / "pt_hip.h").read_text()
    lib = N.hip()
    for name in SYMBOLS:
        assert re.search(rf"PT_API int {name}\(", text), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in N._HIP_SYMBOLS and getattr(lib, name).argtypes == N._HIP_SYMBOLS[name][1]
    assert len(N._HIP_SYMBOLS["pt_adaptive_variance_image"][1]) == 11
    assert N._HIP_SYMBOLS["pt_denoise_adaptive"][1] == [C.c_void_p, C.POINTER(A), C.POINTER(N.PtVDenoiseParams)]
    host_text = (root / "include" / "pt_host.h").read_text()
    for name in HOST_SYMBOLS:
        assert re.search(rf"{name}\(", host_text) and hasattr(N.host(), name) and name in N._HOST_SYMBOLS


def test_struct_layout_and_defaults(root):
    assert C.sizeof(A) == 16
    assert [(n, getattr(A, n).offset) for n, _ in A._fields_] == [("min_batches", 0), ("sigma_plane", 4),
                                                                  ("normal_cos_min", 8), ("flags", 12)]
    text = (root / "include" / "pt_hip.h").read_text()
    d = pa.AVARIANCE_DEFAULTS
    assert int(re.search(r"#define PT_AVARIANCE_DEFAULT_MIN_BATCHES (\d+)", text).group(1)) == d["min_batches"]
    assert float(re.search(r"#define PT_AVARIANCE_DEFAULT_SIGMA_PLANE ([0-9.e-]+)f", text).group(1)) == d["sigma_plane"]
    assert float(re.search(r"#define PT_AVARIANCE_DEFAULT_NORMAL_COS_MIN ([0-9.e-]+)f", text).group(1)) == d["normal_cos_min"]
    assert int(re.search(r"#define PT_AVARIANCE_DEFAULT_FLAGS (\d+)u", text).group(1)) == 1 and d["demodulate"]
    # the window's tests are the temporal pass's shipped ones
    t = pa.TEMPORAL_DEFAULTS
    assert (d["sigma_plane"], d["normal_cos_min"], d["demodulate"], d["same_primitive"]) == \
        (t["sigma_plane"], t["normal_cos_min"], t["demodulate"], t["same_primitive"])
    assert float(re.search(r"#define PT_ADENOISE_DEFAULT_SIGMA_L ([0-9.e-]+)f", text).group(1)) == pa.ADENOISE_SIGMA_L
    p = pa.adaptive_variance_params()
    assert (p.min_batches, p.flags) == (d["min_batches"], 1)


def test_the_image_form_refuses_by_field_name_before_touching_a_device():
    lib = N.hip()
    fp = C.POINTER(C.c_float)
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, fp)
    for params, field in BAD:
        rc = lib.pt_adaptive_variance_image(0, 4, 4, ptr, ptr, ptr, ptr, ptr, C.byref(params), 0, ptr)
        assert rc == N.PT_ERR_ARG and field in lib.pt_last_error(None).decode(), (field, rc)
    good = A(8, 0.3, 0.0, 1)
    assert lib.pt_adaptive_variance_image(0, 4, 4, ptr, ptr, ptr, ptr, ptr, C.byref(good), 3, ptr) == N.PT_ERR_ARG
    assert "staging" in lib.pt_last_error(None).decode()
    assert lib.pt_adaptive_variance_image(0, 4, 4, ptr, ptr, ptr, ptr, None, C.byref(good), 0, ptr) == N.PT_ERR_ARG
    assert "null" in lib.pt_last_error(None).decode()
    assert lib.pt_adaptive_variance_image(0, 4, 4, ptr, ptr, ptr, ptr, ptr, None, 0, ptr) == N.PT_ERR_ARG
    assert lib.pt_adaptive_variance_image(0, 0, 4, ptr, ptr, ptr, ptr, ptr, C.byref(good), 0, ptr) == N.PT_ERR_ARG
    assert "width" in lib.pt_last_error(None).decode()


def refused(word, call, *args, **kw):
    with pytest.raises(pa.PathtracerError) as e:
        call(*args, **kw)
    assert e.value.code == N.PT_ERR_ARG and word in str(e.value), str(e.value)


def test_python_parameters_are_refused_by_name():
    for kw, word in ((dict(min_batches=1), "min_batches"), (dict(min_batches=256), "min_batches"),
                     (dict(min_batches=2.5), "min_batches"), (dict(min_batches=nan), "min_batches"),
                     (dict(sigma_plane=0.0), "sigma_plane"), (dict(sigma_plane=nan), "sigma_plane"),
                     (dict(normal_cos_min=2.0), "normal_cos_min"), (dict(normal_cos_min=nan), "normal_cos_min")):
        refused(word, pa.adaptive_variance_params, **kw)
    p = pa.adaptive_variance_params(min_batches=255, sigma_plane=1e-6, normal_cos_min=-1.0, demodulate=False,
                                    same_primitive=True)
    assert (p.min_batches, p.flags) == (255, 2)
    import numpy as np
    img = np.zeros((4, 4, 4), dtype=np.float32)
    refused("staging", pa.adaptive_variance_image, img, img, img, img, np.zeros((4, 4, 3), np.float32), staging=3)
    refused("moments", pa.adaptive_variance_image, img, img, img, img, np.zeros((4, 4), np.float32))
    refused("plane1", pa.adaptive_variance_image, img, img, img[:2], img, np.zeros((4, 4, 3), np.float32))


def test_denoise_refuses_its_arguments_before_any_device_call():
    # an object with no renderer behind it: any native call through it would fail otherwise than with PT_ERR_ARG
    pt = pa.Pathtracer.__new__(pa.Pathtracer)
    pt._group, pt._r, pt._ctx = None, None, None
    refused("source", pt.denoise, guide="adaptive", source="temporal")
    refused("sigma_color", pt.denoise, guide="adaptive", sigma_color=1.0)
    refused("feedback", pt.denoise, guide="adaptive", feedback=2)
    refused("frames", pt.denoise, guide="adaptive", frames=3)
    refused("min_batches", pt.denoise, guide="adaptive", min_batches=1)
    refused("sigma_l", pt.denoise, guide="adaptive", sigma_l=0.0)
    refused("normal_cos_min", pt.denoise, guide="adaptive", normal_cos_min=3.0)
    refused("sigma_plane", pt.denoise, guide="adaptive", window_sigma_plane=0.0)
    refused("staging", pt.denoise, guide="adaptive", staging=3)
    refused("guide", pt.denoise, guide="moments")
    # the variance of the temporal history is still not to be had on the accumulation
    refused("guide='variance' needs source='temporal'", pt.denoise, guide="variance")
    # and the window's arguments belong to guide="adaptive" alone
    refused("min_batches", pt.denoise, min_batches=4)
    refused("min_batches", pt.denoise, source="temporal", guide="variance", normal_cos_min=0.5)


def test_the_cli_takes_the_guide_only_with_both_options():
    import subprocess
    for args in (["-denoise_guide", "adaptive", "-denoise", "x.json"], ["-denoise_guide", "adaptive", "-adaptive", "0.1", "x.json"],
                 ["-denoise_guide", "color", "-adaptive", "0.1", "-denoise", "x.json"]):
        run = subprocess.run([str(N.CLI)] + args, capture_output=True, text=True, timeout=60)
        assert run.returncode == 0 and "Invalid input for -denoise_guide" in run.stdout and "USAGE" in run.stdout, run.stdout
    run = subprocess.run([str(N.CLI), "-help"], capture_output=True, text=True, timeout=60)
    assert "-denoise_guide adaptive" in run.stdout
