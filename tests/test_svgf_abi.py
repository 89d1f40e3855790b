"""The C ABI of the per-pixel variance and the variance-guided filter: the symbols include/pt_hip.h declares
are exported and bound, and the parameter structs have the sizes and field offsets the header states."""
import ctypes as C
import re

from pathtracercuda_amd import _native as N

SYMBOLS = ("pt_temporal_moments", "pt_read_temporal_variance", "pt_read_temporal_moments_timing", "pt_denoise_variance",
           "pt_temporal_moments_image", "pt_denoise_variance_image")


def test_symbols_are_declared_exported_and_bound(root):
    text = (root / "include" / "pt_hip.h").read_text()
    lib = N.hip()
    for name in SYMBOLS:
        assert re.search(rf"PT_API int {name}\(", text), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in N._HIP_SYMBOLS and getattr(lib, name).argtypes == N._HIP_SYMBOLS[name][1]
    assert len(N._HIP_SYMBOLS["pt_temporal_moments_image"][1]) == 21
    assert len(N._HIP_SYMBOLS["pt_denoise_variance_image"][1]) == 10


def test_struct_layouts():
    assert C.sizeof(N.PtVarianceParams) == 4
    assert C.sizeof(N.PtVDenoiseParams) == 28
    fields = [(n, getattr(N.PtVDenoiseParams, n).offset) for n, _ in N.PtVDenoiseParams._fields_]
    assert fields == [("iterations", 0), ("sigma_l", 4), ("variance_floor", 8), ("sigma_plane", 12),
                      ("normal_power_log2", 16), ("flags", 20), ("staging", 24)]


def test_context_free_calls_refuse_bad_parameters_before_touching_a_device():
    # argument checks come first, so they answer on a machine without a GPU too
    lib = N.hip()
    fp = C.POINTER(C.c_float)
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, fp)
    bad = N.PtVDenoiseParams(3, 0.0, 1e-6, 0.05, 1, 1, 0)
    assert lib.pt_denoise_variance_image(0, 4, 4, ptr, ptr, ptr, ptr, ptr, C.byref(bad), ptr) == N.PT_ERR_ARG
    assert "sigma_l" in lib.pt_last_error(None).decode()
    cam = N.PtCamera()
    good, v = N.PtTemporalParams(0.1, 8, 0.1, 0.5, 1), N.PtVarianceParams(0)
    rc = lib.pt_temporal_moments_image(0, 4, 4, ptr, ptr, ptr, ptr, C.byref(cam), None, None, None, None, None, C.byref(good),
                                       C.byref(v), ptr, ptr, ptr, ptr, ptr, ptr)
    assert rc == N.PT_ERR_ARG and "min_temporal" in lib.pt_last_error(None).decode()
