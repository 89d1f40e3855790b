"""The C ABI of the feedback of the filtered colour into the temporal history: the symbols include/pt_hip.h and
include/pt_host.h declare are exported and bound, pt_vfeedback_params has the size and field order the header
states, and the header's default is Python's."""
import ctypes as C
import inspect
import re

import pathtracercuda_amd as pa
from pathtracercuda_amd import _native as N

SYMBOLS = ("pt_denoise_variance_feedback", "pt_read_feedback_timing", "pt_read_temporal_history",
           "pt_denoise_variance_feedback_image")
HOST_SYMBOLS = (("int", "pth_renderer_denoise_variance_feedback"), (r"const float \*", "pth_renderer_temporal_history"))


def test_symbols_are_declared_exported_and_bound(root):
    text = (root / "include" / "pt_hip.h").read_text()
    lib = N.hip()
    for name in SYMBOLS:
        assert re.search(rf"PT_API int {name}\(", text), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in N._HIP_SYMBOLS and getattr(lib, name).argtypes == N._HIP_SYMBOLS[name][1]
    assert len(N._HIP_SYMBOLS["pt_denoise_variance_feedback_image"][1]) == 13
    assert N._HIP_SYMBOLS["pt_denoise_variance_feedback"][1] == [C.c_void_p, C.POINTER(N.PtVDenoiseParams),
                                                                 C.POINTER(N.PtVFeedbackParams)]
    assert N._HIP_SYMBOLS["pt_read_temporal_history"][1] == [C.c_void_p, C.c_uint32, C.POINTER(C.c_float)]
    host_text = (root / "include" / "pt_host.h").read_text()
    host = N.host()
    for res, name in HOST_SYMBOLS:
        assert re.search(rf"PT_API {res} ?{name}\(", host_text), f"{name} is not declared"
        assert hasattr(host, name) and name in N._HOST_SYMBOLS
    # the existing declarations are what they were
    assert re.search(r"PT_API int pt_denoise_variance\(pt_context \*ctx, const pt_vdenoise_params \*params\);", text)
    assert len(N._HIP_SYMBOLS["pt_denoise_variance_image"][1]) == 10


def test_struct_layout_and_defaults(root):
    assert C.sizeof(N.PtVFeedbackParams) == 4
    assert [(n, getattr(N.PtVFeedbackParams, n).offset) for n, _ in N.PtVFeedbackParams._fields_] == [("level", 0)]
    text = (root / "include" / "pt_hip.h").read_text()
    assert re.search(r"typedef struct pt_vfeedback_params \{\s*uint32_t level;[^}]*\} pt_vfeedback_params;", text)
    level = int(re.search(r"#define PT_VFEEDBACK_DEFAULT_LEVEL (\d+)", text).group(1))
    assert level == pa.VFEEDBACK_DEFAULTS["level"] == pa.vfeedback_params().level
    # the feedback is off unless asked for, and the filter's defaults are what they were
    assert inspect.signature(pa.Pathtracer.denoise).parameters["feedback"].default == 0
    assert float(re.search(r"#define PT_VDENOISE_DEFAULT_SIGMA_L ([0-9.]+)f", text).group(1)) == pa.VDENOISE_DEFAULTS["sigma_l"]


def test_python_refuses_the_level_by_name():
    for level, iterations in ((0, 3), (4, 3), (1.5, 3), (float("nan"), 3), (6, None)):
        try:
            pa.vfeedback_params(level, iterations)
        except pa.PathtracerError as e:
            assert e.code == N.PT_ERR_ARG and "level" in str(e)
        else:
            raise AssertionError(f"level {level!r} of {iterations} was accepted")
    assert pa.vfeedback_params(3, 3).level == 3 and pa.vfeedback_params(5).level == 5


def test_context_free_call_refuses_bad_parameters_before_touching_a_device():
    # argument checks come first, so they answer on a machine without a GPU too
    lib = N.hip()
    fp = C.POINTER(C.c_float)
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, fp)
    good = N.PtVDenoiseParams(3, 1.0, 1e-6, 0.05, 1, 1, 0)

    def call(params, fb, hist0=ptr, out_hist0=ptr):
        return lib.pt_denoise_variance_feedback_image(0, 4, 4, ptr, ptr, ptr, ptr, ptr, hist0, params, fb, ptr, out_hist0)

    for level in (0, 4):
        assert call(C.byref(good), C.byref(N.PtVFeedbackParams(level))) == N.PT_ERR_ARG
        assert "level" in lib.pt_last_error(None).decode()
    assert call(C.byref(good), None) == N.PT_ERR_ARG and "feedback" in lib.pt_last_error(None).decode()
    bad = N.PtVDenoiseParams(3, 0.0, 1e-6, 0.05, 1, 1, 0)
    assert call(C.byref(bad), C.byref(N.PtVFeedbackParams(1))) == N.PT_ERR_ARG and "sigma_l" in lib.pt_last_error(None).decode()
    fb = N.PtVFeedbackParams(1)
    assert call(C.byref(good), C.byref(fb), hist0=None) == N.PT_ERR_ARG and "hist0" in lib.pt_last_error(None).decode()
    assert call(C.byref(good), C.byref(fb), out_hist0=None) == N.PT_ERR_ARG and "out_hist0" in lib.pt_last_error(None).decode()
