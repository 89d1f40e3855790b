"""The denoiser without a GPU: the two restatements of the filter rule (tests/denoise_model.py) against
each other, the Python layer's refusals, the ctypes structs against the header, and the CLI's option."""
import ctypes as C
import inspect
import re
import subprocess

import numpy as np
import pytest

import denoise_model as dm
import pathtracercuda_amd as pa
from pathtracercuda_amd import _native as N


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("iterations,power", [(1, 0), (3, 2), (4, 7)])
def test_model_equals_scalar_restatement(flags, iterations, power):
    inputs = dm.make_inputs(9, 7, seed=11 + flags)
    a = dm.model(*inputs, iterations, 0.3, 0.05, power, flags)
    b = dm.scalar(*inputs, iterations, 0.3, 0.05, power, flags)
    assert dm.same_words(a, b)
    kept, changed, untouched = dm.vacuity(inputs[0], inputs[2], inputs[3], a)
    assert kept >= 0.5 and changed >= 0.5 and untouched
    assert (a[..., 3] == 1).all()


def test_inputs_hold_every_case():
    color, p0, p1, p2 = dm.make_inputs(70, 45, seed=3)
    fl = dm.bits(p2[..., 3])
    ids = dm.bits(p0[..., 3])
    assert (fl == 0).any() and (fl == 3).any() and (fl == 1).sum() > fl.size // 2
    assert np.isnan(color[..., :3]).any() and np.isposinf(color).any() and np.isneginf(color).any()
    assert np.isnan(p1[..., :3]).any()
    hit = fl == 1
    assert (p0[..., :3][hit] == 0).all(-1).any()
    small = (p0[..., :3] > 0) & (p0[..., :3] < 1.0 / 64.0)
    assert small[hit].any()
    both = hit[:, 1:] & hit[:, :-1]
    assert (ids[:, 1:] != ids[:, :-1])[both].any()
    dots = (p1[:, 1:, :3] * p1[:, :-1, :3]).sum(-1)
    assert (dots[both] < -0.9).any(), "no antiparallel neighbours"


def test_non_finite_pixels_pass_through_and_reach_nobody():
    color, p0, p1, p2 = dm.make_inputs(20, 14, seed=5)
    out = dm.model(color, p0, p1, p2, 4, 0.5, 0.05, 1, 1)
    bad = ~np.isfinite(color[..., :3]).all(-1)
    assert bad.any()
    assert np.array_equal(dm.bits(out[..., :3])[bad], dm.bits(color[..., :3])[bad])
    keep = dm.keep_mask(color, p1, p2)
    assert np.isfinite(out[..., :3][keep]).all()


def test_python_refusals_come_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(N, "hip", no_device)
    img = np.zeros((4, 6, 4), dtype=np.float32)
    for kw, field in ((dict(iterations=0), "iterations"), (dict(iterations=9), "iterations"),
                      (dict(sigma_color=0.0), "sigma_color"), (dict(sigma_color=-1.0), "sigma_color"),
                      (dict(sigma_color=float("nan")), "sigma_color"), (dict(sigma_plane=0.0), "sigma_plane"),
                      (dict(normal_power_log2=8), "normal_power_log2"), (dict(staging=3), "staging")):
        with pytest.raises(pa.PathtracerError) as e:
            pa.denoise_image(img, img, img, img, **{"sigma_color": 1.0, **kw})
        assert e.value.code == N.PT_ERR_ARG and field in str(e.value), (kw, str(e.value))
    for k in range(1, 4):
        arrays = [img, img, img, img]
        arrays[k] = np.zeros((4, 5, 4), dtype=np.float32)
        with pytest.raises(pa.PathtracerError) as e:
            pa.denoise_image(*arrays, sigma_color=1.0)
        assert e.value.code == N.PT_ERR_ARG and f"plane{k - 1}" in str(e.value)
    with pytest.raises(pa.PathtracerError):
        pa.denoise_image(np.zeros((4, 6, 3), dtype=np.float32), img, img, img, sigma_color=1.0)
    # the context methods refuse the same way, and a device group is out of scope
    pt = pa.Pathtracer.__new__(pa.Pathtracer)
    pt._group, pt._r = None, None
    with pytest.raises(pa.PathtracerError) as e:
        pt.denoise(iterations=9)
    assert e.value.code == N.PT_ERR_ARG and "iterations" in str(e.value)
    pt._group = 1
    for call in (lambda: pt.denoise(), lambda: pt.features(pa.PtCamera())):
        with pytest.raises(pa.PathtracerError) as e:
            call()
        assert e.value.code == N.PT_ERR_STATE


def test_structs_and_constants_match_the_header(root):
    text = (root / "include" / "pt_hip.h").read_text()
    body = re.search(r"typedef struct pt_denoise_params \{(.*?)\} pt_denoise_params;", text, re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|float)\s+(\w+);", body, re.M)
    ctype = {"uint32_t": C.c_uint32, "float": C.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(N.PtDenoiseParams._fields_)
    assert C.sizeof(N.PtDenoiseParams) == 4 * len(fields) == 24
    for name in ("PT_FEATURE_HIT", "PT_FEATURE_EMISSIVE", "PT_DENOISE_DEMODULATE", "PT_DENOISE_SAME_PRIMITIVE",
                 "PT_DENOISE_TILE_W", "PT_DENOISE_TILE_H"):
        value = int(re.search(rf"#define {name} (\d+)", text).group(1))
        assert getattr(N, name) == value
    assert (dm.TILE_W, dm.TILE_H) == (N.PT_DENOISE_TILE_W, N.PT_DENOISE_TILE_H)
    # one set of defaults for the C++ class, the CLI and Python
    default = {k: v for k, v in re.findall(r"#define PT_DENOISE_DEFAULT_(\w+) ([\d.]+)", text)}
    d = pa.DENOISE_DEFAULTS
    assert int(default["ITERATIONS"]) == d["iterations"] == 5
    assert float(default["SIGMA_FACTOR"]) == pa.DENOISE_SIGMA_FACTOR
    assert float(default["SIGMA_PLANE"]) == d["sigma_plane"]
    assert int(default["NORMAL_POWER_LOG2"]) == d["normal_power_log2"]
    assert int(default["FLAGS"]) == (1 if d["demodulate"] else 0) | (2 if d["same_primitive"] else 0)
    assert (dm.HIT, dm.EMISSIVE, dm.DEMODULATE, dm.SAME_PRIMITIVE) == (1, 2, 1, 2)


def test_python_interface():
    sig = inspect.signature(pa.Pathtracer.denoise)
    assert list(sig.parameters)[:3] == ["self", "iterations", "sigma_color"]
    assert sig.parameters["iterations"].default == 5 and sig.parameters["sigma_color"].default is None
    assert list(inspect.signature(pa.Pathtracer.features).parameters) == ["self", "camera"]
    p = pa.denoise_params()
    d = pa.DENOISE_DEFAULTS
    assert (p.iterations, p.normal_power_log2, p.staging) == (5, d["normal_power_log2"], 0)
    assert p.flags == (1 if d["demodulate"] else 0) | (2 if d["same_primitive"] else 0)
    assert p.sigma_plane == np.float32(d["sigma_plane"])


def test_auto_sigma_is_a_factor_times_the_kept_median():
    color, p0, p1, p2 = dm.make_inputs(40, 30, seed=9)
    keep = dm.keep_mask(color, p1, p2)
    assert np.array_equal(keep, pa.denoise_keep_mask(color, p1, p2))
    lum = color[..., :3][keep] @ np.array([0.2126, 0.7152, 0.0722], dtype=np.float32)
    assert pa.auto_sigma_color(color, p0, p1, p2, demodulate=False, factor=3.0) == pytest.approx(3.0 * np.median(lum))
    assert pa.auto_sigma_color(color, p0, p1, p2, demodulate=False) == pytest.approx(pa.DENOISE_SIGMA_FACTOR * np.median(lum))
    none = p2.copy()
    none[..., 3] = 0
    assert pa.auto_sigma_color(color, p0, p1, none) == 1.0


def test_cli_lists_denoise_and_rejects_a_bad_value(scenes, tmp_path):
    out = subprocess.run([str(N.CLI), "-help"], capture_output=True, text=True, timeout=60)
    assert "-denoise" in out.stdout + out.stderr
    for bad in ("0", "9", "x"):
        r = subprocess.run([str(N.CLI), "-w", "16", "-h", "16", "-spp", "1", "-denoise", bad, "-o", str(tmp_path / "a.png"),
                            str(scenes / "cornell_box.scene.json")], capture_output=True, text=True, timeout=60)
        # refused while the arguments are parsed, as every invalid option is: the message, the usage, no render
        assert "Invalid input for -denoise!" in r.stdout and "USAGE" in r.stdout, (bad, r.stdout, r.stderr)
        assert "Beginning rendering" not in r.stdout and not (tmp_path / "a.png").exists()
    ok = subprocess.run([str(N.CLI), "-w", "16", "-h", "16", "-spp", "1", "-denoise", "-o", str(tmp_path / "a.png"),
                         str(scenes / "cornell_box.scene.json")], capture_output=True, text=True, timeout=60)
    assert "Invalid input" not in ok.stdout and "Beginning rendering" in ok.stdout     # the count is optional
