"""The temporal reprojection rule of include/pt_hip.h on the CPU: its two numpy restatements
(tests/temporal_model.py) against each other word for word, the identity the header states for a camera that
stands still, that the seeded sequence holds every case the rule distinguishes, and the Python layer's
refusals.  tests/test_gpu_temporal.py holds the device against the same model.
"""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import pathtracercuda_amd as pa
import temporal_model as tm
from pathtracercuda_amd import _native as N

F = tm.F


def assert_same(got, want, what):
    for name, g, w in zip(("image", "h0", "h1", "h2"), got, want):
        assert tm.same_words(g, w), f"{what}: {name} differs"


@pytest.fixture(scope="module")
def sequence():
    return tm.make_sequence()


@pytest.mark.parametrize("flags", (0, 1, 2, 3))
def test_model_equals_scalar_restatement(sequence, flags):
    a, b = tm.run_sequence(tm.model, sequence, flags), tm.run_sequence(tm.scalar, sequence, flags)
    for k in range(3):
        assert_same(a[k], b[k], f"flags {flags}, frame {k}")
    # and the frames do differ from their inputs: history was used
    assert not tm.same_words(a[2][0][..., :3], sequence[2][1][0][..., :3])


def test_model_equals_scalar_on_one_pixel():
    for seed in (1, 2, 3):
        seq = tm.make_sequence(1, 1, seed)
        a, b = tm.run_sequence(tm.model, seq, 3), tm.run_sequence(tm.scalar, seq, 3)
        for k in range(3):
            assert_same(a[k], b[k], f"seed {seed}, frame {k}")


def test_a_camera_that_stands_still_gives_the_running_mean():
    cam = tm.cameras()[0]
    frames = [tm.make_frame(tm.WIDTH, tm.HEIGHT, cam, 5, k) for k in range(5)]
    ok = tm.ok_mask(frames[0][0], frames[0][2], frames[0][3])
    for f in frames:                                    # the same pixels are special in every frame
        assert np.array_equal(tm.ok_mask(f[0], f[2], f[3]), ok)
    hist, mean = None, None
    for k, f in enumerate(frames, 1):
        stats = {}
        image, h0, h1, h2 = tm.model(*f, cam, hist, cam, 0.0, 1000, 0.05, 0.9, 0, stats=stats)
        c = f[0][..., :3]
        with np.errstate(all="ignore"):
            mean = c.copy() if mean is None else (mean + F(1.0 / k) * (c - mean)).astype(F)
        assert tm.same_words(h0[..., :3][ok], mean[ok]) and tm.same_words(image[..., :3][ok], mean[ok])
        assert np.all(h0[..., 3][ok] == k) and np.all(h0[..., 3][~ok] == 0)
        if k > 1:                                       # exactly one tap: the pixel itself, weight 1
            assert stats["taps13"] == stats["hits"] == int(ok.sum()) and stats["taps4"] == stats["taps0"] == 0
        hist = (h0, h1, h2)
    assert ok.sum() > ok.size // 2


def test_the_sequence_holds_every_case(sequence):
    stats = []
    tm.run_sequence(tm.model, sequence, tm.SAME_PRIMITIVE | tm.DEMODULATE, stats=stats)
    for k, s in enumerate(stats):
        print(k, s)
    for key in ("taps4", "taps13", "taps0", "outside", "by_id", "no_history"):
        assert max(s[key] for s in stats[1:]) >= 16, (key, stats)
    assert all(s["have"] > s["hits"] // 2 for s in stats[1:]) and stats[0]["have"] == 0
    loose = []
    tm.run_sequence(tm.model, sequence, tm.DEMODULATE, stats=loose)
    for key in ("by_normal", "by_plane"):
        assert max(s[key] for s in loose[1:]) >= 16, (key, loose)
    # the special pixels: colours and a normal that are not finite, both albedo cases, an emissive region, misses
    color, p0, p1, p2 = sequence[1][1]
    fl = tm.bits(p2[..., 3])
    hit = (fl & tm.HIT) != 0
    assert np.isnan(color[..., :3]).any() and np.isposinf(color[..., :3]).any() and np.isneginf(color[..., :3]).any()
    assert np.isnan(p1[..., :3]).any() and (fl & tm.EMISSIVE).any() and (~hit).any()
    assert ((p0[..., :3] == 0).all(-1) & hit).any() and ((p0[..., 0] > 0) & (p0[..., 0] < 1 / 64)).any()
    ok = tm.ok_mask(color, p1, p2)
    assert 0.7 < hit.mean() < 0.95 and (hit & ~ok).sum() >= 8


def test_non_finite_pixels_pass_through_and_reach_nobody(sequence):
    outs = tm.run_sequence(tm.model, sequence, tm.DEMODULATE)
    for (cam, frame), (image, h0, h1, h2) in zip(sequence, outs):
        ok = tm.ok_mask(frame[0], frame[2], frame[3])
        assert np.array_equal(tm.bits(image[..., :3])[~ok], tm.bits(frame[0][..., :3])[~ok])
        assert np.all(image[..., 3][~ok] == 0) and np.all(h0[..., 3][~ok] == 0)
        assert np.isfinite(image[..., :3][ok]).all() and np.all(image[..., 3][ok] >= 1)


def test_an_infinite_history_colour_is_skipped(sequence):
    (c0, f0), (c1, f1) = sequence[:2]
    _, h0, h1, h2 = tm.model(*f0, c0, None, c0, flags=1, **tm.PARAMS)
    bad = h0.copy()
    sel = (bad[..., 3] >= 1) & (np.arange(bad.shape[1])[None, :] % 3 == 0)
    bad[..., 1][sel] = F(np.inf)
    assert sel.sum() >= 16
    stats = {}
    image = tm.model(*f1, c1, (bad, h1, h2), c0, flags=1, stats=stats, **tm.PARAMS)[0]
    assert stats["not_finite"] >= 16
    ok = tm.ok_mask(f1[0], f1[2], f1[3])
    assert np.isfinite(image[..., :3][ok]).all()
    want = tm.scalar(*f1, c1, (bad, h1, h2), c0, flags=1, **tm.PARAMS)
    assert tm.same_words(image, want[0])


def test_a_previous_camera_behind_the_scene_leaves_no_history(sequence):
    (c0, f0), (c1, f1) = sequence[:2]
    hist = tm.model(*f0, c0, None, c0, flags=1, **tm.PARAMS)[1:]
    behind = tm.camera_behind()
    z1 = tm._project(behind, f1[3][..., :3])[2]
    assert np.all(z1[tm.ok_mask(f1[0], f1[2], f1[3])] <= 0)
    stats = {}
    got = tm.model(*f1, c1, hist, behind, flags=1, stats=stats, **tm.PARAMS)
    none = tm.model(*f1, c1, None, c1, flags=1, **tm.PARAMS)
    assert stats["have"] == 0 and got[0][..., 3].max() == 1
    assert_same(got, none, "z1 <= 0")
    assert_same(got, tm.scalar(*f1, c1, hist, behind, flags=1, **tm.PARAMS), "z1 <= 0, scalar")


def test_max_history_caps_n_and_alpha_min_takes_over():
    cam = tm.cameras()[0]
    frames = [tm.make_frame(16, 12, cam, 7, k) for k in range(8)]
    ok = tm.ok_mask(frames[0][0], frames[0][2], frames[0][3])
    hist, ns = None, []
    for f in frames:                                    # alpha_min = 0: n counts up to the cap and stays
        out = tm.model(*f, cam, hist, cam, 0.0, 5, 0.05, 0.9, 0)
        hist = out[1:]
        ns.append(int(out[0][..., 3][ok].max()))
        assert np.all(out[0][..., 3][ok] == ns[-1])
    assert ns == [1, 2, 3, 4, 5, 5, 5, 5]
    hist = None
    for k, f in enumerate(frames, 1):                   # alpha_min = 0.25 replaces 1/n from n = 5 on
        prev = hist
        out = tm.model(*f, cam, hist, cam, 0.25, 100, 0.05, 0.9, 0)
        hist = out[1:]
        a = max(F(1) / F(k), F(0.25))
        if prev is not None:
            with np.errstate(all="ignore"):
                want = (prev[0][..., :3] + a * (f[0][..., :3] - prev[0][..., :3])).astype(F)
            assert tm.same_words(out[1][..., :3][ok], want[ok]), k
    assert np.all(hist[0][..., 3][ok] == 8)


# ---- the Python layer -------------------------------------------------------------------------------
def test_python_refusals_come_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(N, "hip", no_device)
    nan = float("nan")
    for kw, field in ((dict(alpha_min=-0.01), "alpha_min"), (dict(alpha_min=1.5), "alpha_min"), (dict(alpha_min=nan), "alpha_min"),
                      (dict(max_history=0), "max_history"), (dict(max_history=65536), "max_history"),
                      (dict(max_history=2.5), "max_history"), (dict(max_history=nan), "max_history"),
                      (dict(sigma_plane=0.0), "sigma_plane"), (dict(sigma_plane=float("inf")), "sigma_plane"),
                      (dict(sigma_plane=nan), "sigma_plane"), (dict(normal_cos_min=-1.5), "normal_cos_min"),
                      (dict(normal_cos_min=1.01), "normal_cos_min"), (dict(normal_cos_min=nan), "normal_cos_min")):
        with pytest.raises(pa.PathtracerError) as e:
            pa.temporal_params(**kw)
        assert e.value.code == N.PT_ERR_ARG and field in str(e.value), (kw, str(e.value))
    img = np.zeros((4, 6, 4), dtype=np.float32)
    with pytest.raises(pa.PathtracerError) as e:
        pa.temporal_image(img, img, img, img, pa.PtCamera(), alpha_min=2.0)
    assert "alpha_min" in str(e.value)
    with pytest.raises(pa.PathtracerError) as e:
        pa.temporal_image(img, img, np.zeros((4, 5, 4), dtype=np.float32), img, pa.PtCamera())
    assert e.value.code == N.PT_ERR_ARG and "plane1" in str(e.value)
    with pytest.raises(pa.PathtracerError) as e:
        pa.temporal_image(img, img, img, img, pa.PtCamera(), history=(img, img, img))
    assert "prev_camera" in str(e.value)
    pt = pa.Pathtracer.__new__(pa.Pathtracer)
    pt._group, pt._r = None, None
    with pytest.raises(pa.PathtracerError) as e:
        pt.temporal(max_history=0)
    assert e.value.code == N.PT_ERR_ARG and "max_history" in str(e.value)
    with pytest.raises(pa.PathtracerError) as e:
        pt.denoise(source="history")
    assert e.value.code == N.PT_ERR_ARG and "source" in str(e.value)
    pt._group = 1
    for call in (lambda: pt.temporal(), lambda: pt.temporal_image(), lambda: pt.tonemap_temporal(), lambda: pt.temporal_timing()):
        with pytest.raises(pa.PathtracerError) as e:
            call()
        assert e.value.code == N.PT_ERR_STATE


def test_struct_constants_and_defaults_match_the_header(root):
    text = (root / "include" / "pt_hip.h").read_text()
    body = re.search(r"typedef struct pt_temporal_params \{(.*?)\} pt_temporal_params;", text, re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|float)\s+(\w+);", body, re.M)
    ctype = {"uint32_t": C.c_uint32, "float": C.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(N.PtTemporalParams._fields_)
    assert C.sizeof(N.PtTemporalParams) == 4 * len(fields) == 20
    for name in ("PT_TEMPORAL_DEMODULATE", "PT_TEMPORAL_SAME_PRIMITIVE"):
        assert getattr(N, name) == int(re.search(rf"#define {name} (\d+)", text).group(1))
    assert (tm.DEMODULATE, tm.SAME_PRIMITIVE) == (N.PT_TEMPORAL_DEMODULATE, N.PT_TEMPORAL_SAME_PRIMITIVE)
    default = {k: v for k, v in re.findall(r"#define PT_TEMPORAL_DEFAULT_(\w+) (-?[\d.]+)", text)}
    d = pa.TEMPORAL_DEFAULTS
    assert float(default["ALPHA_MIN"]) == d["alpha_min"] and int(default["MAX_HISTORY"]) == d["max_history"]
    assert float(default["SIGMA_PLANE"]) == d["sigma_plane"] and float(default["NORMAL_COS_MIN"]) == d["normal_cos_min"]
    assert int(default["FLAGS"]) == (1 if d["demodulate"] else 0) | (2 if d["same_primitive"] else 0)
    p = pa.temporal_params()
    assert (p.alpha_min, p.max_history, p.flags) == (np.float32(d["alpha_min"]), d["max_history"], int(default["FLAGS"]))
    # the C++ class takes the same defaults from the same macros
    hpp = (root / "include" / "pathtracer_amd.hpp").read_text()
    options = re.search(r"struct TemporalOptions \{(.*?)\};", hpp, re.S).group(1)
    for name in ("ALPHA_MIN", "MAX_HISTORY", "SIGMA_PLANE", "NORMAL_COS_MIN", "FLAGS"):
        assert f"PT_TEMPORAL_DEFAULT_{name}" in options


def test_python_interface():
    sig = inspect.signature(pa.Pathtracer.temporal)
    assert list(sig.parameters)[:8] == ["self", "alpha_min", "max_history", "sigma_plane", "normal_cos_min", "demodulate",
                                        "same_primitive", "reset"]
    assert sig.parameters["reset"].default is False
    assert inspect.signature(pa.Pathtracer.denoise).parameters["source"].default == "accumulation"
    for name in ("temporal_image", "tonemap_temporal", "history_lengths", "temporal_timing"):
        assert callable(getattr(pa.Pathtracer, name))
