"""GPU adaptive sampling (pt_render_adaptive): the device against the numpy restatement of the rule
driven by the CPU oracle (tests/test_adaptive_rule.py), bit for bit -- accumulation, XORWOW state,
moments and per-pixel call counts.  A pixel stopped after n calls holds what n reference render()
calls leave, so everything stays checkable against oracle/.
"""
import numpy as np
import pytest

import pathtracercuda_amd as pa
from oracle import pyoracle as po
from pathtracercuda_amd import _native as N
from test_adaptive_rule import CASES, PARAMS, AdaptiveOracle, check_inputs, expected, make_oracle

pytestmark = pytest.mark.gpu

ADAPTIVE_VARIANTS = (4, 6, 40, 41, 46, 60, 61)      # builds with an adaptive (MODE 5) instantiation


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def gpu_available():
    if pa.device_count() < 1:
        pytest.skip("no GPU")


def tracer(scenes, case):
    name, W, H, band, off, stride = CASES[case]
    pt = pa.Pathtracer(W, H, device=0, row_offset=off, row_stride=stride, band_rows=band)
    cam = pt.load_scene(str(scenes / f"{name}.scene.json"))
    return pt, cam


def assert_state(pt, ad, what):
    for name, got, want in [("accum", pt.accum(), ad.accum), ("moments", pt.moments(), ad.moments()),
                            ("rng", pt.rng_state(), ad.rng_array()), ("counts", pt.sample_counts(), ad.n)]:
        bad = np.argwhere(bits(got) != bits(want))
        assert len(bad) == 0, (f"{what}: {name} differs in {len(bad)} words; first at {tuple(bad[0])}: "
                               f"gpu {got[tuple(bad[0][:2])]} want {want[tuple(bad[0][:2])]}")


@pytest.mark.parametrize("case", list(CASES))
def test_oracle_parity(gpu_available, scenes, case):
    osc, ad = expected(scenes, case)
    check_inputs(case, ad)                      # the oracle alone: every path of the rule is taken
    pt, cam = tracer(scenes, case)
    assert bytes(cam) == bytes(osc.camera)
    res = pt.render_adaptive(cam, **PARAMS)
    assert_state(pt, ad, case)
    assert res["samples"] == sum(ad.steps) * PARAMS["spp"]
    assert res["rounds"] == len(ad.steps) - PARAMS["min_calls"] + 1     # the first min_calls steps are one launch
    assert pt.adaptive and res["gpu_ms"] > 0


def test_tolerance_zero_is_the_plain_render(gpu_available, scenes):
    p = dict(PARAMS, tolerance=0.0)
    pt, cam = tracer(scenes, "shapes")
    pt.render_adaptive(cam, **p)
    a, r = pt.accum(), pt.rng_state()
    assert (pt.sample_counts() == p["max_calls"]).all()
    plain, cam2 = tracer(scenes, "shapes")
    plain.render(cam2, p["spp"], True, chunks=p["max_calls"])
    assert np.array_equal(bits(a), bits(plain.accum())) and np.array_equal(r, plain.rng_state())
    osc, ref = make_oracle(scenes, "shapes")
    ref.render(osc.camera, p["spp"], True, chunks=p["max_calls"])
    assert np.array_equal(bits(a), bits(ref.accum)) and np.array_equal(r, ref.rng_array())
    y = (np.float32(0.2126) * a[..., 0] + np.float32(0.7152) * a[..., 1]) + np.float32(0.0722) * a[..., 2]
    assert np.allclose(pt.moments()[..., 0], y, rtol=1e-5, atol=1e-6)    # m1 is the luminance of the sum


def test_large_tolerance_stops_at_min_calls(gpu_available, scenes):
    p = dict(PARAMS, tolerance=1e9)
    pt, cam = tracer(scenes, "generated")
    res = pt.render_adaptive(cam, **p)
    assert (pt.sample_counts() == p["min_calls"]).all()
    assert res["samples"] == pt.rows * pt.width * p["min_calls"] * p["spp"] and res["rounds"] == 1
    plain, cam2 = tracer(scenes, "generated")
    plain.render(cam2, p["spp"], True, chunks=p["min_calls"])
    assert np.array_equal(pt.rng_state(), plain.rng_state())
    assert np.array_equal(bits(pt.accum()), bits(plain.accum()))


def test_continuation(gpu_available, scenes):
    osc, ad = expected(scenes, "cornell")
    pt, cam = tracer(scenes, "cornell")
    with pytest.raises(pa.PathtracerError) as e:              # nothing to continue on a fresh context
        pt.render_adaptive(cam, **dict(PARAMS, reset=False))
    assert e.value.code == N.PT_ERR_STATE
    first = pt.render_adaptive(cam, **dict(PARAMS, max_calls=4))
    assert pt.sample_counts().max() == 4
    second = pt.render_adaptive(cam, **dict(PARAMS, reset=False))
    assert_state(pt, ad, "4 calls continued to 8")
    assert first["samples"] + second["samples"] == sum(ad.steps) * PARAMS["spp"]
    pt.render_raw(cam, PARAMS["spp"], 1, False)               # a plain device render voids the moments
    with pytest.raises(pa.PathtracerError) as e:
        N.check_ctx(N.hip().pt_render_adaptive(pt._ctx, cam, N.PtAdaptiveParams(4, 2, 8, 0.2, 0.01, 0), None), pt._ctx)
    assert e.value.code == N.PT_ERR_STATE
    with pytest.raises(pa.PathtracerError):
        pt.moments()
    pt.render(cam, PARAMS["spp"], True)                       # and after the host layer's plain render
    with pytest.raises(pa.PathtracerError) as e:
        pt.render_adaptive(cam, **dict(PARAMS, reset=False))
    assert e.value.code == N.PT_ERR_STATE


def test_image_reads_survive_a_scene_or_rng_change(gpu_available, scenes):
    # neither call writes the accumulation or the counts: the image stays readable and the same; only the
    # continuation (reset = False) is refused, as pt_hip.h documents
    pt, cam = tracer(scenes, "cornell")
    pt.render_adaptive(cam, **PARAMS)
    hdr, ldr, m = pt.get_hdr_image_data(), pt.get_image_data(), pt.moments()
    for change in (lambda: pt.set_rng_state(pt.rng_state()), lambda: pt.load_scene(str(scenes / "test_shapes.scene.json"))):
        change()
        assert pt.adaptive and np.array_equal(bits(pt.moments()), bits(m))
        assert np.array_equal(bits(pt.get_hdr_image_data()), bits(hdr)) and np.array_equal(pt.get_image_data(), ldr)
        with pytest.raises(pa.PathtracerError) as e:
            pt.render_adaptive(cam, **dict(PARAMS, reset=False))
        assert e.value.code == N.PT_ERR_STATE


def test_a_device_layer_render_ends_the_adaptive_state(gpu_available, scenes):
    # pt_render past the host layer: the counts no longer describe the buffer, and the flag follows
    pt, cam = tracer(scenes, "cornell")
    pt.render_adaptive(cam, **PARAMS)
    pt.render_raw(cam, PARAMS["spp"], 1, False)
    assert not pt.adaptive and pt.frames == 0
    assert np.array_equal(bits(pt.get_hdr_image_data()), bits(pt.accum())) and pt.get_image_data().shape == (44, 60, 4)


def test_bad_arguments(gpu_available, scenes):
    pt, cam = tracer(scenes, "cornell")
    for bad in (dict(spp=0), dict(min_calls=1), dict(max_calls=1), dict(tolerance=-1.0), dict(floor=-0.5),
                dict(tolerance=float("nan"))):
        with pytest.raises(pa.PathtracerError) as e:
            pt.render_adaptive(cam, **dict(PARAMS, **bad))
        assert e.value.code == N.PT_ERR_ARG, bad
    pt.set_kernel_variant(39)                                 # a shipped variant without an adaptive build
    with pytest.raises(pa.PathtracerError) as e:
        pt.render_adaptive(cam, **PARAMS)
    assert e.value.code == N.PT_ERR_ARG and "adaptive build" in str(e.value)


@pytest.mark.parametrize("W,H", [(8, 8), (7, 5)])
def test_small_images(gpu_available, scenes, W, H):
    # at most one wave of pixels: every round after the first launch is one partial wave
    scene = scenes / "cornell_box.scene.json"
    pt = pa.Pathtracer(W, H)
    cam = pt.load_scene(str(scene))
    osc = po.load_scene(scene, W, H)
    ad = AdaptiveOracle(po.OracleRenderer(osc, W, H)).render(osc.camera, **PARAMS)
    assert len(ad.steps) > PARAMS["min_calls"] and 0 < max(ad.steps[PARAMS["min_calls"]:]) < 64
    pt.render_adaptive(cam, **PARAMS)
    assert_state(pt, ad, f"{W}x{H}")


def test_nothing_active_ends_without_a_launch(gpu_available, scenes):
    # everything converges at min_calls: the evaluation finds no active pixel and the render ends after
    # its one fused launch; continuing it launches nothing at all
    pt, cam = tracer(scenes, "cornell")
    res = pt.render_adaptive(cam, **dict(PARAMS, tolerance=1e9))
    assert res["rounds"] == 1
    a, r, m = pt.accum(), pt.rng_state(), pt.moments()
    res = pt.render_adaptive(cam, **dict(PARAMS, tolerance=1e9, reset=False))
    assert res["rounds"] == 0 and res["samples"] == 0
    assert np.array_equal(bits(a), bits(pt.accum())) and np.array_equal(r, pt.rng_state())
    assert np.array_equal(bits(m), bits(pt.moments()))


def test_plain_render_continues_the_streams(gpu_available, scenes):
    # after an adaptive render a plain device-layer call (pt_render, no history reset) goes on from
    # every pixel's own stream position: the oracle continued the same way (one more call of all pixels)
    osc, ref = make_oracle(scenes, "shapes")
    ad = AdaptiveOracle(ref).render(osc.camera, **PARAMS)
    pt, cam = tracer(scenes, "shapes")
    pt.render_adaptive(cam, **PARAMS)
    pt.render_raw(cam, PARAMS["spp"], 1, False)
    ref.render(osc.camera, PARAMS["spp"], True)
    want = ad.accum.copy()
    want[..., :3] = ref.accum[..., :3] + ad.accum[..., :3]
    assert np.array_equal(bits(pt.accum()), bits(want))
    assert np.array_equal(pt.rng_state(), ref.rng_array())


def test_every_adaptive_build_agrees(gpu_available, scenes):
    osc, ad = expected(scenes, "shapes")
    for v in ADAPTIVE_VARIANTS:
        pt, cam = tracer(scenes, "shapes")
        pt.set_kernel_variant(v)
        pt.render_adaptive(cam, **PARAMS)
        assert pt.last_variant == v
        assert_state(pt, ad, f"variant {v}")


def test_persistent_grid_larger_than_the_chip(gpu_available, scenes):
    # 14,400 waves of active pixels against a few thousand resident ones: the cursor path of the
    # persistent builds.  GPU against GPU (the oracle would take minutes at this size).
    pt = pa.Pathtracer(1280, 720)
    cam = pt.load_scene(str(scenes / "generated_scene.scene.json"))
    st = pt.rng_state()
    pt.render(cam, 4, True, chunks=2)
    want_a, want_r = bits(pt.accum()).copy(), pt.rng_state()
    pt.set_rng_state(st)
    res = pt.render_adaptive(cam, 4, 2, 2, 0.0)
    assert res["rounds"] == 1 and (pt.sample_counts() == 2).all()
    assert np.array_equal(bits(pt.accum()), want_a) and np.array_equal(pt.rng_state(), want_r)


def test_host_layer_outputs(gpu_available, scenes, tmp_path):
    import subprocess
    from PIL import Image
    name, W, H = CASES["cornell"][:3]
    scene = scenes / f"{name}.scene.json"
    p = dict(spp=8, min_calls=2, max_calls=8, tolerance=0.2, floor=0.01)    # the CLI's calls of 8
    pt = pa.Pathtracer(W, H)
    cam = pt.load_scene(str(scene))
    pt.render_adaptive(cam, **p)
    a, n = pt.accum(), pt.sample_counts()
    assert len(np.unique(n)) > 2
    hdr = pt.get_hdr_image_data()
    assert np.array_equal(bits(hdr[..., :3]), bits(a[..., :3] / n[..., None].astype(np.float32)))
    # the oracle's tonemap (tonemap.cu:4-27) with frames = n, run once per distinct n
    holder = po.OracleRenderer(po.OracleScene(), W, H)
    holder.accum[:] = a
    want = np.zeros((H, W, 4), dtype=np.uint8)
    for k in np.unique(n):
        want[n == k] = holder.tonemap(frames=int(k))[n == k]
    img = pt.get_image_data()
    assert np.array_equal(img, want)
    noise = pt.noise_map()
    assert noise.shape == (H, W) and np.isfinite(noise).all() and (noise >= 0).all()
    # the frame counter no longer describes the buffer: the host layer refuses to go on accumulating
    with pytest.raises(pa.PathtracerError) as e:
        pt.render(cam, 8, False)
    assert e.value.code == N.PT_ERR_STATE
    pt.render(cam, 8, True)                                   # ignore_history returns to normal
    assert not pt.adaptive and pt.frames == 1
    png = tmp_path / "adaptive.png"
    r = subprocess.run([str(N.CLI), "-w", str(W), "-h", str(H), "-spp", "64", "-adaptive", "0.2", "-o", str(png), str(scene)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    mean_spp = float(n.sum()) * 8 / (W * H)
    assert f"Finished accumulating {mean_spp:f} samples per pixel on average" in r.stdout, r.stdout
    assert np.array_equal(np.asarray(Image.open(png).convert("RGBA")), want[::-1])
