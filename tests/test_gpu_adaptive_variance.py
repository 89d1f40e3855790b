"""The variance of an adaptive render's image on the GPU against its numpy restatement
(tests/adaptive_variance_model.py): words equal, or both NaN, no tolerance -- through pt_adaptive_variance_image
on the seeded inputs, staged and unstaged, and through the context on an adaptive render of the Cornell box --
then what the call must leave alone (the render state), what it refuses, and that the filter it guides filters.
"""
import numpy as np
import pytest

import adaptive_variance_model as am
import denoise_model as dm
import pathtracercuda_amd as pa
import svgf_model as sm
import temporal_model as tm
from pathtracercuda_amd import _native as N
from test_gpu_parity import assert_bitexact
from test_gpu_temporal import first_difference, tonemapped_mse

pytestmark = pytest.mark.gpu

F = am.F
TW, TH = dm.TILE_W, dm.TILE_H
# degenerate images narrower than the halo of 3; the workgroup tile, one less and one more in both dimensions; several tiles
SIZES = [(1, 1), (1, 7), (5, 1), (TW - 1, TH - 1), (TW, TH), (TW + 1, TH + 1), (am.WIDTH, am.HEIGHT), (70, 45)]
SIGMA_PLANE = am.PARAMS["sigma_plane"]


@pytest.fixture(scope="module")
def gpu_available():
    if pa.device_count() < 1:
        pytest.skip("no GPU")


def device(color, p0, p1, p2, mom, min_batches, sigma_plane, normal_cos_min, flags, staging=0):
    """pt_adaptive_variance_image with adaptive_variance_model.model's signature."""
    return pa.adaptive_variance_image(color, p0, p1, p2, mom, min_batches=min_batches, sigma_plane=sigma_plane,
                                      normal_cos_min=normal_cos_min, demodulate=bool(flags & 1),
                                      same_primitive=bool(flags & 2), staging=staging)


def difference(got, want):
    return first_difference(np.atleast_3d(got), np.atleast_3d(want))


@pytest.mark.parametrize("width,height", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_both_forms_equal_the_model(gpu_available, width, height):
    args = am.make_inputs(width, height, seed=1000 * width + height)[:5]
    young = 0
    for flags in (0, 1, 2, 3):
        for min_batches in (2, 4, 255):
            for cos_min in (0.0, 1.0):
                counts = {}
                want = am.model(*args, min_batches, SIGMA_PLANE, cos_min, flags, counts=counts)
                young += counts["young"]
                assert (min_batches == 2) == (counts["young"] == 0) or width * height < 8
                for staging in (0, 1, 2):
                    got = device(*args, min_batches, SIGMA_PLANE, cos_min, flags, staging)
                    assert sm.same_words(got, want), (f"flags {flags}, min_batches {min_batches}, cos {cos_min}, staging "
                                                      f"{staging}: " + difference(got, want))
    assert young > 0 or width * height == 1


def test_the_seeded_input_reaches_every_branch_on_the_device_too(gpu_available):
    # the branch counts of tests/test_adaptive_variance_rule.py are the model's; here the same input and parameters,
    # and a second plane tolerance at which the window takes almost every tap
    args = am.make_inputs(am.WIDTH, am.HEIGHT, 1)[:5]
    for sigma_plane in (SIGMA_PLANE, 1e-6, 1e3):
        want = am.model(*args, am.PARAMS["min_batches"], sigma_plane, am.PARAMS["normal_cos_min"], 3)
        for staging in (1, 2):
            got = device(*args, am.PARAMS["min_batches"], sigma_plane, am.PARAMS["normal_cos_min"], 3, staging)
            assert sm.same_words(got, want), f"sigma_plane {sigma_plane}, staging {staging}: " + difference(got, want)


# ---- on a context ----------------------------------------------------------------------------------------
ADAPTIVE = dict(spp=1, min_calls=4, max_calls=16, tolerance=0.05)
AVAR = dict(min_batches=8, window_sigma_plane=0.05, normal_cos_min=0.9)
VDN = dict(iterations=3, sigma_l=2.0, variance_floor=1e-6, sigma_plane=0.03, normal_power_log2=3, demodulate=True,
           same_primitive=False)
VDN_ARGS = (3, 2.0, 1e-6, 0.03, 3, 1)


def adaptive_color(pt):
    """The image pt_denoise_adaptive filters: dn_color_kernel's division by every pixel's own count."""
    n = np.maximum(pt.sample_counts(), 1).astype(F)
    return (pt.accum() / n[..., None]).astype(F)


def render_state(pt):
    return (pt.accum(), pt.rng_state(), pt.moments(), pt.last_variant, pt.tile_costs(), pt.frames, pt.adaptive)


def assert_same_state(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, np.ndarray):
            assert np.array_equal(dm.bits(x) if x.dtype == np.float32 else x, dm.bits(y) if y.dtype == np.float32 else y), \
                f"{what}: item {k} of the render state moved"
        else:
            assert x == y, f"{what}: item {k} of the render state moved"


@pytest.fixture(scope="module")
def cornell(gpu_available, scenes):
    """One adaptive render of the Cornell box with its planes, shared and never rendered to again."""
    W = H = 64
    scene = str(scenes / "cornell_box.scene.json")
    pt = pa.Pathtracer(W, H)
    cam = pt.load_scene(scene)
    pt.render(cam, 1, True)                      # (so that tile costs exist: an adaptive render dispatches no tiles)
    pt.render_adaptive(cam, **ADAPTIVE)
    planes = pt.features(cam)["planes"]
    return pt, cam, planes, scene


def test_the_context_equals_the_model_and_leaves_the_render_state_alone(cornell):
    pt, cam, planes, scene = cornell
    before = render_state(pt)
    counts_before = pt.sample_counts()
    assert counts_before.min() >= 4 and (counts_before == 4).sum() > 64 and (counts_before >= 8).sum() > 64
    out = pt.denoise(guide="adaptive", **AVAR, **VDN)
    var = pt.adaptive_variance()
    assert_same_state(render_state(pt), before, "pt_denoise_adaptive")
    color, mom = adaptive_color(pt), pt.moments()
    counts = {}
    want = am.model(color, *planes, mom, 8, 0.05, 0.9, 1, counts=counts)
    print(counts)
    assert counts["young"] > 64 and counts["old"] > 64 and counts["vs_wins"] > 0 and counts["own_wins"] > 0
    assert sm.same_words(var, want), difference(var, want)
    # the filter is pt_denoise_variance_image's on the same inputs (device against device), and the model's
    again = pa.denoise_variance_image(color, *planes, var, **VDN)
    assert sm.same_words(out, again), first_difference(out, again)
    assert sm.same_words(out, sm.filter_model(color, *planes, var, *VDN_ARGS))
    assert sm.same_words(pt.denoised(), out) and not sm.same_words(out[..., :3], color[..., :3])
    assert pt.adaptive_variance_timing() > 0 and pt.denoise_timing()["iterations"][2] > 0
    # staged and unstaged write the same words on the context too
    for staging in (1, 2):
        assert sm.same_words(pt.denoise(guide="adaptive", staging=staging, **AVAR, **VDN), out)
        assert sm.same_words(pt.adaptive_variance(), var)
    # min_batches = 2: nobody is young
    pt.denoise(guide="adaptive", min_batches=2, **VDN)
    assert sm.same_words(pt.adaptive_variance(), am.model(color, *planes, mom, 2, 0.3, 0.0, 1))
    assert_same_state(render_state(pt), before, "pt_denoise_adaptive, again")


def test_a_continued_render_equals_a_twin_that_never_denoised(gpu_available, scenes):
    W = H = 64
    scene = str(scenes / "cornell_box.scene.json")
    pt, twin = pa.Pathtracer(W, H), pa.Pathtracer(W, H)
    cam = pt.load_scene(scene)
    twin.load_scene(scene)
    for p in (pt, twin):
        p.render_adaptive(cam, 1, min_calls=2, max_calls=6, tolerance=0.05)
        p.features(cam)
    pt.denoise(guide="adaptive", **VDN)
    more = dict(spp=1, min_calls=2, max_calls=12, tolerance=0.05, reset=False)
    a, b = pt.render_adaptive(cam, **more), twin.render_adaptive(cam, **more)
    assert a["samples"] == b["samples"] and a["rounds"] == b["rounds"] and a["samples"] > 0
    assert_bitexact(pt.accum(), twin.accum(), "the continued adaptive render")
    assert np.array_equal(pt.rng_state(), twin.rng_state())
    assert np.array_equal(dm.bits(pt.moments()), dm.bits(twin.moments()))
    # the continued render wrote the accumulation: the variance held is no longer of the counts
    with pytest.raises(pa.PathtracerError) as e:
        pt.adaptive_variance()
    assert e.value.code == N.PT_ERR_STATE


def refused(code, word, call, *args, **kw):
    with pytest.raises(pa.PathtracerError) as e:
        call(*args, **kw)
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_context_refusals_name_the_reason(gpu_available, scenes):
    W, H = 40, 36
    scene = str(scenes / "cornell_box.scene.json")
    pt = pa.Pathtracer(W, H)
    cam = pt.load_scene(scene)
    quick = dict(spp=1, min_calls=2, max_calls=4, tolerance=0.1)
    # before any adaptive render, with and without planes
    refused(N.PT_ERR_STATE, "adaptive render", pt.denoise, guide="adaptive")
    pt.features(cam)
    refused(N.PT_ERR_STATE, "adaptive render", pt.denoise, guide="adaptive")
    refused(N.PT_ERR_STATE, "variance", pt.adaptive_variance)
    refused(N.PT_ERR_STATE, "variance", pt.adaptive_variance_timing)
    # after a plain render
    pt.render_adaptive(cam, **quick)
    pt.render(cam, 1, True)
    refused(N.PT_ERR_STATE, "adaptive render", pt.denoise, guide="adaptive")
    # an adaptive render and planes: allowed; a refused call afterwards changes nothing
    pt.render_adaptive(cam, **quick)
    out = pt.denoise(guide="adaptive")
    var = pt.adaptive_variance()
    lib = N.hip()
    A, V = N.PtAdaptiveVarianceParams, N.PtVDenoiseParams
    good_a, good_v = pa.adaptive_variance_params(), pa.vdenoise_params()
    for a, v, field in ((A(1, 0.3, 0.0, 1), good_v, "min_batches"), (A(8, float("nan"), 0.0, 1), good_v, "sigma_plane"),
                        (A(8, 0.3, 2.0, 1), good_v, "normal_cos_min"), (A(8, 0.3, 0.0, 8), good_v, "flags"),
                        (good_a, V(3, 0.0, 1e-6, 0.1, 1, 1, 0), "sigma_l"), (good_a, V(3, 1.0, 1e-6, 0.1, 1, 1, 3), "staging"),
                        # a DEMODULATE bit that differs between the estimate and the filter
                        (A(8, 0.3, 0.0, 0), good_v, "DEMODULATE"), (A(8, 0.3, 0.0, 3), V(3, 1.0, 1e-6, 0.1, 1, 2, 0), "DEMODULATE")):
        assert lib.pt_denoise_adaptive(pt._ctx, N.C.byref(a), N.C.byref(v)) == N.PT_ERR_ARG
        assert field in lib.pt_last_error(pt._ctx).decode(), (field, lib.pt_last_error(pt._ctx).decode())
    assert lib.pt_denoise_adaptive(pt._ctx, None, N.C.byref(good_v)) == N.PT_ERR_ARG
    assert lib.pt_denoise_adaptive(pt._ctx, N.C.byref(good_a), None) == N.PT_ERR_ARG
    assert sm.same_words(pt.denoised(), out) and sm.same_words(pt.adaptive_variance(), var)
    # features rendered since: the variance read is refused (it was made with the planes held then), the filter runs again
    pt.features(cam)
    refused(N.PT_ERR_STATE, "variance", pt.adaptive_variance)
    assert sm.same_words(pt.denoised(), out)
    assert sm.same_words(pt.denoise(guide="adaptive"), out) and sm.same_words(pt.adaptive_variance(), var)
    # a scene change without new features: the counts still describe the buffer, the planes are gone
    cam = pt.load_scene(scene)
    assert pt.adaptive
    refused(N.PT_ERR_STATE, "feature planes", pt.denoise, guide="adaptive")
    assert sm.same_words(pt.adaptive_variance(), var)           # refused: nothing changed
    pt.features(cam)
    pt.denoise(guide="adaptive")


def test_band_partition_is_refused_by_name(gpu_available, scenes):
    pt = pa.Pathtracer(64, 64, band_rows=8, row_offset=1, row_stride=2)
    cam = pt.load_scene(str(scenes / "cornell_box.scene.json"))
    pt.render_adaptive(cam, 1, min_calls=2, max_calls=4, tolerance=0.1)
    pt.features(cam)
    refused(N.PT_ERR_ARG, "whole frame", pt.denoise, guide="adaptive")


def test_host_layer(cornell):
    """The C++ layer (Pathtracer::denoiseAdaptive / adaptiveVariance through its C ABI): the Python path's words, and
    the result is a denoised image.  Runs last on the shared context: it leaves the host's denoised
    flag set."""
    pt, cam, planes, scene = cornell
    host = N.host()
    a = pa.adaptive_variance_params(8, 0.05, 0.9)
    v = pa.vdenoise_params(**VDN)
    want = pt.denoise(guide="adaptive", **AVAR, **VDN)
    var = pt.adaptive_variance()
    assert host.pth_renderer_denoised(pt._r) == 0
    N.check_host(host.pth_renderer_denoise_adaptive(pt._r, N.C.byref(a), N.C.byref(v)))
    assert host.pth_renderer_denoised(pt._r) == 1
    H, W = var.shape
    got = np.ctypeslib.as_array(host.pth_renderer_adaptive_variance(pt._r), shape=(H, W)).copy()
    assert sm.same_words(got, var) and sm.same_words(pt.get_hdr_image_data(), want)
    assert np.array_equal(pt.get_image_data(), pt.tonemap_denoised())
    a.min_batches = 1
    assert host.pth_renderer_denoise_adaptive(pt._r, N.C.byref(a), N.C.byref(v)) == N.PT_ERR_ARG
    assert "min_batches" in host.pth_last_error().decode()
    fresh = pa.Pathtracer(16, 16)
    assert not host.pth_renderer_adaptive_variance(fresh._r)
    assert host.pth_renderer_denoise_adaptive(fresh._r, N.C.byref(pa.adaptive_variance_params()), N.C.byref(v)) == N.PT_ERR_STATE


def test_it_filters_adaptive(gpu_available, scenes):
    """A condition, not a tuned threshold: on an adaptive render of the Cornell box (1-spp calls, 4 to 16 of them,
    tolerance 0.05) the filter guided by the render's own variance, with the defaults, is closer to a 1024-spp render
    of the same camera than the unfiltered adaptive image (tonemapped MSE over the hit, finite pixels).  The plain
    a-trous filter's error and the error with min_batches = 2 (no window) are printed beside it and not asserted.
    Measured on MI355X: adaptive 0.3001, then adaptive-guided 0.1063 (ratio 0.354), min_batches 2 0.1365 (0.455),
    a-trous 0.1170 (0.390); mean calls 11.35."""
    W = H = 64
    scene = str(scenes / "cornell_box.scene.json")
    pt, ref = pa.Pathtracer(W, H), pa.Pathtracer(W, H)
    cam = pt.load_scene(scene)
    ref.load_scene(scene)
    pt.render_adaptive(cam, **ADAPTIVE)
    planes = pt.features(cam)["planes"]
    ref.render(cam, 8, True, chunks=128)
    truth, raw = ref.get_image_data(), pt.get_image_data()
    hdr = pt.get_hdr_image_data()
    pt.denoise(guide="adaptive")
    guided = pt.tonemap_denoised()
    pt.denoise(guide="adaptive", min_batches=2)
    unwindowed = pt.tonemap_denoised()
    pt.denoise()
    plain = pt.tonemap_denoised()
    mask = tm.ok_mask(hdr, planes[1], planes[2]) & np.isfinite(ref.get_hdr_image_data()[..., :3]).all(-1)
    before, after, no_window, atrous = (tonemapped_mse(img, truth, mask) for img in (raw, guided, unwindowed, plain))
    print(f"tonemapped MSE over {int(mask.sum())} hit finite pixels: adaptive {before:.6f}, then adaptive-guided {after:.6f} "
          f"(ratio {after / before:.3f}), min_batches 2 {no_window:.6f} (ratio {no_window / before:.3f}), a-trous {atrous:.6f} "
          f"(ratio {atrous / before:.3f}); mean calls {pt.sample_counts().mean():.2f}")
    assert mask.sum() > W * H // 2
    assert after < before
