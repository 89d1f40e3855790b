"""The per-pixel variance and the variance-guided filter on the GPU against their numpy restatement
(tests/svgf_model.py): words equal, or both NaN, no tolerance -- through the _image entry points on the seeded
inputs, through the context on rendered frames under a moving camera -- then what the passes must leave alone
(the render state, pt_temporal's own words), what they refuse, and that the filter filters.
"""
import numpy as np
import pytest

import denoise_model as dm
import domain_scenes as dsc
import pathtracercuda_amd as pa
import svgf_model as sm
import temporal_model as tm
from pathtracercuda_amd import _native as N
from test_gpu_parity import assert_bitexact
from test_gpu_temporal import copy_camera, first_difference, move, pt_camera, tonemapped_mse

pytestmark = pytest.mark.gpu

F = sm.F
TW, TH = dm.TILE_W, dm.TILE_H
# degenerate images; the workgroup tile, one less and one more in both dimensions; several tiles
SIZES = [(1, 1), (1, 7), (5, 1), (TW, TH), (TW - 1, TH - 1), (TW + 1, TH + 1), (tm.WIDTH, tm.HEIGHT)]
NAMES = ("image", "h0", "h1", "h2", "h3", "variance")


@pytest.fixture(scope="module")
def gpu_available():
    if pa.device_count() < 1:
        pytest.skip("no GPU")


def device_step(color, p0, p1, p2, cur, hist, prev, alpha_min, max_history, sigma_plane, normal_cos_min, flags, min_temporal):
    """pt_temporal_moments_image with svgf_model.model's signature."""
    return pa.temporal_moments_image(color, p0, p1, p2, pt_camera(cur), hist, pt_camera(prev) if hist is not None else None,
                                     alpha_min=alpha_min, max_history=max_history, sigma_plane=sigma_plane,
                                     normal_cos_min=normal_cos_min, demodulate=bool(flags & 1),
                                     same_primitive=bool(flags & 2), min_temporal=min_temporal)


def plain_step(color, p0, p1, p2, cur, hist, prev, alpha_min, max_history, sigma_plane, normal_cos_min, flags):
    return pa.temporal_image(color, p0, p1, p2, pt_camera(cur), hist, pt_camera(prev) if hist is not None else None,
                             alpha_min=alpha_min, max_history=max_history, sigma_plane=sigma_plane,
                             normal_cos_min=normal_cos_min, demodulate=bool(flags & 1), same_primitive=bool(flags & 2))


def difference(got, want):
    g, w = np.atleast_3d(got), np.atleast_3d(want)
    return first_difference(g, w)


def assert_step(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert sm.same_words(g, w), f"{what}, {name}: " + difference(g, w)


# ---- the moments step and the estimate -------------------------------------------------------------------
@pytest.mark.parametrize("width,height", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_three_chained_frames_equal_the_model(gpu_available, width, height):
    seq = sm.make_sequence(width, height, seed=1000 * width + height)
    whole = (width, height) == (tm.WIDTH, tm.HEIGHT)
    for flags in ((0, 1, 2, 3) if whole else (3,)):
        plain = tm.run_sequence(plain_step, seq, flags)
        for mt in ((1, 2, 4) if whole else (4, 1)[:1 + (width * height > 1)]):
            stats = []
            want = sm.run_sequence(sm.model, seq, flags, min_temporal=mt, stats=stats)
            got = sm.run_sequence(device_step, seq, flags, min_temporal=mt)
            print(f"{width}x{height}, flags {flags}, min_temporal {mt}:", [(s["spatial"], s["temporal"], s["restarted"]) for s in stats])
            for k in range(3):
                assert_step(got[k], want[k], f"flags {flags}, min_temporal {mt}, frame {k}")
                # the image and planes 0..2 are pt_temporal's words (device against device)
                for name, g, w in zip(NAMES[:4], got[k][:4], plain[k]):
                    assert sm.same_words(g, w), f"flags {flags}, frame {k}: {name} is not pt_temporal_image's"
            if whole:
                assert (mt == 1 or stats[2]["spatial"] > 0) and (mt == 4 or stats[2]["temporal"] > 0)
                assert max(s["restarted"] for s in stats) > 0


def test_a_history_whose_moments_are_not_finite_restarts(gpu_available):
    (c0, f0), (c1, f1) = sm.make_sequence()[:2]
    first = sm.model(*f0, c0, None, c0, flags=1, **tm.PARAMS)
    h3 = first[4].copy()
    cols = np.arange(h3.shape[1])[None, :]
    h3[..., 0][(cols % 3 == 0) & (h3[..., 2] >= 0)] = F(np.inf)
    h3[..., 1][(cols % 3 == 1) & (h3[..., 2] >= 0)] = F(np.nan)
    hist = (first[1], first[2], first[3], h3)
    stats = {}
    want = sm.model(*f1, c1, hist, c0, flags=1, min_temporal=2, stats=stats, **tm.PARAMS)
    assert stats["restarted"] > 100
    got = device_step(*f1, c1, hist, c0, flags=1, min_temporal=2, **tm.PARAMS)
    assert_step(got, want, "moments that are not finite")


# ---- the filter ----------------------------------------------------------------------------------------
def device_filter(color, p0, p1, p2, var, iterations, flags, staging=0, **kw):
    p = dict(sm.VPARAMS, **kw)
    return pa.denoise_variance_image(color, p0, p1, p2, var, iterations=iterations, sigma_l=p["sigma_l"],
                                     variance_floor=p["variance_floor"], sigma_plane=p["sigma_plane"],
                                     normal_power_log2=p["normal_power_log2"], demodulate=bool(flags & 1),
                                     same_primitive=bool(flags & 2), staging=staging)


@pytest.mark.parametrize("width,height", SIZES[:-1], ids=[f"{w}x{h}" for w, h in SIZES[:-1]])
def test_filter_equals_the_model_at_the_tile_edges(gpu_available, width, height):
    color, p0, p1, p2, var, _ = sm.make_filter_inputs(width, height, 7 * width + height)
    for flags in (3, 0):
        want = sm.filter_model(color, p0, p1, p2, var, 4, flags=flags, **sm.VPARAMS)
        for staging in (0, 1, 2):
            got = device_filter(color, p0, p1, p2, var, 4, flags, staging)
            assert sm.same_words(got, want), f"flags {flags}, staging {staging}: " + first_difference(got, want)


@pytest.mark.parametrize("iterations", (1, 2, 3, 4, 5, 6))
def test_filter_equals_the_model_at_every_depth(gpu_available, iterations):
    color, p0, p1, p2, var, cls = sm.make_filter_inputs(tm.WIDTH, tm.HEIGHT, 21)
    assert set(np.unique(cls)) == set(range(len(sm.CLASSES)))
    for flags in (0, 1, 2, 3):
        want = sm.filter_model(color, p0, p1, p2, var, iterations, flags=flags, **sm.VPARAMS)
        keep = sm.vkeep_mask(color, p0, p1, p2, var, flags)
        assert keep.mean() > 0.5 and (sm.bits(want[..., :3]) != sm.bits(color[..., :3])).any(-1)[keep].mean() > 0.9
        for staging in (0, 1, 2):
            got = device_filter(color, p0, p1, p2, var, iterations, flags, staging)
            assert sm.same_words(got, want), f"flags {flags}, staging {staging}: " + first_difference(got, want)


def test_filter_equals_the_model_over_many_tiles_and_other_parameters(gpu_available):
    color, p0, p1, p2, var, _ = sm.make_filter_inputs(70, 45, 5)
    for flags, kw in ((1, {}), (3, dict(sigma_l=0.25, variance_floor=1e-8, normal_power_log2=0)),
                      (0, dict(sigma_l=2.0 ** 20, variance_floor=1e-4, sigma_plane=1e-6, normal_power_log2=7))):
        p = dict(sm.VPARAMS, **kw)
        want = sm.filter_model(color, p0, p1, p2, var, 6, flags=flags, **p)
        for staging in (0, 1, 2):
            got = device_filter(color, p0, p1, p2, var, 6, flags, staging, **kw)
            assert sm.same_words(got, want), f"flags {flags}, {kw}, staging {staging}: " + first_difference(got, want)


# ---- refusals --------------------------------------------------------------------------------------------
def test_device_refusals_name_the_field(gpu_available):
    img = np.zeros((4, 4, 4), dtype=np.float32)
    fp = N.C.POINTER(N.C.c_float)
    ptr, cam, nan, inf = img.ctypes.data_as(fp), N.C.byref(pa.PtCamera()), float("nan"), float("inf")
    lib = N.hip()
    V = N.PtVDenoiseParams
    for params, field in ((V(0, 1.0, 1e-6, 0.1, 1, 1, 0), "iterations"), (V(9, 1.0, 1e-6, 0.1, 1, 1, 0), "iterations"),
                          (V(3, 0.0, 1e-6, 0.1, 1, 1, 0), "sigma_l"), (V(3, -1.0, 1e-6, 0.1, 1, 1, 0), "sigma_l"),
                          (V(3, 2.0 ** 20 + 1, 1e-6, 0.1, 1, 1, 0), "sigma_l"), (V(3, inf, 1e-6, 0.1, 1, 1, 0), "sigma_l"),
                          (V(3, nan, 1e-6, 0.1, 1, 1, 0), "sigma_l"), (V(3, 1.0, 0.0, 0.1, 1, 1, 0), "variance_floor"),
                          (V(3, 1.0, -1e-6, 0.1, 1, 1, 0), "variance_floor"), (V(3, 1.0, inf, 0.1, 1, 1, 0), "variance_floor"),
                          (V(3, 1.0, nan, 0.1, 1, 1, 0), "variance_floor"), (V(3, 1.0, 1e-6, 1e-7, 1, 1, 0), "sigma_plane"),
                          (V(3, 1.0, 1e-6, inf, 1, 1, 0), "sigma_plane"), (V(3, 1.0, 1e-6, nan, 1, 1, 0), "sigma_plane"),
                          (V(3, 1.0, 1e-6, 0.1, 8, 1, 0), "normal_power_log2"), (V(3, 1.0, 1e-6, 0.1, 1, 4, 0), "flags"),
                          (V(3, 1.0, 1e-6, 0.1, 1, 1, 3), "staging")):
        rc = lib.pt_denoise_variance_image(0, 4, 4, ptr, ptr, ptr, ptr, ptr, N.C.byref(params), ptr)
        assert rc == N.PT_ERR_ARG and field in lib.pt_last_error(None).decode(), (field, rc)
    good = V(3, 2.0 ** 20, 1e-6, 0.1, 1, 1, 0)
    assert lib.pt_denoise_variance_image(0, 4, 4, ptr, ptr, ptr, ptr, ptr, N.C.byref(good), ptr) == N.PT_OK
    assert lib.pt_denoise_variance_image(0, 4, 4, ptr, ptr, ptr, ptr, None, N.C.byref(good), ptr) == N.PT_ERR_ARG
    T, M = N.PtTemporalParams, N.PtVarianceParams
    t_good = T(0.1, 8, 0.1, 0.5, 1)

    def step(t, m, h0=None):
        return lib.pt_temporal_moments_image(0, 4, 4, ptr, ptr, ptr, ptr, cam, h0, None, None, None, None, N.C.byref(t),
                                             N.C.byref(m), ptr, ptr, ptr, ptr, ptr, ptr)

    for m in (M(0), M(256)):
        assert step(t_good, m) == N.PT_ERR_ARG and "min_temporal" in lib.pt_last_error(None).decode()
    for t, field in ((T(1.5, 8, 0.1, 0.5, 1), "alpha_min"), (T(0.1, 0, 0.1, 0.5, 1), "max_history"),
                     (T(0.1, 8, nan, 0.5, 1), "sigma_plane"), (T(0.1, 8, 0.1, 1.5, 1), "normal_cos_min"),
                     (T(0.1, 8, 0.1, 0.5, 4), "flags")):
        assert step(t, M(4)) == N.PT_ERR_ARG and field in lib.pt_last_error(None).decode(), field
    assert step(t_good, M(4), ptr) == N.PT_ERR_ARG and "hist0" in lib.pt_last_error(None).decode()
    assert step(t_good, M(1)) == N.PT_OK and step(t_good, M(255)) == N.PT_OK
    # a context with nothing on it
    pt = pa.Pathtracer(16, 16)
    assert lib.pt_temporal_moments(pt._ctx, 1, N.C.byref(t_good), N.C.byref(M(0)), 0, None) == N.PT_ERR_ARG
    assert "min_temporal" in lib.pt_last_error(pt._ctx).decode()
    assert lib.pt_temporal_moments(pt._ctx, 1, N.C.byref(t_good), N.C.byref(M(4)), 0, None) == N.PT_ERR_STATE
    assert "feature" in lib.pt_last_error(pt._ctx).decode()
    assert lib.pt_read_temporal_variance(pt._ctx, ptr) == N.PT_ERR_STATE
    assert lib.pt_read_temporal_moments_timing(pt._ctx, ptr) == N.PT_ERR_STATE
    assert lib.pt_denoise_variance(pt._ctx, N.C.byref(V(3, 0.0, 1e-6, 0.1, 1, 1, 0))) == N.PT_ERR_ARG
    assert "sigma_l" in lib.pt_last_error(pt._ctx).decode()
    assert lib.pt_denoise_variance(pt._ctx, N.C.byref(good)) == N.PT_ERR_STATE
    assert "variance" in lib.pt_last_error(pt._ctx).decode()


# ---- on a context ----------------------------------------------------------------------------------------
PARAMS = dict(alpha_min=0.1, max_history=16, sigma_plane=0.05, normal_cos_min=0.9, demodulate=True, same_primitive=False)
MODEL_ARGS = (0.1, 16, 0.05, 0.9, 1)
VDN = dict(iterations=3, sigma_l=2.0, variance_floor=1e-6, sigma_plane=0.03, normal_power_log2=3, demodulate=True,
           same_primitive=False)
VDN_ARGS = (3, 2.0, 1e-6, 0.03, 3, 1)
DN = dict(iterations=3, sigma_color=0.4, sigma_plane=0.03, normal_power_log2=3, demodulate=True, same_primitive=False)


def test_a_moving_camera_equals_the_model_and_the_render_state_is_left_alone(gpu_available, scenes):
    W = H = 64
    scene = str(scenes / "cornell_box.scene.json")
    pt, twin, bare = pa.Pathtracer(W, H), pa.Pathtracer(W, H), pa.Pathtracer(W, H)
    cam = pt.load_scene(scene)
    twin.load_scene(scene)
    bare.load_scene(scene)
    hist, prev = None, None
    for k in range(4):
        for p in (pt, twin, bare):
            p.render(cam, 1, True)
        accum, rng = pt.accum(), pt.rng_state()
        variant, costs, frames = pt.last_variant, pt.tile_costs(), pt.frames
        planes = pt.features(cam)["planes"]
        twin.features(cam)
        out = pt.temporal(variance=True, min_temporal=3, **PARAMS)
        var = pt.temporal_variance()
        filtered = pt.denoise(source="temporal", guide="variance", **VDN)
        assert pt.history_used == (k > 0)
        # the image is pt_temporal's on a twin context
        assert sm.same_words(out, twin.temporal(**PARAMS)), f"frame {k}: not pt_temporal's image"
        # nothing of the render state moved
        assert np.array_equal(dm.bits(pt.accum()), dm.bits(accum)) and np.array_equal(pt.rng_state(), rng)
        assert (pt.last_variant, pt.frames) == (variant, frames) and np.array_equal(pt.tile_costs(), costs)
        hdr, cur = pt.get_hdr_image_data(), tm.camera_of(cam)
        stats = {}
        want = sm.model(hdr, *planes, cur, hist, prev if prev is not None else cur, *MODEL_ARGS, 3, stats=stats)
        print(k, stats)
        assert sm.same_words(out, want[0]), f"frame {k}: " + first_difference(out, want[0])
        assert sm.same_words(var, want[5]), f"frame {k}, variance: " + difference(var, want[5])
        fwant = sm.filter_model(out, *planes, var, *VDN_ARGS)
        assert sm.same_words(filtered, fwant), f"frame {k}, filter: " + first_difference(filtered, fwant)
        assert sm.same_words(pt.denoised(), filtered) and not sm.same_words(filtered[..., :3], out[..., :3])
        hist, prev = want[1:5], cur
        cam = move(copy_camera(cam), k)
    assert stats["spatial"] > 0 and stats["temporal"] > stats["spatial"]
    ms = pt.temporal_moments_timing()
    assert ms["step"] > 0 and ms["estimate"] > 0 and pt.temporal_timing() == ms["step"]
    assert pt.denoise_timing()["iterations"][2] > 0 and pt.denoise_timing()["iterations"][3] == 0
    # the plain filter of the same image is what it was, and the next render continues as on a context that ran no pass
    assert sm.same_words(pt.denoise(source="temporal", **DN), dm.model(out, *planes, 3, 0.4, 0.03, 3, 1))
    pt.render(cam, 4, False)
    bare.render(cam, 4, False)
    assert_bitexact(pt.accum(), bare.accum(), "the render after the passes")
    assert np.array_equal(pt.rng_state(), bare.rng_state()) and pt.frames == bare.frames


def test_context_refusals_name_the_reason(gpu_available, scenes):
    W, H = 40, 36
    scene = str(scenes / "cornell_box.scene.json")
    pt = pa.Pathtracer(W, H)
    cam = pt.load_scene(scene)

    def frame(**kw):
        pt.render(cam, 1, True)
        pt.features(cam)
        pt.temporal(**PARAMS, **kw)
        return pt.history_used

    def refused(code, word, call, *args, **kw):
        with pytest.raises(pa.PathtracerError) as e:
            call(*args, **kw)
        assert e.value.code == code and word in str(e.value), str(e.value)

    # no variance held: nothing yet, and after a plain step
    refused(N.PT_ERR_STATE, "variance", pt.temporal_variance)
    assert not frame()
    refused(N.PT_ERR_STATE, "variance", pt.temporal_variance)
    refused(N.PT_ERR_STATE, "variance", pt.denoise, source="temporal", guide="variance")
    refused(N.PT_ERR_STATE, "variance", pt.temporal_moments_timing)
    # a history without moments: the step acts as reset
    assert not frame(variance=True)
    assert float(pt.history_lengths().max()) == 1.0
    assert frame(variance=True) and float(pt.history_lengths().max()) == 2.0
    pt.temporal_variance()
    pt.denoise(source="temporal", guide="variance")
    # a plain step may reproject the colour history of a moments step, and ends the moments
    assert frame() and float(pt.history_lengths().max()) == 3.0
    refused(N.PT_ERR_STATE, "variance", pt.temporal_variance)
    assert not frame(variance=True)
    assert frame(variance=True)
    # a DEMODULATE bit that differs from the moments'
    refused(N.PT_ERR_ARG, "DEMODULATE", pt.denoise, source="temporal", guide="variance", demodulate=False)
    pt.denoise(source="temporal", guide="variance", demodulate=True, same_primitive=True)
    # features rendered since: the variance is still read, the filter has lost its planes
    pt.features(cam)
    pt.temporal_variance()
    refused(N.PT_ERR_STATE, "pt_render_features", pt.denoise, source="temporal", guide="variance")
    # what ends the history ends the variance: reset, a scene load
    assert not frame(variance=True, reset=True)
    assert frame(variance=True)
    cam = pt.load_scene(scene)
    refused(N.PT_ERR_STATE, "variance", pt.temporal_variance)
    assert not frame(variance=True)
    # the Python layer's own refusals
    refused(N.PT_ERR_ARG, "guide", pt.denoise, guide="variance")
    refused(N.PT_ERR_ARG, "sigma_color", pt.denoise, source="temporal", guide="variance", sigma_color=1.0)
    refused(N.PT_ERR_ARG, "sigma_l", pt.denoise, source="temporal", sigma_l=1.0)
    refused(N.PT_ERR_ARG, "min_temporal", pt.temporal, min_temporal=4)
    refused(N.PT_ERR_ARG, "min_temporal", pt.temporal, variance=True, min_temporal=0)


def test_band_partition_is_refused_by_name(gpu_available, scenes):
    pt = pa.Pathtracer(64, 64, band_rows=8, row_offset=1, row_stride=2)
    cam = pt.load_scene(str(scenes / "cornell_box.scene.json"))
    pt.render(cam, 1, True)
    pt.features(cam)
    with pytest.raises(pa.PathtracerError) as e:
        pt.temporal(variance=True, **PARAMS)
    assert e.value.code == N.PT_ERR_ARG and "whole frame" in str(e.value)


def test_nan_pixels_stay_and_reach_nobody(gpu_available, tmp_path):
    W, H = 64, 48
    pt = pa.Pathtracer(W, H)
    cam = pt.load_scene(str(dsc.directed_scene(tmp_path, "rough_normal_16")))
    hist, prev = None, None
    for k in range(2):
        pt.render(cam, 8, True)
        hdr = pt.get_hdr_image_data()
        nan = np.isnan(hdr[..., :3]).any(-1)
        assert nan.any(), "the scene gives no NaN pixel"
        planes = pt.features(cam)["planes"]
        out = pt.temporal(variance=True, min_temporal=2, **PARAMS)
        var = pt.temporal_variance()
        filtered = pt.denoise(source="temporal", guide="variance", **VDN)
        assert np.all(var[nan] == -1)
        assert np.array_equal(dm.bits(filtered[..., :3])[nan], dm.bits(hdr[..., :3])[nan])
        cur = tm.camera_of(cam)
        want = sm.model(hdr, *planes, cur, hist, prev if prev is not None else cur, *MODEL_ARGS, 2)
        assert sm.same_words(out, want[0]) and sm.same_words(var, want[5]), difference(var, want[5])
        keep = sm.vkeep_mask(out, *planes, var, 1)
        assert keep.any() and np.isfinite(filtered[..., :3][keep]).all() and np.isfinite(var[~nan]).all()
        assert sm.same_words(filtered, sm.filter_model(out, *planes, var, *VDN_ARGS))
        hist, prev = want[1:5], cur
        cam = pa.camera_translate(copy_camera(cam), 4e-4, 1e-4, 0.0)
    assert (out[..., 3] > 1).sum() > keep.sum() // 2


def test_it_filters(gpu_available, scenes):
    """A condition, not a tuned threshold: after eight 1-spp frames on the slow orbit of test_it_accumulates, the
    variance-guided filter with the defaults brings the temporal image closer to a 1024-spp render at the last
    camera (tonemapped MSE over the hit, finite pixels).  The plain a-trous figure for the same frames is
    printed beside it; no other ratio is asserted.  Measured on MI355X: temporal 0.2554, then variance-guided 0.0711
    (ratio 0.278), then a-trous 0.2281 (ratio 0.893)."""
    W = H = 64
    pt, ref = pa.Pathtracer(W, H), pa.Pathtracer(W, H)
    cam = pt.load_scene(str(scenes / "cornell_box.scene.json"))
    ref.load_scene(str(scenes / "cornell_box.scene.json"))
    for k in range(8):
        pt.render(cam, 1, True)
        planes = pt.features(cam)["planes"]
        pt.temporal(variance=True)
        if k < 7:
            cam = copy_camera(cam)
            pa.camera_translate(cam, 0.03, 0.0, 0.0)
            pa.camera_rotate(cam, 0.0, -0.006)
    ref.render(cam, 8, True, chunks=128)
    truth, temporal = ref.get_image_data(), pt.tonemap_temporal()
    pt.denoise(source="temporal", guide="variance")
    guided = pt.tonemap_denoised()
    pt.denoise(source="temporal")
    plain = pt.tonemap_denoised()
    mask = tm.ok_mask(pt.get_hdr_image_data(), planes[1], planes[2]) & np.isfinite(ref.get_hdr_image_data()[..., :3]).all(-1)
    before, after, atrous = (tonemapped_mse(img, truth, mask) for img in (temporal, guided, plain))
    print(f"tonemapped MSE over {int(mask.sum())} hit finite pixels: temporal {before:.6f}, then variance-guided {after:.6f} "
          f"(ratio {after / before:.3f}), then a-trous {atrous:.6f} (ratio {atrous / before:.3f})")
    assert mask.sum() > W * H // 2
    assert after < before


def test_host_layer(gpu_available, scenes):
    """The C++ layer (Pathtracer::temporalMoments / temporalVariance / denoiseVariance through its C ABI) end to
    end: the model's words, and a denoiseVariance result is a denoised image."""
    W, H = 64, 40
    pt = pa.Pathtracer(W, H)
    cam = pt.load_scene(str(scenes / "test_shapes.scene.json"))
    host = N.host()
    params, vparams, dn = pa.temporal_params(**PARAMS), pa.variance_params(2), pa.vdenoise_params(**VDN)
    used = N.C.c_int(7)
    assert host.pth_renderer_temporal_moments(pt._r, N.C.byref(params), N.C.byref(vparams), 0, N.C.byref(used)) == N.PT_ERR_STATE
    assert not host.pth_renderer_temporal_variance(pt._r)
    assert host.pth_renderer_denoise_variance(pt._r, N.C.byref(dn)) == N.PT_ERR_STATE
    hist, prev = None, None
    for k in range(3):
        pt.render(cam, 2, True)
        N.check_host(host.pth_renderer_features(pt._r, N.C.byref(cam)))
        hdr, ldr = pt.get_hdr_image_data(), pt.get_image_data()
        planes = [np.ctypeslib.as_array(host.pth_renderer_feature_plane(pt._r, j), shape=(H, W, 4)).copy() for j in range(3)]
        N.check_host(host.pth_renderer_temporal_moments(pt._r, N.C.byref(params), N.C.byref(vparams), 0, N.C.byref(used)))
        assert used.value == (k > 0)
        got = np.ctypeslib.as_array(host.pth_renderer_temporal_hdr(pt._r), shape=(H, W, 4)).copy()
        var = np.ctypeslib.as_array(host.pth_renderer_temporal_variance(pt._r), shape=(H, W)).copy()
        cur = tm.camera_of(cam)
        want = sm.model(hdr, *planes, cur, hist, prev if prev is not None else cur, *MODEL_ARGS, 2)
        assert sm.same_words(got, want[0]), first_difference(got, want[0])
        assert sm.same_words(var, want[5]), difference(var, want[5])
        # the image calls return what they did, until the filter has run: then they return its result
        assert sm.same_words(pt.get_hdr_image_data(), hdr) and np.array_equal(pt.get_image_data(), ldr)
        assert host.pth_renderer_denoised(pt._r) == 0
        N.check_host(host.pth_renderer_denoise_variance(pt._r, N.C.byref(dn)))
        assert host.pth_renderer_denoised(pt._r) == 1
        fwant = sm.filter_model(got, *planes, var, *VDN_ARGS)
        assert sm.same_words(pt.get_hdr_image_data(), fwant), first_difference(pt.get_hdr_image_data(), fwant)
        assert np.array_equal(pt.get_image_data(), pt.tonemap_denoised())
        hist, prev = want[1:5], cur
        cam = move(copy_camera(cam), k)
    assert (got[..., 3] > 1).any() and (var > 0).any()
    # a plain step takes the moments away; the next moments step starts anew
    N.check_host(host.pth_renderer_temporal(pt._r, N.C.byref(params), 0, N.C.byref(used)))
    assert used.value == 1 and not host.pth_renderer_temporal_variance(pt._r)
    N.check_host(host.pth_renderer_temporal_moments(pt._r, N.C.byref(params), N.C.byref(vparams), 0, N.C.byref(used)))
    assert used.value == 0
    vparams.min_temporal = 0
    assert host.pth_renderer_temporal_moments(pt._r, N.C.byref(params), N.C.byref(vparams), 0, None) == N.PT_ERR_ARG
    dn.sigma_l = 0.0
    assert host.pth_renderer_denoise_variance(pt._r, N.C.byref(dn)) == N.PT_ERR_ARG
