"""The feedback of the filtered colour into the temporal history on the GPU against its numpy restatement
(tests/feedback_model.py): words equal, or both NaN, no tolerance -- through the _image entry point on the seeded
inputs at the tile's edges, at both ping/pong parities and every staging; through the context on rendered frames
under a moving camera beside a twin without feedback -- then what the call must leave alone, what it refuses, and
that the fed chain's filter still filters.
"""
import numpy as np
import pytest

import denoise_model as dm
import feedback_model as fm
import pathtracercuda_amd as pa
import svgf_model as sm
import temporal_model as tm
from pathtracercuda_amd import _native as N
from test_gpu_temporal import copy_camera, first_difference, move, tonemapped_mse

pytestmark = pytest.mark.gpu

F = sm.F
TW, TH = dm.TILE_W, dm.TILE_H
SIZES = [(1, 1), (1, 7), (5, 1), (TW, TH), (TW - 1, TH - 1), (TW + 1, TH + 1), (tm.WIDTH, tm.HEIGHT)]
LEVELS = [(it, L) for it in (1, 2, 3, 6) for L in range(1, it + 1)]        # both parities, first and last level


@pytest.fixture(scope="module")
def gpu_available():
    if pa.device_count() < 1:
        pytest.skip("no GPU")


def seeded_history(width, height, seed):
    """An h0 as a moments step leaves it: finite colours, n = 0 on some pixels and 1..6 on the others."""
    rng = np.random.default_rng([seed, 3])
    h0 = rng.random((height, width, 4), dtype=F)
    h0[..., 3] = rng.integers(0, 7, (height, width)).astype(F)
    return h0


def device_feedback(color, p0, p1, p2, var, hist0, level, iterations, flags, staging=0, **kw):
    p = dict(sm.VPARAMS, **kw)
    return pa.denoise_variance_feedback_image(color, p0, p1, p2, var, hist0, level=level, iterations=iterations,
                                              sigma_l=p["sigma_l"], variance_floor=p["variance_floor"],
                                              sigma_plane=p["sigma_plane"], normal_power_log2=p["normal_power_log2"],
                                              demodulate=bool(flags & 1), same_primitive=bool(flags & 2), staging=staging)


def device_filter(color, p0, p1, p2, var, iterations, flags, staging=0, **kw):
    p = dict(sm.VPARAMS, **kw)
    return pa.denoise_variance_image(color, p0, p1, p2, var, iterations=iterations, sigma_l=p["sigma_l"],
                                     variance_floor=p["variance_floor"], sigma_plane=p["sigma_plane"],
                                     normal_power_log2=p["normal_power_log2"], demodulate=bool(flags & 1),
                                     same_primitive=bool(flags & 2), staging=staging)


def check_against_model(inputs, hist0, flags, levels=LEVELS, **kw):
    """Every (iterations, level) and every staging: out and the fed h0 are the model's, out is
    pt_denoise_variance_image's.  Returns the largest count of fed pixels whose words changed."""
    color, p0, p1, p2, var = inputs
    p = dict(sm.VPARAMS, **kw)
    most = 0
    plain = {}
    for iterations, level in levels:
        stats = {}
        want_out, want_h0 = fm.filter_feedback_model(color, p0, p1, p2, var, hist0, level, iterations, flags=flags, stats=stats, **p)
        most = max(most, stats["changed"])
        for staging in (0, 1, 2):
            what = f"flags {flags}, iterations {iterations}, level {level}, staging {staging}"
            out, h0 = device_feedback(color, p0, p1, p2, var, hist0, level, iterations, flags, staging, **kw)
            assert sm.same_words(h0, want_h0), f"{what}, h0: " + first_difference(h0, want_h0)
            assert sm.same_words(out, want_out), f"{what}, out: " + first_difference(out, want_out)
            if (iterations, staging) not in plain:
                plain[iterations, staging] = device_filter(color, p0, p1, p2, var, iterations, flags, staging, **kw)
            assert sm.same_words(out, plain[iterations, staging]), f"{what}: out is not pt_denoise_variance_image's"
    return most


# ---- the _image form ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height", SIZES[:-1], ids=[f"{w}x{h}" for w, h in SIZES[:-1]])
def test_feedback_equals_the_model_at_the_tile_edges(gpu_available, width, height):
    inputs = sm.make_filter_inputs(width, height, 7 * width + height)[:5]
    hist0 = seeded_history(width, height, width + height)
    for flags in (3, 0):
        changed = check_against_model(inputs, hist0, flags)
        assert changed > 0 or width * height < 8


@pytest.mark.parametrize("flags", (0, 1, 2, 3))
def test_feedback_equals_the_model_under_every_flag(gpu_available, flags):
    inputs = sm.make_filter_inputs(tm.WIDTH, tm.HEIGHT, 21)
    assert set(np.unique(inputs[5])) == set(range(len(sm.CLASSES)))     # 0, tiny, 1e30, +inf, NaN, negative variances
    assert np.isnan(inputs[2][..., :3]).any() and (inputs[0][..., :3] == F(3e38)).any()    # a NaN normal, colours of 3e38
    hist0 = seeded_history(tm.WIDTH, tm.HEIGHT, 9)
    changed = check_against_model(inputs[:5], hist0, flags)
    print(f"flags {flags}: up to {changed} fed pixels changed")
    assert changed > tm.WIDTH * tm.HEIGHT // 2


def test_feedback_equals_the_model_over_many_tiles_and_other_parameters(gpu_available):
    inputs = sm.make_filter_inputs(70, 45, 5)[:5]
    hist0 = seeded_history(70, 45, 2)
    for flags, kw in ((1, {}), (3, dict(sigma_l=0.25, variance_floor=1e-8, normal_power_log2=0)),
                      (0, dict(sigma_l=2.0 ** 20, variance_floor=1e-4, sigma_plane=1e-6, normal_power_log2=7))):
        assert check_against_model(inputs, hist0, flags, levels=[(6, 1), (6, 4), (6, 6), (3, 2)], **kw) > 1000


def test_a_filtered_colour_that_is_not_finite_is_not_fed_back(gpu_available):
    """feedback_model.make_overflow_inputs: kept pixels with a colour of 3e38 and a normal of length 1.5, whose
    filtered colour is +inf or NaN (checked in the model first).  They keep their history."""
    color, p0, p1, p2, var, cls, big = fm.make_overflow_inputs(tm.WIDTH, tm.HEIGHT, 21)
    hist0 = seeded_history(tm.WIDTH, tm.HEIGHT, 4)
    for level, iterations in ((1, 2), (2, 2), (3, 3)):
        stats = {}
        want_out, want_h0 = fm.filter_feedback_model(color, p0, p1, p2, var, hist0, level, iterations, flags=0, stats=stats,
                                                     **sm.VPARAMS)
        print(f"level {level} of {iterations}: {stats}")
        assert stats["kept_not_finite"] >= 1
        for staging in (0, 1, 2):
            out, h0 = device_feedback(color, p0, p1, p2, var, hist0, level, iterations, 0, staging)
            assert sm.same_words(h0, want_h0), f"level {level}, staging {staging}: " + first_difference(h0, want_h0)
            assert sm.same_words(out, want_out) and np.isfinite(h0[..., :3]).all()
            assert np.array_equal(dm.bits(h0[..., 3]), dm.bits(hist0[..., 3]))


def test_device_refusals_name_the_field(gpu_available):
    img = np.zeros((4, 4, 4), dtype=np.float32)
    fp = N.C.POINTER(N.C.c_float)
    ptr = img.ctypes.data_as(fp)
    lib = N.hip()
    V, B = N.PtVDenoiseParams, N.PtVFeedbackParams
    good = V(3, 1.0, 1e-6, 0.1, 1, 1, 0)

    def call(params, fb, hist0=ptr, out_hist0=ptr):
        return lib.pt_denoise_variance_feedback_image(0, 4, 4, ptr, ptr, ptr, ptr, ptr, hist0, params, fb, ptr, out_hist0)

    for level in (0, 4, 0xffffffff):
        assert call(N.C.byref(good), N.C.byref(B(level))) == N.PT_ERR_ARG and "level" in lib.pt_last_error(None).decode()
    assert call(N.C.byref(good), None) == N.PT_ERR_ARG and "feedback" in lib.pt_last_error(None).decode()
    assert call(None, N.C.byref(B(1))) == N.PT_ERR_ARG and "params" in lib.pt_last_error(None).decode()
    assert call(N.C.byref(V(3, 0.0, 1e-6, 0.1, 1, 1, 0)), N.C.byref(B(1))) == N.PT_ERR_ARG
    assert "sigma_l" in lib.pt_last_error(None).decode()
    assert call(N.C.byref(good), N.C.byref(B(1)), hist0=None) == N.PT_ERR_ARG and "hist0" in lib.pt_last_error(None).decode()
    assert call(N.C.byref(good), N.C.byref(B(1)), out_hist0=None) == N.PT_ERR_ARG
    assert "out_hist0" in lib.pt_last_error(None).decode()
    for level in (1, 3):
        assert call(N.C.byref(good), N.C.byref(B(level))) == N.PT_OK
    # a context with nothing on it
    pt = pa.Pathtracer(16, 16)
    assert lib.pt_denoise_variance_feedback(pt._ctx, N.C.byref(good), N.C.byref(B(0))) == N.PT_ERR_ARG
    assert "level" in lib.pt_last_error(pt._ctx).decode()
    assert lib.pt_denoise_variance_feedback(pt._ctx, N.C.byref(good), N.C.byref(B(4))) == N.PT_ERR_ARG
    assert "level" in lib.pt_last_error(pt._ctx).decode()
    assert lib.pt_denoise_variance_feedback(pt._ctx, N.C.byref(good), None) == N.PT_ERR_ARG
    assert "feedback" in lib.pt_last_error(pt._ctx).decode()
    assert lib.pt_denoise_variance_feedback(pt._ctx, N.C.byref(good), N.C.byref(B(1))) == N.PT_ERR_STATE
    assert "variance" in lib.pt_last_error(pt._ctx).decode()
    assert lib.pt_read_temporal_history(pt._ctx, 0, ptr) == N.PT_ERR_STATE and "history" in lib.pt_last_error(pt._ctx).decode()
    assert lib.pt_read_feedback_timing(pt._ctx, ptr) == N.PT_ERR_STATE


# ---- on a context ----------------------------------------------------------------------------------------
PARAMS = dict(alpha_min=0.1, max_history=16, sigma_plane=0.05, normal_cos_min=0.9, demodulate=True, same_primitive=False)
MODEL_ARGS = (0.1, 16, 0.05, 0.9, 1)
VDN = dict(iterations=3, sigma_l=2.0, variance_floor=1e-6, sigma_plane=0.03, normal_power_log2=3, demodulate=True,
           same_primitive=False)
VDN_ARGS = (3, 2.0, 1e-6, 0.03, 3, 1)
HNAMES = ("h0", "h1", "h2", "h3")


def assert_history(got, want, what):
    for name, g, w in zip(HNAMES, got, want):
        assert sm.same_words(g, w), f"{what}, {name}: " + first_difference(g, w)


def test_a_moving_camera_equals_the_model_chain_beside_a_twin_without_feedback(gpu_available, scenes):
    W, H = 48, 40
    scene = str(scenes / "cornell_box.scene.json")
    pt, twin = pa.Pathtracer(W, H), pa.Pathtracer(W, H)
    cam = pt.load_scene(scene)
    twin.load_scene(scene)
    hist, prev, thist = None, None, None
    fed_pixels = []
    for k in range(4):
        for p in (pt, twin):
            p.render(cam, 1, True)
        accum, rng = pt.accum(), pt.rng_state()
        variant, costs, frames = pt.last_variant, pt.tile_costs(), pt.frames
        planes = pt.features(cam)["planes"]
        twin.features(cam)
        image = pt.temporal(variance=True, min_temporal=3, **PARAMS)
        timage = twin.temporal(variance=True, min_temporal=3, **PARAMS)
        var, tvar = pt.temporal_variance(), twin.temporal_variance()
        unfed = pt.temporal_history()
        filtered = pt.denoise(source="temporal", guide="variance", feedback=1, **VDN)
        tfiltered = twin.denoise(source="temporal", guide="variance", **VDN)
        assert pt.history_used == (k > 0) and pt.feedback_timing() > 0
        # nothing of the render state moved
        assert np.array_equal(dm.bits(pt.accum()), dm.bits(accum)) and np.array_equal(pt.rng_state(), rng)
        assert (pt.last_variant, pt.frames) == (variant, frames) and np.array_equal(pt.tile_costs(), costs)
        hdr, cur = pt.get_hdr_image_data(), tm.camera_of(cam)
        pcam = prev if prev is not None else cur
        want = sm.model(hdr, *planes, cur, hist, pcam, *MODEL_ARGS, 3)
        twant = sm.model(hdr, *planes, cur, thist, pcam, *MODEL_ARGS, 3)
        stats = {}
        fwant, h0want = fm.filter_feedback_model(want[0], *planes, want[5], want[1], 1, *VDN_ARGS, stats=stats)
        print(k, stats)
        fed_pixels.append(stats["changed"])
        # the temporal image (of the history the previous frame fed), the variance, the filter's result
        assert sm.same_words(image, want[0]), f"frame {k}, image: " + first_difference(image, want[0])
        assert sm.same_words(var, want[5]), f"frame {k}: the variance is not the model's"
        assert sm.same_words(filtered, fwant), f"frame {k}, filter: " + first_difference(filtered, fwant)
        assert sm.same_words(pt.denoised(), filtered)
        assert_history(unfed, want[1:5], f"frame {k}, before the feedback")
        fed = pt.temporal_history()
        assert_history(fed, (h0want,) + tuple(want[2:5]), f"frame {k}")
        # the twin: today's history and image; it differs from the fed context in plane 0's colours only
        assert sm.same_words(timage, twant[0]) and sm.same_words(tfiltered, sm.filter_model(twant[0], *planes, twant[5], *VDN_ARGS))
        thistory = twin.temporal_history()
        assert_history(thistory, twant[1:5], f"frame {k}, the twin")
        assert np.array_equal(dm.bits(fed[0][..., 3]), dm.bits(thistory[0][..., 3])), f"frame {k}: an n word differs from the twin's"
        assert not sm.same_words(fed[0][..., :3], thistory[0][..., :3])
        if k == 0:
            for j in (1, 2, 3):
                assert sm.same_words(fed[j], thistory[j]), f"frame 0: {HNAMES[j]} differs from the twin's"
            assert sm.same_words(var, tvar) and sm.same_words(image, timage) and sm.same_words(filtered, tfiltered)
        else:
            assert not sm.same_words(image[..., :3], timage[..., :3]), f"frame {k}: the fed history was not reprojected"
        # a second call in the same frame leaves the same words
        again = pt.denoise(source="temporal", guide="variance", feedback=1, **VDN)
        assert sm.same_words(again, filtered)
        assert_history(pt.temporal_history(), fed, f"frame {k}, second call")
        hist, thist, prev = (h0want,) + tuple(want[2:5]), twant[1:5], cur
        cam = move(copy_camera(cam), k)
    assert min(fed_pixels) >= 64
    # a plain pt_temporal step after a fed frame reprojects the fed colours
    pt.render(cam, 1, True)
    planes = pt.features(cam)["planes"]
    image = pt.temporal(**PARAMS)
    assert pt.history_used
    hdr, cur = pt.get_hdr_image_data(), tm.camera_of(cam)
    want = tm.model(hdr, *planes, cur, hist[:3], prev, *MODEL_ARGS)
    assert sm.same_words(image, want[0]), "the plain step: " + first_difference(image, want[0])
    plain_history = pt.temporal_history()
    assert plain_history[3] is None
    assert_history(plain_history[:3], want[1:4], "the plain step")
    untouched = tm.model(hdr, *planes, cur, thist[:3], prev, *MODEL_ARGS)
    assert not sm.same_words(want[0][..., :3], untouched[0][..., :3])


def test_context_refusals_name_the_reason(gpu_available, scenes):
    W, H = 40, 36
    scene = str(scenes / "cornell_box.scene.json")
    pt = pa.Pathtracer(W, H)
    cam = pt.load_scene(scene)
    lib = N.hip()
    buf = np.zeros((H, W, 4), dtype=np.float32)
    ptr = buf.ctypes.data_as(N.C.POINTER(N.C.c_float))

    def frame(**kw):
        pt.render(cam, 1, True)
        pt.features(cam)
        pt.temporal(**PARAMS, **kw)
        return pt.history_used

    def refused(code, word, call, *args, **kw):
        with pytest.raises(pa.PathtracerError) as e:
            call(*args, **kw)
        assert e.value.code == code and word in str(e.value), str(e.value)

    def history_plane(plane):
        N.check_ctx(lib.pt_read_temporal_history(pt._ctx, plane, ptr), pt._ctx)

    fed = dict(source="temporal", guide="variance", feedback=1)
    # before any moments step: nothing yet, and after a plain step
    refused(N.PT_ERR_STATE, "variance", pt.denoise, **fed)
    refused(N.PT_ERR_STATE, "history", pt.temporal_history)
    refused(N.PT_ERR_STATE, "feedback", pt.feedback_timing)
    assert not frame()
    refused(N.PT_ERR_STATE, "variance", pt.denoise, **fed)
    refused(N.PT_ERR_ARG, "plane", history_plane, 3)
    refused(N.PT_ERR_ARG, "plane", history_plane, 4)
    assert pt.temporal_history()[3] is None
    # a moments step: allowed, and the timing is there from the first call on
    assert not frame(variance=True)
    refused(N.PT_ERR_STATE, "feedback", pt.feedback_timing)
    pt.denoise(**fed)
    assert pt.feedback_timing() > 0 and pt.temporal_history()[3] is not None
    refused(N.PT_ERR_ARG, "plane", history_plane, 4)
    # the next moments step holds another history: no feedback call has run on it
    assert frame(variance=True)
    refused(N.PT_ERR_STATE, "feedback", pt.feedback_timing)
    # the level against the iterations, by the device too
    refused(N.PT_ERR_ARG, "level", pt.denoise, iterations=2, **dict(fed, feedback=3))
    V, B = N.PtVDenoiseParams, N.PtVFeedbackParams
    good = V(2, 1.0, 1e-6, 0.1, 1, 1, 0)
    assert lib.pt_denoise_variance_feedback(pt._ctx, N.C.byref(good), N.C.byref(B(3))) == N.PT_ERR_ARG
    assert "level" in lib.pt_last_error(pt._ctx).decode()
    # a DEMODULATE bit that differs from the moments'
    refused(N.PT_ERR_ARG, "DEMODULATE", pt.denoise, demodulate=False, **fed)
    pt.denoise(demodulate=True, same_primitive=True, **fed)
    # a refused call wrote nothing: the history is what the allowed call left
    before = pt.temporal_history()
    refused(N.PT_ERR_ARG, "DEMODULATE", pt.denoise, demodulate=False, **fed)
    for g, w in zip(pt.temporal_history(), before):
        assert sm.same_words(g, w)
    # features rendered since: the filter has lost its planes
    pt.features(cam)
    refused(N.PT_ERR_STATE, "pt_render_features", pt.denoise, **fed)
    pt.temporal_history()
    # a scene change ends the history
    assert frame(variance=True)
    cam = pt.load_scene(scene)
    refused(N.PT_ERR_STATE, "variance", pt.denoise, **fed)
    refused(N.PT_ERR_STATE, "history", pt.temporal_history)
    refused(N.PT_ERR_STATE, "feedback", pt.feedback_timing)
    # the Python layer's own refusals
    refused(N.PT_ERR_ARG, "feedback", pt.denoise, feedback=1)
    refused(N.PT_ERR_ARG, "feedback", pt.denoise, source="temporal", feedback=1)
    refused(N.PT_ERR_ARG, "feedback", pt.denoise, guide="variance", feedback=1)
    refused(N.PT_ERR_ARG, "level", pt.denoise, **dict(fed, feedback=6))
    refused(N.PT_ERR_ARG, "level", pt.denoise, **dict(fed, feedback=-1))


def test_feedback_filters(gpu_available, scenes):
    """A condition, not a tuned threshold: on test_it_filters' orbit (cornell 64 x 64, eight 1-spp frames), with the
    shipped defaults and the filtered colour fed back after every frame (level PT_VFEEDBACK_DEFAULT_LEVEL), the last
    filtered frame is closer to a 1024-spp render at the last camera than the same frame's temporal image
    (tonemapped MSE over the hit, finite pixels).  The chain without feedback is run beside it and printed; nothing
    is asserted between the two.  Measured on MI355X at level 3: the fed chain's temporal image 0.0833, then
    filtered 0.0735 (ratio 0.882); the chain without feedback 0.2554, then 0.0711."""
    W = H = 64
    level = pa.VFEEDBACK_DEFAULTS["level"]
    fed, bare, ref = pa.Pathtracer(W, H), pa.Pathtracer(W, H), pa.Pathtracer(W, H)
    cam = fed.load_scene(str(scenes / "cornell_box.scene.json"))
    for p in (bare, ref):
        p.load_scene(str(scenes / "cornell_box.scene.json"))
    for k in range(8):
        for p, fb in ((fed, level), (bare, 0)):
            p.render(cam, 1, True)
            planes = p.features(cam)["planes"]
            p.temporal(variance=True)
            p.denoise(source="temporal", guide="variance", feedback=fb)
        if k < 7:
            cam = copy_camera(cam)
            pa.camera_translate(cam, 0.03, 0.0, 0.0)
            pa.camera_rotate(cam, 0.0, -0.006)
    ref.render(cam, 8, True, chunks=128)
    truth = ref.get_image_data()
    mask = tm.ok_mask(fed.get_hdr_image_data(), planes[1], planes[2]) & np.isfinite(ref.get_hdr_image_data()[..., :3]).all(-1)
    before, after = tonemapped_mse(fed.tonemap_temporal(), truth, mask), tonemapped_mse(fed.tonemap_denoised(), truth, mask)
    b0, b1 = tonemapped_mse(bare.tonemap_temporal(), truth, mask), tonemapped_mse(bare.tonemap_denoised(), truth, mask)
    print(f"tonemapped MSE over {int(mask.sum())} hit finite pixels, level {level}: fed chain temporal {before:.6f}, then filtered "
          f"{after:.6f} (ratio {after / before:.3f}); chain without feedback temporal {b0:.6f}, then filtered {b1:.6f}")
    assert mask.sum() > W * H // 2
    assert after < before


def test_host_layer(gpu_available, scenes):
    """The C++ layer (Pathtracer::denoiseVariance(options, feedbackLevel) / temporalHistory through its C ABI) end
    to end: the model's words over chained frames."""
    W, H = 64, 40
    pt = pa.Pathtracer(W, H)
    cam = pt.load_scene(str(scenes / "test_shapes.scene.json"))
    host = N.host()
    params, vparams, dn = pa.temporal_params(**PARAMS), pa.variance_params(2), pa.vdenoise_params(**VDN)
    fb = pa.vfeedback_params(2, 3)
    used = N.C.c_int(7)
    assert host.pth_renderer_denoise_variance_feedback(pt._r, N.C.byref(dn), N.C.byref(fb)) == N.PT_ERR_STATE
    assert host.pth_renderer_denoise_variance_feedback(pt._r, N.C.byref(dn), None) == N.PT_ERR_ARG
    assert not host.pth_renderer_temporal_history(pt._r, 0)
    hist, prev = None, None
    for k in range(2):
        pt.render(cam, 2, True)
        N.check_host(host.pth_renderer_features(pt._r, N.C.byref(cam)))
        hdr = pt.get_hdr_image_data()
        planes = [np.ctypeslib.as_array(host.pth_renderer_feature_plane(pt._r, j), shape=(H, W, 4)).copy() for j in range(3)]
        N.check_host(host.pth_renderer_temporal_moments(pt._r, N.C.byref(params), N.C.byref(vparams), 0, N.C.byref(used)))
        assert used.value == (k > 0)
        got = np.ctypeslib.as_array(host.pth_renderer_temporal_hdr(pt._r), shape=(H, W, 4)).copy()
        cur = tm.camera_of(cam)
        want = sm.model(hdr, *planes, cur, hist, prev if prev is not None else cur, *MODEL_ARGS, 2)
        assert sm.same_words(got, want[0]), first_difference(got, want[0])
        assert host.pth_renderer_denoised(pt._r) == 0
        N.check_host(host.pth_renderer_denoise_variance_feedback(pt._r, N.C.byref(dn), N.C.byref(fb)))
        assert host.pth_renderer_denoised(pt._r) == 1
        fwant, h0want = fm.filter_feedback_model(want[0], *planes, want[5], want[1], 2, *VDN_ARGS)
        assert sm.same_words(pt.get_hdr_image_data(), fwant), first_difference(pt.get_hdr_image_data(), fwant)
        hist = (h0want,) + tuple(want[2:5])
        for j in range(4):
            plane = np.ctypeslib.as_array(host.pth_renderer_temporal_history(pt._r, j), shape=(H, W, 4)).copy()
            assert sm.same_words(plane, hist[j]), f"frame {k}, {HNAMES[j]}: " + first_difference(plane, hist[j])
        assert not sm.same_words(h0want, want[1])
        assert not host.pth_renderer_temporal_history(pt._r, 4)
        prev = cur
        cam = move(copy_camera(cam), k)
    fb.level = 4
    assert host.pth_renderer_denoise_variance_feedback(pt._r, N.C.byref(dn), N.C.byref(fb)) == N.PT_ERR_ARG
