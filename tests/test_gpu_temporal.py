"""Temporal reprojection on the GPU against its numpy restatement (tests/temporal_model.py): words equal, or
both NaN, no tolerance -- through pt_temporal_image on the seeded sequence, through pt_temporal on rendered
frames under a moving camera -- then what the pass must leave alone (the render state), what ends a history,
and that it accumulates.
"""
import numpy as np
import pytest

import denoise_model as dm
import domain_scenes as dsc
import pathtracercuda_amd as pa
import temporal_model as tm
from oracle import pyoracle as po
from pathtracercuda_amd import _native as N
from test_gpu_parity import assert_bitexact

pytestmark = pytest.mark.gpu

F = tm.F
TW, TH = dm.TILE_W, dm.TILE_H
# degenerate images; the workgroup tile, one less and one more in both dimensions; several tiles
SIZES = [(1, 1), (1, 7), (5, 1), (TW, TH), (TW - 1, TH - 1), (TW + 1, TH + 1), (tm.WIDTH, tm.HEIGHT)]
NAMES = ("image", "h0", "h1", "h2")


@pytest.fixture(scope="module")
def gpu_available():
    if pa.device_count() < 1:
        pytest.skip("no GPU")


def pt_camera(cam):
    """A pt_camera from temporal_model's camera (the fields the rule reads)."""
    c = pa.PtCamera()
    c.tan_half_fovy, c.aspect_ratio = float(cam["tan_half_fovy"]), float(cam["aspect_ratio"])
    for name in ("origin", "right", "up", "backward"):
        for k in range(3):
            getattr(c, name)[k] = float(cam[name][k])
    return c


def copy_camera(cam):
    return pa.PtCamera.from_buffer_copy(cam)


def device_step(color, p0, p1, p2, cur, hist, prev, alpha_min, max_history, sigma_plane, normal_cos_min, flags):
    """pt_temporal_image with temporal_model.model's signature."""
    return pa.temporal_image(color, p0, p1, p2, pt_camera(cur), hist, pt_camera(prev) if hist is not None else None,
                             alpha_min=alpha_min, max_history=max_history, sigma_plane=sigma_plane,
                             normal_cos_min=normal_cos_min, demodulate=bool(flags & 1), same_primitive=bool(flags & 2))


def first_difference(got, want, inputs=None):
    bad = np.argwhere(~((dm.bits(got) == dm.bits(want)) | (np.isnan(got) & np.isnan(want))))
    y, x, k = bad[0]
    text = f"{len(bad)} words differ; first at row {y}, x {x}, channel {k}: {got[y, x, k]!r} != {want[y, x, k]!r}"
    if inputs is not None:
        text += "".join(f"\n  {name}[{y}, {x}] = {a[y, x]!r}" for name, a in inputs)
    return text


def assert_step(got, want, what, frame=None):
    inputs = list(zip(("color", "plane0", "plane1", "plane2"), frame)) if frame is not None else None
    for name, g, w in zip(NAMES, got, want):
        assert dm.same_words(g, w), f"{what}, {name}: " + first_difference(g, w, inputs)


@pytest.mark.parametrize("width,height", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_three_chained_frames_equal_the_model(gpu_available, width, height):
    seq = tm.make_sequence(width, height, seed=1000 * width + height)
    for flags in ((0, 1, 2, 3) if (width, height) == (tm.WIDTH, tm.HEIGHT) else (3,)):
        stats = []
        want = tm.run_sequence(tm.model, seq, flags, stats=stats)
        got = tm.run_sequence(device_step, seq, flags)
        print(f"{width}x{height}, flags {flags}:", [(s["hits"], s["have"]) for s in stats])
        for k in range(3):
            assert_step(got[k], want[k], f"flags {flags}, frame {k}", seq[k][1])
        if width * height >= TW * TH:                 # history was used, and not everywhere
            assert all(0 < s["have"] < s["hits"] for s in stats[1:])


def test_a_previous_camera_behind_the_scene_and_an_infinite_history(gpu_available):
    (c0, f0), (c1, f1) = tm.make_sequence()[:2]
    first = tm.model(*f0, c0, None, c0, flags=3, **tm.PARAMS)
    behind = tm.camera_behind()
    want = tm.model(*f1, c1, first[1:], behind, flags=3, **tm.PARAMS)
    assert want[0][..., 3].max() == 1
    assert_step(device_step(*f1, c1, first[1:], behind, flags=3, **tm.PARAMS), want, "z1 <= 0", f1)
    bad = first[1].copy()
    sel = (bad[..., 3] >= 1) & (np.arange(bad.shape[1])[None, :] % 3 == 0)
    bad[..., 1][sel] = F(np.inf)
    bad[..., 2][sel & (np.arange(bad.shape[0])[:, None] % 2 == 0)] = F(np.nan)
    hist = (bad, first[2], first[3])
    stats = {}
    want = tm.model(*f1, c1, hist, c0, flags=1, stats=stats, **tm.PARAMS)
    assert stats["not_finite"] >= 16
    assert_step(device_step(*f1, c1, hist, c0, flags=1, **tm.PARAMS), want, "infinite history", f1)


def test_device_refusals_name_the_field(gpu_available):
    img = np.zeros((4, 4, 4), dtype=np.float32)
    fp = N.C.POINTER(N.C.c_float)
    ptr, cam, nan = img.ctypes.data_as(fp), N.C.byref(pa.PtCamera()), float("nan")
    T = N.PtTemporalParams
    for params, field in ((T(-0.5, 8, 0.1, 0.5, 1), "alpha_min"), (T(1.5, 8, 0.1, 0.5, 1), "alpha_min"), (T(nan, 8, 0.1, 0.5, 1), "alpha_min"),
                          (T(0.1, 0, 0.1, 0.5, 1), "max_history"), (T(0.1, 65536, 0.1, 0.5, 1), "max_history"),
                          (T(0.1, 8, 1e-7, 0.5, 1), "sigma_plane"), (T(0.1, 8, float("inf"), 0.5, 1), "sigma_plane"),
                          (T(0.1, 8, nan, 0.5, 1), "sigma_plane"), (T(0.1, 8, 0.1, -1.5, 1), "normal_cos_min"),
                          (T(0.1, 8, 0.1, 1.5, 1), "normal_cos_min"), (T(0.1, 8, 0.1, nan, 1), "normal_cos_min"),
                          (T(0.1, 8, 0.1, 0.5, 4), "flags")):
        rc = N.hip().pt_temporal_image(0, 4, 4, ptr, ptr, ptr, ptr, cam, None, None, None, None, N.C.byref(params),
                                       ptr, ptr, ptr, ptr)
        assert rc == N.PT_ERR_ARG and field in N.hip().pt_last_error(None).decode(), (field, rc)
    good = T(0.1, 8, 0.1, 0.5, 1)
    rc = N.hip().pt_temporal_image(0, 4, 4, ptr, ptr, ptr, ptr, cam, ptr, None, None, None, N.C.byref(good), ptr, ptr, ptr, ptr)
    assert rc == N.PT_ERR_ARG and "hist0" in N.hip().pt_last_error(None).decode()
    pt = pa.Pathtracer(16, 16)
    bad = T(0.1, 0, 0.1, 0.5, 1)
    assert N.hip().pt_temporal(pt._ctx, 1, N.C.byref(bad), 0, None) == N.PT_ERR_ARG
    assert "max_history" in N.hip().pt_last_error(pt._ctx).decode()
    assert N.hip().pt_temporal(pt._ctx, 1, N.C.byref(good), 0, None) == N.PT_ERR_STATE
    assert "feature" in N.hip().pt_last_error(pt._ctx).decode()
    assert N.hip().pt_read_temporal(pt._ctx, ptr) == N.PT_ERR_STATE
    ms = N.C.c_float(0.0)
    assert N.hip().pt_read_temporal_timing(pt._ctx, N.C.byref(ms)) == N.PT_ERR_STATE
    dn = N.PtDenoiseParams(3, 1.0, 0.1, 1, 1, 0)
    assert N.hip().pt_denoise_temporal(pt._ctx, N.C.byref(dn)) == N.PT_ERR_STATE
    assert "temporal" in N.hip().pt_last_error(pt._ctx).decode()


PARAMS = dict(alpha_min=0.1, max_history=16, sigma_plane=0.05, normal_cos_min=0.9, demodulate=True, same_primitive=False)
MODEL_ARGS = (0.1, 16, 0.05, 0.9, 1)
DN = dict(iterations=3, sigma_color=0.4, sigma_plane=0.03, normal_power_log2=3, demodulate=True, same_primitive=False)
DN_ARGS = (3, 0.4, 0.03, 3, 1)


def move(cam, k):
    """The k-th step of a walk to the right with a turn to the left, so the view stays on the scene."""
    pa.camera_translate(cam, 0.06 + 0.01 * k, 0.01, -0.02)
    pa.camera_rotate(cam, 0.002, -0.012)
    return cam


def test_a_moving_camera_equals_the_model_and_the_render_state_is_left_alone(gpu_available, scenes):
    W, H = 72, 52
    scene = str(scenes / "cornell_box.scene.json")
    pt = pa.Pathtracer(W, H)
    cam = pt.load_scene(scene)
    hist, prev = None, None
    for k in range(4):
        pt.render(cam, 1, True)
        accum, rng = pt.accum(), pt.rng_state()
        variant, costs, frames = pt.last_variant, pt.tile_costs(), pt.frames
        planes = pt.features(cam)["planes"]
        out = pt.temporal(**PARAMS)
        assert pt.history_used == (k > 0)
        assert np.array_equal(dm.bits(pt.accum()), dm.bits(accum)) and np.array_equal(pt.rng_state(), rng)
        assert (pt.last_variant, pt.frames) == (variant, frames) and np.array_equal(pt.tile_costs(), costs)
        hdr, cur = pt.get_hdr_image_data(), tm.camera_of(cam)
        stats = {}
        want = tm.model(hdr, *planes, cur, hist, prev if prev is not None else cur, *MODEL_ARGS, stats=stats)
        print(k, stats)
        assert dm.same_words(out, want[0]), f"frame {k}: " + first_difference(out, want[0], [("hdr", hdr), ("plane2", planes[2])])
        assert dm.same_words(pt.temporal_image(), out) and np.array_equal(pt.history_lengths(), out[..., 3])
        if k > 0:
            n = pt.history_lengths()
            ok = tm.ok_mask(hdr, planes[1], planes[2])
            assert (n[ok] == 1).any() and (n > 1).sum() > ok.sum() // 2 and stats["taps4"] > 0 and stats["taps13"] > 0
        hist, prev = want[1:], cur
        cam = move(copy_camera(cam), k)
    assert pt.temporal_timing() > 0
    # the tonemap is the denoised image's; the filter takes the temporal image and the planes it was made from
    ldr = np.zeros((H, W, 4), dtype=np.uint8)
    po.lib().or_tonemap(po.fptr(np.ascontiguousarray(out)), W * H, 1, ldr.ctypes.data_as(N.C.POINTER(N.C.c_uint8)))
    assert np.array_equal(pt.tonemap_temporal(), ldr)
    before = pt.denoise(**DN)
    want = dm.model(hdr, *planes, *DN_ARGS)
    assert dm.same_words(before, want), "denoise(): " + first_difference(before, want)
    got = pt.denoise(source="temporal", **DN)
    want = dm.model(out, *planes, *DN_ARGS)
    assert dm.same_words(got, want), "denoise(source='temporal'): " + first_difference(got, want)
    assert dm.same_words(pt.denoised(), got) and not dm.same_words(got, before)
    d = pa.DENOISE_DEFAULTS
    sigma = pa.auto_sigma_color(out, *planes, demodulate=d["demodulate"])
    want = dm.model(out, *planes, d["iterations"], sigma, d["sigma_plane"], d["normal_power_log2"], 1)
    assert dm.same_words(pt.denoise(source="temporal"), want)
    assert dm.same_words(pt.denoise(**DN), before)            # the default is what it was


def test_the_next_render_is_that_of_a_context_that_ran_no_pass(gpu_available, scenes):
    W, H = 72, 52
    scene = str(scenes / "cornell_box.scene.json")
    pt, other = pa.Pathtracer(W, H), pa.Pathtracer(W, H)
    cam = pt.load_scene(scene)
    other.load_scene(scene)
    for k in range(2):
        pt.render(cam, 1, True)
        other.render(cam, 1, True)
        pt.features(cam)
        pt.temporal(**PARAMS)
        pt.denoise(source="temporal", **DN)
        if k == 0:
            cam = move(copy_camera(cam), k)
    pt.render(cam, 4, False)
    other.render(cam, 4, False)
    assert_bitexact(pt.accum(), other.accum(), "the render after the passes")
    assert np.array_equal(pt.rng_state(), other.rng_state()) and pt.frames == other.frames
    # a features call after the temporal pass takes its planes away from under the image
    pt.features(cam)
    with pytest.raises(pa.PathtracerError) as e:
        pt.denoise(source="temporal", **DN)
    assert e.value.code == N.PT_ERR_STATE and "pt_render_features" in str(e.value)
    pt.temporal(**PARAMS)
    pt.denoise(source="temporal", **DN)


def test_a_camera_that_stands_still_gives_the_running_mean(gpu_available, scenes):
    W, H = 40, 36
    pt = pa.Pathtracer(W, H)
    cam = pt.load_scene(str(scenes / "cornell_box.scene.json"))
    planes = pt.features(cam)["planes"]
    mean = None
    for k in range(1, 5):
        pt.render(cam, 1, True)
        c = pt.get_hdr_image_data()[..., :3]
        out = pt.temporal(alpha_min=0.0, max_history=1000, sigma_plane=0.05, normal_cos_min=0.9, demodulate=False,
                          same_primitive=False)
        with np.errstate(all="ignore"):
            mean = c.copy() if mean is None else (mean + F(1.0 / k) * (c - mean)).astype(F)
        ok = tm.ok_mask(pt.get_hdr_image_data(), planes[1], planes[2])
        assert dm.same_words(out[..., :3][ok], mean[ok]), k
        assert np.all(out[..., 3][ok] == k) and np.all(out[..., 3][~ok] == 0)
    assert ok.sum() > W * H // 2


def test_what_ends_a_history_and_what_does_not(gpu_available, scenes):
    W, H = 40, 36
    scene = str(scenes / "cornell_box.scene.json")
    pt = pa.Pathtracer(W, H)
    cam = pt.load_scene(scene)
    fp = N.C.POINTER(N.C.c_float)
    tex = np.ones((4, 4, 4), dtype=np.float32)

    def frame(**kw):
        pt.render(cam, 1, True)
        pt.features(cam)
        pt.temporal(**PARAMS, **kw)
        return pt.history_used, float(pt.history_lengths().max())

    assert frame() == (False, 1.0)
    assert frame() == (True, 2.0)
    # a camera change, a render and an RNG write end nothing
    cam = move(copy_camera(cam), 0)
    pt.render(cam, 2, False)
    pt.set_rng_state(pt.rng_state())
    used, longest = frame()
    assert used and longest == 3.0
    # reset, a scene load, a texture and a sky change to another handle each do
    assert frame(reset=True) == (False, 1.0)
    assert frame()[0]
    cam = pt.load_scene(scene)
    assert frame() == (False, 1.0)
    assert frame()[0]
    N.check_ctx(N.hip().pt_set_texture(pt._ctx, 1, tex.ctypes.data_as(fp), 4, 4), pt._ctx)
    assert frame() == (False, 1.0)
    assert frame()[0]
    N.check_ctx(N.hip().pt_set_skybox(pt._ctx, 1), pt._ctx)
    assert frame() == (False, 1.0)
    N.check_ctx(N.hip().pt_set_skybox(pt._ctx, 1), pt._ctx)          # the sky that is set, set again
    assert frame() == (True, 2.0)
    # without planes
    pt.load_scene(scene)
    with pytest.raises(pa.PathtracerError) as e:
        pt.temporal(**PARAMS)
    assert e.value.code == N.PT_ERR_STATE and "feature" in str(e.value)


def test_band_partition_is_refused_by_name(gpu_available, scenes):
    pt = pa.Pathtracer(64, 64, band_rows=8, row_offset=1, row_stride=2)
    cam = pt.load_scene(str(scenes / "cornell_box.scene.json"))
    pt.render(cam, 1, True)
    pt.features(cam)
    with pytest.raises(pa.PathtracerError) as e:
        pt.temporal(**PARAMS)
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
        out = pt.temporal(**PARAMS)
        assert np.array_equal(dm.bits(out[..., :3])[nan], dm.bits(hdr[..., :3])[nan]) and np.all(out[..., 3][nan] == 0)
        ok = tm.ok_mask(hdr, planes[1], planes[2])
        assert ok.any() and np.isfinite(out[..., :3][ok]).all()
        cur = tm.camera_of(cam)
        stats = {}
        want = tm.model(hdr, *planes, cur, hist, prev if prev is not None else cur, *MODEL_ARGS, stats=stats)
        assert dm.same_words(out, want[0]), first_difference(out, want[0])
        hist, prev = want[1:], cur
        cam = pa.camera_translate(copy_camera(cam), 4e-4, 1e-4, 0.0)      # a pixel and a half: the view is 0.2 degrees wide
    # the second frame's taps met the first frame's NaN pixels (n = 0) and skipped them
    assert stats["no_history"] > 0 and (out[..., 3] > 1).sum() > ok.sum() // 2


def tonemapped_mse(img, ref, mask):
    a, r = img[..., :3][mask].astype(np.float64) / 255.0, ref[..., :3][mask].astype(np.float64) / 255.0
    return float(np.mean((a - r) ** 2))


def test_it_accumulates(gpu_available, scenes):
    """A condition, not a tuned threshold: after eight 1-spp frames on a slow orbit the temporal image is closer
    to a 1024-spp render at the last camera than the last frame alone (tonemapped MSE over the hit, finite
    pixels).  Measured on MI355X: 0.4043 -> 0.2554, ratio 0.632, mean history length 7.9."""
    W = H = 64
    pt, ref = pa.Pathtracer(W, H), pa.Pathtracer(W, H)
    cam = pt.load_scene(str(scenes / "cornell_box.scene.json"))
    ref.load_scene(str(scenes / "cornell_box.scene.json"))
    for k in range(8):
        pt.render(cam, 1, True)
        planes = pt.features(cam)["planes"]
        out = pt.temporal()
        if k < 7:
            cam = copy_camera(cam)
            pa.camera_translate(cam, 0.03, 0.0, 0.0)
            pa.camera_rotate(cam, 0.0, -0.006)
    ref.render(cam, 8, True, chunks=128)
    truth, raw, temporal = ref.get_image_data(), pt.get_image_data(), pt.tonemap_temporal()
    mask = tm.ok_mask(pt.get_hdr_image_data(), planes[1], planes[2]) & np.isfinite(ref.get_hdr_image_data()[..., :3]).all(-1)
    before, after = tonemapped_mse(raw, truth, mask), tonemapped_mse(temporal, truth, mask)
    print(f"tonemapped MSE over {int(mask.sum())} hit finite pixels: raw {before:.6f}, temporal {after:.6f}, "
          f"ratio {after / before:.3f}; mean history length {out[..., 3][mask].mean():.2f}")
    assert mask.sum() > W * H // 2
    assert after / before < 1


def test_host_layer(gpu_available, scenes):
    W, H = 64, 40
    pt = pa.Pathtracer(W, H)
    cam = pt.load_scene(str(scenes / "test_shapes.scene.json"))
    host = N.host()
    params = pa.temporal_params(**PARAMS)
    used = N.C.c_int(7)
    assert host.pth_renderer_temporal(pt._r, N.C.byref(params), 0, N.C.byref(used)) == N.PT_ERR_STATE     # no planes
    assert not host.pth_renderer_temporal_hdr(pt._r)
    hist, prev = None, None
    for k in range(2):
        pt.render(cam, 2, True)
        N.check_host(host.pth_renderer_features(pt._r, N.C.byref(cam)))
        hdr = pt.get_hdr_image_data()
        ldr = pt.get_image_data()
        planes = [np.ctypeslib.as_array(host.pth_renderer_feature_plane(pt._r, j), shape=(H, W, 4)).copy() for j in range(3)]
        N.check_host(host.pth_renderer_temporal(pt._r, N.C.byref(params), 0, N.C.byref(used)))
        assert used.value == k
        got = np.ctypeslib.as_array(host.pth_renderer_temporal_hdr(pt._r), shape=(H, W, 4)).copy()
        cur = tm.camera_of(cam)
        want = tm.model(hdr, *planes, cur, hist, prev if prev is not None else cur, *MODEL_ARGS)
        assert dm.same_words(got, want[0]), first_difference(got, want[0])
        # the image calls return what they did
        assert dm.same_words(pt.get_hdr_image_data(), hdr) and np.array_equal(pt.get_image_data(), ldr)
        assert host.pth_renderer_denoised(pt._r) == 0
        hist, prev = want[1:], cur
        cam = move(copy_camera(cam), k)
    assert (got[..., 3] > 1).any()
    N.check_host(host.pth_renderer_temporal(pt._r, N.C.byref(params), 1, N.C.byref(used)))
    assert used.value == 0
    params.max_history = 0
    assert host.pth_renderer_temporal(pt._r, N.C.byref(params), 0, None) == N.PT_ERR_ARG
