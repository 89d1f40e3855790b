"""The a-trous filter on the GPU against its numpy restatement (tests/denoise_model.py): words equal, or
both NaN, no tolerance -- through pt_denoise_image on seeded inputs, through pt_denoise on rendered
frames -- then what the passes must leave alone (the render state), and that the filter denoises.
"""
import numpy as np
import pytest

import denoise_model as dm
import domain_scenes as dsc
import pathtracercuda_amd as pa
from oracle import pyoracle as po
from pathtracercuda_amd import _native as N
from test_gpu_parity import assert_bitexact, pair

pytestmark = pytest.mark.gpu

TW, TH = dm.TILE_W, dm.TILE_H
# (width, height, iteration counts): degenerate images; the workgroup tile, one less and one more in each
# dimension; every iteration count on several tiles; taps past both borders at the largest step (32 > 45 / 2)
SIZES = ([(1, 1, (1, 3)), (1, 7, (3,)), (5, 1, (3,))] +
         [(w, h, (3,)) for w, h in ((TW, TH), (TW - 1, TH), (TW + 1, TH), (TW, TH - 1), (TW, TH + 1), (TW - 1, TH - 1),
                                    (TW + 1, TH + 1))] +
         [(48, 40, (1, 2, 3, 4, 5, 6)), (70, 45, (6,))])
SIGMA_COLOR, SIGMA_PLANE, POWER = 0.3, 0.05, 2


@pytest.fixture(scope="module")
def gpu_available():
    if pa.device_count() < 1:
        pytest.skip("no GPU")


def first_difference(got, want):
    bad = np.argwhere(~((dm.bits(got) == dm.bits(want)) | (np.isnan(got) & np.isnan(want))))
    y, x, k = bad[0]
    return f"{len(bad)} words differ; first at row {y}, x {x}, channel {k}: {got[y, x, k]!r} != {want[y, x, k]!r}"


@pytest.mark.parametrize("width,height,iterations", SIZES, ids=[f"{w}x{h}" for w, h, _ in SIZES])
def test_filter_equals_model(gpu_available, width, height, iterations):
    inputs = dm.make_inputs(width, height, seed=1000 * width + height)
    for flags in (0, 1, 2, 3):
        for it in iterations:
            want = dm.model(*inputs, it, SIGMA_COLOR, SIGMA_PLANE, POWER, flags)
            kept, changed, untouched = dm.vacuity(inputs[0], inputs[2], inputs[3], want)
            print(f"{width}x{height}, flags {flags}, {it} iterations: kept {kept:.2f}, changed {changed:.2f}")
            assert kept >= 0.5 and untouched
            if width * height > 1:        # (the filter of a one-pixel image is the identity up to rounding)
                assert changed >= 0.5
            for staging in (0, 1, 2):
                got = pa.denoise_image(*inputs, iterations=it, sigma_color=SIGMA_COLOR, sigma_plane=SIGMA_PLANE,
                                       normal_power_log2=POWER, demodulate=bool(flags & 1), same_primitive=bool(flags & 2),
                                       staging=staging)
                assert dm.same_words(got, want), (f"flags {flags}, {it} iterations, staging {staging}: "
                                                  + first_difference(got, want))


def test_every_normal_power_and_a_wide_sigma(gpu_available):
    inputs = dm.make_inputs(45, 23, seed=77)
    for power in range(8):
        for sigma_color, sigma_plane in ((1e-3, 1e-6), (50.0, 10.0)):
            want = dm.model(*inputs, 4, sigma_color, sigma_plane, power, 1)
            got = pa.denoise_image(*inputs, iterations=4, sigma_color=sigma_color, sigma_plane=sigma_plane,
                                   normal_power_log2=power, demodulate=True, same_primitive=False)
            assert dm.same_words(got, want), (power, sigma_color, first_difference(got, want))


def test_device_refusals_name_the_field(gpu_available):
    img = np.zeros((4, 4, 4), dtype=np.float32)
    fp = N.C.POINTER(N.C.c_float)
    ptr = img.ctypes.data_as(fp)
    for params, field in ((N.PtDenoiseParams(0, 1.0, 0.1, 1, 1, 0), "iterations"), (N.PtDenoiseParams(9, 1.0, 0.1, 1, 1, 0), "iterations"),
                          (N.PtDenoiseParams(3, 0.0, 0.1, 1, 1, 0), "sigma_color"),
                          (N.PtDenoiseParams(3, float("nan"), 0.1, 1, 1, 0), "sigma_color"),
                          (N.PtDenoiseParams(3, 1.0, 1e-7, 1, 1, 0), "sigma_plane"),
                          (N.PtDenoiseParams(3, 1.0, 0.1, 8, 1, 0), "normal_power_log2"),
                          (N.PtDenoiseParams(3, 1.0, 0.1, 1, 4, 0), "flags"), (N.PtDenoiseParams(3, 1.0, 0.1, 1, 1, 3), "staging")):
        assert N.hip().pt_denoise_image(0, 4, 4, ptr, ptr, ptr, ptr, N.C.byref(params), ptr) == N.PT_ERR_ARG
        assert field in N.hip().pt_last_error(None).decode()
    pt = pa.Pathtracer(16, 16)
    good = N.PtDenoiseParams(3, 1.0, 0.1, 1, 1, 0)
    assert N.hip().pt_denoise(pt._ctx, 1, N.C.byref(good)) == N.PT_ERR_STATE
    assert "feature" in N.hip().pt_last_error(pt._ctx).decode()
    assert N.hip().pt_read_denoised(pt._ctx, ptr) == N.PT_ERR_STATE
    assert N.hip().pt_render_features(pt._ctx, N.C.byref(pa.PtCamera())) == N.PT_ERR_STATE      # no scene


PARAMS = dict(iterations=4, sigma_color=0.4, sigma_plane=0.03, normal_power_log2=3, demodulate=True, same_primitive=False)
MODEL_ARGS = (4, 0.4, 0.03, 3, 1)


def test_render_state_is_left_alone_and_denoise_equals_model(gpu_available, scenes):
    W, H = 72, 52
    pt, cam, ref, osc = pair(scenes / "cornell_box.scene.json", W, H)
    pt.set_run_ahead(2)                      # every launch makes a stash for the next call
    pt.render(cam, 4, True)
    accum, rng = pt.accum(), pt.rng_state()
    variant, costs, frames = pt.last_variant, pt.tile_costs(), pt.frames
    feats = pt.features(cam)
    out = pt.denoise(**PARAMS)
    assert np.array_equal(dm.bits(pt.accum()), dm.bits(accum)) and np.array_equal(pt.rng_state(), rng)
    assert (pt.last_variant, pt.frames) == (variant, frames) and np.array_equal(pt.tile_costs(), costs)
    hdr = pt.get_hdr_image_data()
    want = dm.model(hdr, *feats["planes"], *MODEL_ARGS)
    assert dm.same_words(out, want), first_difference(out, want)
    assert dm.same_words(pt.denoised(), out)
    # the tonemap is the existing one with divisor 1
    ldr = np.zeros((H, W, 4), dtype=np.uint8)
    po.lib().or_tonemap(po.fptr(np.ascontiguousarray(out)), W * H, 1, ldr.ctypes.data_as(N.C.POINTER(N.C.c_uint8)))
    assert np.array_equal(pt.tonemap_denoised(), ldr)
    # the automatic sigma is the documented statistic
    auto = pt.denoise()
    d = pa.DENOISE_DEFAULTS
    sigma = pa.auto_sigma_color(hdr, *feats["planes"], demodulate=d["demodulate"])
    want = dm.model(hdr, *feats["planes"], d["iterations"], sigma, d["sigma_plane"], d["normal_power_log2"], 1)
    assert dm.same_words(auto, want), first_difference(auto, want)
    # the render goes on as the oracle's does, from the stash of the first call
    pt.render(cam, 4, False)
    ref.render(osc.camera, 4, True)
    ref.render(osc.camera, 4, False)
    assert_bitexact(pt.accum(), ref.accum, "the call after the passes")
    assert np.array_equal(pt.rng_state(), ref.rng_array())
    # a scene change voids the planes
    pt.load_scene(str(scenes / "cornell_box.scene.json"))
    with pytest.raises(pa.PathtracerError) as e:
        pt.denoise(**PARAMS)
    assert e.value.code == N.PT_ERR_STATE and "feature" in str(e.value)


def test_band_partition_is_refused_by_name(gpu_available, scenes):
    pt = pa.Pathtracer(64, 64, band_rows=8, row_offset=1, row_stride=2)
    cam = pt.load_scene(str(scenes / "cornell_box.scene.json"))
    pt.render(cam, 1, True)
    pt.features(cam)
    with pytest.raises(pa.PathtracerError) as e:
        pt.denoise(**PARAMS)
    assert e.value.code == N.PT_ERR_ARG and "whole frame" in str(e.value)


def test_nan_pixels_stay_and_reach_nobody(gpu_available, tmp_path):
    W, H = 64, 48
    pt = pa.Pathtracer(W, H)
    cam = pt.load_scene(str(dsc.directed_scene(tmp_path, "rough_normal_16")))
    pt.render(cam, 8, True)
    hdr = pt.get_hdr_image_data()
    nan = np.isnan(hdr[..., :3])
    assert nan.any(), "the scene gives no NaN pixel"
    feats = pt.features(cam)
    out = pt.denoise(**PARAMS)
    assert np.array_equal(dm.bits(out[..., :3])[nan], dm.bits(hdr[..., :3])[nan])
    keep = dm.keep_mask(hdr, feats["planes"][1], feats["planes"][2])
    assert keep.any() and np.isfinite(out[..., :3][keep]).all()
    assert dm.same_words(out, dm.model(hdr, *feats["planes"], *MODEL_ARGS))


def test_after_an_adaptive_render_every_pixel_is_over_its_own_count(gpu_available, scenes):
    W, H = 60, 44
    pt = pa.Pathtracer(W, H)
    cam = pt.load_scene(str(scenes / "cornell_box.scene.json"))
    pt.render_adaptive(cam, spp=4, min_calls=2, max_calls=8, tolerance=0.2)
    n = pt.sample_counts()
    assert n.min() < n.max()
    feats = pt.features(cam)
    out = pt.denoise(**PARAMS)
    hdr = pt.get_hdr_image_data()                      # pt_read_adaptive_hdr
    want = dm.model(hdr, *feats["planes"], *MODEL_ARGS)
    assert dm.same_words(out, want), first_difference(out, want)
    assert np.array_equal(pt.sample_counts(), n)


def test_after_an_adaptive_render_and_a_scene_load_the_counts_still_divide(gpu_available, scenes):
    # the scene load voids the planes and the continuation, not the counts: the filter's input is the image the reads return
    pt = pa.Pathtracer(60, 44)
    cam = pt.load_scene(str(scenes / "cornell_box.scene.json"))
    pt.render_adaptive(cam, spp=4, min_calls=2, max_calls=8, tolerance=0.2)
    hdr = pt.accum() / pt.sample_counts().astype(np.float32)[..., None]
    cam = pt.load_scene(str(scenes / "cornell_box.scene.json"))
    feats = pt.features(cam)
    out = pt.denoise(**PARAMS)
    want = dm.model(hdr, *feats["planes"], *MODEL_ARGS)
    assert dm.same_words(out, want), first_difference(out, want)
    assert dm.same_words(pt.get_hdr_image_data(), hdr)


def test_the_automatic_sigma_is_of_the_undenoised_image_and_a_refusal_changes_nothing(gpu_available, scenes):
    pt = pa.Pathtracer(60, 44)
    cam = pt.load_scene(str(scenes / "cornell_box.scene.json"))
    pt.render_adaptive(cam, spp=4, min_calls=2, max_calls=8, tolerance=0.2)
    hdr, feats = pt.get_hdr_image_data(), pt.features(cam)
    params, host = pa.denoise_params(iterations=3, sigma_color=0.4), N.host()
    N.check_host(host.pth_renderer_denoise(pt._r, N.C.byref(params), 0, None))       # the image calls return the denoised image now
    denoised = pt.get_hdr_image_data()
    assert not dm.same_words(denoised, hdr)
    d = pa.DENOISE_DEFAULTS
    sigma = pa.auto_sigma_color(hdr, *feats["planes"], demodulate=d["demodulate"])
    want = dm.model(hdr, *feats["planes"], d["iterations"], sigma, d["sigma_plane"], d["normal_power_log2"], 1)
    assert dm.same_words(pt.denoise(), want)
    # a refused host-layer denoise (the planes are void) leaves the image calls where they were
    tex = np.ones((4, 4, 4), dtype=np.float32)
    N.check_ctx(N.hip().pt_set_texture(pt._ctx, 1, tex.ctypes.data_as(N.C.POINTER(N.C.c_float)), 4, 4), pt._ctx)
    assert host.pth_renderer_denoise(pt._r, N.C.byref(params), 1, None) == N.PT_ERR_STATE
    assert host.pth_renderer_denoised(pt._r) == 1 and dm.same_words(pt.get_hdr_image_data(), want)


def test_host_layer_and_cli(gpu_available, scenes, tmp_path):
    import subprocess
    from PIL import Image
    W, H = 64, 40
    scene = scenes / "test_shapes.scene.json"
    pt = pa.Pathtracer(W, H)
    cam = pt.load_scene(str(scene))
    pt.render(cam, 8, True)
    hdr = pt.get_hdr_image_data()
    planes = pt.features(cam)["planes"]
    host = N.host()
    # the host C ABI: features, planes, denoise with the automatic sigma, the image calls
    N.check_host(host.pth_renderer_features(pt._r, N.C.byref(cam)))
    for k in range(3):
        p = host.pth_renderer_feature_plane(pt._r, k)
        assert dm.same_words(np.ctypeslib.as_array(p, shape=(H, W, 4)), planes[k])
    assert not host.pth_renderer_feature_plane(pt._r, 3)
    params = pa.denoise_params(iterations=3, sigma_color=123.0)            # sigma_color is not read with auto_sigma
    used = N.C.c_float(0.0)
    assert host.pth_renderer_denoised(pt._r) == 0
    N.check_host(host.pth_renderer_denoise(pt._r, N.C.byref(params), 1, N.C.byref(used)))
    assert host.pth_renderer_denoised(pt._r) == 1
    sigma = pa.auto_sigma_color(hdr, *planes, demodulate=True)
    assert used.value == pytest.approx(sigma, rel=1e-5)                       # the same statistic, summed in another order
    d = pa.DENOISE_DEFAULTS
    want = dm.model(hdr, *planes, 3, used.value, d["sigma_plane"], d["normal_power_log2"], 1)
    got = pt.get_hdr_image_data()                                            # the denoised image now
    assert dm.same_words(got, want), first_difference(got, want)
    ldr = pt.get_image_data()
    assert np.array_equal(ldr, pt.tonemap_denoised())
    params.sigma_color = 0.0
    assert host.pth_renderer_denoise(pt._r, N.C.byref(params), 0, None) == N.PT_ERR_ARG
    # the CLI applies it before the image is written: the same launch, the same C++ path
    png = tmp_path / "denoised.png"
    r = subprocess.run([str(N.CLI), "-w", str(W), "-h", str(H), "-spp", "8", "-denoise", "3", "-o", str(png), str(scene)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Denoised: 3 a-trous iterations" in r.stdout, r.stdout + r.stderr
    assert np.array_equal(np.asarray(Image.open(png).convert("RGBA")), ldr[::-1])
    # the next render returns the image calls to the accumulation
    pt.render(cam, 8, False)
    assert host.pth_renderer_denoised(pt._r) == 0
    assert not dm.same_words(pt.get_hdr_image_data(), got)


def relative_mse(img, ref, mask):
    """Mean over the masked pixels and the three channels of (img - ref)^2 / (ref^2 + 0.01)."""
    a, r = img[..., :3][mask].astype(np.float64), ref[..., :3][mask].astype(np.float64)
    return float(np.mean((a - r) ** 2 / (r * r + 0.01)))


def test_it_denoises(gpu_available, scenes):
    """A condition, not a tuned threshold.  Measured on MI355X: 11.99 -> 11.59, ratio 0.967 -- the relative MSE
    of an 8-spp cornell is decided by its fireflies, which an edge-stopping filter leaves alone."""
    W = H = 128
    pt = pa.Pathtracer(W, H)
    cam = pt.load_scene(str(scenes / "cornell_box.scene.json"))
    pt.render(cam, 8, True, chunks=512)
    ref = pt.get_hdr_image_data()
    pt.render(cam, 8, True)
    noisy = pt.get_hdr_image_data()
    feats = pt.features(cam)
    out = pt.denoise()
    mask = dm.keep_mask(noisy, feats["planes"][1], feats["planes"][2]) & np.isfinite(ref[..., :3]).all(-1)
    before, after = relative_mse(noisy, ref, mask), relative_mse(out, ref, mask)
    print(f"relative MSE over {int(mask.sum())} kept finite pixels: noisy {before:.5f}, denoised {after:.5f}, "
          f"ratio {after / before:.3f}")
    assert mask.sum() > W * H // 2
    assert after < before
