"""The guided upsampling on the GPU against its numpy restatement (tests/upsample_model.py): words equal, or both NaN,
and both counts exactly, no tolerance -- through pt_upsample_image on the seeded size pairs and planted cases, staged
and unstaged, and through two contexts on renders of the Cornell box and of a textured quad -- then what the call must
leave alone (both render states), what it refuses and what ends the held image, the C++ layer and the CLI, and that it
brings back what bilinear resampling cannot.
"""
import json
import subprocess

import numpy as np
import pytest

import upsample_model as um
import pathtracercuda_amd as pa
from pathtracercuda_amd import _native as N
from test_gpu_adaptive_variance import assert_same_state
from test_gpu_despike import render_state
from test_gpu_parity import assert_bitexact
from test_gpu_temporal import first_difference

pytestmark = pytest.mark.gpu

F, U = um.F, um.U
W, H, LW, LH = 64, 64, 32, 32


@pytest.fixture(scope="module")
def gpu_available():
    if pa.device_count() < 1:
        pytest.skip("no GPU")


def device(lo, hi, sigma_plane, power, flags, staging=0):
    return pa.upsample_image(*lo, *hi, sigma_plane=sigma_plane, normal_power_log2=power, demodulate=bool(flags & 1),
                             same_primitive=bool(flags & 2), staging=staging, return_counts=True)


def assert_equals_model(lo, hi, sigma_plane, power, flags, what, stagings=(0, 1, 2)):
    stats = {}
    want, counts = um.model(lo, hi, sigma_plane, power, flags, stats)
    for staging in stagings:
        got, n = device(lo, hi, sigma_plane, power, flags, staging)
        where = f"{what}, sigma_plane {sigma_plane}, power {power}, flags {flags}, staging {staging}: "
        assert um.same_words(got, want), where + first_difference(got, want)
        assert n == counts, where + f"counts {n} != {counts}"
    return stats


@pytest.mark.parametrize("sizes", um.SIZE_PAIRS, ids=lambda s: "%dx%d_from_%dx%d" % s)
def test_every_form_equals_the_model(gpu_available, sizes):
    Wd, Hd, w, h = sizes
    lo, hi = um.make_case(Wd, Hd, w, h, seed=Wd * 100 + Hd)
    served = 0
    for flags in (0, 1, 2, 3):
        for sigma_plane, power in um.PARAM_SETS:
            served += assert_equals_model(lo, hi, sigma_plane, power, flags, "seeded")["ring1"]
    assert served > 0


def flat_pair(Wd=40, Hd=24, w=13, h=8):
    """One surface facing the camera at both sizes (ratio about 3, so b takes many values), every pixel kept."""
    def planes(X, Y):
        n = X.shape
        p0 = np.full(n + (4,), 0.5, dtype=F)
        p0[..., 3] = np.full(n, 7, dtype=U).view(F)
        p1 = np.zeros(n + (4,), dtype=F)
        p1[..., 2], p1[..., 3] = 1, 4
        p2 = np.zeros(n + (4,), dtype=F)
        p2[..., 0], p2[..., 1] = F(0.1) * X, F(0.1) * Y
        p2[..., 3] = np.full(n, um.HIT, dtype=U).view(F)
        return [p0, p1, p2]

    yh, xh = np.mgrid[0:Hd, 0:Wd]
    yl, xl = np.mgrid[0:h, 0:w]
    X = ((xl.astype(F) + F(0.5)) * (F(Wd) / F(w)) - F(0.5)).astype(F)
    Y = ((yl.astype(F) + F(0.5)) * (F(Hd) / F(h)) - F(0.5)).astype(F)
    color = np.ones((h, w, 4), dtype=F)
    color[..., :3] = (F(0.2) + F(0.01) * (xl + 2 * yl).astype(F))[..., None]
    return [color] + planes(X, Y), planes(xh.astype(F), yh.astype(F))


def test_planted_cases_on_the_device(gpu_available):
    def run(lo, hi, what, flags=3, sigma_plane=0.3, power=3):
        return assert_equals_model(lo, hi, sigma_plane, power, flags, what)

    lo, hi = flat_pair()
    s = run(lo, hi, "flat")
    assert (s["guided"], s["wide"], s["nearest"], s["unguided"]) == (40 * 24, 0, 0, 0)
    # infinite and NaN low colours and normals: not kept, and they reach nobody
    lo, hi = flat_pair()
    lo[0][2, 3, 0], lo[0][2, 4, 1], lo[0][5, 9, 2] = np.nan, np.inf, -np.inf
    lo[2][3, 6, 1], lo[2][6, 2, 0] = np.nan, np.inf
    s = run(lo, hi, "low NaN and infinity")
    assert s["not_kept"] > 20 and s["nearest"] == 0
    out, _ = um.model(lo, hi, 0.3, 3, 3)
    assert np.isfinite(out).all()
    # a NaN high normal: no guide, and none of the low pixels is of its class (all are kept): the nearest words
    lo, hi = flat_pair()
    hi[1][7, 20, 0] = np.nan
    s = run(lo, hi, "high NaN normal")
    assert (s["unguided"], s["u_nearest"], s["u_kept"]) == (1, 1, 1)
    # antiparallel normals: w_n = 0 for every tap, the sums stay 0, both rings fail
    lo, hi = flat_pair()
    hi[1][10:14, 8:12, 2] = -1
    s = run(lo, hi, "antiparallel")
    assert s["nearest"] == 16 and s["wide"] == 0
    assert run(lo, hi, "antiparallel, power 0", power=0)["nearest"] == 16
    # albedo 0 on both sides (the divisor's floor), and a high albedo that differs from the low one
    lo, hi = flat_pair()
    lo[1][..., :3], hi[0][::2, ::3, :3], hi[0][1::2, 1::3, :3] = 0, 0, F(0.9)
    run(lo, hi, "albedo 0")
    run(lo, hi, "albedo 0, no demodulation", flags=2)
    # t_p = 0: mm = 0, the plane weight is 0 or NaN, the pixel ends at the nearest low pixel
    lo, hi = flat_pair()
    hi[1][5, 5, 3] = hi[1][20, 33, 3] = 0
    hi[2][20, 33, 2] = F(0.5)                                   # off the plane: g != 0 and g * g / 0 = inf
    assert run(lo, hi, "t = 0")["nearest"] == 2
    # ids that never match: with the id test the nearest pixel, without it the ordinary result
    lo, hi = flat_pair()
    hi[0][3:6, 30:34, 3] = np.full((3, 4), 999, dtype=U).view(F)
    assert run(lo, hi, "ids")["nearest"] == 12
    assert run(lo, hi, "ids, no id test", flags=1)["nearest"] == 0
    # a high pixel whose 16 taps are all rejected, one rescued by ring 2, beside a hole in the low image
    lo, hi = flat_pair()
    lo[0][2:7, 4:9, 0] = np.nan
    s = run(lo, hi, "hole")
    assert s["nearest"] > 0 and s["wide"] > 0
    # low pixels of every class beside each other: kept, emitter, miss, not finite -- under high pixels of every class
    lo, hi = flat_pair()
    for planes, scale in ((lo, 1), (hi, 3)):
        fl = planes[-1][..., 3].view(U)
        fl[:, 4 * scale:5 * scale] = um.HIT | um.EMISSIVE
        fl[:, 5 * scale:6 * scale] = 0
        planes[-3][:, 5 * scale:6 * scale, 3] = np.full(1, 0xffffffff, dtype=U).view(F)
    lo[0][3, 3:7, 1] = np.nan
    s = run(lo, hi, "classes")
    assert s["u_interpolated"] > 50 and s["u_flags"] > 0 and s["u_kept"] > 0 and s["u_not_raw"] > 0 and s["u_nearest"] > 0
    assert s["u_miss"] > 0 and s["u_emitter"] > 0
    run(lo, hi, "classes, flags 0", flags=0)


# ---- on two contexts -------------------------------------------------------------------------------------
PARAMS = dict(sigma_plane=0.02, normal_power_log2=3)


def obj(t, pos, rot, scale, base, emissive=(0.0, 0.0, 0.0), tex=""):
    return {"type": t, "position": list(pos), "rotation": list(rot), "scale": list(scale),
            "material": {"type": "LAMBERT", "baseColor": list(base), "emissive": list(emissive), "roughness": 0.5,
                         "metalness": 0.0, "texture": tex}}


@pytest.fixture(scope="module")
def textured_scene(scenes, tmp_path_factory):
    """A wall textured with scenes/checker.png (object 0) that fills most of the view, over a floor, under an emissive
    ceiling.  Its checker cells are about 16 pixels wide at 64 x 64."""
    scene = {"camera": {"position": [0.0, 1.0, 4.0], "look_at": [0.0, 1.0, 0.0], "fovy": 45.0},
             "objects": [obj("QUAD", (0, 1, -1), (90, 0, 0), (3.6, 1.0, 1.8), (1, 1, 1), tex=str(scenes / "checker.png")),
                         obj("QUAD", (0, -0.2, 0), (0, 0, 0), (12, 12, 12), (0.7, 0.7, 0.7)),
                         obj("QUAD", (0, 3.5, 1.0), (0, 0, 0), (10, 10, 10), (1, 1, 1), emissive=(0.15, 0.15, 0.15))]}
    path = tmp_path_factory.mktemp("upsample") / "textured.scene.json"
    path.write_text(json.dumps(scene))
    return str(path)


def pair(scene, spp=8, chunks=1):
    hi, lo = pa.Pathtracer(W, H), pa.Pathtracer(LW, LH)
    cam = hi.load_scene(scene)
    lo.load_scene(scene)
    lo.render(cam, spp, True, chunks=chunks)
    return hi, lo, cam, hi.features(cam)["planes"], lo.features(cam)["planes"]


@pytest.fixture(scope="module", params=["cornell", "textured"])
def contexts(request, gpu_available, scenes, textured_scene):
    scene = str(scenes / "cornell_box.scene.json") if request.param == "cornell" else textured_scene
    return pair(scene) + (scene,)


def test_every_source_equals_the_model_and_both_render_states_stay(contexts):
    hi, lo, cam, hi_planes, lo_planes, scene = contexts
    hi.render(cam, 2, True)                                          # a render state on the larger context too
    states = render_state(hi), render_state(lo)

    def check(source, color, what, **kw):
        got = hi.upsample(lo, source=source, **PARAMS, **kw)
        flags = (1 if kw.get("demodulate", True) else 0) | (2 if kw.get("same_primitive", True) else 0)
        stats = {}
        want, counts = um.model([color] + list(lo_planes), hi_planes, PARAMS["sigma_plane"], PARAMS["normal_power_log2"], flags,
                                stats)
        assert um.same_words(got, want), what + ": " + first_difference(got, want)
        assert hi.upsample_counts() == {"wide": counts[0], "nearest": counts[1]}, what
        assert um.same_words(hi.upsampled(), got)
        assert_same_state(render_state(hi), states[0], what + ", the larger context")
        assert_same_state(render_state(lo), states[1], what + ", the smaller context")
        return got, stats

    hdr = lo.get_hdr_image_data()
    out, stats = check("accum", hdr, "accum")
    print({k: v for k, v in stats.items() if not k.endswith("_mask")})
    assert stats["ring1"] > W * H // 4 and stats["by_id"] > 0
    t = hi.upsample_timing()
    assert t["prepare"] > 0 and t["upsample"] > 0
    assert hi.tonemap_upsampled().shape == (H, W, 4)
    for staging in (1, 2):
        assert um.same_words(hi.upsample(lo, staging=staging, **PARAMS), out)
    check("accum", hdr, "accum, flags 1", same_primitive=False)
    check("accum", hdr, "accum, flags 2", demodulate=False)
    quarter = (lo.accum() * (F(1) / F(4))).astype(F)                 # frames: the image is the accumulation over them
    check("accum", quarter, "accum over 4 frames", frames=4)
    despiked = lo.despike()
    states = states[0], render_state(lo)
    check("despiked", despiked, "despiked")
    denoised = lo.denoise(source="despiked", iterations=2, sigma_color=0.5)
    check("denoised", denoised, "denoised")
    temporal = lo.temporal(reset=True)
    check("temporal", temporal, "temporal")
    assert um.same_words(lo.despiked(), despiked) and um.same_words(lo.denoised(), denoised)   # nothing of lo ended


def test_after_an_adaptive_render_every_low_pixel_is_over_its_own_count(gpu_available, scenes):
    hi, lo, cam, hi_planes, _ = pair(str(scenes / "cornell_box.scene.json"), spp=1)
    lo.render_adaptive(cam, spp=2, min_calls=2, max_calls=8, tolerance=0.1)
    n = lo.sample_counts()
    assert n.min() < n.max()
    lo_planes = lo.features(cam)["planes"]
    before = render_state(lo)
    got = hi.upsample(lo, **PARAMS)
    color = (lo.accum() / np.maximum(n, 1).astype(F)[..., None]).astype(F)
    want, counts = um.model([color] + list(lo_planes), hi_planes, PARAMS["sigma_plane"], 3, 3)
    assert um.same_words(got, want), first_difference(got, want)
    assert_same_state(render_state(lo), before, "pt_upsample after an adaptive render")


def test_a_continued_render_equals_a_twin_that_never_upsampled(gpu_available, scenes):
    scene = str(scenes / "cornell_box.scene.json")
    hi, lo, cam, _, _ = pair(scene, spp=4)
    twin = pa.Pathtracer(LW, LH)
    twin.load_scene(scene)
    twin.render(cam, 4, True)
    twin.features(cam)
    hi.upsample(lo)
    for p in (lo, twin):
        p.render(cam, 4, False)
    assert_bitexact(lo.accum(), twin.accum(), "the continued render")
    assert np.array_equal(lo.rng_state(), twin.rng_state())
    assert lo.frames == twin.frames == 2
    hi.render(cam, 4, True)                                          # and the larger context renders as one that never did
    big = pa.Pathtracer(W, H)
    big.load_scene(scene)
    big.render(cam, 4, True)
    assert_bitexact(hi.accum(), big.accum(), "the larger context's render")


def refused(code, word, call, *args, **kw):
    with pytest.raises(pa.PathtracerError) as e:
        call(*args, **kw)
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_refusals_and_what_ends_the_image(gpu_available, scenes):
    scene = str(scenes / "cornell_box.scene.json")
    hi, lo = pa.Pathtracer(W, H), pa.Pathtracer(LW, LH)
    cam = hi.load_scene(scene)
    lo.load_scene(scene)
    lib = N.hip()
    readers = (hi.upsampled, hi.tonemap_upsampled, hi.upsample_counts, hi.upsample_timing)

    def none_held():
        assert lib.pt_holds_upsampled(hi._ctx) == 0
        for call in readers:
            refused(N.PT_ERR_STATE, "no upsampled image", call)

    lo.render(cam, 2, True)
    hi.render(cam, 1, True)                                          # (a render state to compare, nothing the call needs)
    none_held()
    refused(N.PT_ERR_STATE, "hi has no feature planes", hi.upsample, lo)
    hi.features(cam)
    refused(N.PT_ERR_STATE, "lo has no feature planes", hi.upsample, lo)
    lo.features(cam)
    none_held()
    # a source that lo does not hold
    refused(N.PT_ERR_STATE, "no denoised image", hi.upsample, lo, source="denoised")
    refused(N.PT_ERR_STATE, "no temporal image", hi.upsample, lo, source="temporal")
    refused(N.PT_ERR_STATE, "no despiked image", hi.upsample, lo, source="despiked")
    lo.temporal(reset=True)
    lo.features(cam)                                                 # the temporal image is no longer of lo's planes
    refused(N.PT_ERR_STATE, "no temporal image", hi.upsample, lo, source="temporal")
    none_held()
    out = hi.upsample(lo)
    counts = hi.upsample_counts()
    assert lib.pt_holds_upsampled(hi._ctx) == 1 and lib.pt_holds_upsampled(lo._ctx) == 0
    states = render_state(hi), render_state(lo)
    # calls refused for their arguments change nothing
    fields = ("sigma_plane", "normal_power_log2", "flags", "staging")
    good = dict(sigma_plane=0.005, normal_power_log2=3, flags=3, staging=0)
    nan = float("nan")
    for over in (dict(sigma_plane=0.0), dict(sigma_plane=nan), dict(sigma_plane=float("inf")), dict(normal_power_log2=8),
                 dict(flags=4), dict(staging=3)):
        v = dict(good, **over)
        params = N.PtUpsampleParams(*[v[f] for f in fields])
        assert lib.pt_upsample(hi._ctx, lo._ctx, 0, 1, N.C.byref(params)) == N.PT_ERR_ARG
        assert list(over)[0] in lib.pt_last_error(hi._ctx).decode(), (over, lib.pt_last_error(hi._ctx).decode())
    ok = pa.upsample_params()
    assert lib.pt_upsample(hi._ctx, lo._ctx, 0, 1, None) == N.PT_ERR_ARG
    assert lib.pt_upsample(hi._ctx, None, 0, 1, N.C.byref(ok)) == N.PT_ERR_ARG and "lo is null" in lib.pt_last_error(hi._ctx).decode()
    assert lib.pt_upsample(hi._ctx, lo._ctx, 4, 1, N.C.byref(ok)) == N.PT_ERR_ARG and "source" in lib.pt_last_error(hi._ctx).decode()
    refused(N.PT_ERR_ARG, "larger", lo.upsample, hi)                  # lo larger than hi, in either dimension
    wide = pa.Pathtracer(W + 8, LH)
    wide.load_scene(scene)
    wide.features(cam)
    wide.render(cam, 1, True)
    refused(N.PT_ERR_ARG, "larger", hi.upsample, wide)
    assert um.same_words(hi.upsampled(), out) and hi.upsample_counts() == counts
    assert_same_state(render_state(hi), states[0], "refused calls, the larger context")
    assert_same_state(render_state(lo), states[1], "refused calls, the smaller context")
    # what does not end it: anything but the next call -- renders, features, a texture, a scene on either context
    hi.render(cam, 2, True)
    hi.features(cam)
    lo.render(cam, 2, False)
    lo.features(cam)
    assert um.same_words(hi.upsampled(), out)
    cam = hi.load_scene(scene)
    assert um.same_words(hi.upsampled(), out) and lib.pt_holds_upsampled(hi._ctx) == 1
    refused(N.PT_ERR_STATE, "hi has no feature planes", hi.upsample, lo)     # refused for the state: nothing changes either
    assert um.same_words(hi.upsampled(), out)
    hi.features(cam)
    again = hi.upsample(lo, frames=2)
    assert not um.same_words(again, out) and um.same_words(hi.upsampled(), again)
    # equal sizes are accepted, and a context may be its own source
    assert hi.upsample(hi, frames=1).shape == (H, W, 4)


def test_band_partitions_and_another_device_are_refused_by_name(gpu_available, scenes):
    scene = str(scenes / "cornell_box.scene.json")
    whole, bands = pa.Pathtracer(W, H), pa.Pathtracer(W, H, band_rows=8, row_offset=1, row_stride=2)
    cam = whole.load_scene(scene)
    bands.load_scene(scene)
    for p in (whole, bands):
        p.render(cam, 1, True)
        p.features(cam)
    refused(N.PT_ERR_ARG, "hi holds a band partition", bands.upsample, whole)
    refused(N.PT_ERR_ARG, "lo holds a band partition", whole.upsample, bands)
    if pa.device_count() > 1:
        other = pa.Pathtracer(LW, LH, device=1)
        other.load_scene(scene)
        other.render(cam, 1, True)
        other.features(cam)
        refused(N.PT_ERR_ARG, "different devices", whole.upsample, other)


def test_host_layer_and_cli(gpu_available, scenes, tmp_path):
    from PIL import Image
    scene = scenes / "cornell_box.scene.json"
    hi, lo, cam, _, _ = pair(str(scene), spp=8)
    host = N.host()
    want = hi.upsample(lo)                                           # the Python path at the defaults
    ldr, counts = hi.tonemap_upsampled(), hi.upsample_counts()
    hi.render(cam, 1, True)
    plain = hi.get_hdr_image_data()
    assert not um.same_words(want, plain)                            # the host layer has not upsampled yet
    params = pa.upsample_params()
    n = (N.C.c_uint32 * 2)()
    N.check_host(host.pth_renderer_upsample(hi._r, lo._r, 0xffffffff, N.C.byref(params)))
    N.check_host(host.pth_renderer_upsample_counts(hi._r, n))
    assert {"wide": n[0], "nearest": n[1]} == counts
    assert um.same_words(hi.get_hdr_image_data(), want) and np.array_equal(hi.get_image_data(), ldr)
    # the automatic source is what lo's image calls return: its despiked image, then its denoised one
    ds = pa.despike_params()
    N.check_host(host.pth_renderer_despike(lo._r, N.C.byref(ds)))
    N.check_host(host.pth_renderer_upsample(hi._r, lo._r, 0xffffffff, N.C.byref(params)))
    assert um.same_words(hi.get_hdr_image_data(), hi.upsample(lo, source="despiked"))
    dn = pa.denoise_params(iterations=3, sigma_color=0.5)
    N.check_host(host.pth_renderer_denoise(lo._r, N.C.byref(dn), 0, None))
    N.check_host(host.pth_renderer_upsample(hi._r, lo._r, 0xffffffff, N.C.byref(params)))
    filtered = hi.upsample(lo, source="denoised")
    assert um.same_words(hi.get_hdr_image_data(), filtered) and not um.same_words(filtered, want)
    filtered_ldr = hi.get_image_data()
    params.staging = 3
    assert host.pth_renderer_upsample(hi._r, lo._r, 0, N.C.byref(params)) == N.PT_ERR_ARG and "staging" in host.pth_last_error().decode()
    # the next render returns the image calls to the accumulation
    hi.render(cam, 1, True)
    assert um.same_words(hi.get_hdr_image_data(), hi.accum()) and not um.same_words(hi.get_hdr_image_data(), filtered)
    # the CLI: the same launches through the same C++ path, written at the full size
    base = [str(N.CLI), "-w", str(W), "-h", str(H), "-spp", "8", "-upsample", "2"]
    png = tmp_path / "upsampled.png"
    r = subprocess.run(base + ["-o", str(png), str(scene)], capture_output=True, text=True, timeout=120)
    line = f"Upsampled: {W} x {H} from {LW} x {LH}, {counts['wide']} pixels from the wider ring, {counts['nearest']} from the nearest pixel"
    assert r.returncode == 0 and line in r.stdout, r.stdout + r.stderr
    assert np.array_equal(np.asarray(Image.open(png).convert("RGBA")), ldr[::-1])
    png2 = tmp_path / "upsampled_filtered.png"
    r = subprocess.run(base + ["-despike", "-denoise", "3", "-o", str(png2), str(scene)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Despiked:" in r.stdout and "Denoised: 3" in r.stdout and "Upsampled:" in r.stdout, r.stdout + r.stderr
    assert Image.open(png2).size == (W, H)


def tonemapped(img):
    """x / (1 + x), then the display gamma: monotone, bounded, and not saturating anywhere."""
    x = np.maximum(img[..., :3].astype(np.float64), 0.0)
    return (x / (1.0 + x)) ** (1.0 / 2.2)


def test_it_upsamples(gpu_available, textured_scene):
    """On the textured wall: low image 32 x 32 at 256 spp, reference 64 x 64 at 256 spp.  Over the wall's interior
    pixels (the pixel and its eight neighbours are first hits of the wall) the tonemapped MSE of the guided result is
    strictly below that of the numpy bilinear resampling of the same low image: the checker's edges and gradients are
    in the full-size albedo plane, and no resampling of the low colour can bring them back.  What is left in the guided
    result is the aliasing of the one-sample albedo plane along the checker's edges."""
    hi, lo, cam, hi_planes, lo_planes = pair(textured_scene, spp=8, chunks=32)
    guided = hi.upsample(lo)
    low = lo.get_hdr_image_data()
    hi.render(cam, 8, True, chunks=32)
    ref = hi.get_hdr_image_data()
    plain = um.bilinear(low, W, H)
    wall = hi_planes[0][..., 3].view(U) == 0
    interior = wall.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            interior &= np.roll(np.roll(wall, dy, 0), dx, 1)
    interior[[0, -1], :] = interior[:, [0, -1]] = False
    e_guided, e_plain, e_near = (float(((tonemapped(img) - tonemapped(ref)) ** 2)[interior].mean())
                                 for img in (guided, plain, um.nearest(low, W, H)))
    message = (f"tonemapped MSE over {int(interior.sum())} interior pixels of the wall: guided {e_guided:.6f}, "
               f"bilinear {e_plain:.6f}, nearest {e_near:.6f}; counts {hi.upsample_counts()}")
    print(message)
    assert interior.sum() > W * H // 3, message
    assert e_guided < e_plain, message
