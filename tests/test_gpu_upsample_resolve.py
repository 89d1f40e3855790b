"""The guided upsampling onto supersampled planes on the GPU against its numpy restatement
(tests/upsample_resolve_model.py) and against the box mean, in rule 9's order, of pt_upsample_image run at the S-times
size: words equal, or both NaN, and both counts exactly, no tolerance -- through pt_upsample_resolve_image on the seeded
size pairs and planted cases, staged and unstaged, and through three contexts on renders of the Cornell box and of a
textured quad -- then what the call must leave alone (all three render states), what it refuses, the C++ layer and the
CLI, and that it antialiases the silhouettes that one first-hit sample per pixel leaves stair-stepped.
"""
import subprocess

import numpy as np
import pytest

import upsample_model as um
import upsample_resolve_model as rm
import pathtracercuda_amd as pa
from pathtracercuda_amd import _native as N
from test_gpu_adaptive_variance import assert_same_state
from test_gpu_despike import render_state
from test_gpu_temporal import first_difference
from test_gpu_upsample import flat_pair, refused, textured_scene, tonemapped   # noqa: F401  (textured_scene: a fixture)

pytestmark = pytest.mark.gpu

F, U = um.F, um.U
W, H, LW, LH = 32, 32, 16, 16


@pytest.fixture(scope="module")
def gpu_available():
    if pa.device_count() < 1:
        pytest.skip("no GPU")


def device(lo, ss, S, sigma_plane, power, flags, staging=0):
    return pa.upsample_resolve_image(*lo, *ss, S, sigma_plane=sigma_plane, normal_power_log2=power, demodulate=bool(flags & 1),
                                     same_primitive=bool(flags & 2), staging=staging, return_counts=True)


def assert_equals_model(lo, ss, S, sigma_plane, power, flags, what, stagings=(0, 1, 2)):
    stats = {}
    want, counts = rm.model(lo, ss, S, sigma_plane, power, flags, stats)
    # what a user of pt_upsample_image does today: the S-times image, read back and averaged on the host
    full, full_counts = pa.upsample_image(*lo, *ss, sigma_plane=sigma_plane, normal_power_log2=power, demodulate=bool(flags & 1),
                                          same_primitive=bool(flags & 2), return_counts=True)
    mean = rm.box_mean(full, S)
    for staging in stagings:
        got, n = device(lo, ss, S, sigma_plane, power, flags, staging)
        where = f"{what}, S {S}, sigma_plane {sigma_plane}, power {power}, flags {flags}, staging {staging}: "
        assert got.shape == want.shape, where + f"{got.shape}"
        assert um.same_words(got, want), where + "model: " + first_difference(got, want)
        assert um.same_words(got, mean), where + "box mean of pt_upsample_image: " + first_difference(got, mean)
        assert n == counts == full_counts, where + f"counts {n} != {counts}"
    return stats


@pytest.mark.parametrize("S", rm.FACTORS)
@pytest.mark.parametrize("sizes", rm.SIZE_PAIRS, ids=lambda s: "%dx%d_from_%dx%d" % s)
def test_every_form_equals_the_model_and_the_box_mean(gpu_available, sizes, S):
    Wd, Hd, w, h = sizes
    lo, ss = rm.make_case(Wd, Hd, w, h, S, seed=Wd * 100 + Hd + S)
    served = 0
    for flags in rm.FLAG_SETS:
        for sigma_plane, power in um.PARAM_SETS:
            served += assert_equals_model(lo, ss, S, sigma_plane, power, flags, "seeded")["ring1"]
    assert served > 0


@pytest.mark.parametrize("S", rm.FACTORS)
def test_planted_cases_inside_one_block(gpu_available, S):
    """tests/test_gpu_upsample.py's planted cases, each placed at some of the sub-pixels of one output pixel's block, so
    the output pixel mixes the rare branch with the ordinary one."""
    Wo, Ho = 20, 12
    bx, by = S * 7, S * 5                                       # the block of output pixel (7, 5)

    def pair_():
        return flat_pair(Wd=S * Wo, Hd=S * Ho, w=13, h=8)

    def run(lo, ss, what, flags=3, sigma_plane=0.3, power=3):
        return assert_equals_model(lo, ss, S, sigma_plane, power, flags, what)

    lo, ss = pair_()
    s = run(lo, ss, "flat")
    assert (s["guided"], s["wide"], s["nearest"], s["unguided"]) == (S * S * Wo * Ho, 0, 0, 0)
    # a NaN high normal at one sub-pixel: no guide, the nearest words, one sub-pixel among S * S
    lo, ss = pair_()
    ss[1][by + 1, bx, 0] = np.nan
    s = run(lo, ss, "high NaN normal")
    assert (s["unguided"], s["u_nearest"]) == (1, 1)
    # antiparallel normals on the block's first row: both rings fail there, the other rows are ordinary
    lo, ss = pair_()
    ss[1][by, bx:bx + S, 2] = -1
    s = run(lo, ss, "antiparallel")
    assert s["nearest"] == S and s["wide"] == 0
    assert run(lo, ss, "antiparallel, power 0", power=0)["nearest"] == S
    # t_p = 0 at the block's last sub-pixel, off the plane
    lo, ss = pair_()
    ss[1][by + S - 1, bx + S - 1, 3] = 0
    ss[2][by + S - 1, bx + S - 1, 2] = F(0.5)
    assert run(lo, ss, "t = 0")["nearest"] == 1
    # ids that never match on the block's last column: with the id test the nearest pixel, without it the ordinary result
    lo, ss = pair_()
    ss[0][by:by + S, bx + S - 1, 3] = np.full(S, 999, dtype=U).view(F)
    assert run(lo, ss, "ids")["nearest"] == S
    assert run(lo, ss, "ids, no id test", flags=1)["nearest"] == 0
    # a sub-pixel that is not finite makes its output pixel not finite, and no other
    lo, ss = pair_()
    lo[0][:, :, :3] = F(0.25)
    ss[0][by, bx + 1, 0] = np.inf                               # an infinite albedo: the divisor, and so the product
    run(lo, ss, "infinite albedo")
    out, _ = device(lo, ss, S, 0.3, 3, 3)
    bad = ~np.isfinite(out[..., :3]).all(-1)
    assert bad[5, 7] and bad.sum() == 1
    # a hole in the low image: sub-pixels rescued by ring 2 and sub-pixels that end at the nearest pixel
    lo, ss = pair_()
    lo[0][2:7, 4:9, 0] = np.nan
    s = run(lo, ss, "hole")
    assert s["nearest"] > 0 and s["wide"] > 0
    blocks = rm.block_stats(ss[0], S, s["wide_mask"], s["nearest_mask"])
    assert s["wide"] > blocks["wide"] or s["nearest"] > blocks["nearest"]     # counted per sub-pixel, not per output pixel
    # albedo 0 on both sides (the divisor's floor)
    lo, ss = pair_()
    lo[1][..., :3], ss[0][::2, ::3, :3], ss[0][1::2, 1::3, :3] = 0, 0, F(0.9)
    run(lo, ss, "albedo 0")
    run(lo, ss, "albedo 0, no demodulation", flags=2)
    # infinite and NaN low colours and normals: not kept, and they reach nobody
    lo, ss = pair_()
    lo[0][2, 3, 0], lo[0][2, 4, 1], lo[0][5, 9, 2] = np.nan, np.inf, -np.inf
    lo[2][3, 6, 1], lo[2][6, 2, 0] = np.nan, np.inf
    s = run(lo, ss, "low NaN and infinity")
    assert s["not_kept"] > 20 * S * S and s["nearest"] == 0
    out, _ = device(lo, ss, S, 0.3, 3, 3)
    assert np.isfinite(out).all()
    # low pixels of every class beside each other: kept, emitter, miss, not finite -- under sub-pixels of every class.
    # The S-times stripes begin and end inside output blocks, so those blocks mix unguided sub-pixels with guided ones
    # and emitters with misses: the unguided sums, their skips and the uncounted nearest fallback, inside the mean.
    lo, ss = classes_pair(S, Wo, Ho)
    s = run(lo, ss, "classes")
    assert s["u_interpolated"] > 50 and s["u_flags"] > 0 and s["u_kept"] > 0 and s["u_not_raw"] > 0 and s["u_nearest"] > 0
    assert s["u_miss"] > 0 and s["u_emitter"] > 0 and s["u_id"] > 0
    unguided = ~s["guide_mask"].reshape(Ho, S, Wo, S)
    assert (unguided.any(axis=(1, 3)) & ~unguided.all(axis=(1, 3))).sum() >= 2 * Ho      # blocks that mix the two paths
    run(lo, ss, "classes, flags 0", flags=0)


def classes_pair(S, Wo, Ho):
    """flat_pair with a stripe of emitters and a stripe of misses at both sizes: low columns 4 and 5, and the S-times
    columns over them, from 6 S + 1 to 8 S - 2 and from 8 S - 1 to 9 S (neither boundary a multiple of S); one emitter of
    another id in the stripe (the emissive-id clause), and NaN colours on kept, emissive and missed low pixels."""
    lo, ss = flat_pair(Wd=S * Wo, Hd=S * Ho, w=13, h=8)
    for planes, emit, miss in ((lo, (4, 5), (5, 6)), (ss, (6 * S + 1, 8 * S - 1), (8 * S - 1, 9 * S + 1))):
        fl = planes[-1][..., 3].view(U)
        fl[:, emit[0]:emit[1]] = um.HIT | um.EMISSIVE
        fl[:, miss[0]:miss[1]] = 0
        planes[-3][:, miss[0]:miss[1], 3] = np.full(1, 0xffffffff, dtype=U).view(F)
    ss[0][S * 3 + 1, 6 * S + 1:8 * S - 1, 3] = np.full(1, 55, dtype=U).view(F)      # an emitter no low emitter has the id of
    lo[0][3, 3:7, 1] = np.nan
    return lo, ss


# ---- on three contexts -----------------------------------------------------------------------------------
PARAMS = dict(sigma_plane=0.02, normal_power_log2=3)
S3 = 2


def triple(scene, spp=8, chunks=1, out=(W, H), low=(LW, LH), S=S3):
    hi, lo, ss = pa.Pathtracer(*out), pa.Pathtracer(*low), pa.Pathtracer(S * out[0], S * out[1])
    cam = hi.load_scene(scene)
    lo.load_scene(scene)
    ss.load_scene(scene)
    lo.render(cam, spp, True, chunks=chunks)
    return hi, lo, ss, cam, ss.features(cam)["planes"], lo.features(cam)["planes"]


@pytest.fixture(scope="module", params=["cornell", "textured"])
def contexts(request, gpu_available, scenes, textured_scene):
    scene = str(scenes / "cornell_box.scene.json") if request.param == "cornell" else textured_scene
    return triple(scene) + (scene,)


def test_every_source_equals_the_model_and_all_three_render_states_stay(contexts):
    hi, lo, ss, cam, ss_planes, lo_planes, scene = contexts
    hi.render(cam, 2, True)                                          # render states on the other two contexts too
    ss.render(cam, 1, True)
    assert N.hip().pt_holds_upsampled(hi._ctx) == 0                  # hi has neither planes nor an upsampled image yet
    states = [render_state(p) for p in (hi, lo, ss)]

    def check(source, color, what, **kw):
        got = hi.upsample(lo, planes=ss, source=source, **PARAMS, **kw)
        flags = (1 if kw.get("demodulate", True) else 0) | (2 if kw.get("same_primitive", True) else 0)
        lows = [color] + list(lo_planes)
        want, counts = rm.model(lows, ss_planes, S3, PARAMS["sigma_plane"], PARAMS["normal_power_log2"], flags)
        assert got.shape == (H, W, 4)
        assert um.same_words(got, want), what + ": " + first_difference(got, want)
        assert hi.upsample_counts() == {"wide": counts[0], "nearest": counts[1]}, what
        image, n = device(lows, ss_planes, S3, PARAMS["sigma_plane"], PARAMS["normal_power_log2"], flags)
        assert um.same_words(hi.upsampled(), image) and n == counts, what + ": the image form"
        for p, before, name in zip((hi, lo, ss), states, ("hi", "lo", "planes")):
            assert_same_state(render_state(p), before, f"{what}, {name}")
        return got

    hdr = lo.get_hdr_image_data()
    out = check("accum", hdr, "accum")
    assert N.hip().pt_holds_upsampled(hi._ctx) == 1
    assert N.hip().pt_holds_upsampled(lo._ctx) == 0 and N.hip().pt_holds_upsampled(ss._ctx) == 0
    t = hi.upsample_timing()
    assert t["prepare"] > 0 and t["upsample"] > 0
    assert hi.tonemap_upsampled().shape == (H, W, 4)
    for staging in (1, 2):
        assert um.same_words(hi.upsample(lo, planes=ss, staging=staging, **PARAMS), out)
    check("accum", hdr, "accum, flags 1", same_primitive=False)
    check("accum", hdr, "accum, flags 2", demodulate=False)
    quarter = (lo.accum() * (F(1) / F(4))).astype(F)
    check("accum", quarter, "accum over 4 frames", frames=4)
    despiked = lo.despike()
    states[1] = render_state(lo)
    check("despiked", despiked, "despiked")
    denoised = lo.denoise(source="despiked", iterations=2, sigma_color=0.5)
    check("denoised", denoised, "denoised")
    temporal = lo.temporal(reset=True)
    check("temporal", temporal, "temporal")
    assert um.same_words(lo.despiked(), despiked) and um.same_words(lo.denoised(), denoised)   # nothing of lo ended
    # the one-sample call on the same context serves the same readers afterwards, and the other way round
    hi.features(cam)
    single = hi.upsample(lo, **PARAMS)
    assert not um.same_words(single, out)
    assert um.same_words(hi.upsample(lo, planes=ss, **PARAMS), out)


def test_refusals_change_nothing(gpu_available, scenes):
    scene = str(scenes / "cornell_box.scene.json")
    hi, lo, ss = pa.Pathtracer(W, H), pa.Pathtracer(LW, LH), pa.Pathtracer(2 * W, 2 * H)
    cam = hi.load_scene(scene)
    for p in (lo, ss):
        p.load_scene(scene)
    lib = N.hip()
    lo.render(cam, 2, True)
    hi.render(cam, 1, True)
    ss.render(cam, 1, True)
    states = [render_state(p) for p in (hi, lo, ss)]                 # (a features call touches nothing of them)

    def states_stay(what):
        assert lib.pt_holds_upsampled(hi._ctx) == 0
        refused(N.PT_ERR_STATE, "no upsampled image", hi.upsampled)
        for p, before, name in zip((hi, lo, ss), states, ("hi", "lo", "planes")):
            assert_same_state(render_state(p), before, f"{what}, {name}")

    refused(N.PT_ERR_STATE, "planes has no feature planes", hi.upsample, lo, planes=ss)
    states_stay("planes not current on planes")
    ss.features(cam)
    refused(N.PT_ERR_STATE, "lo has no feature planes", hi.upsample, lo, planes=ss)
    states_stay("planes not current on lo")
    lo.features(cam)
    for source in ("denoised", "temporal", "despiked"):
        refused(N.PT_ERR_STATE, f"no {source} image", hi.upsample, lo, planes=ss, source=source)
        states_stay(f"lo holds no {source} image")
    lo.temporal(reset=True)
    lo.features(cam)                                                 # the temporal image is no longer of lo's planes
    refused(N.PT_ERR_STATE, "no temporal image", hi.upsample, lo, planes=ss, source="temporal")
    states_stay("a temporal image of other planes")
    out = hi.upsample(lo, planes=ss)                                 # hi has no planes of its own
    counts = hi.upsample_counts()
    for p, before, name in zip((hi, lo, ss), states, ("hi", "lo", "planes")):
        assert_same_state(render_state(p), before, f"the accepted call, {name}")
    ok = pa.upsample_params()
    by = N.C.byref

    def said(word):
        return word in lib.pt_last_error(hi._ctx).decode()

    fields = ("sigma_plane", "normal_power_log2", "flags", "staging")
    good = dict(sigma_plane=0.005, normal_power_log2=3, flags=3, staging=0)
    for over in (dict(sigma_plane=0.0), dict(sigma_plane=float("nan")), dict(sigma_plane=float("inf")),
                 dict(normal_power_log2=8), dict(flags=4), dict(staging=3)):
        v = dict(good, **over)
        params = N.PtUpsampleParams(*[v[f] for f in fields])
        assert lib.pt_upsample_resolve(hi._ctx, ss._ctx, lo._ctx, 0, 1, 2, by(params)) == N.PT_ERR_ARG and said(list(over)[0]), over
    assert lib.pt_upsample_resolve(None, ss._ctx, lo._ctx, 0, 1, 2, by(ok)) == N.PT_ERR_ARG
    assert lib.pt_upsample_resolve(hi._ctx, None, lo._ctx, 0, 1, 2, by(ok)) == N.PT_ERR_ARG and said("planes is null")
    assert lib.pt_upsample_resolve(hi._ctx, ss._ctx, None, 0, 1, 2, by(ok)) == N.PT_ERR_ARG and said("lo is null")
    assert lib.pt_upsample_resolve(hi._ctx, ss._ctx, lo._ctx, 0, 1, 2, None) == N.PT_ERR_ARG and said("params is null")
    assert lib.pt_upsample_resolve(hi._ctx, ss._ctx, lo._ctx, 4, 1, 2, by(ok)) == N.PT_ERR_ARG and said("source")
    for factor in (0, 1, 5):
        assert lib.pt_upsample_resolve(hi._ctx, ss._ctx, lo._ctx, 0, 1, factor, by(ok)) == N.PT_ERR_ARG and said("factor must be")
    # planes that are not exactly factor x hi: another factor, and one dimension off
    assert lib.pt_upsample_resolve(hi._ctx, ss._ctx, lo._ctx, 0, 1, 3, by(ok)) == N.PT_ERR_ARG and said("not factor x hi")
    odd = pa.Pathtracer(2 * W, 2 * H + 1)
    odd.load_scene(scene)
    odd.features(cam)
    refused(N.PT_ERR_ARG, "not factor x hi", hi.upsample, lo, planes=odd)
    refused(N.PT_ERR_ARG, "factor must be", hi.upsample, lo, planes=hi)          # 1 x
    # lo larger than hi in either dimension
    wide = pa.Pathtracer(W + 8, LH)
    wide.load_scene(scene)
    wide.features(cam)
    wide.render(cam, 1, True)
    refused(N.PT_ERR_ARG, "larger", hi.upsample, wide, planes=ss)
    tall = pa.Pathtracer(LW, H + 8)
    tall.load_scene(scene)
    tall.features(cam)
    tall.render(cam, 1, True)
    refused(N.PT_ERR_ARG, "larger", hi.upsample, tall, planes=ss)
    # band partitions on any of the three
    for shape, name in (((W, H), "hi"), ((2 * W, 2 * H), "planes"), ((LW, LH), "lo")):
        bands = pa.Pathtracer(*shape, band_rows=8, row_offset=1, row_stride=2)
        bands.load_scene(scene)
        bands.render(cam, 1, True)
        bands.features(cam)
        trio = {"hi": hi, "planes": ss, "lo": lo}
        trio[name] = bands
        refused(N.PT_ERR_ARG, f"{name} holds a band partition", trio["hi"].upsample, trio["lo"], planes=trio["planes"])
    if pa.device_count() > 1:
        other = pa.Pathtracer(2 * W, 2 * H, device=1)
        other.load_scene(scene)
        other.features(cam)
        refused(N.PT_ERR_ARG, "different devices", hi.upsample, lo, planes=other)
    def nothing_changed(what, trio):
        assert um.same_words(hi.upsampled(), out) and hi.upsample_counts() == counts and lib.pt_holds_upsampled(hi._ctx) == 1
        for p, before, name in trio:
            assert_same_state(render_state(p), before, f"{what}, {name}")

    nothing_changed("refused calls", zip((hi, lo, ss), states, ("hi", "lo", "planes")))
    # a scene set on planes: its planes are no longer current
    ss.load_scene(scene)
    refused(N.PT_ERR_STATE, "planes has no feature planes", hi.upsample, lo, planes=ss)
    nothing_changed("refused for the state", zip((hi, lo), states, ("hi", "lo")))


def test_host_layer_and_cli(gpu_available, scenes, tmp_path):
    from PIL import Image
    scene = scenes / "cornell_box.scene.json"
    Wc, Hc = 64, 64
    hi, lo, ss, cam, _, _ = triple(str(scene), spp=8, out=(Wc, Hc), low=(32, 32))
    host = N.host()
    want = hi.upsample(lo, planes=ss)                                # the Python path at the defaults
    ldr, counts = hi.tonemap_upsampled(), hi.upsample_counts()
    hi.render(cam, 1, True)
    assert not um.same_words(want, hi.get_hdr_image_data())         # the host layer has not upsampled yet
    params = pa.upsample_params()
    n = (N.C.c_uint32 * 2)()
    N.check_host(host.pth_renderer_upsample_resolve(hi._r, ss._r, lo._r, 0xffffffff, N.C.byref(params)))
    N.check_host(host.pth_renderer_upsample_counts(hi._r, n))
    assert {"wide": n[0], "nearest": n[1]} == counts
    assert um.same_words(hi.get_hdr_image_data(), want) and np.array_equal(hi.get_image_data(), ldr)
    # the automatic source is what lo's image calls return
    ds = pa.despike_params()
    N.check_host(host.pth_renderer_despike(lo._r, N.C.byref(ds)))
    N.check_host(host.pth_renderer_upsample_resolve(hi._r, ss._r, lo._r, 0xffffffff, N.C.byref(params)))
    assert um.same_words(hi.get_hdr_image_data(), hi.upsample(lo, planes=ss, source="despiked"))
    params.staging = 3
    assert host.pth_renderer_upsample_resolve(hi._r, ss._r, lo._r, 0, N.C.byref(params)) == N.PT_ERR_ARG
    assert "staging" in host.pth_last_error().decode()
    assert host.pth_renderer_upsample_resolve(hi._r, None, lo._r, 0, N.C.byref(params)) == N.PT_ERR_ARG
    params.staging = 0
    assert host.pth_renderer_upsample_resolve(hi._r, lo._r, lo._r, 0, N.C.byref(params)) == N.PT_ERR_ARG     # planes of 1/2 x
    assert "factor" in host.pth_last_error().decode()
    hi.render(cam, 1, True)                                          # the next render returns the image calls to the accumulation
    assert um.same_words(hi.get_hdr_image_data(), hi.accum())
    # the CLI: the same launches through the same C++ path, written at the full size
    base = [str(N.CLI), "-w", str(Wc), "-h", str(Hc), "-spp", "8", "-upsample", "2", "-upsample_aa", "2"]
    png = tmp_path / "resolved.png"
    r = subprocess.run(base + ["-o", str(png), str(scene)], capture_output=True, text=True, timeout=120)
    line = f"Upsampled: {Wc} x {Hc} from 32 x 32, {counts['wide']} samples from the wider ring, {counts['nearest']} from the nearest pixel"
    assert r.returncode == 0 and line in r.stdout and "Antialiased: 2 x 2 first-hit samples per pixel" in r.stdout, r.stdout + r.stderr
    assert np.array_equal(np.asarray(Image.open(png).convert("RGBA")), ldr[::-1])
    png2 = tmp_path / "resolved_filtered.png"
    r = subprocess.run(base[:-1] + ["3", "-despike", "-denoise", "3", "-o", str(png2), str(scene)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "Despiked:" in r.stdout and "Denoised: 3" in r.stdout and "Antialiased: 3 x 3" in r.stdout, r.stdout + r.stderr
    assert Image.open(png2).size == (Wc, Hc)


MIN_EDGE_PIXELS = 200


def test_it_antialiases(gpu_available, scenes):
    """On the Cornell box: output 64 x 64, low image 32 x 32 at 256 spp, planes 128 x 128 (S = 2), reference 64 x 64 at
    1,024 spp.  Edge pixels are the output pixels whose 2 x 2 sub-pixel ids are not all equal.  The tonemapped MSE of the
    resolved result is below that of pt_upsample's one-sample result from the same low image over the edge pixels, and
    not above it over all pixels.  The measured values, and bilinear's, are in DESIGN.md 5.16."""
    Wo, Ho, S = 64, 64, 2
    hi, lo, ss, cam, ss_planes, _ = triple(str(scenes / "cornell_box.scene.json"), spp=8, chunks=32, out=(Wo, Ho), low=(32, 32), S=S)
    resolved = hi.upsample(lo, planes=ss)
    hi.features(cam)
    single = hi.upsample(lo)
    low = lo.get_hdr_image_data()
    hi.render(cam, 8, True, chunks=128)
    ref = hi.get_hdr_image_data()
    plain = um.bilinear(low, Wo, Ho)
    ids = ss_planes[0][..., 3].view(U).reshape(Ho, S, Wo, S)
    edge = (ids != ids[:, :1, :, :1]).any(axis=(1, 3))
    everywhere = np.ones_like(edge)

    def mse(img, where):
        return float(((tonemapped(img) - tonemapped(ref)) ** 2)[where].mean())

    e = {name: (mse(img, edge), mse(img, everywhere)) for name, img in (("resolved", resolved), ("one sample", single),
                                                                         ("bilinear", plain))}
    message = (f"tonemapped MSE over {int(edge.sum())} edge pixels / all {Wo * Ho}: "
               + ", ".join(f"{k} {a:.6f} / {b:.6f}" for k, (a, b) in e.items()) + f"; counts {hi.upsample_counts()}")
    print(message)
    assert edge.sum() >= MIN_EDGE_PIXELS, message
    assert e["resolved"][0] < e["one sample"][0], message
    assert e["resolved"][1] <= e["one sample"][1], message
