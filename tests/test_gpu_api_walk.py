"""The render API walked in seeded random order on the GPU, against the oracle and the model of
tests/api_walk.py after every step: accumulation and XORWOW state bit for bit, the frame counter, the
adaptive flag and every refusal (code and a word of the message) against the model, moments and counts
against AdaptiveOracle while they describe the buffer, both image reads in the arithmetic the model
selects, the primitive plane after a features call against the twin-scene oracle, and a denoise against
tests/denoise_model.py.  One test per seed; a failure names the seed, the step, the call and the three
calls before it, with the kernel variant and launch of every step so that the walk can be replayed by hand.

Measured on MI355X, per seed of 40 steps (pytest --durations, the oracle's side included): 0.37 s for the
first seed (1984), 0.05 to 0.10 s for the others; 1.5 s once for creating the first context.
"""
import ctypes as C

import numpy as np
import pytest

import api_walk as aw
import denoise_model as dm
import pathtracercuda_amd as pa
from pathtracercuda_amd import _native as N
from test_gpu_parity import assert_bitexact

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_available():
    if pa.device_count() < 1:
        pytest.skip("no GPU")


def tile_costs(pt):
    try:
        return pt.tile_costs()
    except pa.PathtracerError as e:          # no launch yet
        return e.code


def call(pt, st, oracle, op, scenes):
    """One call on the device; returns what a denoise gives: (result, sigma used or None)."""
    k, a, cam = op.kind, op.args, st["cam"]
    if k == "render":
        pt.render(cam, a["spp"], a["ignore"], chunks=a["chunks"])
    elif k == "render_raw":
        pt.render_raw(cam, a["spp"], a["chunks"], a["ignore"])
    elif k == "adaptive":
        pt.render_adaptive(cam, a["spp"], a["min_calls"], a["max_calls"], a["tolerance"], aw.ADAPTIVE_FLOOR, a["reset"])
    elif k == "features":
        st["planes"] = pt.features(cam)
    elif k == "denoise" and not a["host"]:
        return pt.denoise(sigma_color=a["sigma"], **aw.DENOISE), None
    elif k == "denoise":
        params = pa.denoise_params(sigma_color=1.0 if a["sigma"] is None else a["sigma"], **aw.DENOISE)
        used = C.c_float(0.0)
        N.check_host(N.host().pth_renderer_denoise(pt._r, C.byref(params), int(a["sigma"] is None), C.byref(used)))
        return pt.denoised(), float(used.value)
    elif k == "camera":
        (pa.camera_rotate if a["how"] == "rotate" else pa.camera_translate)(cam, a["x"], a["y"], a["z"])
    elif k == "rng":
        pt.set_rng_state(pt.rng_state())
    elif k == "scene":
        st["cam"] = pt.load_scene(str(scenes / f"{a['name']}.scene.json"))
    elif k == "texture":
        tex = np.tile(np.array(a["texel"], dtype=np.float32), (4, 4, 1))
        N.check_ctx(N.hip().pt_set_texture(pt._ctx, oracle.texture_handle(a["slot"]), tex.ctypes.data_as(C.POINTER(C.c_float)),
                                           4, 4), pt._ctx)
    elif k == "variant":
        pt.set_kernel_variant(a["variant"])
    elif k == "run_ahead":
        pt.set_run_ahead(a["mode"])
    elif k == "groups":
        pt.set_sample_groups(a["mode"])
    elif k == "knob":
        if a["which"] == "cold_start":
            pt.set_cold_start(*a["value"])
        else:
            getattr(pt, "set_" + a["which"])(a["value"])
    return None


def check_state(pt, st, model, oracle):
    assert_bitexact(pt.accum(), oracle.accum, "accum")
    assert np.array_equal(pt.rng_state(), oracle.rng_array()), "RNG streams diverged"
    assert (pt.frames, pt.adaptive) == (model.frames, model.adaptive), "frames, adaptive"
    if model.counts_valid:
        assert dm.same_words(pt.moments(), oracle.ad.moments()), "moments"
        assert np.array_equal(pt.sample_counts(), oracle.ad.n), "sample counts"
    else:
        with pytest.raises(pa.PathtracerError) as e:
            pt.moments()
        assert e.value.code == N.PT_ERR_STATE
    # the image reads never raise: the model has an arithmetic for every state
    how = model.image()
    hdr, ldr = pt.get_hdr_image_data(), pt.get_image_data()
    if how == "denoised":
        want_hdr, want_ldr = st["denoised"], oracle.tonemap_denoised(st["denoised"])
    else:
        want_hdr, want_ldr = oracle.image(how, model.frames)
    assert dm.same_words(hdr, want_hdr), f"get_hdr_image_data is not the '{how}' image"
    assert np.array_equal(ldr, want_ldr), f"get_image_data is not the '{how}' image"


def step(pt, st, model, oracle, op, scenes):
    want = model.outcome(op)
    before = (pt.accum(), pt.rng_state(), tile_costs(pt), pt.last_variant) if op.kind == "features" else None
    handle_planes = st["planes"]
    err = result = None
    try:
        result = call(pt, st, oracle, op, scenes)
    except pa.PathtracerError as e:
        err = e
    if want.code:
        assert err is not None, f"the model expects error {want.code} ('{want.word}'); the call succeeded"
        assert err.code == want.code and want.word in str(err), f"the model expects error {want.code} ('{want.word}'): {err}"
        st["planes"] = handle_planes
    else:
        assert err is None, f"the model expects success: {err}"
        color = oracle.image(model.color(), model.frames)[0] if op.kind == "denoise" else None
        model.apply(op, bytes(st["cam"]))
        oracle.apply(op)
        assert bytes(st["cam"]) == bytes(oracle.camera), "camera"
        if op.kind == "features":
            prim, hit, emissive = oracle.first_hit()
            f = st["planes"]
            assert np.array_equal(f["primitive"], prim), f"{(f['primitive'] != prim).sum()} pixels name another primitive"
            assert np.array_equal(f["hit"], hit) and np.array_equal(f["emissive"], emissive), "flags"
            assert np.array_equal(dm.bits(pt.accum()), dm.bits(before[0])) and np.array_equal(pt.rng_state(), before[1])
            assert np.array_equal(tile_costs(pt), before[2]) and pt.last_variant == before[3], "features moved the render state"
        if op.kind == "denoise":
            out, used = result
            planes = st["planes"]["planes"]
            sigma = op.args["sigma"]
            if sigma is None:
                sigma = pa.auto_sigma_color(color, *planes, demodulate=aw.DENOISE["demodulate"])
                if used is not None:         # the host layer's statistic: the same, summed in another order
                    assert used == pytest.approx(sigma, rel=1e-5), "automatic sigma"
                    sigma = used
            st["denoised"] = oracle.denoise(color, planes, sigma)
            assert dm.same_words(out, st["denoised"]), "denoise is not the model's filter of the current image"
            assert np.array_equal(pt.tonemap_denoised(), oracle.tonemap_denoised(st["denoised"])), "tonemap_denoised"
    check_state(pt, st, model, oracle)


@pytest.mark.parametrize("seed", aw.SEEDS)
def test_walk(gpu_available, scenes, seed):
    cfg = aw.CONFIGS[seed]
    ops = aw.generate(seed)
    pt = pa.Pathtracer(cfg.width, cfg.height, band_rows=cfg.band_rows, row_offset=cfg.row_offset, row_stride=cfg.row_stride)
    st = {"cam": pt.load_scene(str(scenes / f"{aw.START_SCENE}.scene.json")), "planes": None, "denoised": None}
    model, oracle = aw.Model(cfg.band_rows == 1), aw.OracleWalk(scenes, cfg)
    assert bytes(st["cam"]) == bytes(oracle.camera)
    check_state(pt, st, model, oracle)
    launches = []
    for i, op in enumerate(ops):
        try:
            step(pt, st, model, oracle, op, scenes)
        except (AssertionError, pa.PathtracerError) as e:
            try:                             # of the failing step too: it is the one to replay
                launches.append((pt.last_variant, pt.last_launch))
            except pa.PathtracerError as again:
                launches.append(("unreadable", str(again)))
            earlier = "\n".join(f"  step {j}: {aw.describe(ops[j])}" for j in range(max(0, i - 3), i))
            trail = "\n".join(f"  step {j}: variant {v}, launch {l}" for j, (v, l) in enumerate(launches))
            raise AssertionError(f"seed {seed}, step {i}: {aw.describe(op)}: {e}\nthe steps before it:\n{earlier}\n"
                                 f"last_variant and last_launch after every step:\n{trail}") from e
        launches.append((pt.last_variant, pt.last_launch))
