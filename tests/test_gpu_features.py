"""First-hit feature buffers (pt_render_features) against the unmodified oracle, exactly.

The pass traces the ray of each pixel's first sample of a reset render, so OracleRenderer.render(cam, 1, True)
follows the same ray.  A TWIN scene -- same primitives and BVH, every material replaced by LAMBERT with base
colour 0 and emission e_i -- makes the oracle's getColor return e_i of the first primitive hit and stop
(emission is added at the hit, diffuse_lambert(0) is 0 and ends the path), or 0 on a miss:
  e_i = (i + 1, 0, 0)        -> the primitive index of plane 0, and HIT
  e_i = the albedo of i      -> plane 0's colour
A textured material's albedo varies over the surface, so every texture is replaced by one whose texels
are all (0.5, 0.25, 0.75): bilinear weights are multiples of 2^-16 and the sum of weight x texel is exact,
so the lookup returns the texel for every (u, v); the expected albedo is pm_powf of or_tex2d's value.
"""
import ctypes as C

import numpy as np
import pytest

import pathtracercuda_amd as pa
import size_scenes as ss
from first_hit import first_hits, twin  # noqa: F401  (test_gpu_features_geometry imports them from here)
from oracle import pyoracle as po
from pathtracercuda_amd import _native as N
from test_gpu_parity import _set_caller_bvh

pytestmark = pytest.mark.gpu

TEXEL = (0.5, 0.25, 0.75, 1.0)


@pytest.fixture(scope="module")
def gpu_available():
    if pa.device_count() < 1:
        pytest.skip("no GPU")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def constant_textures(pt, osc):
    """Every texture of the scene replaced by a 4 x 4 one of TEXEL, on the device and in the oracle scene."""
    tex = np.tile(np.array(TEXEL, dtype=np.float32), (4, 4, 1))
    for handle in range(1, len(osc.textures) + 1):
        N.check_ctx(N.hip().pt_set_texture(pt._ctx, handle, tex.ctypes.data_as(C.POINTER(C.c_float)), 4, 4), pt._ctx)
    osc.textures = [tex.copy() for _ in osc.textures]


def albedo_table(osc):
    """Per primitive: the base colour as shade forms it."""
    L = po.lib()
    out = np.zeros((osc.prim_count, 3), dtype=np.float32)
    table = osc.texture_table()
    for i in range(osc.prim_count):
        m = osc.prims[i].mat
        if m.textureIndex:
            rgba = (C.c_float * 4)()
            L.or_tex2d(C.byref(table[m.textureIndex - 1]), 0.3, 0.6, rgba)
            out[i] = [L.pm_powf(rgba[k], 2.2) for k in range(3)]
        else:
            out[i] = list(m.baseColor)
    return out


CASES = {
    "cornell": ("cornell_box", 64, 64, (1, 0, 1)),
    "shapes": ("test_shapes", 96, 64, (1, 0, 1)),
    "banded": ("test_shapes", 96, 64, (8, 1, 2)),
    # (a caller BVH without shell spheres around the camera: with them every ray ends on one shell)
    "caller_bvh": ("d_small", ss.IMAGE[0], ss.IMAGE[1], (1, 0, 1)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_primitive_albedo_and_flags_equal_the_oracle(gpu_available, scenes, tmp_path, case):
    name, W, H, (band, off, stride) = CASES[case]
    pt = pa.Pathtracer(W, H, band_rows=band, row_offset=off, row_stride=stride)
    if case == "caller_bvh":
        sc = ss.case(name)
        path = sc.write(tmp_path, name)
        osc = ss.oracle_scene(sc, path, W, H)
        cam = pt.load_scene(str(path))
        _set_caller_bvh(pt, osc, sc.nodes)
    else:
        path = scenes / f"{name}.scene.json"
        osc = po.load_scene(path, W, H)
        cam = pt.load_scene(str(path))
    assert bytes(cam) == bytes(osc.camera)
    constant_textures(pt, osc)
    n = osc.prim_count
    rng = pt.rng_state()
    f = pt.features(cam)
    # primitive index and HIT: emission (i + 1, 0, 0)
    ids = first_hits(osc, [(i + 1, 0, 0) for i in range(n)], W, H, (band, off, stride))[..., 0]
    assert (ids == np.round(ids)).all() and ids.max() <= n
    want = np.where(ids > 0, ids.astype(np.int64) - 1, 0xffffffff).astype(np.uint32)
    assert np.array_equal(f["primitive"], want), f"{(f['primitive'] != want).sum()} pixels name another primitive"
    hit = ids > 0
    assert np.array_equal(f["hit"], hit)
    assert 0.1 < hit.mean() and len(np.unique(want[hit])) >= min(n, 5)
    if case in ("shapes", "banded"):
        types = {int(osc.prims[int(i)].type) for i in np.unique(want[hit])}
        assert types == set(range(7)), f"shapes seen: {sorted(types)}"
    # albedo: emission = the albedo
    alb = albedo_table(osc)
    assert np.isfinite(alb).all()
    if case in ("shapes", "banded"):
        assert any(osc.prims[int(i)].mat.textureIndex for i in np.unique(want[hit])), "no textured primitive is seen"
    expect = first_hits(osc, alb, W, H, (band, off, stride))[..., :3]
    assert np.array_equal(bits(f["albedo"]), bits(expect))
    # EMISSIVE against the scene's materials
    em = np.array([any(v != 0 for v in osc.prims[i].mat.emissive) for i in range(n)])
    assert np.array_equal(f["emissive"], hit & em[np.where(hit, want, 0)])
    if case != "caller_bvh":
        assert f["emissive"].any()
    # a miss is all +0 with flags 0
    for k in range(3):
        p = f["planes"][k]
        assert (bits(p[..., :3])[~hit] == 0).all()
    assert (bits(f["planes"][1][..., 3])[~hit] == 0).all() and (bits(f["planes"][2][..., 3])[~hit] == 0).all()
    # hits carry a unit normal against the ray and a distance inside the walk's interval
    nrm, t = f["normal"][hit], f["depth"][hit]
    assert np.allclose(np.linalg.norm(nrm.astype(np.float64), axis=-1), 1.0, atol=1e-5) and (t > 0.001).all()
    # a second pass gives the same words, and the RNG buffer was neither read nor written
    g = pt.features(cam)
    for k in range(3):
        assert np.array_equal(bits(g["planes"][k]), bits(f["planes"][k]))
    assert np.array_equal(pt.rng_state(), rng)
    # the pass does not depend on what was rendered before it
    pt.render(cam, 2, True)
    g = pt.features(cam)
    for k in range(3):
        assert np.array_equal(bits(g["planes"][k]), bits(f["planes"][k]))


def test_band_partitions_compose_the_full_frame(gpu_available, scenes):
    W, H = 96, 64
    path = str(scenes / "test_shapes.scene.json")
    full = pa.Pathtracer(W, H)
    want = full.features(full.load_scene(path))["planes"]
    for i in range(2):
        part = pa.Pathtracer(W, H, band_rows=8, row_offset=i, row_stride=2)
        got = part.features(part.load_scene(path))["planes"]
        rows = np.array([y for y in range(H) if (y // 8) % 2 == i])
        for k in range(3):
            assert np.array_equal(bits(got[k]), bits(want[k][rows]))
