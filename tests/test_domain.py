"""The oracle and the host layer against the reference's own source over the whole accepted input
range (DESIGN.md §3 "Input domain"): the directed scenes and the seeded random scenes of
tests/domain_scenes.py, checked the way tests/test_ref_source.py checks its scenes.

Build products are byte-equal across reference source, oracle and host layer.  render(4, True) then
render(4, False) agree between reference source and oracle under same_bits_or_both_nan (an x86
NaN's sign depends on the operand order the compiler picked, see test_nan_signs_differ_somewhere);
RNG states and tonemapped bytes are strictly equal.  What a scene claims to contain -- NaN, negative
and infinite pixels -- is judged from the reference's output alone.
"""
import collections

import numpy as np
import pytest

import domain_scenes as ds
import pathtracercuda_amd as pa
from oracle import pyoracle as po
from oracle import pyref as pr
from test_ref_source import as_bytes, oracle_objects, same_bits

DIRECTED = list(ds.DIRECTED)


@pytest.fixture(scope="module", autouse=True)
def ref_library():
    if not pr.available():
        if pr.reference_tree() is None:
            pytest.skip("neither oracle/_ref/libptref.so nor a checkout of the reference to build it from")
        pytest.fail(f"the reference is at {pr.reference_tree()} but {pr.LIB_PATH} is not built: run `make`")
    return pr.lib()


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("domain_scenes")


def check_build_products(path, W, H, what):
    """test_ref_source.test_build_products: reference source == oracle == host layer."""
    ref = pr.load_scene(path, W, H)
    osc = po.load_scene(path, W, H)
    n = ref.count
    assert ref.validate(), what
    rh, ra = ref.objects()
    oh, oa = oracle_objects(osc)
    same_bits(rh, oh, f"{what}: hittables, oracle")
    same_bits(ra, oa, f"{what}: boxes, oracle")
    rn, rp, _ = ref.bvh()
    assert n == len(osc.cpu) and ref.node_count == osc.node_count, what
    same_bits(rn, as_bytes(osc.nodes, osc.node_count, 32), f"{what}: BVH nodes, oracle")
    same_bits(rp, as_bytes(osc.prims, n, 96), f"{what}: BVH-order hittables, oracle")
    assert bytes(ref.camera) == bytes(osc.camera), f"{what}: camera, oracle"
    refused = ds.refused_by_loader(path)
    if refused is not None:
        # a non-finite inverse transform (zero scale): the host layer refuses the file by name, and the
        # refusal is exactly the objects whose hittable the reference builds with inf or NaN rows
        rows = rh[:, :48].view(np.float32)
        assert not np.isfinite(rows[refused]).all() and np.isfinite(rows[:refused]).all(), what
        with pytest.raises(pa.PathtracerError, match=rf"objects\[{refused}\]\.scale = .*inverse transform is not finite"):
            pa.Scene(path, W, H)
        return ref, osc
    assert np.isfinite(rh[:, :48].view(np.float32)).all(), f"{what}: accepted with a non-finite inverse transform"
    host = pa.Scene(path, W, H)
    assert n == host.object_count, what
    hobjs, ha = host.objects()
    same_bits(rh, as_bytes(hobjs, n, 96), f"{what}: hittables, host layer")
    same_bits(ra, ha, f"{what}: boxes, host layer")
    assert ref.node_count == host.node_count, what
    assert ref.depth() == host.bvh_depth, what
    hn, hp = host.bvh()
    same_bits(rn, as_bytes(hn, host.node_count, 32), f"{what}: BVH nodes, host layer")
    same_bits(rp, as_bytes(hp, n, 96), f"{what}: BVH-order hittables, host layer")
    assert bytes(ref.camera) == bytes(host.camera()), f"{what}: camera, host layer"
    assert ref.inputs.skybox == osc.skybox == host.skybox, what
    return ref, osc


def check_render(ref, osc, W, H, what, seed=None, path=None):
    """render(4, True) then render(4, False): (the reference's, the oracle's) accumulation after each."""
    rr = pr.RefRenderer(ref, W, H)
    orr = po.OracleRenderer(osc, W, H)
    same_bits(rr.rng_array(), orr.rng_array(), f"{what}: initRandState")
    out = []
    for ignore in (True, False):
        rr.render(ref.camera, 4, ignore)
        orr.render(osc.camera, 4, ignore)
        ds.same_bits_or_both_nan(rr.accum, orr.accum, f"{what}: accumulation after render(4, {ignore})", seed, path)
        same_bits(rr.rng_array(), orr.rng_array(), f"{what}: RNG state after render(4, {ignore})")
        out.append((rr.accum.copy(), orr.accum.copy()))
    assert np.array_equal(rr.tonemap(), orr.tonemap()), f"{what}: tonemap"
    return out


_directed = {}


@pytest.fixture(scope="module")
def directed(scene_dir):
    """name -> [(reference accumulation, oracle accumulation) after each of the two renders]; every
    scene is built, compared and rendered once per module."""
    def get(name):
        if name not in _directed:
            path = ds.directed_scene(scene_dir, name)
            ref, osc = check_build_products(path, ds.W, ds.H, name)
            _directed[name] = check_render(ref, osc, ds.W, ds.H, name)
        return _directed[name]
    return get


@pytest.mark.parametrize("name", DIRECTED)
def test_directed_scene(directed, name):
    directed(name)


def rgb(directed, name):
    return directed(name)[1][0][..., :3]          # the reference's accumulation after both renders


def test_high_roughness_scenes_hold_nan(directed):
    # NdotV^2 (1 - a2) + a2 < 0 under sqrtf: NaN pixels above roughness ~14.95 and none at the twin below
    for name in ds.ROUGH_NAN:
        nan = int(np.isnan(rgb(directed, name)).any(-1).sum())
        print(f"{name}: {nan} NaN pixels")
        assert nan > 0, f"{name}: no NaN pixel in the reference's output"
    for name in ("rough_normal_16", "rough_normal_64"):
        assert np.isnan(rgb(directed, name)).any(-1).mean() > 0.5, name
    for name in ("rough_normal_14", "rough_spheres_2"):
        assert not np.isnan(rgb(directed, name)).any(), f"{name}: NaN in the reference's output"


def test_out_of_range_colours_show(directed):
    assert (rgb(directed, "metal_out") < 0).any(-1).sum() > 100, "metal_out: few negative pixels"
    b = rgb(directed, "base_out")
    assert np.isinf(b).any() and np.isnan(b).any() and (b < 0).any(), "base_out: inf, NaN and negative pixels"
    assert np.isinf(rgb(directed, "sky_bright")).any(), "sky_bright: no infinite pixel"
    for name in ("cam_lookat_eq", "cam_along_up"):
        assert np.isnan(rgb(directed, name)).all(), f"{name}: a pixel that is not NaN"
    assert np.isnan(rgb(directed, "domain_combined")).any() and np.isfinite(rgb(directed, "domain_combined")).any()


def test_nan_signs_differ_somewhere(directed):
    # why the NaN rule exists: with a zero scale the reference's source and the oracle produce NaNs of
    # opposite sign in the same words (the operand order of an x86 addss/mulss decides which operand's
    # NaN, or the default NaN with its sign bit set, comes out)
    with_nan, differ = [], 0
    for name in ds.ZERO_SCALE:
        r, o = directed(name)[1]
        if np.isnan(r).any():
            with_nan.append(name)
        differ += ds.nan_signs_differ(r, o)
    print(f"zero-scale scenes with NaN: {with_nan}; NaN words of differing sign: {differ}")
    assert np.isnan(rgb(directed, "scale_zero_SPHERE")).any()
    assert differ > 0, "no zero-scale scene has NaN words whose bits differ between reference and oracle"


_random = {}


def random_set(scene_dir):
    """Every seed of SEEDS_CPU built, compared and rendered once: per-seed reference accumulation, and
    the generator's count of drawn edge values."""
    if not _random:
        draws = collections.Counter()
        acc = {}
        for seed in ds.SEEDS_CPU:
            path = ds.random_scene(scene_dir, seed, draws)
            what = f"random seed {seed} ({path})"
            ref, osc = check_build_products(path, ds.RW, ds.RH, what)
            acc[seed] = check_render(ref, osc, ds.RW, ds.RH, what, seed, path)[1][0]
            if ds.refused_by_loader(path) is not None:       # refused: the host layer on what is left of it
                rest = ds.without_refused_objects(path)
                if rest is not None:
                    assert ds.refused_by_loader(rest) is None
                    check_build_products(rest, ds.RW, ds.RH, f"{what}, accepted objects")
        _random.update(acc=acc, draws=draws)
    return _random


def test_random_scenes(scene_dir):
    # no scene of the seed range aborts the reference (an abort ends this process), and all agree
    assert len(random_set(scene_dir)["acc"]) == len(ds.SEEDS_CPU)


def test_random_set_is_not_vacuous(scene_dir):
    r = random_set(scene_dir)
    n = len(r["acc"])
    lit = sum(bool((np.isfinite(a[..., :3]) & (a[..., :3] != 0)).any()) for a in r["acc"].values())
    nan = sum(bool(np.isnan(a[..., :3]).any()) for a in r["acc"].values())
    print(f"{n} seeds: {lit} with a finite non-zero pixel, {nan} with a NaN word")
    assert lit >= 0.8 * n, f"{lit} of {n} scenes have a finite non-zero pixel"
    assert nan >= 0.25 * n, f"{nan} of {n} scenes contain a NaN word"
    missing = [k for k in ds.every_edge_value() if r["draws"][k] == 0]
    assert not missing, f"edge values never drawn: {missing}"


def test_loader_refuses_a_non_finite_inverse_transform(scene_dir):
    # the bound comes from the expression: 1 / s is a finite float32 iff |s| > 2^-128 (2.9387e-39)
    import json

    def load(shape, scale):
        p = scene_dir / "bound.json"
        p.write_text(json.dumps({"camera": ds.cam(*ds.STD_CAM), "skybox": "", "objects": [ds.floor(), ds.obj(shape, scale=scale)]}))
        return pa.Scene(p, 8, 8), ds.refused_by_loader(p)
    for shape, scale in (("SPHERE", (0.0, 1.0, 1.0)), ("CUBE", (1.0, -0.0, 1.0)), ("CONE", (1.0, 1.0, 2.93e-39)),
                         ("QUAD", (0.0, 1.0, 1.0)), ("DISK", (1.0, 1.0, 0.0))):
        with pytest.raises(pa.PathtracerError, match=r"objects\[1\]\.scale = .*larger in magnitude than 2\^-128") as e:
            load(shape, scale)
        assert e.value.code == pa._native.PT_ERR_ARG and ds.refused_by_loader(scene_dir / "bound.json") == 1
    # exactness just inside the bound, and a flat shape's unused y scale
    for shape, scale in (("CONE", (1.0, 1.0, 2.95e-39)), ("SPHERE", (1e-6, 1e-6, 1e-6)), ("QUAD", (1.0, 0.0, 1.0)),
                         ("DISK", (1.0, 0.0, 1.0))):
        host, refused = load(shape, scale)
        assert refused is None
        ref = pr.load_scene(scene_dir / "bound.json", 8, 8)
        same_bits(ref.objects()[0], as_bytes(host.objects()[0], 2, 96), f"{shape} {scale}: hittables, host layer")


def test_comparison_rule():
    nan_p, nan_n = np.uint32(0x7fc00000), np.uint32(0xffc00000)
    a = np.array([[[1.0, 0.0, -0.0, 2.0]]], dtype=np.float32)
    b = a.copy()
    a.view(np.uint32)[0, 0, 3], b.view(np.uint32)[0, 0, 3] = nan_p, nan_n
    ds.same_bits_or_both_nan(a, b, "NaNs of either sign")
    assert ds.nan_signs_differ(a, b) == 1
    b[0, 0, 1] = -0.0                                        # zeros of different sign are different words
    with pytest.raises(AssertionError, match="seed 7; scene x.json"):
        ds.same_bits_or_both_nan(a, b, "signed zero", 7, "x.json")
    b[0, 0, 1], b[0, 0, 3] = 0.0, 1.0                        # NaN against a number
    with pytest.raises(AssertionError, match=r"pixel \(row, x\) = \(0, 0\)"):
        ds.same_bits_or_both_nan(a, b, "NaN against a number")
