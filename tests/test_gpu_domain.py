"""GPU: the HIP megakernel against the reference's own source (oracle/_ref/libptref.so, loaded as
tests/test_gpu_ref_source.py loads it; the reference's tree is never read) over the whole accepted
input range: the directed scenes and 128 seeded random scenes of tests/domain_scenes.py.

An accepted input renders exactly as the reference or is refused by name; it is never silently
different (DESIGN.md §3 "Input domain").  Accumulation buffers and adaptive moments are compared
under domain_scenes.same_bits_or_both_nan; RNG states, tonemapped bytes and camera bytes strictly.

A scene whose inverse transforms are not finite (a zero scale) is refused by the loader and by
pt_set_scene, by name; the tests assert the refusal (domain_scenes.refused_by_loader says which).

Every index and loop bound of the kernel that depends on a scene float, read before these scenes
first ran on a device (NaN, infinite and huge values cannot index out of bounds or loop forever):
  * tex2d (pt_dev_scene.h): u - floorf(u) is in [0, 1] or NaN for any u (inf - inf = NaN, |u| >= 2^23
    gives 0), so fx is in [-1, w - 1] or NaN; the float -> int conversions sit behind |f| < 1e9 with
    the NaN case selecting 0 (column) and -1 (row), the column wraps by one conditional add or
    subtract into [0, w - 1] (w = 1: both columns 0), and the row is clamped into [0, h - 1] after the
    conversion.  The sky lookup and the material textures go through the same function; no other
    index is computed from u, v.
  * f2i_x86 (pt_math.h) is used by the tonemap kernel only, on a value that is first tested for NaN
    and afterwards masked to a byte as an integer; it indexes nothing.
  * the LDS stack: the walks push at most one entry per interior node on the path from the root, so
    the depth is bounded by the tree's depth, which pt_set_scene measures from the node array (not
    from any float) when it sizes stackDepth, and refuses trees it cannot hold.  A NaN or infinite box
    or ray changes which children are hit, never how deep the path is.  walk_interior's unconditional
    store above the top stays inside the column for the same reason.
  * the rise repair (repair_pending) descends from the root by comparing the leaf's first primitive
    index with Q3.w of each record: integers from pt_set_scene, which checks the DFS order they rely
    on; the loop ends at the leaf after at most depth steps, whatever the floats hold.  `rose =
    !(tMax <= tLeaf)` is true for a NaN t_max, so a lane whose t_max is NaN runs the repair after every
    leaf it tests: one bounded descent per leaf, and the leaves a traversal tests are bounded by the
    tree (each pending entry is popped once; a repair only rebuilds entries for subtrees not yet
    visited, to the right of the leaf's path).
  * a phase of the resumable walk that resumes with a NaN t_max takes NaN reciprocals and keeps them
    until the phase ends, also when a hit makes t_max a number again: every box then passes its slab
    test, the lane visits at most every node of the tree once, and the stack stays within the depth
    bound above, which holds for any hit pattern.
  * the leaf loops run `count` (an integer of the node word) times; the bounce loop ends at bounce 4
    whatever the throughput holds; the sample and call loops count integers.
  * sincos_pos converts x * (4 / pi) to int32: its operand is 2 pi u for a uniform u in (0, 1], never
    a scene float.
"""
import numpy as np
import pytest

import domain_scenes as ds
import pathtracercuda_amd as pa
from oracle import pyoracle as po
from oracle import pyref as pr
from pathtracercuda_amd import _native as N
from test_adaptive_rule import AdaptiveOracle
from test_gpu_ref_source import VARIANTS

pytestmark = pytest.mark.gpu

W, H = ds.W, ds.H
ADAPTIVE = dict(spp=4, min_calls=2, max_calls=4, tolerance=0.2, floor=0.01)
NAN_SCENES = ("rough_normal_16", "rough_spheres_1e10")     # NaN pixels beside finite ones; a zero-scale scene is refused
GROUP_VARIANTS = (40, 60)                                  # from tests/test_gpu_ssg.py


@pytest.fixture(scope="module", autouse=True)
def ref_library():
    if not pr.available():
        pytest.skip(f"{pr.LIB_PATH} is absent: it is built by `make` where a checkout of the reference is present")
    if pa.device_count() < 1:
        pytest.skip("no GPU")
    return pr.lib()


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("gpu_domain_scenes")


def reference_calls(path, width, height, calls):
    """render(4, True) then calls - 1 times render(4, False) by the reference's code: the scene and
    (accum, rng, tonemapped) after each call."""
    scene = pr.load_scene(path, width, height)
    r = pr.RefRenderer(scene, width, height)
    out = []
    for i in range(calls):
        r.render(scene.camera, 4, i == 0)
        out.append((r.accum.copy(), r.rng_array().copy(), r.tonemap()))
    return scene, out


_reference = {}


@pytest.fixture(scope="module")
def directed(scene_dir):
    """name, calls -> (path, scene, reference results): rendered once per module, never modified."""
    def get(name, calls=2):
        if (name, calls) not in _reference:
            path = ds.directed_scene(scene_dir, name)
            _reference[(name, calls)] = (path, *reference_calls(path, W, H, calls))
        return _reference[(name, calls)]
    return get


def check_two_renders(pt, cam, want, what, seed=None, path=None):
    for ignore, (accum, rng, image) in zip((True, False), want):
        pt.render(cam, 4, ignore)
        ds.same_bits_or_both_nan(pt.accum(), accum, f"{what}: accumulation after render(4, {ignore}), gpu vs reference",
                                 seed, path)
        assert np.array_equal(pt.rng_state(), rng), f"{what}: RNG state after render(4, {ignore})"
        assert np.array_equal(pt.get_image_data(), image), f"{what}: tonemap after render(4, {ignore})"


def assert_refused(pt, path, index, what):
    with pytest.raises(pa.PathtracerError, match=rf"objects\[{index}\]\.scale = .*inverse transform is not finite") as e:
        pt.load_scene(str(path))
    assert e.value.code == N.PT_ERR_ARG, what


@pytest.mark.parametrize("name", list(ds.DIRECTED))
def test_directed_scene_equals_reference_source(directed, name):
    path, scene, want = directed(name)
    pt = pa.Pathtracer(W, H, device=0)
    refused = ds.refused_by_loader(path)
    assert (refused is not None) == (name in ds.ZERO_SCALE), name
    if refused is not None:
        assert_refused(pt, path, refused, name)
        return
    cam = pt.load_scene(str(path))
    assert bytes(cam) == bytes(scene.camera), f"{name}: camera"
    check_two_renders(pt, cam, want, name)
    assert pt.frames == 2


def test_every_variant_on_the_combined_scene(directed):
    path, scene, want = directed("domain_combined")
    pt = pa.Pathtracer(W, H, device=0)
    cam = pt.load_scene(str(path))
    start = pt.rng_state()
    for variant in VARIANTS:
        pt.set_kernel_variant(variant)
        pt.set_rng_state(start)
        check_two_renders(pt, cam, want, f"domain_combined, variant {variant}")


@pytest.mark.parametrize("block", range(len(ds.SEEDS_GPU) // 32))
def test_random_scenes_equal_reference_source(scene_dir, block):
    for seed in ds.SEEDS_GPU[32 * block:32 * block + 32]:
        variant = VARIANTS[seed % len(VARIANTS)]
        path = ds.random_scene(scene_dir, seed)
        what = f"random seed {seed}, variant {variant}"
        # a renderer per scene: like the reference's, its texture table takes 64 textures in its
        # lifetime, and a scene loaded after that loses its sky
        pt = pa.Pathtracer(ds.RW, ds.RH, device=0)
        refused = ds.refused_by_loader(path)
        if refused is not None:                      # refused by name; what is left of it is rendered
            assert_refused(pt, path, refused, what)
            path = ds.without_refused_objects(path)
        if path is not None:
            scene, want = reference_calls(path, ds.RW, ds.RH, 2)
            cam = pt.load_scene(str(path))
            assert bytes(cam) == bytes(scene.camera), f"{what}: camera ({path})"
            pt.set_kernel_variant(variant)
            check_two_renders(pt, cam, want, what, seed, path)
        pt.close()


def test_set_scene_refuses_non_finite_rows(directed):
    # the C ABI's half of the refusal: one inf or NaN among a primitive's inverse-transform rows
    import ctypes as C
    path, scene, want = directed("metal_out")
    osc = po.load_scene(path, W, H)
    pt = pa.Pathtracer(W, H, device=0)
    nodes = (pa.PtBvhNode * osc.node_count).from_buffer_copy(bytes(osc.nodes)[:osc.node_count * C.sizeof(pa.PtBvhNode)])
    for bad, (i, r, c) in ((float("inf"), (0, 0, 0)), (float("nan"), (2, 1, 3)), (float("-inf"), (3, 2, 2))):
        prims = (pa.PtHittable * osc.prim_count).from_buffer_copy(bytes(osc.prims)[:osc.prim_count * C.sizeof(pa.PtHittable)])
        prims[i].inv_transform_rows[r][c] = bad
        with pytest.raises(pa.PathtracerError, match=rf"primitive {i}: inv_transform_rows\[{r}\]\[{c}\] is not finite") as e:
            N.check_ctx(N.hip().pt_set_scene(pt._ctx, nodes, osc.node_count, prims, osc.prim_count), pt._ctx)
        assert e.value.code == N.PT_ERR_ARG
    prims = (pa.PtHittable * osc.prim_count).from_buffer_copy(bytes(osc.prims)[:osc.prim_count * C.sizeof(pa.PtHittable)])
    N.check_ctx(N.hip().pt_set_scene(pt._ctx, nodes, osc.node_count, prims, osc.prim_count), pt._ctx)   # unchanged: accepted


@pytest.mark.parametrize("name", NAN_SCENES)
def test_adaptive_on_nan_pixels(directed, name):
    # pt_render_adaptive where a call's colour sum, and so the moments, are NaN: against the oracle's
    # adaptive model.  The contract (include/pt_hip.h) counts a non-finite pixel as converged -- more
    # samples cannot repair it -- so a NaN pixel itself never asks for more calls: it stops at min_calls
    # unless an unconverged finite neighbour keeps its 3x3 block active.
    path, scene, want = directed(name)
    osc = po.load_scene(path, W, H)
    ad = AdaptiveOracle(po.OracleRenderer(osc, W, H)).render(osc.camera, **ADAPTIVE)
    nan = np.isnan(want[1][0][..., :3]).any(-1)              # NaN after min_calls plain calls of the reference
    assert nan.any() and np.isnan(ad.m2[nan]).all(), f"{name}: no NaN moment in the oracle's adaptive render"
    pt = pa.Pathtracer(W, H, device=0)
    cam = pt.load_scene(str(path))
    pt.render_adaptive(cam, **ADAPTIVE)
    assert np.array_equal(pt.sample_counts(), ad.n), f"{name}: calls per pixel"
    assert np.array_equal(pt.rng_state(), ad.rng_array()), f"{name}: RNG state"
    ds.same_bits_or_both_nan(pt.accum(), ad.accum, f"{name}: adaptive accumulation, gpu vs oracle model")
    m = pt.moments()
    ds.same_bits_or_both_nan(m[..., :2], ad.moments()[..., :2], f"{name}: adaptive moments, gpu vs oracle model")
    # a NaN pixel never reports itself unconverged: where every pixel of a 3x3 block is NaN the centre
    # stopped at min_calls
    pad = np.pad(nan, 1, constant_values=True)
    block = np.ones_like(nan)
    for dy in range(3):
        for dx in range(3):
            block &= pad[dy:dy + H, dx:dx + W]
    assert (pt.sample_counts()[block] == ADAPTIVE["min_calls"]).all(), f"{name}: a NaN pixel kept sampling"
    # a stopped pixel holds what n plain calls of the reference's source leave
    stopped = pt.sample_counts() == ADAPTIVE["min_calls"]
    assert stopped.any()
    ds.same_bits_or_both_nan(pt.accum()[stopped], want[1][0][stopped], f"{name}: pixels stopped after 2 calls")
    assert np.array_equal(pt.rng_state()[stopped], want[1][1][stopped]), f"{name}: RNG of pixels stopped after 2 calls"


@pytest.mark.parametrize("variant", GROUP_VARIANTS)
@pytest.mark.parametrize("name", NAN_SCENES)
def test_sample_groups_on_nan_pixels(directed, name, variant):
    # the fold of speculative sample groups compares and replays logged path colours that are NaN
    calls = 8
    path, scene, want = directed(name, calls)
    pt = pa.Pathtracer(W, H, device=0)
    cam = pt.load_scene(str(path))
    pt.set_kernel_variant(variant)
    pt.set_sample_groups(2)
    pt.render(cam, 4, True, chunks=calls)
    assert pt.last_sample_groups == 2
    accum, rng, _ = want[calls - 1]
    assert np.isnan(accum).any()
    ds.same_bits_or_both_nan(pt.accum(), accum, f"{name}, variant {variant}, 2 groups: accumulation after {calls} calls")
    assert np.array_equal(pt.rng_state(), rng), f"{name}, variant {variant}, 2 groups: RNG state"


@pytest.mark.parametrize("name", NAN_SCENES)
def test_run_ahead_on_nan_pixels(directed, name):
    # the run-ahead stash carries a call's colour sum so far, here NaN, into the next launch
    calls = 4
    path, scene, want = directed(name, calls)
    pt = pa.Pathtracer(W, H, device=0)
    cam = pt.load_scene(str(path))
    pt.set_run_ahead(2)                                       # a stash at every launch
    for i, (accum, rng, image) in enumerate(want):
        pt.render(cam, 4, i == 0)
        ds.same_bits_or_both_nan(pt.accum(), accum, f"{name}, run-ahead: accumulation after call {i}")
        assert np.array_equal(pt.rng_state(), rng), f"{name}, run-ahead: RNG state after call {i}"
    assert np.array_equal(pt.get_image_data(), want[-1][2]), f"{name}, run-ahead: tonemap"
