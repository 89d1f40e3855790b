"""The trace kernel along the size axis: BVH depth, scene size and launch policy.

The scenes are those of tests/size_scenes.py (caller BVHs with chosen interior-node count I and LDS
stack rows R; tests/test_size_scenes.py checks the scenes themselves on the CPU).  The bar is the
suite's: accumulation words and XORWOW states equal the oracle's on the same caller BVH -- or, on
frames too large for the oracle, the reference's control flow (variant 1) on the same context.

  A  stack rows R = 1, 2, 3, 16, 31 and 32 (three forms), every shipped variant and every launch mode
     of the resumable walks; the instrumented launch repairs as often as the oracle's t_max rises
  B  each staged build at the largest scene that still stages (the launch uses all 163,840 B of LDS)
     and at the next one (the same walk with nothing staged), plain and persistent; pt_last_launch
     reports the table's byte count and staging level
  C  the automatic choice of the build, pinned to the hand-written table of size_scenes.py
  D  scenes replaced on a live context (small, deep and large, small, from file, one that fills the
     LDS), in three orders, persistent and plain: each equals the scene on a context of its own
  E  depth 33 renders, depth 34 is refused and leaves the context's scene as it was

The shell scenes have no NaN pixels (tests/test_size_scenes.py asserts it), so words are compared
plainly.
"""
import numpy as np
import pytest

import pathtracercuda_amd as pa
import size_scenes as ss
from oracle import pyoracle as po
from pathtracercuda_amd import _native as N
from test_gpu_parity import SHIPPED_VARIANTS, _set_caller_bvh, assert_bitexact

pytestmark = pytest.mark.gpu

W, H = ss.IMAGE[:2]
RESUMABLE = (40, 41, 46, 60, 61)
ROW_SCENES = ("r1", "r2", "r3", "r16", "r31", "r32_spine", "r32_bushy", "r32_mirror")


@pytest.fixture(scope="module")
def gpu_available():
    if pa.device_count() < 1:
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def cus(gpu_available):
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


class Lab:
    """Scene files, oracle scenes and oracle renders, each made once per module."""

    def __init__(self, directory):
        self.dir = directory
        self._osc = {}
        self._ref = {}

    def path(self, name):
        return self.dir / f"{name}.scene.json"

    def osc(self, name):
        if name not in self._osc:
            sc = ss.case(name)
            self._osc[name] = ss.oracle_scene(sc, sc.write(self.dir, name), W, H)
        return self._osc[name]

    def oracle(self, name, spp, calls):
        """(accumulation, RNG state, rises) of `calls` render() calls of spp samples, the first one
        ignoring the history, from the seeded RNG state."""
        key = (name, spp, calls)
        if key not in self._ref:
            osc = self.osc(name)
            ref = po.OracleRenderer(osc, W, H)
            ref.render(osc.camera, spp, True, chunks=calls, collect_stats=True)
            self._ref[key] = (ref.accum.copy(), ref.rng_array().copy(), int(ref.stats[7]))
        return self._ref[key]

    def load(self, pt, name):
        """The scene's file through the host layer (camera, textures, sky), then its caller BVH."""
        osc = self.osc(name)
        cam = pt.load_scene(self.path(name))
        _set_caller_bvh(pt, osc, ss.case(name).nodes)
        return cam


@pytest.fixture(scope="module")
def lab(gpu_available, tmp_path_factory):
    return Lab(tmp_path_factory.mktemp("gpu_size_scenes"))


def check(pt, want, what):
    assert_bitexact(pt.accum(), want[0], what)
    assert np.array_equal(pt.rng_state(), want[1]), f"{what}: RNG state"


# ---- A. stack rows ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROW_SCENES)
def test_rows_every_variant(lab, name):
    pt = pa.Pathtracer(W, H)
    cam = lab.load(pt, name)
    assert bytes(cam) == bytes(lab.osc(name).camera)
    want = lab.oracle(name, 4, 2)
    st = pt.rng_state()
    for variant in (0,) + SHIPPED_VARIANTS:
        pt.set_kernel_variant(variant)
        pt.set_rng_state(st)
        pt.render_raw(cam, 4, 2, True)
        check(pt, want, f"{name}, variant {variant}")


@pytest.mark.parametrize("name", ROW_SCENES)
def test_rows_every_launch_mode(lab, name):
    pt = pa.Pathtracer(W, H)
    cam = lab.load(pt, name)
    plain, strip, three, four = (lab.oracle(name, *k) for k in ((4, 2), (1, 2), (2, 3), (2, 4)))
    st = pt.rng_state()
    for variant in RESUMABLE:
        pt.set_kernel_variant(variant)
        tag = f"{name}, variant {variant}"
        pt.set_rng_state(st)
        stats = pt.render_instrumented(cam, 4, 2, True)
        check(pt, plain, f"{tag}, instrumented")
        if ss.case(name).S:
            assert plain[2] > 0
        assert stats["repairs"] == plain[2], (tag, stats["repairs"], plain[2])
        pt.set_occupancy(1)                       # the persistent grid whatever the frame's size
        pt.set_rng_state(st)
        pt.render_raw(cam, 4, 2, True)
        pt.set_occupancy(0)
        check(pt, plain, f"{tag}, persistent")
        pt.set_strip_units(4)
        pt.set_rng_state(st)
        pt.render_raw(cam, 1, 2, True)
        pt.set_strip_units(0)
        check(pt, strip, f"{tag}, strips of 4 tiles")
        for groups in (2, 4):
            pt.set_sample_groups(groups)
            pt.set_rng_state(st)
            pt.render_raw(cam, 4, 2, True)
            assert pt.last_sample_groups == groups
            check(pt, plain, f"{tag}, {groups} sample groups")
        pt.set_sample_groups(0)
        pt.set_run_ahead(2)
        pt.set_rng_state(st)
        for call in range(3):
            pt.render_raw(cam, 2, 1, call == 0)
        pt.set_run_ahead(0)
        check(pt, three, f"{tag}, run-ahead over three calls")
        pt.set_rng_state(st)
        pt.render_adaptive(cam, spp=2, min_calls=2, max_calls=4, tolerance=0.0)
        assert (pt.sample_counts() == 4).all()
        check(pt, four, f"{tag}, adaptive")


# ---- B. LDS limits ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,build,lds,staged", ss.LDS_CASES)
def test_staging_limit(lab, cus, name, build, lds, staged):
    I, R, nodes, prims = ss.SIZES[name]
    assert ss.lds_bytes(build, I, R, nodes, prims) == (lds, staged)
    pt = pa.Pathtracer(W, H)
    cam = lab.load(pt, name)
    want = lab.oracle(name, 2, 2)
    st = pt.rng_state()
    for variant in (build, 0):
        for occupancy in (0, 1):
            pt.set_kernel_variant(variant)
            pt.set_occupancy(occupancy)
            pt.set_rng_state(st)
            pt.render_raw(cam, 2, 2, True)        # a launch the runtime refuses raises with its message
            print(f"{name}: I {I}, R {R}, {nodes} nodes, {prims} primitives; forced {variant} ran {pt.last_variant}"
                  f"{', persistent' if occupancy else ''}; table: build {build} uses {lds} B, staging level {staged}")
            if variant:
                launch = pt.last_launch
                print(f"    launched: {launch}")
                assert pt.last_variant == build
                assert (launch["lds_bytes"], launch["staged"]) == (lds, staged), (launch, "the table", lds, staged)
                assert launch["waves_per_group"] == ss.BUILDS[build][1]
                if build != 6:                    # (variant 6 has no persistent form)
                    assert launch["groups"] == (cus if occupancy else (W // 8) * (H // 8) // launch["waves_per_group"])
            check(pt, want, f"{name}, variant {variant}, occupancy {occupancy}")


# ---- C. the automatic choice ------------------------------------------------------------------
class Frame:
    def __init__(self, size):
        self.W, self.H = size
        self.pt = pa.Pathtracer(self.W, self.H)
        self.st = self.pt.rng_state()
        self.tiles = ((self.W + 7) // 8) * ((self.H + 7) // 8)

    def auto_against_reference_flow(self, lab, name, cus, literal):
        """The automatic launch runs the table's build and gives the bits of the reference's control
        flow (variant 1) on this context from the same RNG state."""
        pt = self.pt
        cam = lab.load(pt, name)
        sc = ss.case(name)
        I, R, nodes, prims = ss.SIZES[name]
        import bvh_edit as be
        build, lds = ss.expected_build(I, R, nodes, prims, sc.child_box_ok, be.dfs_ordered(sc.nodes), self.tiles,
                                       self.tiles, cus)
        if cus == 256:
            assert build == literal, "the table disagrees with the written expectation"
        pt.set_kernel_variant(0)
        pt.set_rng_state(self.st)
        pt.render_raw(cam, 2, 2, True)
        ran = pt.last_variant
        launch = pt.last_launch
        got = (pt.accum().view(np.uint32).copy(), pt.rng_state())
        print(f"{name} at {self.W}x{self.H}: I {I}, R {R}; ran {ran}, table {build} ({lds} B of LDS)")
        pt.set_kernel_variant(1)
        pt.set_rng_state(self.st)
        pt.render_raw(cam, 2, 2, True)
        assert ran == build, f"{name}: build {ran} ran, the documented policy gives {build}"
        assert launch["lds_bytes"] == lds, (launch, "the table", lds)
        assert np.array_equal(got[0], pt.accum().view(np.uint32)), f"{name}: build {ran} differs from variant 1"
        assert np.array_equal(got[1], pt.rng_state()), f"{name}: RNG state"


@pytest.fixture(scope="module")
def large(cus):
    return Frame(ss.large_frame(cus))


@pytest.fixture(scope="module")
def small(cus):
    return Frame(ss.small_frame(cus))


@pytest.mark.parametrize("name,build", list(ss.AUTO_LARGE.items()))
def test_automatic_build_large_frame(lab, large, cus, name, build):
    assert large.tiles >= 4 * cus * 24
    large.auto_against_reference_flow(lab, name, cus, build)


@pytest.mark.parametrize("name,build", list(ss.AUTO_SMALL.items()))
def test_automatic_build_small_frame(lab, small, cus, name, build):
    assert small.tiles <= 16 * cus
    small.auto_against_reference_flow(lab, name, cus, build)


# ---- D. scene replacement ---------------------------------------------------------------------
GENERATED = "generated_scene"
_fresh = {}


def _load_any(lab, scenes, pt, name):
    return pt.load_scene(scenes / f"{GENERATED}.scene.json") if name == GENERATED else lab.load(pt, name)


def fresh_reference(lab, scenes, size, name):
    """The scene on a context of its own, by the reference's control flow (variant 1: no staging, no
    persistent grid, nothing cached per build)."""
    key = (size, name)
    if key not in _fresh:
        pt = pa.Pathtracer(*size)
        cam = _load_any(lab, scenes, pt, name)
        pt.set_kernel_variant(1)
        st = pt.rng_state()
        pt.render_raw(cam, 1, 2, True)
        _fresh[key] = (st, pt.accum().view(np.uint32).copy(), pt.rng_state())
        pt.close()
    return _fresh[key]


# (b60_r32_fit: between d_small and it the staged builds keep their instantiation, and its LDS need
#  goes from a few KB to all of it -- r32_bushy is too large to stage with eight waves or with its
#  primitives, so forced 60 and 48 run their unstaged instantiations there)
@pytest.mark.parametrize("order", [("d_small", "r32_bushy", "d_small", GENERATED, "b60_r32_fit", "d_small"),
                                   ("d_small", "b60_r32_fit", GENERATED, "d_small", "r32_bushy", "d_small"),
                                   ("r32_bushy", "b60_r32_fit", "d_small", GENERATED, "d_small")],
                         ids=["small-first", "reversed", "deep-first"])
@pytest.mark.parametrize("frame", ["persistent", "plain"])
def test_scene_replacement(lab, scenes, cus, frame, order):
    size = ss.persistent_frame(cus) if frame == "persistent" else (W, H)
    pt = pa.Pathtracer(*size)
    for variant in (0, 60, 48):
        pt.set_kernel_variant(variant)
        for step, name in enumerate(order):
            st, accum, rng = fresh_reference(lab, scenes, size, name)
            cam = _load_any(lab, scenes, pt, name)
            pt.set_rng_state(st)
            pt.render_raw(cam, 1, 2, True)
            what = f"{frame} frame, variant {variant}, step {step} ({name})"
            print(f"{what}: ran {pt.last_variant}, {pt.last_launch}")
            assert np.array_equal(pt.accum().view(np.uint32), accum), what
            assert np.array_equal(pt.rng_state(), rng), f"{what}: RNG state"


# ---- E. refusals ------------------------------------------------------------------------------
def test_depth_34_is_refused_and_the_scene_stays(lab):
    pt = pa.Pathtracer(W, H)
    cam = lab.load(pt, "r32_spine")                  # depth 33: accepted (and exact, part A)
    want = lab.oracle("r32_spine", 2, 2)
    st = pt.rng_state()
    pt.render_raw(cam, 2, 2, True)
    check(pt, want, "depth 33")
    deep = ss.case("e_depth34")
    osc = lab.osc("e_depth34")
    with pytest.raises(pa.PathtracerError) as e:
        _set_caller_bvh(pt, osc, deep.nodes)
    assert e.value.code == N.PT_ERR_DEPTH
    assert "stack" in str(e.value)
    for variant in (0, 60, 1):
        pt.set_kernel_variant(variant)
        pt.set_rng_state(st)
        pt.render_raw(cam, 2, 2, True)
        check(pt, want, f"the depth-33 scene after the refusal, variant {variant}")
