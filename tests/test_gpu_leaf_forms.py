"""GPU: the kernel's cube test (on the inputs that separate its exact form from the min/max form) and
its quadric test (constants read from the primitive record) against the reference's own source where
oracle/_ref/libptref.so is built, else against the oracle: the directed scenes of tests/leaf_scenes.py,
domain_combined and every other accepted directed scene of tests/domain_scenes.py that holds a cube.

Images are 48 x 32, render(8, True) then render(8, False); accumulation and RNG state are compared bit
for bit after each call (float words that are NaN in both count as equal, domain_scenes'
same_bits_or_both_nan: the sign of a NaN is the host compiler's choice).  Every build that reads the
primitive record is run: the default pick and variants 4, 6, 20, 40, 41, 46, 60 and 61; adaptive
sampling, sample groups and run-ahead read the same records and get one case each.  With the quadric
constants of one shape zeroed in a test-only upload the all-quadrics scene must differ: the kernel reads
them from the record; with NaN in their place for a disk, quad or cube it must not: those paths never do.
"""
import numpy as np
import pytest

import domain_scenes as ds
import leaf_scenes as ls
import pathtracercuda_amd as pa
from oracle import pyoracle as po
from oracle import pyref as pr
from test_adaptive_rule import AdaptiveOracle

pytestmark = pytest.mark.gpu

W, H = ls.W, ls.H
SPP = 8
BUILDS = (0, 4, 6, 20, 40, 41, 46, 60, 61)                 # 0 = the default pick


# every directed scene of tests/domain_scenes.py that the loader accepts and that holds a cube, its own or
# still_life's (test_domain_cube_scene_list_is_complete derives the list from the scene files)
DOMAIN_CUBE_SCENES = ("metal_out", "scale_neg", "scale_extreme", "cam_lookat_eq", "cam_along_up", "fovy_0.0001",
                      "fovy_1e-06", "fovy_179.9", "fovy_180", "fovy_-60", "cam_on_surface", "sky_1x1", "domain_combined")
SCENES = [f"leaf:{n}" for n in ls.LEAF_SCENES] + [f"domain:{n}" for n in DOMAIN_CUBE_SCENES]
ADAPTIVE = dict(spp=4, min_calls=2, max_calls=4, tolerance=0.2, floor=0.01)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if pa.device_count() < 1:
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("gpu_leaf_scenes")


def expected_calls(path, spp, calls):
    """(accum, rng) after render(spp, True) and calls - 1 times render(spp, False): by the reference's
    compiled source where its library is present, else by the oracle."""
    if pr.available():
        scene = pr.load_scene(path, W, H)
        r = pr.RefRenderer(scene, W, H)
    else:
        scene = po.load_scene(path, W, H)
        r = po.OracleRenderer(scene, W, H)
    out = []
    for i in range(calls):
        r.render(scene.camera, spp, i == 0)
        out.append((r.accum.copy(), r.rng_array().copy()))
    return out


_cache = {}


@pytest.fixture(scope="module")
def case(scene_dir):
    """key, spp, calls -> (path, expected): rendered once per module, never modified."""
    def get(key, spp=SPP, calls=2):
        if (key, spp, calls) not in _cache:
            group, name = key.split(":")
            path = ls.leaf_scene(scene_dir, name) if group == "leaf" else ds.directed_scene(scene_dir, name)
            _cache[(key, spp, calls)] = (path, expected_calls(path, spp, calls))
        return _cache[(key, spp, calls)]
    return get


def check_calls(pt, cam, want, spp, what):
    for i, (accum, rng) in enumerate(want):
        pt.render(cam, spp, i == 0)
        ds.same_bits_or_both_nan(pt.accum(), accum, f"{what}: accumulation after call {i}")
        assert np.array_equal(pt.rng_state(), rng), f"{what}: RNG state after call {i}"


def test_domain_cube_scene_list_is_complete(scene_dir):
    import json
    derived = []
    for name in ds.DIRECTED:
        path = ds.directed_scene(scene_dir, name)
        objects = json.loads(path.read_text()).get("objects", [])
        if ds.refused_by_loader(path) is None and any(o.get("type") == "CUBE" for o in objects):
            derived.append(name)
    assert tuple(derived) == DOMAIN_CUBE_SCENES


@pytest.mark.parametrize("key", SCENES)
def test_every_build_equals_reference(case, key):
    path, want = case(key)
    pt = pa.Pathtracer(W, H, device=0)
    cam = pt.load_scene(str(path))
    start = pt.rng_state()
    for build in BUILDS:
        pt.set_kernel_variant(build)
        pt.set_rng_state(start)
        check_calls(pt, cam, want, SPP, f"{key}, build {build}")
    pt.close()


@pytest.mark.parametrize("key", ["leaf:all_quadrics", "leaf:cube_axis_z"])
def test_adaptive_reads_the_same_records(case, key):
    path, _ = case(key)
    osc = po.load_scene(path, W, H)
    ad = AdaptiveOracle(po.OracleRenderer(osc, W, H)).render(osc.camera, **ADAPTIVE)
    pt = pa.Pathtracer(W, H, device=0)
    cam = pt.load_scene(str(path))
    pt.render_adaptive(cam, **ADAPTIVE)
    assert np.array_equal(pt.sample_counts(), ad.n), f"{key}: calls per pixel"
    assert np.array_equal(pt.rng_state(), ad.rng_array()), f"{key}: RNG state"
    ds.same_bits_or_both_nan(pt.accum(), ad.accum, f"{key}: adaptive accumulation, gpu vs oracle model")
    pt.close()


@pytest.mark.parametrize("variant", (40, 60))
def test_sample_groups_read_the_same_records(case, variant):
    calls = 8
    key = "leaf:all_quadrics"
    path, want = case(key, 4, calls)
    pt = pa.Pathtracer(W, H, device=0)
    cam = pt.load_scene(str(path))
    pt.set_kernel_variant(variant)
    pt.set_sample_groups(2)
    pt.render(cam, 4, True, chunks=calls)
    assert pt.last_sample_groups == 2
    accum, rng = want[calls - 1]
    ds.same_bits_or_both_nan(pt.accum(), accum, f"{key}, variant {variant}, 2 groups: accumulation after {calls} calls")
    assert np.array_equal(pt.rng_state(), rng), f"{key}, variant {variant}, 2 groups: RNG state"
    pt.close()


@pytest.mark.parametrize("key", ["leaf:all_quadrics", "leaf:cube_face_plane"])
def test_run_ahead_reads_the_same_records(case, key):
    path, want = case(key, SPP, 4)
    pt = pa.Pathtracer(W, H, device=0)
    cam = pt.load_scene(str(path))
    pt.set_run_ahead(2)                                       # a stash at every launch
    check_calls(pt, cam, want, SPP, f"{key}, run-ahead")
    pt.close()


@pytest.mark.parametrize("shape", ["SPHERE", "CYLINDER", "CONE", "PARABOLOID"])
def test_zeroed_constants_change_the_image(case, shape):
    # negative control: B = H = J = 0 for one quadric shape makes its test read x^2 + z^2 = 0, so the
    # shape all but vanishes; planes' and cubes' constants are never read
    key = "leaf:all_quadrics"
    path, want = case(key)
    pt = pa.Pathtracer(W, H, device=0)
    pt.set_zero_quadric_consts(po.SHAPES.index(shape))
    cam = pt.load_scene(str(path))
    start = pt.rng_state()
    pt.render(cam, SPP, True)
    differs = (pt.accum().view(np.uint32) != want[0][0].view(np.uint32)).any(-1)
    print(f"{shape} zeroed: {int(differs.sum())} of {W * H} pixels differ")
    assert differs.any(), f"{shape}: zeroed constants changed no pixel"
    pt.set_zero_quadric_consts(-1)
    cam = pt.load_scene(str(path))
    pt.set_rng_state(start)
    check_calls(pt, cam, want, SPP, f"{key}, constants restored after {shape}")
    pt.close()


@pytest.mark.parametrize("shape", ["QUAD", "DISK", "CUBE"])
def test_planes_and_cubes_never_read_the_constants(case, shape):
    # for a disk, quad or cube the knob uploads NaN in place of the three words: a plane or cube path
    # that read them would turn its hit distance, and so the pixel, into NaN or a miss
    key = "leaf:all_quadrics"
    path, want = case(key)
    pt = pa.Pathtracer(W, H, device=0)
    pt.set_zero_quadric_consts(po.SHAPES.index(shape))
    cam = pt.load_scene(str(path))
    start = pt.rng_state()
    for build in (0, 4, 20, 41):
        pt.set_kernel_variant(build)
        pt.set_rng_state(start)
        check_calls(pt, cam, want, SPP, f"{key}, {shape} poisoned, build {build}")
    pt.close()
