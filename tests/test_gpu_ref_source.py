"""GPU: the HIP megakernel against the reference's own source compiled for the host
(oracle/_ref/libptref.so, see tests/test_ref_source.py).  The library is built where a checkout of
the reference is at hand and is only loaded here; the reference's tree itself is never read.

Bit-exact accumulation sums, XORWOW states and tonemapped bytes on cornell_box and on every edge scene
of tests/ref_scenes.py, at 48 x 32.
"""
import numpy as np
import pytest

import pathtracercuda_amd as pa
import ref_scenes
from oracle import pyref as pr

pytestmark = pytest.mark.gpu

W, H = ref_scenes.W, ref_scenes.H
VARIANTS = (0, 1, 20, 40, 46, 60, 61)


@pytest.fixture(scope="module", autouse=True)
def ref_library():
    if not pr.available():
        pytest.skip(f"{pr.LIB_PATH} is absent: it is built by `make` where a checkout of the reference is present")
    if pa.device_count() < 1:
        pytest.skip("no GPU")
    return pr.lib()


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("gpu_ref_scenes")


def same_bits(gpu, ref, what):
    a, b = np.ascontiguousarray(gpu).view(np.uint32), np.ascontiguousarray(ref).view(np.uint32)
    assert a.shape == b.shape, f"{what}: shapes {a.shape} vs {b.shape}"
    if not np.array_equal(a, b):
        d = np.argwhere(a != b)
        y, x = d[0][:2]
        raise AssertionError(f"{what}: {len(d)} words differ; first pixel (row {y}, x {x}) gpu={gpu[y, x]} ref={ref[y, x]}")


def reference_render(path):
    """render(4, True) then render(4, False) by the reference's code: (accum, rng, tonemapped) after each."""
    scene = pr.load_scene(path, W, H)
    r = pr.RefRenderer(scene, W, H)
    out = []
    for ignore in (True, False):
        r.render(scene.camera, 4, ignore)
        out.append((r.accum.copy(), r.rng_array().copy(), r.tonemap()))
    return scene, out


def scene_path(scenes, scene_dir, name):
    if name == "cornell_box":
        return ref_scenes.drop_unset_uv_textures(scenes / "cornell_box.scene.json", scene_dir)
    return ref_scenes.edge_scene(scene_dir, name)


@pytest.mark.parametrize("name", ["cornell_box"] + list(ref_scenes.EDGE_SCENES))
def test_kernel_equals_reference_source(scenes, scene_dir, name):
    path = scene_path(scenes, scene_dir, name)
    scene, want = reference_render(path)
    pt = pa.Pathtracer(W, H, device=0)
    cam = pt.load_scene(str(path))
    assert bytes(cam) == bytes(scene.camera), f"{name}: camera"
    for ignore, (accum, rng, image) in zip((True, False), want):
        pt.render(cam, 4, ignore)
        same_bits(pt.accum(), accum, f"{name}: accumulation after render(4, {ignore})")
        assert np.array_equal(pt.rng_state(), rng), f"{name}: RNG state after render(4, {ignore})"
        assert np.array_equal(pt.get_image_data(), image), f"{name}: tonemap after render(4, {ignore})"
    assert pt.frames == 2


def test_every_variant_equals_reference_source(scenes, scene_dir):
    # all seven shapes, the ties and the material set in one BVH, under each kernel variant
    path = scene_path(scenes, scene_dir, "combined")
    scene, want = reference_render(path)
    pt = pa.Pathtracer(W, H, device=0)
    cam = pt.load_scene(str(path))
    start = pt.rng_state()
    for variant in VARIANTS:
        pt.set_kernel_variant(variant)
        pt.set_rng_state(start)
        for ignore, (accum, rng, image) in zip((True, False), want):
            pt.render(cam, 4, ignore)
            same_bits(pt.accum(), accum, f"variant {variant}: accumulation after render(4, {ignore})")
            assert np.array_equal(pt.rng_state(), rng), f"variant {variant}: RNG state after render(4, {ignore})"
        assert np.array_equal(pt.get_image_data(), image), f"variant {variant}: tonemap"
