"""CPU: the directed scenes of tests/leaf_scenes.py (cubes on both sides of the kernel's fast-form
guard, all four quadrics beside planes and cubes) rendered by the reference's own source
(oracle/_ref/libptref.so) and by the oracle, bit for bit; and the scenes' own claims, so a later edit
cannot quietly remove the edge.  The two forms of the cube test themselves are compared by
tools/leaf_forms_check.cpp (`make leafcheck`); tests/test_gpu_leaf_forms.py runs the kernel.
"""
import numpy as np
import pytest

import leaf_scenes as ls
from oracle import pyoracle as po
from oracle import pyref as pr
from test_ref_source import same_bits

W, H = ls.W, ls.H


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("leaf_scenes")


@pytest.fixture(scope="module")
def oracle_scene(scene_dir):
    cache = {}

    def get(name):
        if name not in cache:
            path = ls.leaf_scene(scene_dir, name)
            cache[name] = (path, po.load_scene(path, W, H))
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(ls.LEAF_SCENES))
def test_reference_source_equals_oracle(oracle_scene, name):
    # render(8, True) then render(8, False): hitBox as written (Hittable.inl:331-358, AABB.inl:46-69) and
    # the quadric templates against the oracle's restatement
    if not pr.available():
        if pr.reference_tree() is None:
            pytest.skip("neither oracle/_ref/libptref.so nor a checkout of the reference to build it from")
        pytest.fail(f"the reference is at {pr.reference_tree()} but {pr.LIB_PATH} is not built: run `make`")
    path, osc = oracle_scene(name)
    ref = pr.load_scene(path, W, H)
    assert bytes(ref.camera) == bytes(osc.camera), f"{name}: camera"
    rr = pr.RefRenderer(ref, W, H)
    orr = po.OracleRenderer(osc, W, H)
    for ignore in (True, False):
        rr.render(ref.camera, 8, ignore)
        orr.render(osc.camera, 8, ignore)
        same_bits(rr.accum, orr.accum, f"{name}: accumulation after render(8, {ignore})")
        same_bits(rr.rng_array(), orr.rng_array(), f"{name}: RNG state after render(8, {ignore})")
    lit = (np.nan_to_num(orr.accum[..., :3], nan=1.0).sum(-1) > 0).mean()
    print(f"{name}: {lit:.0%} of the pixels are lit")
    assert lit > 0.5, f"{name}: {lit:.0%} of the pixels are lit"


@pytest.mark.parametrize("name", list(ls.LEAF_SCENES))
def test_scene_holds_what_it_claims(oracle_scene, name):
    path, osc = oracle_scene(name)
    kind_at, zero = ls.scene_facts(osc)
    cube_px, zero_px = int((kind_at == ls.CUBE).sum()), int(zero.sum())
    print(f"{name}: primary hit is a cube at {cube_px} pixels; a cube's local direction has an exact zero at {zero_px}")
    if name in ls.CUBE_PRIMARY:
        assert cube_px >= 1, f"{name}: no pixel's primary hit is a cube"
    if name in ls.ZERO_COMPONENT:
        assert zero_px >= 1, f"{name}: no pixel's local direction has an exact zero component"
        assert (zero & (kind_at == ls.CUBE)).any(), f"{name}: no such pixel hits the cube"
    leaves = ls.leaf_types(osc)
    if name == "cube_leaf4":
        assert (ls.CUBE,) * 4 in leaves, f"{name}: no BVH leaf holds four cubes ({leaves})"
    if name == "all_quadrics":
        assert {t for leaf in leaves for t in leaf} >= set(ls.QUADRICS), f"{name}: a quadric shape is missing"
        shared = [leaf for leaf in leaves if set(leaf) & set(ls.QUADRICS)]
        assert shared and all(ls.CUBE in leaf and set(leaf) & {ls.DISK, ls.QUAD} for leaf in shared), \
            f"{name}: a leaf with a quadric holds no plane or no cube ({leaves})"
    if name == "cube_face_plane":
        # the camera is on the face plane: the local origin's x is exactly 1 where the direction's is 0
        o, d = ls.camera_rays(osc.camera)
        cubes = [osc.prims[i] for i in range(osc.prim_count) if osc.prims[i].type == ls.CUBE]
        lo, ld = ls.to_local(cubes[0].rows, o, d)
        assert lo[0] == 1.0 and (ld[..., 0] == 0).all(), f"{name}: local origin x {lo[0]}, direction x not all zero"
    if name == "cube_inside":
        o, d = ls.camera_rays(osc.camera)
        inside = [i for i in range(osc.prim_count)
                  if osc.prims[i].type == ls.CUBE and (np.abs(ls.to_local(osc.prims[i].rows, o, d)[0]) < 1).all()]
        assert inside, f"{name}: the camera is inside no cube"
    if name == "cubes_scaled":
        si = po.parse_scene(path)
        scales = np.array(si.scales, dtype=np.float32)
        assert scales.min() == np.float32(1e-3) and scales.max() == np.float32(1e3)
