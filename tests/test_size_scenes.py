"""The size-axis scenes of tests/size_scenes.py are what they claim, on the CPU.

tests/test_gpu_size_scenes.py runs the trace kernel on them; here the scenes themselves are checked,
so a later edit cannot quietly take the edge away: the trees obey the reference's rules, their sizes
are the hand-written ones, the reference's walk fills its stack to exactly R entries, the kernel's
walk (the CPU model of tests/test_walk_model.py) uses all R rows on every primary ray of the R = 32
scenes, t_max rises, the images are not flat, and the hand-written policy table gives the builds
and LDS byte counts the GPU tests expect.
"""
import numpy as np
import pytest

import bvh_edit as be
import size_scenes as ss
from oracle import pyoracle as po

W, H, SPP, CALLS = ss.IMAGE
RENDERABLE = [n for n in ss.CASES if n != "e_depth34"]


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("size_scenes")


@pytest.mark.parametrize("name", list(ss.CASES))
def test_tree_and_sizes(name):
    sc = ss.case(name)
    depth = be.check_tree(sc.nodes, sc.prim_count)      # full binary, children after parents, ranges consecutive
    if name == "e_depth34":
        assert depth == 34
    else:
        assert depth <= 33
    I, R, nodes, prims = ss.SIZES[name]
    assert (sc.interior, sc.node_count, sc.prim_count) == (I, nodes, prims)
    assert be.stack_rows_tree(sc.nodes) == R == sc.rows
    assert R <= depth - 1                               # pt_set_scene takes min(rows, depth - 1): the rows
    assert be.dfs_ordered(sc.nodes) == ("swap" not in name)
    assert sc.child_box_ok == ("big" not in name)
    sizes = [n[3] >> 16 for n in sc.nodes if n[3] >> 16]
    assert len(sizes) == (nodes + 1) // 2 and min(sizes) == 1
    assert max(sizes) == (256 if "big" in name else 1 + prims - len(sizes))    # one leaf holds what is extra
    # the root's box holds the camera (with it every box down to the deepest leaf: unions)
    cam = ss.camera_position(sc.octant)
    lo, hi = sc.nodes[0][0], sc.nodes[0][1]
    assert all(lo[k] < cam[k] < hi[k] for k in range(3))


@pytest.mark.parametrize("name", RENDERABLE)
def test_oracle_fills_its_stack_and_sees_light(name, scene_dir):
    sc = ss.case(name)
    osc = ss.oracle_scene(sc, sc.write(scene_dir, name), W, H)
    ref = po.OracleRenderer(osc, W, H)
    ref.render(osc.camera, SPP, True, chunks=CALLS, collect_stats=True)
    assert int(ref.stats[6]) == ss.SIZES[name][1], "the reference's stack does not reach R entries"
    if sc.S:
        assert int(ref.stats[7]) > 0, "no leaf raised t_max"
    words = ref.accum.reshape(-1, 4).view(np.uint32)
    distinct = len(np.unique(words, axis=0)) / len(words)
    print(f"{name}: max stack {int(ref.stats[6])}, rises {int(ref.stats[7])}, distinct colours {distinct:.0%}")
    assert distinct >= 0.25
    assert np.isfinite(ref.accum).all(), "the shell scenes have no NaN pixels"


def test_depth_34_overflows_the_reference_stack(scene_dir):
    sc = ss.case("e_depth34")
    osc = ss.oracle_scene(sc, sc.write(scene_dir, "e_depth34"), W, H)
    ref = po.OracleRenderer(osc, W, H)
    with pytest.raises(RuntimeError, match="stack overflow"):
        ref.render(osc.camera, 1, True)


@pytest.mark.parametrize("name", ["r32_spine", "r32_bushy", "r32_mirror"])
def test_every_primary_ray_uses_all_32_rows(name, scene_dir):
    """The kernel's walk keeps a far child only when the ray meets its box now, so a bound of R rows
    says little about the rows in use; on these scenes every box on the path holds the camera, and
    the model of the kernel's walk has R = 32 rows in use on every ray through a pixel centre."""
    from test_gpu_parity import _bvh_array
    from test_walk_model import F, cb_walk, first_prims
    sc = ss.case(name)
    osc = ss.oracle_scene(sc, sc.write(scene_dir, name), W, H)
    nodes = list(_bvh_array(sc.nodes))
    first = first_prims(nodes)
    cam = osc.camera
    o = np.array(cam.origin, F)
    llc, hor, ver = (np.array(v, F) for v in (cam.lowerLeftCorner, cam.horizontal, cam.vertical))
    signs = set()
    for y in range(H):
        for x in range(W):
            d = llc + F((x + 0.5) / W) * hor + F((y + 0.5) / H) * ver
            d = (d / np.linalg.norm(d)).astype(F)
            signs.add(tuple(bool(c < 0) for c in d))
            _, peak = cb_walk(nodes, first, o, d, y * W + x, with_peak=True, stop_rows=32)
            assert peak == 32, (x, y, peak)
    assert signs == {tuple(bool((sc.octant >> a) & 1) for a in range(3))}, "primary rays leave the octant"


@pytest.mark.parametrize("S,content", [(31, 2), (22, 785), (0, 2210)])
def test_natural_bvh_matches_reference_source(S, content, scene_dir):
    """The JSON as written, with the reference's own BVH build: reference source == oracle."""
    from oracle import pyref as pr
    if not pr.available():
        pytest.skip("oracle/_ref/libptref.so is not built")
    from test_ref_source import same_bits
    path = ss.scene(S, content).write(scene_dir, f"natural_{S}_{content}")
    ref = pr.load_scene(path, W, H)
    osc = po.load_scene(path, W, H)
    assert ref.count == len(osc.cpu) == S + content
    rn, rp, _ = ref.bvh()
    same_bits(rn, np.frombuffer(bytes(osc.nodes), dtype=np.uint8)[:osc.node_count * 32].reshape(-1, 32), "BVH nodes")
    rr, orr = pr.RefRenderer(ref, W, H), po.OracleRenderer(osc, W, H)
    for ignore in (True, False):
        rr.render(ref.camera, SPP, ignore)
        orr.render(osc.camera, SPP, ignore)
        same_bits(rr.accum, orr.accum, f"accumulation after render({SPP}, {ignore})")
        same_bits(rr.rng_array(), orr.rng_array(), f"RNG state after render({SPP}, {ignore})")


# ---- the policy table -------------------------------------------------------------------------
CUS = 256
LARGE = (1920 // 8) * (1080 // 8)        # 32,400 tiles >= 4 * 256 * 24 = 24,576
SMALL = 80 * 50                          # 4,000 tiles <= 16 * 256


def test_frames_for_256_compute_units():
    assert ss.large_frame(CUS) == (1920, 1080)
    assert ss.small_frame(CUS) == (640, 400)
    assert ss.persistent_frame(CUS)[0] * ss.persistent_frame(CUS)[1] // 64 >= 2 * CUS * 24


@pytest.mark.parametrize("name,build", list(ss.AUTO_LARGE.items()))
def test_policy_table_large_frame(name, build):
    I, R, nodes, prims = ss.SIZES[name]
    sc = ss.case(name)
    got = ss.expected_build(I, R, nodes, prims, sc.child_box_ok, be.dfs_ordered(sc.nodes), LARGE, LARGE, CUS)[0]
    assert got == build


@pytest.mark.parametrize("name,build", list(ss.AUTO_SMALL.items()))
def test_policy_table_small_frame(name, build):
    I, R, nodes, prims = ss.SIZES[name]
    assert ss.expected_build(I, R, nodes, prims, True, True, SMALL, SMALL, CUS)[0] == build


def test_policy_table_few_units_per_slot():
    # a large scene on a frame between the two: the five-wave builds
    I, R, nodes, prims = ss.SIZES["c_r9_181"]
    assert ss.expected_build(I, R, nodes, prims, True, True, 14400, 14400, CUS)[0] == 40
    I, R, nodes, prims = ss.SIZES["c_r9_182"]
    assert ss.expected_build(I, R, nodes, prims, True, True, 14400, 14400, CUS)[0] == 41


@pytest.mark.parametrize("name,build,bytes_,staged", ss.LDS_CASES)
def test_lds_bytes_at_the_limit(name, build, bytes_, staged):
    I, R, nodes, prims = ss.SIZES[name]
    assert ss.lds_bytes(build, I, R, nodes, prims) == (bytes_, staged)
    assert bytes_ <= ss.LDS_CAP
