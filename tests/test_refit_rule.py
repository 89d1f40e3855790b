"""Rule 10 of include/pt_hip.h (the refit) on the CPU: the two numpy restatements of tests/refit_model.py agree word
for word, the C++ host refit (pa.refit_boxes, ptamd::refitBoxes) equals them word for word, the refit with the boxes
the host build folded its nodes from reproduces BVH::build's node boxes as float values, unreachable nodes and the
records' fourth quad keep their words, and the host layer refuses what it must.  No tolerance anywhere."""
import ctypes as C
import json

import numpy as np
import pytest

import bvh_edit as be
import pathtracercuda_amd as pa
import refit_model as rm
from pathtracercuda_amd import _native as N

F, U = np.float32, np.uint32
SHIPPED = ("cornell_box", "test_shapes", "generated_scene", "rise_pair", "rise_repair")


def random_tree(seed, prims=None):
    """A seeded topology in the reference's layout (first child next, second child after the first subtree) with leaves
    of 1..5 primitives, junk boxes on every node, and seeded primitive boxes that hold equal values, zeros of both
    signs and degenerate (min == max) axes."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 40)) if prims is None else prims
    nodes = []

    def build(first, count):
        i = len(nodes)
        junk = (tuple(rng.uniform(-9, 9, 3)), tuple(rng.uniform(-9, 9, 3)))
        nodes.append(None)
        if count <= 5 and (count == 1 or rng.random() < 0.5):
            nodes[i] = (*junk, first, count << 16)
            return
        left = int(rng.integers(1, count))
        build(first, left)
        second = len(nodes)
        build(first + left, count - left)
        nodes[i] = (*junk, second, int(rng.integers(0, 3)) << 8)

    build(0, n)
    lo = rng.choice(np.array([-2.0, -1.0, -0.0, 0.0, 0.5, 1.0], dtype=F), size=(n, 3))
    ext = rng.choice(np.array([0.0, 0.0, 0.5, 1.0, 2.5], dtype=F), size=(n, 3))
    boxes = np.concatenate([lo, (lo + ext).astype(F)], axis=1).astype(F)
    return nodes, boxes


def node_array(nodes):
    arr = (pa.PtBvhNode * len(nodes))()
    for i, (lo, hi, off, pca) in enumerate(nodes):
        arr[i].aabb_min[:], arr[i].aabb_max[:], arr[i].offset, arr[i].primitive_count_axis = list(lo), list(hi), off, pca
    return arr


def arrays_of(arr):
    lo = np.array([list(n.aabb_min) for n in arr], dtype=F)
    hi = np.array([list(n.aabb_max) for n in arr], dtype=F)
    return lo, hi, np.array([n.offset for n in arr], dtype=U), np.array([n.primitive_count_axis for n in arr], dtype=U)


def edited(nodes):
    """The same tree with unreachable nodes: an inserted orphan where the layout allows one, malformed ones at the end."""
    for p in range(1, len(nodes)):
        if (nodes[p - 1][3] >> 16) != 0 and (nodes[p][3] >> 16) == 0:
            nodes = be.insert_orphan(nodes, p)
            break
    return be.append_malformed_orphans(nodes)


@pytest.mark.parametrize("seed", range(32))
def test_the_restatements_and_the_host_refit_agree_word_for_word(seed):
    nodes, boxes = random_tree(seed)
    for tree in (nodes, edited(nodes)):
        lo, hi, off, pca = rm.from_tuples(tree)
        a, b = rm.refit(lo, hi, off, pca, boxes), rm.refit_by_node(lo, hi, off, pca, boxes)
        assert rm.same_words(a[0], b[0]) and rm.same_words(a[1], b[1])
        got = arrays_of(pa.refit_boxes(node_array(tree), boxes))
        assert rm.same_words(got[0], a[0]) and rm.same_words(got[1], a[1])
        assert np.array_equal(got[2], off) and np.array_equal(got[3], pca)
        # an unreachable node keeps every word
        out = rm.depths(off, pca) < 0
        assert rm.same_words(a[0][out], lo[out]) and rm.same_words(a[1][out], hi[out])
        assert len(tree) == len(nodes) or out.sum() >= 3
        # a refit of the refitted tree with the same boxes changes nothing
        again = rm.refit(a[0], a[1], off, pca, boxes)
        assert rm.same_words(again[0], a[0]) and rm.same_words(again[1], a[1])


def test_the_records_keep_their_fourth_quad_and_the_unreachable_ones_every_word():
    nodes, boxes = random_tree(7, prims=23)
    tree = edited(nodes)
    lo, hi, off, pca = rm.from_tuples(tree)
    before = rm.records(lo, hi, off, pca)
    rng = np.random.default_rng(3)
    marked = before.copy()
    reach = rm.depths(off, pca) >= 0
    rec = rm.record_index(pca)
    unreachable = [int(rec[i]) for i in np.flatnonzero(~reach & (rec >= 0))]
    assert len(unreachable) >= 2
    marked[unreachable] = rng.uniform(-5, 5, (len(unreachable), 16)).astype(F)      # whatever they hold stays
    moved = boxes.copy()
    moved[:, :3] -= F(1.5)
    got = arrays_of(pa.refit_boxes(node_array(tree), moved))        # the C++ refit's boxes feed the records
    nl, nh = got[0], got[1]
    assert rm.same_words(nl, rm.refit(lo, hi, off, pca, moved)[0]) and not rm.same_words(nl, lo)
    after = rm.refit_records(marked, nl, nh, off, pca)
    assert rm.same_words(after[:, 12:], marked[:, 12:])
    assert rm.same_words(after[unreachable], marked[unreachable])
    reachable = [int(rec[i]) for i in np.flatnonzero(reach & (rec >= 0))]
    assert not rm.same_words(after[reachable, :12], marked[reachable, :12])
    assert rm.same_words(after[reachable], rm.records(nl, nh, off, pca)[reachable])  # what pt_set_scene makes of the new tree


def element_boxes(scene):
    """A host scene's nodes, and its objects' boxes in the build's element order."""
    nodes, prims = scene.bvh()
    objs, aabbs = scene.objects()
    n = scene.object_count
    taken, boxes = set(), np.zeros((n, 6), dtype=F)
    by_words = {}
    for i in range(n):
        by_words.setdefault(bytes(objs[i]), []).append(i)
    for e in range(n):
        i = by_words[bytes(prims[e])].pop(0)
        assert i not in taken
        taken.add(i)
        boxes[e] = aabbs[i]
    return nodes, boxes


def seeded_scene_file(path, seed):
    rng = np.random.default_rng(1000 + seed)
    shapes = ["SPHERE", "CYLINDER", "DISK", "CONE", "PARABOLOID", "QUAD", "CUBE"]
    objs = [{"type": shapes[int(rng.integers(0, 7))], "position": [float(x) for x in rng.uniform(-6, 6, 3)],
             "rotation": [float(x) for x in rng.uniform(-180, 180, 3)], "scale": [float(x) for x in rng.uniform(0.1, 1.5, 3)],
             "material": {"type": "LAMBERT", "baseColor": [0.5, 0.5, 0.5], "emissive": [0.0, 0.0, 0.0], "roughness": 1.0,
                          "metalness": 0.0}} for _ in range(int(rng.integers(1, 70)))]
    path.write_text(json.dumps({"camera": {"position": [0, 0, 12], "look_at": [0, 0, 0], "fovy": 40.0}, "objects": objs}))
    return path


def check_build(scene):
    nodes, boxes = element_boxes(scene)
    want = arrays_of(nodes)
    got = arrays_of(pa.refit_boxes(nodes, boxes))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])       # as float values: -0.0 == 0.0
    model = rm.refit(*want, boxes)
    assert rm.same_words(model[0], got[0]) and rm.same_words(model[1], got[1])


@pytest.mark.parametrize("name", SHIPPED)
def test_the_builds_own_boxes_reproduce_a_shipped_scenes_nodes(scenes, name):
    check_build(pa.Scene(str(scenes / f"{name}.scene.json"), 64, 64))


def test_the_builds_own_boxes_reproduce_the_nodes_of_seeded_scenes(tmp_path):
    for seed in range(32):
        check_build(pa.Scene(str(seeded_scene_file(tmp_path / f"s{seed}.scene.json", seed)), 64, 64))


def refused(word, call, *args, code=N.PT_ERR_ARG):
    with pytest.raises(pa.PathtracerError) as e:
        call(*args)
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_the_host_layer_refuses():
    nodes, boxes = random_tree(5, prims=9)
    arr = node_array(nodes)
    held = bytes(arr)
    refused("empty", pa.refit_boxes, [], boxes)
    refused("prim_count x 6", pa.refit_boxes, arr, boxes[:, :5])
    refused("out of range", pa.refit_boxes, arr, boxes[:8])                  # a leaf reaches past the boxes
    for (i, k), word in (((4, 2), "min[2]"), ((0, 4), "max[1]")):
        bad = boxes.copy()
        bad[i, k] = np.inf
        refused(f"primitive {i}", pa.refit_boxes, arr, bad)
        refused(word, pa.refit_boxes, arr, bad)
    bad = boxes.copy()
    bad[3, 0] = bad[3, 3] + F(1.0)
    refused("primitive 3", pa.refit_boxes, arr, bad)
    loop = list(nodes)
    i = next(k for k, n in enumerate(loop) if (n[3] >> 16) == 0)
    loop[i] = (loop[i][0], loop[i][1], i, loop[i][3])                        # a second child that is the node itself
    refused("not a tree", pa.refit_boxes, node_array(loop), boxes)
    far = list(nodes)
    far[i] = (far[i][0], far[i][1], len(nodes) + 5, far[i][3])
    refused("not a tree", pa.refit_boxes, node_array(far), boxes)
    assert bytes(arr) == held
    # the arguments of move_objects, before any native call (an object with no renderer behind it)
    pt = pa.Pathtracer.__new__(pa.Pathtracer)
    pt._group, pt._r, pt._ctx = None, None, None
    z = np.zeros((2, 3), dtype=F)
    refused("empty", pt.move_objects, [], z[:0], z[:0], z[:0])
    refused("indices", pt.move_objects, [0, -1], z, z, z)
    refused("position", pt.move_objects, [0, 1], z[:1], z, z)
    refused("rotation", pt.move_objects, [0, 1], z, z.T, z)
    refused("scale", pt.move_objects, [0, 1], z, z, np.zeros((2, 4), dtype=F))
    pt._group = 1
    for call, args in ((pt.move_objects, ([0], z[:1], z[:1], z[:1])), (pt.rebuild_scene, ()), (pt.refit_timing, ())):
        refused("device group", call, *args, code=N.PT_ERR_STATE)
    host = N.host()
    assert host.pth_renderer_move_objects(None, 1, None, None, None, None) == N.PT_ERR_ARG
    assert host.pth_renderer_rebuild_scene(None) == N.PT_ERR_ARG
    assert host.pth_renderer_object_transforms(None, None, None, None) == 0
    assert host.pth_refit_boxes(None, 0, None, 0) == N.PT_ERR_ARG
