"""Moving primitives without a rebuild (pt_set_primitive_boxes, pt_move_primitives; rule 10 of include/pt_hip.h) on
the GPU.  No tolerance anywhere: after a move the device's nodes, child-box records, primitive and material quads
equal, word for word, the numpy model (tests/refit_model.py) and a twin context that was given pt_set_scene with the
model's nodes and the new primitives; renders equal the twin's and the oracle's walking the same tree; a held
temporal history survives a move with a table exactly as it survives pt_set_scene_moved with the full table; every
refusal leaves every word and every held fact as it was.

The trees are the smallest at which each path can go wrong: a root that is a leaf, two leaves under a root, a leaf
of four, tests/bvh_edit.py's caterpillar at depth 33 (32 level launches) and at depth 2, trees with unreachable nodes
(an inserted orphan, malformed orphans at the end) whose words must come back unchanged, a leaf of 300 primitives (no
child-box records), a tree whose leaves are not in DFS order, one with an unreachable leaf of a valid range, and the host build of cornell_box and test_shapes.
"""
import ctypes as C

import numpy as np
import pytest

import bvh_edit as be
import pathtracercuda_amd as pa
import refit_model as rm
from oracle import pyoracle as po
from pathtracercuda_amd import _native as N
from test_bvh_validation import scene_nodes
from test_gpu_parity import _bvh_array, assert_bitexact

pytestmark = pytest.mark.gpu

W, H = 48, 32
F, U = np.float32, np.uint32
VARIANTS = (1, 20, 40, 41, 46, 60, 61)
fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def gpu_available():
    if pa.device_count() < 1:
        pytest.skip("no GPU")


# ---- scenes ------------------------------------------------------------------------------------------------
def make(spec):
    """The oracle's CpuHittable (transform rows, material, AABB) of (type, position, rotation, scale, material)."""
    L = po.lib()
    t, pos, rot, scale, (mtype, base, emis, rough, metal, tex) = spec
    mat, h = po.Material(), po.CpuHittable()
    L.or_material_make(mtype, po.f3(base), po.f3(emis), rough, metal, tex, C.byref(mat))
    L.or_cpu_hittable_make(t, po.f3(pos), po.f3(rot), po.f3(scale), C.byref(mat), C.byref(h))
    return h


def random_spec(rng, k, spread=2.0, size=(0.6, 1.1)):
    emis = [2.0, 1.6, 1.2] if k % 2 == 0 else [0.0, 0.0, 0.0]
    mat = (k % 3, [0.3 + 0.6 * rng.random() for _ in range(3)], emis, 0.2 + 0.7 * rng.random(), float(k % 2), 0)
    return (k % 7, list(rng.uniform(-spread, spread, 3)), list(rng.uniform(-3.0, 3.0, 3)), list(rng.uniform(*size, 3)), mat)


def aabb(h):
    return (tuple(h.aabbMin), tuple(h.aabbMax))


def boxes_of(elems):
    return np.array([list(h.aabbMin) + list(h.aabbMax) for h in elems], dtype=F)


def gpu_prims(elems):
    L = po.lib()
    out = (po.Hittable * len(elems))()
    for i, h in enumerate(elems):
        L.or_gpu_hittable(C.byref(h), C.byref(out[i]))
    return out


def pt_prims(elems):
    return (pa.PtHittable * len(elems)).from_buffer_copy(bytes(gpu_prims(elems)))


def leaf(elems, first, count):
    lo, hi = be._union([aabb(h) for h in elems[first:first + count]])
    return (lo, hi, first, count << 16)


def under_root(a, b, axis=0):
    lo, hi = be._union([(a[0], a[1]), (b[0], b[1])])
    return [(lo, hi, 2, axis << 8), a, b]


class Case:
    def __init__(self, name, specs, tree, path=None, osc=None):
        self.name, self.specs, self.path = name, list(specs), path
        self.elems = [make(s) for s in specs]
        self.nodes = tree(self.elems)
        self.osc = osc
        if osc is None:
            self.osc = po.OracleScene()
            po.lib().or_camera_make(po.f3([1.0, 0.5, 12.0]), po.f3([1.0, 0.0, 0.0]), po.f3([0.0, 1.0, 0.0]), 0.8,
                                    po.aspect_of(W, H), C.byref(self.osc.camera))
        self.cam = pa.PtCamera.from_buffer_copy(bytes(self.osc.camera))

    @property
    def interior(self):
        return sum(1 for n in self.nodes if (n[3] >> 16) == 0)

    def oracle(self, nodes, elems):
        """The oracle's scene walking `nodes` over `elems`."""
        o = po.OracleScene()
        o.textures, o.skybox, o.camera = self.osc.textures, self.osc.skybox, self.osc.camera
        arr = (po.BVHNode * len(nodes))()
        for i, (lo, hi, off, pca) in enumerate(nodes):
            arr[i].bmin[:], arr[i].bmax[:], arr[i].offset, arr[i].primitiveCountAxis = list(lo), list(hi), off, pca
        o.nodes, o.node_count, o.prims, o.prim_count = arr, len(nodes), gpu_prims(elems), len(elems)
        return o


def synthetic(name, count, tree, seed, **kw):
    rng = np.random.default_rng(seed)
    return Case(name, [random_spec(rng, k, **kw) for k in range(count)], tree)


def singles(elems):
    return [leaf(elems, k, 1) for k in range(len(elems))]


def file_case(scenes, name):
    """The host build's tree of a shipped scene: the oracle's build is the same one, word for word."""
    path = scenes / f"{name}.scene.json"
    osc, si = po.load_scene(path, W, H), po.parse_scene(path)
    taken, specs = set(), []
    for e in range(osc.prim_count):                # which object of the file each element is
        i = next(i for i in range(len(osc.cpu)) if i not in taken and bytes(osc.cpu[i]) == bytes(osc.bvh_elements[e]))
        taken.add(i)
        mat = (si.material_types[i], list(si.base_colors[i]), list(si.emissives[i]), si.roughness[i], si.metalness[i],
               si.texture_handles[i])
        specs.append((si.types[i], list(si.positions[i]), list(si.rotations[i]), list(si.scales[i]), mat))
    case = Case(name, specs, lambda elems: scene_nodes(osc), path=path, osc=osc)
    assert all(bytes(a) == bytes(osc.bvh_elements[e]) for e, a in enumerate(case.elems))
    return case


def not_dfs(elems):
    a, b = leaf(elems, 2, 2), leaf(elems, 0, 2)            # the first child holds the higher primitives
    return under_root(a, b)


def orphan_leaf(elems):
    """Two leaves under a root, then a leaf nothing names, with a valid primitive range and a box of its own: a refit
    that walks the node array instead of the tree would give it primitive 0's box."""
    return under_root(leaf(elems, 0, 2), leaf(elems, 2, 1)) + [((-7.0, -8.0, -9.0), (7.5, 8.5, 9.5), 0, 1 << 16)]


CASES = {
    "root_leaf": lambda s: synthetic("root_leaf", 3, lambda e: [leaf(e, 0, 3)], 1),
    "two_leaves": lambda s: synthetic("two_leaves", 2, lambda e: under_root(leaf(e, 0, 1), leaf(e, 1, 1)), 2),
    "leaf_of_four": lambda s: synthetic("leaf_of_four", 5, lambda e: under_root(leaf(e, 0, 4), leaf(e, 4, 1), 1), 3),
    "caterpillar_33": lambda s: synthetic("caterpillar_33", 33, lambda e: be.caterpillar(singles(e), 33), 4),
    "caterpillar_2": lambda s: synthetic("caterpillar_2", 4, lambda e: be.caterpillar(singles(e), 2), 5),
    "orphans": lambda s: synthetic("orphans", 7, lambda e: be.append_malformed_orphans(
        be.insert_orphan(be.caterpillar(singles(e), 6), 2)), 6),
    "big_leaf": lambda s: synthetic("big_leaf", 301, lambda e: under_root(leaf(e, 0, 300), leaf(e, 300, 1), 2), 7,
                                    size=(0.05, 0.12)),
    "not_dfs": lambda s: synthetic("not_dfs", 4, not_dfs, 8),
    "orphan_leaf": lambda s: synthetic("orphan_leaf", 3, orphan_leaf, 9),
    "cornell_box": lambda s: file_case(s, "cornell_box"),
    "test_shapes": lambda s: file_case(s, "test_shapes"),
}
_cases = {}


@pytest.fixture(scope="module")
def case_of(gpu_available, scenes):
    def get(name):
        if name not in _cases:
            _cases[name] = CASES[name](scenes)
        return _cases[name]
    return get


# ---- moves -------------------------------------------------------------------------------------------------
def moved_spec(rng, spec, how):
    t, pos, rot, scale, mat = spec
    if isinstance(how, tuple):                      # ("far", x): to x, beyond the old root box
        return (t, [how[1], pos[1] + 0.5, pos[2] - 1.0], rot, scale, mat)
    if how == "retype":                             # another shape and another material
        mtype, base, emis, rough, metal, tex = mat
        return ((t + 3) % 7, pos, rot, scale, ((mtype + 1) % 3, base[::-1], [1.5, 1.5, 0.5], 0.5 * rough, 1.0 - metal, tex))
    return (t, [p + d for p, d in zip(pos, rng.uniform(-0.8, 0.8, 3))], [r + d for r, d in zip(rot, rng.uniform(-1.0, 1.0, 3))],
            [s * f for s, f in zip(scale, rng.uniform(0.7, 1.3, 3))], mat)


def plan_move(case, which, seed, how="jitter", specs=None):
    """(indices, new specs of every element, new elements of every element)."""
    rng = np.random.default_rng(seed)
    specs = list(case.specs if specs is None else specs)
    for j in which:
        specs[j] = moved_spec(rng, specs[j], how)
    return np.array(list(which), dtype=U), specs, [make(s) for s in specs]


def model_nodes(nodes, elems):
    lo, hi, off, pca = rm.from_tuples(nodes)
    nl, nh = rm.refit(lo, hi, off, pca, boxes_of(elems))
    return rm.to_tuples(nl, nh, off, pca)


# ---- the device --------------------------------------------------------------------------------------------
def lib():
    return N.hip()


def error(pt):
    return lib().pt_last_error(pt._ctx).decode()


def fresh(case, nodes=None, elems=None):
    """A context holding the case's textures and sky and the given tree and primitives."""
    pt = pa.Pathtracer(W, H)
    if case.path is not None:
        pt.load_scene(str(case.path))
    nodes, elems = case.nodes if nodes is None else nodes, case.elems if elems is None else elems
    N.check_ctx(lib().pt_set_scene(pt._ctx, _bvh_array(nodes), len(nodes), pt_prims(elems), len(elems)), pt._ctx)
    return pt


def set_boxes(pt, elems):
    b = boxes_of(elems)
    N.check_ctx(lib().pt_set_primitive_boxes(pt._ctx, b.ctypes.data_as(fp)), pt._ctx)


def move_call(pt, index, elems, rows=None, prev=None, boxes=None):
    """pt_move_primitives of elements `index` to their records in `elems` (the whole scene's elements)."""
    index = np.ascontiguousarray(index, dtype=U)
    sub = [elems[int(j)] for j in index]
    b = np.ascontiguousarray(boxes_of(sub) if boxes is None else boxes, dtype=F)
    return lib().pt_move_primitives(pt._ctx, len(index), index.ctypes.data_as(up), pt_prims(sub), b.ctypes.data_as(fp),
                                    None if rows is None else rows.ctypes.data_as(fp), None if prev is None else prev.ctypes.data_as(up))


SENTINEL = F(-77.0)


def read_all(pt, case):
    """(nodes as bytes, records, primitive and material quads) the device holds."""
    n, np_ = len(case.nodes), len(case.elems)
    nodes = (pa.PtBvhNode * n)()
    records = np.full((max(case.interior, 1), 16), SENTINEL, dtype=F)
    N.check_ctx(lib().pt_read_bvh(pt._ctx, nodes, records.ctypes.data_as(fp)), pt._ctx)
    prims = np.zeros((np_, 28), dtype=F)
    for i in range(np_):
        N.check_ctx(lib().pt_read_primitive(pt._ctx, i, prims[i].ctypes.data_as(fp)), pt._ctx)
    return bytes(nodes), records, prims


def assert_same_device_words(got, want, what):
    assert got[0] == want[0], f"{what}: nodes differ"
    assert rm.same_words(got[1], want[1]), f"{what}: records differ at {np.argwhere(rm.bits(got[1]) != rm.bits(want[1]))[:4]}"
    assert rm.same_words(got[2], want[2]), f"{what}: primitive quads differ"


def check_against_model_and_twin(pt, case, nodes_before, records_before, elems, what):
    """The device's words after a move to `elems`: the model's, and a twin's that was given the model's tree."""
    want_nodes = model_nodes(nodes_before, elems)
    got = read_all(pt, case)
    assert got[0] == bytes(_bvh_array(want_nodes)), f"{what}: nodes differ from the model"
    lo, hi, off, pca = rm.from_tuples(want_nodes)
    if rm.has_records(off, pca, len(elems)):
        assert rm.same_words(got[1], rm.refit_records(records_before, lo, hi, off, pca)), f"{what}: records differ from the model"
        assert rm.same_words(got[1], rm.records(lo, hi, off, pca)), f"{what}: records differ from pt_set_scene's restated"
    else:
        assert (got[1] == SENTINEL).all()               # no records are held: nothing is read
    twin = fresh(case, want_nodes, elems)
    assert_same_device_words(got, read_all(twin, case), f"{what}, against the twin")
    return want_nodes, twin


# ---- 1. device words ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_device_words_equal_the_model_and_the_twin(case_of, name):
    case = case_of(name)
    n = len(case.elems)
    pt = fresh(case)
    assert not lib().pt_holds_primitive_boxes(pt._ctx)
    set_boxes(pt, case.elems)
    assert lib().pt_holds_primitive_boxes(pt._ctx)
    before = read_all(pt, case)
    assert before[0] == bytes(_bvh_array(case.nodes))       # the upload of the boxes changed nothing
    nodes, specs, records = case.nodes, case.specs, before[1]
    some = sorted(set(int(x) for x in np.random.default_rng(n).choice(n, size=max(1, n // 3), replace=False)))
    moves = [([n - 1], "jitter"), (some, "jitter"), (list(range(n)), "jitter"), ([0], "retype"),
             ([n // 2], ("far", case.nodes[0][1][0] + 2.0))]
    for k, (which, how) in enumerate(moves):
        index, specs, elems = plan_move(case, which, 100 * k + n, how, specs)
        index = index[::-1].copy()                          # (the order of the call's entries does not matter)
        assert move_call(pt, index, elems) == N.PT_OK, error(pt)
        assert lib().pt_holds_primitive_boxes(pt._ctx)      # a move keeps the boxes
        nodes, twin = check_against_model_and_twin(pt, case, nodes, records, elems, f"{name}, move {k} ({how})")
        records = read_all(pt, case)[1]
    # an identity move: every word is what it was
    held = read_all(pt, case)
    assert move_call(pt, np.arange(n, dtype=U), elems) == N.PT_OK, error(pt)
    assert_same_device_words(read_all(pt, case), held, f"{name}, the identity move")
    ms = (C.c_float * 3)(-1.0)
    assert lib().pt_read_refit_timing(pt._ctx, ms) == N.PT_OK and ms[0] >= 0.0


# ---- 2. renders --------------------------------------------------------------------------------------------
def render_twice(pt, cam, variant):
    pt.set_kernel_variant(variant)
    pt.render(cam, 4, True)
    pt.render(cam, 4, False)
    return pt.accum(), pt.rng_state()


def same_or_both_nan(a, b):
    return bool(np.all((rm.bits(a) == rm.bits(b)) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("name", list(CASES))
def test_renders_equal_the_twin_and_the_oracle(case_of, name):
    case = case_of(name)
    n = len(case.elems)
    pt = fresh(case)
    set_boxes(pt, case.elems)
    rng0 = pt.rng_state()
    # one primitive leaves the old root box, the others jitter: rootBox is checked by the render
    index, specs, _ = plan_move(case, [n - 1], 5, ("far", case.nodes[0][1][0] + 2.0))
    index, specs, elems = plan_move(case, [j for j in range(n) if j != n - 1][:max(1, n // 2)], 6, "jitter", specs)
    index = np.array(sorted(set(index) | {n - 1}), dtype=U)
    old_lo, old_hi = case.nodes[0][0], case.nodes[0][1]
    assert any(elems[n - 1].aabbMax[k] > old_hi[k] or elems[n - 1].aabbMin[k] < old_lo[k] for k in range(3))
    assert move_call(pt, index, elems) == N.PT_OK, error(pt)
    nodes = model_nodes(case.nodes, elems)
    twin = fresh(case, nodes, elems)
    osc = case.oracle(nodes, elems)
    ref = po.OracleRenderer(osc, W, H)
    ref.render(osc.camera, 4, True, chunks=2)
    want, want_rng = ref.accum, ref.rng_array()
    for variant in VARIANTS:
        for p in (pt, twin):
            p.set_rng_state(rng0)
        got, got_rng = render_twice(pt, case.cam, variant)
        tw, tw_rng = render_twice(twin, case.cam, variant)
        what = f"{name}, variant {variant}"
        assert same_or_both_nan(got, tw) and np.array_equal(got_rng, tw_rng), f"{what}: differs from the twin"
        assert same_or_both_nan(got, want), f"{what}: differs from the oracle"
        assert np.array_equal(got_rng, want_rng), f"{what}: RNG differs from the oracle"
    hit = np.isfinite(want[..., :3]).all(-1) & (want[..., :3].sum(-1) > 0)
    assert hit.sum() >= 4            # the frame is not empty (the smallest emissive object covers more pixels than that)


# ---- 3. the temporal history -------------------------------------------------------------------------------
PARAMS = dict(alpha_min=0.1, max_history=16, sigma_plane=0.05, normal_cos_min=0.9, demodulate=True, same_primitive=True)


def frame(p, cam, moments):
    p.render(cam, 1, True)
    p.features(cam)
    return p.temporal(variance=True, min_temporal=3, **PARAMS) if moments else p.temporal(**PARAMS)


def motion_of(case, index, elems):
    """Rule 7's entries of the moved elements, and the full table the twin needs."""
    n = len(case.elems)
    old, new = pt_prims(case.elems), pt_prims(elems)
    rows, valid = pa.motion_table([old[int(j)] for j in index], [new[int(j)] for j in index])
    prev = np.where(valid, index, U(NONE)).astype(U)
    full = np.tile(np.eye(3, 4, dtype=F), (n, 1, 1))
    full_prev = np.arange(n, dtype=U)
    full[index], full_prev[index] = rows, prev
    return np.ascontiguousarray(rows), prev, np.ascontiguousarray(full), full_prev


@pytest.mark.parametrize("moments", [False, True], ids=["temporal", "moments"])
@pytest.mark.parametrize("name", ["leaf_of_four", "cornell_box"])
def test_the_history_survives_a_move_as_it_survives_set_scene_moved(case_of, name, moments):
    case = case_of(name)
    n = len(case.elems)
    pt, twin = fresh(case), fresh(case)
    set_boxes(pt, case.elems)
    for p in (pt, twin):
        frame(p, case.cam, moments)
    which = [n - 1, 0] if name == "leaf_of_four" else [n - 1, n - 3]
    index, specs, elems = plan_move(case, which, 11)
    rows, prev, full, full_prev = motion_of(case, index, elems)
    assert move_call(pt, index, elems, rows, prev) == N.PT_OK, error(pt)
    nodes = model_nodes(case.nodes, elems)
    N.check_ctx(lib().pt_set_scene_moved(twin._ctx, _bvh_array(nodes), len(nodes), pt_prims(elems), n, full.ctypes.data_as(fp),
                                         full_prev.ctypes.data_as(up)), twin._ctx)
    assert pt.holds_motion() and twin.holds_motion()
    with pytest.raises(pa.PathtracerError):                  # the feature planes are stale after a move
        pt.temporal(**PARAMS)
    assert pt.holds_motion()                                 # (and the refusal ended nothing)
    got, want = frame(pt, case.cam, moments), frame(twin, case.cam, moments)
    assert pt.history_used and twin.history_used and not pt.holds_motion()
    assert rm.same_words(got, want) or same_or_both_nan(got, want)
    planes, twin_planes = pt.temporal_history(), twin.temporal_history()
    assert (planes[3] is not None) == moments and (twin_planes[3] is not None) == moments
    for k, (a, b) in enumerate(zip(planes, twin_planes)):
        assert a is None or same_or_both_nan(a, b), f"history plane {k}"
    assert (got[..., 3] > 1).any()                           # some pixel's history is longer than this frame
    # a second move before the next pass ends the history; a move without rows ends it too
    frame(pt, case.cam, moments)
    assert move_call(pt, index, elems, rows, prev) == N.PT_OK and pt.holds_motion()
    assert move_call(pt, index, elems, rows, prev) == N.PT_OK and not pt.holds_motion()
    frame(pt, case.cam, moments)
    assert not pt.history_used
    assert move_call(pt, index, elems) == N.PT_OK and not pt.holds_motion()
    frame(pt, case.cam, moments)
    assert not pt.history_used


# ---- 4. refusals and state ---------------------------------------------------------------------------------
def test_every_refusal_changes_nothing(case_of):
    case = case_of("leaf_of_four")
    n = len(case.elems)
    pt = fresh(case)
    index, specs, elems = plan_move(case, [1, 4], 21)
    rows, prev, _, _ = motion_of(case, index, elems)
    # before any boxes are held
    assert move_call(pt, index, elems) == N.PT_ERR_STATE and "boxes" in error(pt)
    ms = (C.c_float * 3)()
    assert lib().pt_read_refit_timing(pt._ctx, ms) == N.PT_ERR_STATE
    # pt_set_primitive_boxes names the primitive and the component
    b = boxes_of(case.elems)
    for (i, k), word in (((2, 1), "min[1]"), ((3, 5), "max[2]")):
        bad = b.copy()
        bad[i, k] = np.nan
        assert lib().pt_set_primitive_boxes(pt._ctx, bad.ctypes.data_as(fp)) == N.PT_ERR_ARG
        assert f"primitive {i}" in error(pt) and word in error(pt), error(pt)
    bad = b.copy()
    bad[1, 0], bad[1, 3] = bad[1, 3] + 1.0, bad[1, 0]
    assert lib().pt_set_primitive_boxes(pt._ctx, bad.ctypes.data_as(fp)) == N.PT_ERR_ARG and "primitive 1" in error(pt)
    assert lib().pt_set_primitive_boxes(pt._ctx, None) == N.PT_ERR_ARG
    assert not lib().pt_holds_primitive_boxes(pt._ctx)
    empty = pa.Pathtracer(W, H)
    assert lib().pt_set_primitive_boxes(empty._ctx, b.ctypes.data_as(fp)) == N.PT_ERR_STATE and "no scene" in error(empty)
    set_boxes(pt, case.elems)
    frame(pt, case.cam, False)
    assert move_call(pt, index, elems, rows, prev) == N.PT_OK and pt.holds_motion()
    pt.features(case.cam)
    held = read_all(pt, case)

    def refused(code, word, rc):
        assert rc == code and word in error(pt), (rc, error(pt))
        assert_same_device_words(read_all(pt, case), held, word)
        assert pt.holds_motion() and lib().pt_holds_primitive_boxes(pt._ctx)      # no event was raised

    sub, sb = pt_prims([elems[1], elems[4]]), boxes_of([elems[1], elems[4]])
    ip, bp, rp, pp = index.ctypes.data_as(up), sb.ctypes.data_as(fp), rows.ctypes.data_as(fp), prev.ctypes.data_as(up)
    call = lib().pt_move_primitives
    refused(N.PT_ERR_ARG, "null", call(pt._ctx, 2, None, sub, bp, None, None))
    refused(N.PT_ERR_ARG, "null", call(pt._ctx, 2, ip, None, bp, None, None))
    refused(N.PT_ERR_ARG, "null", call(pt._ctx, 2, ip, sub, None, None, None))
    refused(N.PT_ERR_ARG, "together", call(pt._ctx, 2, ip, sub, bp, rp, None))
    refused(N.PT_ERR_ARG, "count is 0", call(pt._ctx, 0, ip, sub, bp, None, None))
    refused(N.PT_ERR_ARG, "twice", move_call(pt, [1, 1], elems))
    refused(N.PT_ERR_ARG, f"index {n}", move_call(pt, [1, n], elems + [elems[0]]))
    bad_prev = prev.copy()
    bad_prev[0] = 0
    refused(N.PT_ERR_ARG, "prev_index", move_call(pt, index, elems, rows, bad_prev))
    nb = sb.copy()
    nb[1, 4] = np.inf
    refused(N.PT_ERR_ARG, f"primitive {int(index[1])}", move_call(pt, index, elems, boxes=nb))
    for field, value, word in (("type", 7, "hittable type"), ("texture_index", 65, "texture index")):
        wrong = pt_prims([elems[1], elems[4]])
        setattr(wrong[1], field, value)
        refused(N.PT_ERR_ARG, word, call(pt._ctx, 2, ip, wrong, bp, None, None))
    wrong = pt_prims([elems[1], elems[4]])
    wrong[0].inv_transform_rows[2][1] = float("nan")
    refused(N.PT_ERR_ARG, "inv_transform_rows[2][1]", call(pt._ctx, 2, ip, wrong, bp, None, None))
    # and the history is still there for the next pass
    frame(pt, case.cam, False)
    assert pt.history_used


def test_what_ends_the_boxes(case_of):
    case = case_of("two_leaves")
    pt = fresh(case)
    held = lambda: bool(lib().pt_holds_primitive_boxes(pt._ctx))
    prims, n = pt_prims(case.elems), len(case.elems)
    arr = _bvh_array(case.nodes)
    rows, prev = np.tile(np.eye(3, 4, dtype=F), (n, 1, 1)), np.arange(n, dtype=U)
    tex = np.ones((2, 2, 4), dtype=F)
    enders = (lambda: lib().pt_set_scene(pt._ctx, arr, len(case.nodes), prims, n),
              lambda: lib().pt_set_scene_moved(pt._ctx, arr, len(case.nodes), prims, n, rows.ctypes.data_as(fp), prev.ctypes.data_as(up)),
              lambda: lib().pt_set_texture(pt._ctx, 1, tex.ctypes.data_as(fp), 2, 2))
    for end in enders:
        set_boxes(pt, case.elems)
        assert held()
        assert move_call(pt, [0], case.elems) == N.PT_OK and held()
        pt.render(case.cam, 1, True)
        pt.features(case.cam)
        assert held()
        assert end() == N.PT_OK and not held()
        assert move_call(pt, [0], case.elems) == N.PT_ERR_STATE
    assert lib().pt_holds_primitive_boxes(None) == 0


# ---- 5. the host layer and Python --------------------------------------------------------------------------
import json

CUBE, SPHERE = 6, 8                                  # the tall cube and the sphere of cornell_box.scene.json


def moved_file(tmp_path, scenes, name, shift, turn=(0.0, 0.0, 0.0)):
    d = json.loads((scenes / "cornell_box.scene.json").read_text())
    d["objects"][CUBE]["position"] = [p + s for p, s in zip(d["objects"][CUBE]["position"], shift)]
    d["objects"][SPHERE]["rotation"] = list(turn)
    path = tmp_path / f"{name}.scene.json"
    path.write_text(json.dumps(d))
    return str(path)


def tree_words(pt):
    nodes, prims = pt.bvh()
    return bytes(nodes), bytes(prims)


def device_nodes(pt):
    nodes, _ = pt.bvh()
    out = (pa.PtBvhNode * len(nodes))()
    N.check_ctx(lib().pt_read_bvh(pt._ctx, out, None), pt._ctx)
    return bytes(out)


def same_tree_as_values(a, b):
    """Nodes equal as float values (a refit and a build may differ in the sign of a zero), offsets and counts as words."""
    (an, ap), (bn, bp) = a.bvh(), b.bvh()
    f = lambda arr: np.frombuffer(bytes(arr), dtype=F).reshape(-1, 8)
    return len(an) == len(bn) and np.array_equal(f(an)[:, :6], f(bn)[:, :6]) and \
        np.array_equal(f(an)[:, 6:].view(U), f(bn)[:, 6:].view(U)) and bytes(ap) == bytes(bp)


def py_frame(p, cam):
    p.render(cam, 1, True)
    p.features(cam)
    return p.temporal(**PARAMS)


def move_to(pt, target, objects):
    pos, rot, scale = target.object_transforms()
    pt.move_objects(objects, pos[objects], rot[objects], scale[objects])


@pytest.mark.parametrize("shift,turn", [((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), ((0.01, 0.0, 0.01), (10.0, 25.0, 0.0))],
                         ids=["by_zero", "a_small_step"])
def test_move_objects_equals_load_scene_moved_where_the_trees_coincide(gpu_available, scenes, tmp_path, shift, turn):
    base = str(scenes / "cornell_box.scene.json")
    path = moved_file(tmp_path, scenes, "moved", shift, turn)
    pt, twin = pa.Pathtracer(W, H), pa.Pathtracer(W, H)
    cam = pt.load_scene(base)
    twin.load_scene(base)
    for p in (pt, twin):
        py_frame(p, cam)
    twin.load_scene_moved(path)
    move_to(pt, twin, [CUBE, SPHERE])
    assert same_tree_as_values(pt, twin)                     # the step does not change the SAH partition
    assert device_nodes(pt) == tree_words(pt)[0]             # the class mirrors the device
    for a, b in zip(pt.object_transforms(), twin.object_transforms()):
        assert rm.same_words(a, b)
    # the motion table: pa.motion_table of the two pose sets, permuted by the object-to-primitive map
    old, new = pa.Scene(base, W, H).objects()[0], pa.Scene(path, W, H).objects()[0]
    n = len(new)
    rows, valid = pa.motion_table(list(old)[:n], list(new)[:n])
    prims = pt.bvh()[1]
    where = {bytes(prims[p]): p for p in range(n)}
    perm = np.array([where[bytes(new[k])] for k in range(n)])
    got_rows, got_prev = pt.motion_table()
    assert valid.all() and rm.same_words(got_rows[perm], rows) and np.array_equal(got_prev[perm], perm)
    for a, b in zip(pt.motion_table(), twin.motion_table()):
        assert rm.same_words(a, b)
    assert pt.holds_motion() and twin.holds_motion()
    rng = twin.rng_state()
    pt.set_rng_state(rng)
    got, want = py_frame(pt, cam), py_frame(twin, cam)
    assert pt.history_used and twin.history_used
    assert same_or_both_nan(pt.accum(), twin.accum()) and np.array_equal(pt.rng_state(), twin.rng_state())
    assert same_or_both_nan(got, want)
    assert pt.refit_timing() >= 0.0


def test_move_objects_equals_the_oracle_on_the_refitted_tree_and_rebuild_scene_returns_to_the_builds(gpu_available, scenes, tmp_path):
    base = str(scenes / "cornell_box.scene.json")
    path = moved_file(tmp_path, scenes, "far", (-0.9, 0.0, 0.5), (40.0, 0.0, 15.0))
    pt, target, fresh_pt = pa.Pathtracer(W, H), pa.Pathtracer(W, H), pa.Pathtracer(W, H)
    cam = pt.load_scene(base)
    target.load_scene(path)
    py_frame(pt, cam)
    before = tree_words(pt)
    # a refusal changes nothing of the class
    pos, rot, scale = target.object_transforms()
    for bad in ([CUBE, CUBE], [CUBE, 99]):
        with pytest.raises(pa.PathtracerError) as e:
            pt.move_objects(bad, pos[[CUBE, SPHERE]], rot[[CUBE, SPHERE]], scale[[CUBE, SPHERE]])
        assert e.value.code == N.PT_ERR_ARG
    zero = scale[[CUBE]].copy()
    zero[0, 1] = 0.0
    with pytest.raises(pa.PathtracerError) as e:                 # a zero scale: the inverse transform is not finite
        pt.move_objects([CUBE], pos[[CUBE]], rot[[CUBE]], zero)
    assert e.value.code == N.PT_ERR_ARG and "not finite" in str(e.value)
    assert tree_words(pt) == before and device_nodes(pt) == before[0] and pt.motion_table() is None
    move_to(pt, target, [CUBE, SPHERE])
    assert not same_tree_as_values(pt, target)               # the build partitions these poses otherwise
    assert device_nodes(pt) == tree_words(pt)[0]
    nodes, prims = pt.bvh()
    osc = po.load_scene(path, W, H)
    osc.nodes = (po.BVHNode * len(nodes)).from_buffer_copy(bytes(nodes))
    osc.prims = (po.Hittable * len(prims)).from_buffer_copy(bytes(prims))
    osc.node_count, osc.prim_count = len(nodes), len(prims)
    ref = po.OracleRenderer(osc, W, H)
    ref.render(osc.camera, 4, True, chunks=2)
    rng0 = fresh_pt.rng_state()
    pt.set_rng_state(rng0)
    got, got_rng = render_twice(pt, cam, 0)
    assert same_or_both_nan(got, ref.accum) and np.array_equal(got_rng, ref.rng_array())
    # rebuild_scene: the build's tree of the moved poses, bit for bit, and the history kept
    pt.features(cam)
    pt.temporal(**PARAMS)
    pt.rebuild_scene()
    fresh_pt.load_scene(path)
    assert tree_words(pt) == tree_words(fresh_pt) and device_nodes(pt) == device_nodes(fresh_pt)
    assert pt.holds_motion()
    pt.set_rng_state(rng0)
    got, got_rng = render_twice(pt, cam, 0)
    want, want_rng = render_twice(fresh_pt, cam, 0)
    assert same_or_both_nan(got, want) and np.array_equal(got_rng, want_rng)
    pt.features(cam)
    pt.temporal(**PARAMS)
    assert pt.history_used


# ---- the rule's compares, where only the sign of a zero can tell them apart ----------------------------------
@pytest.mark.parametrize("name", ["leaf_of_four", "caterpillar_2", "orphans"])
def test_zeros_of_both_signs_follow_the_rule(case_of, name):
    """`<` against `<=`, and which child or primitive a tie keeps, show only where two boxes hold +0.0 and -0.0 on the
    same axis.  The boxes are the caller's, so the test gives such boxes (nothing is rendered with them)."""
    case = case_of(name)
    n = len(case.elems)
    pt = fresh(case)
    set_boxes(pt, case.elems)
    records = read_all(pt, case)[1]
    zeros = np.array([0.0, -0.0], dtype=F)
    for flip in (0, 1):
        boxes = np.zeros((n, 6), dtype=F)
        for j in range(n):
            boxes[j, :3] = zeros[(j + flip + np.arange(3)) % 2]
            boxes[j, 3:] = zeros[(j + flip + 1 + np.arange(3)) % 2]
        assert move_call(pt, np.arange(n, dtype=U), case.elems, boxes=boxes) == N.PT_OK, error(pt)
        lo, hi, off, pca = rm.from_tuples(case.nodes)
        nl, nh = rm.refit(lo, hi, off, pca, boxes)
        got = read_all(pt, case)
        assert got[0] == bytes(_bvh_array(rm.to_tuples(nl, nh, off, pca))), f"{name}, flip {flip}: nodes"
        assert rm.same_words(got[1], rm.refit_records(records, nl, nh, off, pca)), f"{name}, flip {flip}: records"
        signs = np.signbit(np.concatenate([nl, nh])[np.concatenate([rm.depths(off, pca) >= 0] * 2)])
        assert signs.any() and not signs.all()


# ---- a context of a device group is refused by name ----------------------------------------------------------
def test_a_device_group_is_refused_and_nothing_changes(gpu_available, scenes):
    g = pa.Pathtracer(W, H, devices=[0])                     # a one-device group: the whole group path on one GPU
    g.load_scene(str(scenes / "cornell_box.scene.json"))
    ctx = lib().pt_group_context(g._group, 0)
    scene = pa.Scene(str(scenes / "cornell_box.scene.json"), W, H)
    nodes, prims = scene.bvh()
    n, nn = scene.object_count, scene.node_count

    def words():
        out = (pa.PtBvhNode * nn)()
        assert lib().pt_read_bvh(ctx, out, None) == N.PT_OK
        quads = np.zeros((n, 28), dtype=F)
        for i in range(n):
            assert lib().pt_read_primitive(ctx, i, quads[i].ctypes.data_as(fp)) == N.PT_OK
        return bytes(out), quads.tobytes()

    held = words()
    assert held[0] == bytes(nodes)[:32 * nn]
    boxes = np.tile(np.array([-1, -1, -1, 1, 1, 1], dtype=F), (n, 1))
    assert lib().pt_set_primitive_boxes(ctx, boxes.ctypes.data_as(fp)) == N.PT_ERR_STATE
    assert "device group" in lib().pt_last_error(ctx).decode()
    assert not lib().pt_holds_primitive_boxes(ctx)
    index = np.array([0], dtype=U)
    rc = lib().pt_move_primitives(ctx, 1, index.ctypes.data_as(up), prims, boxes.ctypes.data_as(fp), None, None)
    assert rc == N.PT_ERR_STATE and "device group" in lib().pt_last_error(ctx).decode()
    assert words() == held
    # the host layer, past Python's own check: the C functions refuse by the same name
    pos = np.zeros((1, 3), dtype=F)
    one = np.ones((1, 3), dtype=F)
    rc = N.host().pth_renderer_move_objects(g._r, 1, index.ctypes.data_as(up), pos.ctypes.data_as(fp), pos.ctypes.data_as(fp),
                                            one.ctypes.data_as(fp))
    assert rc == N.PT_ERR_STATE and "device group" in N.host().pth_last_error().decode()
    assert N.host().pth_renderer_rebuild_scene(g._r) == N.PT_ERR_STATE and "device group" in N.host().pth_last_error().decode()
    for call, args in ((g.move_objects, ([0], pos, pos, one)), (g.rebuild_scene, ()), (g.refit_timing, ())):
        with pytest.raises(pa.PathtracerError) as e:
            call(*args)
        assert e.value.code == N.PT_ERR_STATE and "device group" in str(e.value)
    assert words() == held
    # and a renderer without a scene says so, whatever the indices
    empty = pa.Pathtracer(W, H)
    far = np.array([7], dtype=U)
    rc = N.host().pth_renderer_move_objects(empty._r, 1, far.ctypes.data_as(up), pos.ctypes.data_as(fp), pos.ctypes.data_as(fp),
                                            one.ctypes.data_as(fp))
    assert rc == N.PT_ERR_STATE and "no scene" in N.host().pth_last_error().decode()
