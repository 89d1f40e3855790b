"""Scenes with caller BVHs of chosen size and depth, and the documented build policy as a table.

The value axis (every shape, material, tie, the float range) has its own scene builders; this one
moves along the SIZE axis, where pt_kernels.hip decides how a launch runs: interior-node count I
(child-box records, 64 B each), LDS stack rows R (ctx->stackDepth), node and primitive counts.

Scene (scene()):
  * S "shell" spheres centred on the camera, radii growing with the shell index (or shuffled).  The
    camera is inside every shell, so a shell's leaf always returns its far root (Hittable.inl:152-158,
    accepted whatever t_max is): leaves raise t_max all the time and repair_pending runs at depth.
    One shell is weakly emissive and the sky is kept, so paths carry light.
  * then the first `content` objects of tools/make_stress_scene.make_scene(grid, seed).
  * the camera sits on the diagonal of direction octant `octant` (bit a set: ray directions negative
    along axis a), looks at the origin with a 30 degree field of view: every primary ray of a 1.6:1
    image lies strictly inside that octant.
Tree:
  * a spine of S interior nodes, each with its shell's leaf on one side and the rest on the other,
    then a median split over the content's leaves with the larger half on the same side.  The split
    axes cycle through `axes`; at a node with axis a the deep side is the SECOND child when the
    octant's rays are negative along a (trace.cu:69-76 visits the second child first then) and the
    first otherwise.  So for the octant's rays the near child is the deep one at every node, the far
    children pile up, and R = S + ceil(log2(leaves)) (the +1 of pt_set_scene's bound is the write
    above the top at the deepest interior node, whose pend is R - 1).
  * primitives in DFS order; leaf sizes given by the caller (1..255 inside the child-box encoding,
    256+ outside it); `swap` exchanges the primitive ranges of the content root's two subtrees (the
    tree stays valid, dfsOrder becomes false).
  * boxes are computed here from position and scale, padded; parity does not depend on tight boxes
    because kernel and oracle get the same nodes.  enclose="all" pads every content node's box so that
    it contains the camera: then every primary ray meets every box on its path and the walk's rows are
    as full as the bound says (tests/test_size_scenes.py proves it with the CPU walk model), at the
    price of every ray testing every primitive.  enclose="path" (the default) pads only the deepest
    leaf, and with it its ancestors: the reference's walk, which pushes a far child whether or not
    the ray meets it, still fills its stack to R on every primary ray.

Policy (expected_build()): a transcription BY HAND of the comments above picked_build and
small_grid_build (csrc/pt_launch_plan.h) and launch_one and of DESIGN.md §4.1/§4.4 -- it never calls the library.  A policy
change must edit it knowingly.
"""
from __future__ import annotations

import importlib.util
import json
import pathlib
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import bvh_edit as be

ROOT = pathlib.Path(__file__).resolve().parents[1]
CAM_DIST = 9.0
FOVY = 30.0


def _stress_module():
    spec = importlib.util.spec_from_file_location("make_stress_scene", ROOT / "tools" / "make_stress_scene.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ceil_log2(n: int) -> int:
    return (n - 1).bit_length()


def solve(I: int, R: int) -> Tuple[int, int]:
    """(S, leaves) of a scene with I interior nodes and R stack rows: I = S + leaves - 1 and
    R = S + ceil(log2(leaves))."""
    for S in range(0, R + 1):
        L = I - S + 1
        if L >= 2 and S + ceil_log2(L) == R:
            return S, L
    raise ValueError(f"no spine/leaf split gives I = {I}, R = {R}")


def camera_position(octant: int) -> List[float]:
    return [CAM_DIST if (octant >> a) & 1 else -CAM_DIST for a in range(3)]


class SizeScene:
    """What scene() returns: the JSON document, the caller BVH as tests/bvh_edit.py node tuples, the
    file-order object index of every primitive slot, and the sizes the policy reads."""

    def __init__(self) -> None:
        self.doc: Dict = {}
        self.nodes: List[be.Node] = []
        self.order: List[int] = []
        self.S = 0
        self.leaves = 0
        self.octant = 7

    @property
    def node_count(self) -> int:
        return len(self.nodes)

    @property
    def prim_count(self) -> int:
        return len(self.order)

    @property
    def interior(self) -> int:
        return sum(1 for n in self.nodes if (n[3] >> 16) == 0)

    @property
    def rows(self) -> int:
        """R by the formula in the module docstring (the tests compare it with stack_rows_tree)."""
        return max(1, self.S + ceil_log2(self.leaves))

    @property
    def child_box_ok(self) -> bool:
        return all((n[3] >> 16) <= 255 for n in self.nodes)

    def write(self, directory: pathlib.Path, name: str = "size") -> pathlib.Path:
        path = pathlib.Path(directory) / f"{name}.scene.json"
        path.write_text(json.dumps(self.doc, separators=(",", ":")))
        return path


def _shell(cam: Sequence[float], radius: float, k: int, emissive: bool, texture: str) -> Dict:
    tint = [0.55 + 0.4 * ((k * 5) % 7) / 6.0, 0.55 + 0.4 * ((k * 3) % 5) / 4.0, 0.55 + 0.4 * ((k * 2) % 3) / 2.0]
    return {"type": "SPHERE", "position": [float(c) for c in cam], "rotation": [0.0, 0.0, 0.0], "scale": [float(radius)] * 3,
            "material": {"type": "LAMBERT", "baseColor": tint, "emissive": [0.6, 0.5, 0.4] if emissive else [0.0, 0.0, 0.0],
                         "roughness": 1.0, "metalness": 0.0, "texture": texture}}


def _box(obj: Dict, pad: float = 1.25) -> Tuple[Tuple[float, ...], Tuple[float, ...]]:
    """Every shape lies inside [-1, 1]^3 of its object space and the scenes use no rotation: position
    +- |scale|, padded (a flat shape's box keeps its full height; tightness is not needed)."""
    p = np.array(obj["position"], dtype=np.float32)
    s = np.abs(np.array(obj["scale"], dtype=np.float32)) * np.float32(pad) + np.float32(0.01)
    return tuple(float(x) for x in (p - s)), tuple(float(x) for x in (p + s))


def _spatial_order(idx: List[int], centre: np.ndarray, axis: int = 0) -> List[int]:
    """Recursive median split on the centres (axes cycling): consecutive runs are compact clusters."""
    if len(idx) <= 2:
        return idx
    idx = sorted(idx, key=lambda i: (float(centre[i][axis]), i))
    mid = len(idx) // 2
    return _spatial_order(idx[:mid], centre, (axis + 1) % 3) + _spatial_order(idx[mid:], centre, (axis + 1) % 3)


def scene(S: int, content: int, leaf_sizes: Optional[Sequence[int]] = None, octant: int = 7,
          axes: Sequence[int] = (0, 1, 2), enclose: str = "path", radii: str = "growing", swap: bool = False,
          seed: int = 1984, skybox: Optional[str] = None) -> SizeScene:
    assert S >= 0 and content >= 1 and 0 <= octant < 8 and radii in ("growing", "shuffled")
    assert enclose in ("none", "path", "all")
    leaf_sizes = [1] * content if leaf_sizes is None else [int(x) for x in leaf_sizes]
    assert sum(leaf_sizes) == content and min(leaf_sizes) >= 1
    grid = 1
    while grid * grid + 1 < content:
        grid += 1
    sky = str(ROOT / "scenes" / "skybox.hdr") if skybox is None else skybox
    doc = _stress_module().make_scene(grid, seed, sky)
    cam = camera_position(octant)
    rng = np.random.default_rng(seed + 17 * S + octant)
    rad = [80.0 + 4.0 * k for k in range(S)]
    if radii == "shuffled":
        rad = [rad[i] for i in rng.permutation(S)]
    shells = [_shell(cam, rad[k], k, emissive=(k == 0), texture=sky) for k in range(S)]
    objs = shells + doc["objects"][:content]
    doc["objects"] = objs
    doc["camera"] = {"position": cam, "look_at": [0.0, 0.0, 0.0], "fovy": FOVY}
    boxes = [_box(o) for o in objs]
    cam_box = (tuple(c - 0.5 for c in cam), tuple(c + 0.5 for c in cam))

    # content leaves: consecutive runs of a spatial order
    centre = np.array([o["position"] for o in objs], dtype=np.float64)
    ordered = _spatial_order(list(range(S, S + content)), centre)
    leaves, at = [], 0
    for n in leaf_sizes:
        leaves.append(ordered[at:at + n])
        at += n

    def deep_second(level: int) -> Tuple[int, bool]:
        a = axes[level % len(axes)]
        return a, bool((octant >> a) & 1)

    # nested tree: ("leaf", [objects], box encloses the camera) or ("node", axis, first, second, swapped)
    def content_tree(lo: int, hi: int, level: int, top: bool, deep: bool):
        if hi - lo == 1:
            return ("leaf", leaves[lo], enclose == "all" or (enclose == "path" and deep))
        small = (hi - lo) // 2
        a, second = deep_second(level)
        mid = lo + (small if second else (hi - lo) - small)
        return ("node", a, content_tree(lo, mid, level + 1, False, deep and not second),
                content_tree(mid, hi, level + 1, False, deep and second), top and swap)

    tree = content_tree(0, len(leaves), S, True, True)
    for k in range(S - 1, -1, -1):
        a, second = deep_second(k)
        leaf = ("leaf", [k], False)           # (a shell's own box holds the camera)
        tree = ("node", a, leaf, tree, False) if second else ("node", a, tree, leaf, False)

    # primitive slots in DFS order (a swapped node hands out its second subtree's slots first)
    order: List[int] = []
    slot_of: Dict[int, int] = {}

    def assign(t) -> None:
        if t[0] == "leaf":
            slot_of[id(t)] = len(order)
            order.extend(t[1])
            return
        for child in ((t[3], t[2]) if t[4] else (t[2], t[3])):
            assign(child)

    assign(tree)
    nodes: List[Optional[be.Node]] = []

    def flatten(t):
        i = len(nodes)
        nodes.append(None)
        if t[0] == "leaf":
            lo, hi = be._union([boxes[o] for o in t[1]])
            if t[2]:                          # interior boxes are unions, so they follow
                lo, hi = be._union([(lo, hi), cam_box])
            nodes[i] = (lo, hi, slot_of[id(t)], len(t[1]) << 16)
            return lo, hi
        b1 = flatten(t[2])
        second = len(nodes)
        b2 = flatten(t[3])
        lo, hi = be._union([b1, b2])
        nodes[i] = (lo, hi, second, t[1] << 8)
        return lo, hi

    flatten(tree)
    out = SizeScene()
    out.doc, out.nodes, out.order = doc, nodes, order
    out.S, out.leaves, out.octant = S, len(leaves), octant
    return out


# ------------------------------------------------------------------------------------------------
# glue to the oracle (lazy import: the builder itself needs numpy only)
# ------------------------------------------------------------------------------------------------
def oracle_scene(sc: SizeScene, path: pathlib.Path, W: int, H: int):
    """The oracle's scene for the JSON at `path` with the caller BVH and primitive order of `sc`."""
    import ctypes as C
    from oracle import pyoracle as po
    osc = po.load_scene(path, W, H)
    assert len(osc.cpu) == len(sc.order)
    L = po.lib()
    prims = (po.Hittable * len(sc.order))()
    for slot, o in enumerate(sc.order):
        L.or_gpu_hittable(C.byref(osc.cpu[o]), C.byref(prims[slot]))
    ref_nodes = (po.BVHNode * len(sc.nodes))()
    for i, (lo, hi, off, pca) in enumerate(sc.nodes):
        ref_nodes[i].bmin[:] = list(lo)
        ref_nodes[i].bmax[:] = list(hi)
        ref_nodes[i].offset = off
        ref_nodes[i].primitiveCountAxis = pca
    osc.nodes, osc.node_count = ref_nodes, len(sc.nodes)
    osc.prims, osc.prim_count = prims, len(sc.order)
    return osc


# ------------------------------------------------------------------------------------------------
# the documented policy, by hand
# ------------------------------------------------------------------------------------------------
LDS_CAP = 160 * 1024          # bytes of LDS a workgroup may use (launch_one: "lds > kLdsLimit")
KB48 = 48 * 1024              # "staged in LDS when they fit in 48 KB" (picked_build)

# build -> (what is staged: 0 nothing, 1 records / nodes, 2 records and primitives;
#           waves per workgroup; walks child-box records)
BUILDS = {1: (0, 4, False), 4: (0, 4, False), 6: (1, 4, False), 20: (0, 4, True), 39: (1, 4, True), 40: (1, 4, True),
          41: (0, 4, True), 46: (0, 4, True), 47: (1, 4, True), 48: (2, 4, True), 60: (1, 8, True), 61: (0, 4, True)}


def lds_bytes(build: int, I: int, R: int, nodes: int, prims: int, child_box: bool = True) -> Tuple[int, int]:
    """(dynamic LDS bytes of the launch, staging level that runs).  Layout (launch_one): the staged
    scene, then per wave R rows of 64 stack entries (8 B with the entry distance in the child-box
    walks, 4 B in the node-at-a-time walks) and 768 B of accumulation slice.  A child-box record is
    64 B, a node 32 B, a primitive 64 B.  A launch that does not fit re-instantiates the same walk
    with nothing staged."""
    staged, wpb, cb = BUILDS[build]
    cb = cb and child_box                     # without the layout the node-at-a-time walk runs
    entry = 8 if cb else 4
    per_wave = R * 64 * entry + 768
    scene_bytes = (64 * I if cb else 32 * nodes) if staged >= 1 else 0
    if staged >= 2:
        scene_bytes += 64 * prims
    total = scene_bytes + wpb * per_wave
    if total > LDS_CAP and staged:
        return wpb * per_wave, 0
    return total, staged


def expected_build(I: int, R: int, nodes: int, prims: int, child_box: bool, dfs: bool, tiles: int, units: int,
                   cus: int) -> Tuple[int, int]:
    """(build, dynamic LDS bytes) of an automatic plain launch (variant 0; no sample groups, strip
    units or run-ahead in play) of `tiles` 8x8 tiles in `units` dispatch units on `cus` compute units."""
    wave = R * 512 + 768                      # a wave's stack and accumulation slice
    cb = 64 * I
    if not child_box or not dfs:              # node-at-a-time walks: nodes in LDS up to 48 KB
        build = 6 if 32 * nodes <= KB48 else 4
    elif cb <= KB48 and 3 * (cb + 8 * wave) <= LDS_CAP:
        build = 60                            # three 8-wave workgroups per CU: six waves per SIMD
    elif cb <= KB48 and 5 * (cb + 4 * wave) <= LDS_CAP:
        build = 40                            # five 4-wave workgroups per CU
    elif 6 * 4 * wave <= LDS_CAP:
        build = 61                            # records through the caches, six 4-wave workgroups
    elif cb <= KB48:
        build = 40
    else:
        build = 46 if 5 * 4 * wave > LDS_CAP else 41
    # small grids: at most four tiles per SIMD run in one pass at four waves per SIMD
    if tiles <= cus * 4 * 4:
        if build in (41, 61):
            build = 46
        elif build in (40, 60):
            group = 64 * I + 64 * prims + 4 * R * 512 + 4 * 768
            build = 48 if 4 * group <= LDS_CAP else 47
    # the sixth wave slot only with at least 4 dispatch units per six-wave slot
    if build in (60, 61) and units < 4 * cus * 4 * 6:
        build = 40 if build == 60 else 41
    return build, lds_bytes(build, I, R, nodes, prims, child_box and dfs)[0]


def large_frame(cus: int) -> Tuple[int, int]:
    """The smallest 16:9 frame in steps of 320 x 180 with at least 4 * cus * 24 tiles, the six-wave
    builds' threshold: 1920 x 1080 at 256 compute units."""
    k = 1
    while ((320 * k + 7) // 8) * ((180 * k + 7) // 8) < 4 * cus * 24:
        k += 1
    return 320 * k, 180 * k


def small_frame(cus: int) -> Tuple[int, int]:
    """The largest 8:5 frame of whole tiles with at most 16 * cus tiles."""
    k = 1
    while (8 * (k + 1)) * (5 * (k + 1)) <= 16 * cus:
        k += 1
    return 64 * k, 40 * k


def persistent_frame(cus: int) -> Tuple[int, int]:
    """The smallest 16:9 frame with at least 2 * cus * 24 tiles: more workgroups than any build keeps
    resident (at most six waves per SIMD), so every persistent build takes tiles from the cursor."""
    k = 1
    while ((16 * k + 7) // 8) * ((9 * k + 7) // 8) < 2 * cus * 24:
        k += 1
    return 16 * k, 9 * k


IMAGE = (64, 40, 2, 2)        # width, height, samples per call, calls of the oracle comparisons

# automatic build on the large frame (units >= 4 * CUs * 24) and on the small one (tiles <= 16 * CUs)
AUTO_LARGE = {"c_r9_181": 60, "c_r9_182": 61, "c_r10_117": 60, "c_r10_118": 40, "c_r10_144": 40, "c_r10_145": 61,
              "c_r11_769": 61, "c_r12_768": 40, "c_r12_769": 41, "c_r14_769": 41, "c_r15_768": 40, "c_r15_769": 46,
              "c_big_1535": 6, "c_big_1537": 4, "c_swap_1535": 6, "c_swap_1537": 4}
AUTO_SMALL = {"c_r9_182": 46, "c_r11_769": 46, "c_r12_769": 46, "c_r9_181": 47, "s_r9_151": 48, "s_r9_152": 47}

# (scene, forced build, dynamic LDS bytes, what is staged): each build's largest staged scene and the
# next one, from the layout in lds_bytes()'s docstring, worked out by hand
LDS_CASES = [
    ("b40_r12_fit", 40, 163840, 1), ("b40_r12_over", 40, 27648, 0),      # 64 * 2128 + 4 * (12 * 512 + 768)
    ("b40_r12_fit", 39, 163840, 1), ("b40_r12_over", 39, 27648, 0),
    ("b40_r12_fit", 47, 163840, 1), ("b40_r12_over", 47, 27648, 0),
    ("b40_r32_fit", 40, 163840, 1), ("b40_r32_over", 40, 68608, 0),      # 64 * 1488 + 4 * (32 * 512 + 768)
    ("b60_r12_fit", 60, 163840, 1), ("b60_r12_over", 60, 55296, 0),      # 64 * 1696 + 8 * (12 * 512 + 768)
    ("b60_r32_fit", 60, 163840, 1), ("b60_r32_over", 60, 137216, 0),     # 64 * 416 + 8 * (32 * 512 + 768)
    ("b48_fit", 48, 163840, 2), ("b48_over", 48, 27648, 0),              # 64 * (1062 + 1066) + 4 * 6912
    ("b6_fit", 6, 163808, 1), ("b6_over", 6, 15360, 0),                  # 32 * 4639 + 4 * (12 * 256 + 768)
]


# ------------------------------------------------------------------------------------------------
# the scenes the tests use, and their sizes written out by hand
# ------------------------------------------------------------------------------------------------
def ir(I: int, R: int, extra: int = 0, big: int = 0, **kw) -> Dict:
    """scene() arguments for I interior nodes and R rows: leaves of one primitive, except that one
    leaf holds `extra` more (odd primitive counts) or `big` primitives in all."""
    S, L = solve(I, R)
    sizes = [1] * L
    sizes[L // 3] = big if big else 1 + extra
    return dict(S=S, content=sum(sizes), leaf_sizes=sizes, **kw)


CASES: Dict[str, Dict] = {
    # A. stack rows
    "r1": dict(S=0, content=2), "r2": dict(S=1, content=2), "r3": dict(S=2, content=2), "r16": ir(17, 16),
    "r31": dict(S=30, content=2),
    "r32_spine": dict(S=31, content=2, enclose="all"),
    "r32_bushy": dict(S=22, content=785, enclose="all"),
    "r32_mirror": dict(S=29, content=5, octant=2, radii="shuffled", enclose="all"),
    # B. the largest scene that stages and the first that does not
    "b40_r12_fit": ir(2128, 12), "b40_r12_over": ir(2129, 12, extra=1),
    "b40_r32_fit": ir(1488, 32), "b40_r32_over": ir(1489, 32, extra=1),
    "b60_r12_fit": ir(1696, 12), "b60_r12_over": ir(1697, 12, extra=1),
    "b60_r32_fit": ir(416, 32), "b60_r32_over": ir(417, 32, extra=1),
    "b48_fit": ir(1062, 12, extra=3), "b48_over": ir(1063, 12, extra=3),
    "b6_fit": ir(2319, 12), "b6_over": ir(2320, 12),
    # C. the automatic choice
    "c_r9_181": ir(181, 9), "c_r9_182": ir(182, 9),
    "c_r10_117": ir(117, 10), "c_r10_118": ir(118, 10), "c_r10_144": ir(144, 10), "c_r10_145": ir(145, 10),
    "c_r11_769": ir(769, 11), "c_r12_768": ir(768, 12), "c_r12_769": ir(769, 12), "c_r14_769": ir(769, 14),
    "c_r15_768": ir(768, 15), "c_r15_769": ir(769, 15),
    "c_big_1535": ir(767, 10, big=256), "c_big_1537": ir(768, 10, big=256),
    "c_swap_1535": ir(767, 10, swap=True), "c_swap_1537": ir(768, 10, swap=True),
    "s_r9_151": ir(151, 9), "s_r9_152": ir(152, 9),
    # D. scene replacement
    "d_small": ir(9, 4),
    # E. one level too deep
    "e_depth34": dict(S=32, content=2),
}

# name -> (I, R, nodes, primitives): what the scene must be, not what the builder happens to give
SIZES: Dict[str, Tuple[int, int, int, int]] = {
    "r1": (1, 1, 3, 2), "r2": (2, 2, 5, 3), "r3": (3, 3, 7, 4), "r16": (17, 16, 35, 18), "r31": (31, 31, 63, 32),
    "r32_spine": (32, 32, 65, 33), "r32_bushy": (806, 32, 1613, 807), "r32_mirror": (33, 32, 67, 34),
    "b40_r12_fit": (2128, 12, 4257, 2129), "b40_r12_over": (2129, 12, 4259, 2131),
    "b40_r32_fit": (1488, 32, 2977, 1489), "b40_r32_over": (1489, 32, 2979, 1491),
    "b60_r12_fit": (1696, 12, 3393, 1697), "b60_r12_over": (1697, 12, 3395, 1699),
    "b60_r32_fit": (416, 32, 833, 417), "b60_r32_over": (417, 32, 835, 419),
    "b48_fit": (1062, 12, 2125, 1066), "b48_over": (1063, 12, 2127, 1067),
    "b6_fit": (2319, 12, 4639, 2320), "b6_over": (2320, 12, 4641, 2321),
    "c_r9_181": (181, 9, 363, 182), "c_r9_182": (182, 9, 365, 183),
    "c_r10_117": (117, 10, 235, 118), "c_r10_118": (118, 10, 237, 119), "c_r10_144": (144, 10, 289, 145),
    "c_r10_145": (145, 10, 291, 146), "c_r11_769": (769, 11, 1539, 770), "c_r12_768": (768, 12, 1537, 769),
    "c_r12_769": (769, 12, 1539, 770), "c_r14_769": (769, 14, 1539, 770), "c_r15_768": (768, 15, 1537, 769),
    "c_r15_769": (769, 15, 1539, 770),
    "c_big_1535": (767, 10, 1535, 1023), "c_big_1537": (768, 10, 1537, 1024),
    "c_swap_1535": (767, 10, 1535, 768), "c_swap_1537": (768, 10, 1537, 769),
    "s_r9_151": (151, 9, 303, 152), "s_r9_152": (152, 9, 305, 153),
    "d_small": (9, 4, 19, 10),
    "e_depth34": (33, 33, 67, 34),
}

_built: Dict[str, SizeScene] = {}


def case(name: str) -> SizeScene:
    if name not in _built:
        _built[name] = scene(**CASES[name])
    return _built[name]
