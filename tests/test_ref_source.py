"""The oracle and the host layer against the reference's own source compiled for the host
(oracle/_ref/libptref.so: oracle/ref_wrap.cpp over oracle/ref_shim/, driven by oracle/pyref.py).

The oracle is a restatement of the reference; here the restatement meets the original.  The
constructors, BVH::build, Camera, hitBVH, getColor, traceKernel and tonemap run exactly as written,
on the shipped scenes and on the edge scenes of tests/ref_scenes.py.  Only cuRAND, the texture
sampler and CUDA's libm are not in the reference's tree; they come from liboracle.so and have their
own known-answer tests in tests/test_oracle.py.

Every comparison is bit for bit.  A disagreement is a finding about the oracle (or about the shim's
fidelity to nvcc), never a tolerance to widen.
"""
import ctypes as C

import numpy as np
import pytest

import pathtracercuda_amd as pa
import ref_scenes
from oracle import pyoracle as po
from oracle import pyref as pr

SHIPPED = {"cornell_box": (48, 32), "generated_scene": (64, 36), "test_shapes": (48, 32), "rise_repair": (48, 32),
           "rise_pair": (48, 32)}
EDGE = list(ref_scenes.EDGE_SCENES)
ALL = list(SHIPPED) + EDGE


@pytest.fixture(scope="module", autouse=True)
def ref_library():
    if not pr.available():
        if pr.reference_tree() is None:
            pytest.skip("neither oracle/_ref/libptref.so nor a checkout of the reference to build it from")
        pytest.fail(f"the reference is at {pr.reference_tree()} but {pr.LIB_PATH} is not built: run `make`")
    return pr.lib()


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("ref_scenes")


@pytest.fixture(scope="module")
def case(scenes, scene_dir):
    """name -> (path, W, H): shipped scenes as they are, edge scenes written once per module."""
    cache = {}

    def get(name):
        if name not in cache:
            if name in SHIPPED:
                cache[name] = (ref_scenes.drop_unset_uv_textures(scenes / f"{name}.scene.json", scene_dir), *SHIPPED[name])
            else:
                cache[name] = (ref_scenes.edge_scene(scene_dir, name), ref_scenes.W, ref_scenes.H)
        return cache[name]
    return get


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b, what):
    a, b = u32(a), u32(b)
    assert a.shape == b.shape, f"{what}: shapes {a.shape} vs {b.shape}"
    if not np.array_equal(a, b):
        d = np.argwhere(a != b)
        raise AssertionError(f"{what}: {len(d)} words differ, first at {tuple(d[0])}: "
                             f"{a[tuple(d[0])]:#010x} vs {b[tuple(d[0])]:#010x}")


def oracle_objects(osc):
    """The oracle's constructor products in file order: 96-byte hittables and boxes."""
    L = po.lib()
    h = np.zeros((len(osc.cpu), 96), dtype=np.uint8)
    a = np.zeros((len(osc.cpu), 6), dtype=np.float32)
    for i, c in enumerate(osc.cpu):
        g = po.Hittable()
        L.or_gpu_hittable(C.byref(c), C.byref(g))
        h[i] = np.frombuffer(bytes(g), dtype=np.uint8)
        a[i] = [*c.aabbMin, *c.aabbMax]
    return h, a


def as_bytes(ctypes_array, n, size):
    return np.frombuffer(bytes(ctypes_array), dtype=np.uint8)[:n * size].reshape(n, size)


def test_layouts():
    L = pr.lib()
    assert [L.ref_sizeof(k) for k in (0, 1, 3, 4, 5)] == [40, 96, 32, 92, 24]
    assert [po.lib().or_sizeof(k) for k in (0, 1, 3, 4, 5)] == [40, 96, 32, 92, 24]
    assert C.sizeof(pa.PtHittable) == 96 and C.sizeof(pa.PtBvhNode) == 32 and C.sizeof(pa.PtCamera) == 92


@pytest.mark.parametrize("name", ALL)
def test_build_products(case, name):
    # CpuHittable's constructor (worldTransform, the adjusted y scale, the box), getGpuHittable,
    # BVH::build with its std::partition / std::nth_element order, and the Camera constructor:
    # reference source == oracle == host layer
    path, W, H = case(name)
    ref = pr.load_scene(path, W, H)
    osc = po.load_scene(path, W, H)
    host = pa.Scene(path, W, H)
    n = ref.count
    assert n == len(osc.cpu) == host.object_count
    assert ref.validate()

    rh, ra = ref.objects()
    oh, oa = oracle_objects(osc)
    hobjs, ha = host.objects()
    same_bits(rh, oh, f"{name}: hittables, oracle")
    same_bits(rh, as_bytes(hobjs, n, 96), f"{name}: hittables, host layer")
    same_bits(ra, oa, f"{name}: boxes, oracle")
    same_bits(ra, ha, f"{name}: boxes, host layer")

    rn, rp, _ = ref.bvh()
    assert ref.node_count == osc.node_count == host.node_count
    assert ref.depth() == host.bvh_depth
    hn, hp = host.bvh()
    same_bits(rn, as_bytes(osc.nodes, osc.node_count, 32), f"{name}: BVH nodes, oracle")
    same_bits(rn, as_bytes(hn, host.node_count, 32), f"{name}: BVH nodes, host layer")
    same_bits(rp, as_bytes(osc.prims, n, 96), f"{name}: BVH-order hittables, oracle")
    same_bits(rp, as_bytes(hp, n, 96), f"{name}: BVH-order hittables, host layer")

    assert bytes(ref.camera) == bytes(osc.camera), f"{name}: camera, oracle"
    assert bytes(ref.camera) == bytes(host.camera()), f"{name}: camera, host layer"
    assert ref.inputs.skybox == osc.skybox == host.skybox


@pytest.mark.parametrize("name", ["generated_scene", "transforms", "axis_QUAD"])
def test_camera_moves(case, name):
    # Camera::rotate and Camera::translate (Camera.inl:30-62), ten steps from the scene's camera
    path, W, H = case(name)
    L = po.lib()
    r = pr.load_scene(path, W, H).camera
    o = po.Camera.from_buffer_copy(bytes(r))
    h = pa.PtCamera.from_buffer_copy(bytes(r))
    steps = [("rotate", 0.05, -0.1, 0.0), ("translate", 0.5, -0.25, 2.0), ("rotate", -1.3, 2.9, 0.4),
             ("rotate", 0.0, 1e-4, 0.0), ("translate", 1e3, 0.0, -1e-3), ("rotate", 3.0, -3.0, 0.0),
             ("translate", -7.5, 3.25, 0.125), ("rotate", 1e-6, 0.7, 0.0), ("translate", 0.0, 0.0, 0.0),
             ("rotate", -0.4, 0.0, 0.0)]
    assert len(steps) == 10
    for i, (kind, a, b, c) in enumerate(steps):
        a, b, c = (float(np.float32(v)) for v in (a, b, c))
        if kind == "rotate":
            pr.camera_rotate(r, a, b, c)
            L.or_camera_rotate(C.byref(o), a, b, c)
            pa.camera_rotate(h, a, b, c)
        else:
            pr.camera_translate(r, a, b, c)
            L.or_camera_translate(C.byref(o), a, b, c)
            pa.camera_translate(h, a, b, c)
        assert bytes(r) == bytes(o), f"{name}: step {i} ({kind}), oracle"
        assert bytes(r) == bytes(h), f"{name}: step {i} ({kind}), host layer"


@pytest.mark.parametrize("name", ALL)
def test_render_and_tonemap(case, name):
    # hitBVH, the seven hit routines, getColor, the materials, traceKernel's accumulation, tonemap:
    # render(4, True) then render(4, False), reference source == oracle
    path, W, H = case(name)
    ref = pr.load_scene(path, W, H)
    osc = po.load_scene(path, W, H)
    rr = pr.RefRenderer(ref, W, H)
    orr = po.OracleRenderer(osc, W, H)
    same_bits(rr.rng_array(), orr.rng_array(), f"{name}: initRandState")
    for ignore in (True, False):
        rr.render(ref.camera, 4, ignore)
        orr.render(osc.camera, 4, ignore)
        same_bits(rr.accum, orr.accum, f"{name}: accumulation after render(4, {ignore})")
        same_bits(rr.rng_array(), orr.rng_array(), f"{name}: RNG state after render(4, {ignore})")
    assert rr.frames == orr.frames == 2
    assert np.array_equal(rr.tonemap(), orr.tonemap()), f"{name}: tonemap"
    # the scene shows something: two black images would compare equal and check nothing.  Every edge
    # scene is under the sky, so most of its pixels carry light after 8 samples; the shipped cornell
    # box has one small lamp and no sky, so there only some do.
    lit = (np.nan_to_num(rr.accum[..., :3], nan=1.0).sum(-1) > 0).mean()
    print(f"{name}: {lit:.0%} of the pixels are lit")
    assert lit > (0.5 if name in EDGE else 0.0), f"{name}: {lit:.0%} of the pixels are lit"


def test_edge_scenes_hold_what_they_claim(case):
    # properties of the scenes themselves, so a later edit cannot quietly remove the edge
    def load(name):
        path, W, H = case(name)
        return pr.load_scene(path, W, H)
    for name in ("ties", "combined"):
        nodes, _, _ = load(name).bvh()
        counts = nodes.view(np.uint32).reshape(-1, 8)[:, 7] >> 16
        assert (counts == 4).any(), f"{name}: no BVH leaf holds 4 primitives"
    t = load("transforms")
    assert all(np.hypot.reduce(np.array(p, dtype=np.float64)) >= 9.9e3 for p in t.inputs.positions)
    flat = [i for i, k in enumerate(t.inputs.types) if po.SHAPES[k] in ("DISK", "QUAD")]
    assert flat and all(t.inputs.scales[i][1] != 1.0 for i in flat)
    scales = np.array(t.inputs.scales)
    assert scales.min() == np.float32(1e-3) and scales.max() == np.float32(1e3)
    m = load("materials").inputs
    assert min(m.roughness) == 0.0 and max(m.roughness) == 1.0 and {0.0, 0.5, 1.0} <= set(m.metalness)
    x = load("textured").inputs
    with_tex = {po.SHAPES[k] for k, h in zip(x.types, x.texture_handles) if h}
    assert with_tex == {"SPHERE", "CYLINDER", "DISK", "QUAD"}


def test_textures_leave_the_shapes_without_uv(scene_dir):
    # the reference leaves u, v unset for cone, paraboloid and cube: the JSON helper and pyref's own
    # guard both take the texture off, and RefScene refuses a scene that still has one
    full = ref_scenes.textured(scene_dir)
    si = po.parse_scene(full)
    assert sum(1 for h in si.texture_handles if h) == 7
    with pytest.raises(ValueError):
        pr.RefScene(si, 8, 8)
    a = pr.load_scene(full, 8, 8)                                            # pyref's array-level drop
    b = pr.load_scene(ref_scenes.drop_unset_uv_textures(full), 8, 8)         # the JSON-level drop
    same_bits(a.objects()[0], b.objects()[0], "textured: the two drops")
