"""The temporal passes across moved objects (rule 7 of include/pt_hip.h) on the GPU against their numpy restatement
(tests/motion_model.py): words equal, or both NaN, no tolerance -- through the two _motion_image forms on the seeded
sequence, through load_scene_moved / temporal on rendered frames of a scene whose objects move -- then the state on
the device, and that it does what it is for: a moving object keeps its history.
"""
import json

import numpy as np
import pytest

import bvh_edit
import denoise_model as dm
import motion_model as mm
import pathtracercuda_amd as pa
import svgf_model as sm
import temporal_model as tm
from pathtracercuda_amd import _native as N

pytestmark = pytest.mark.gpu

F, U = mm.F, mm.U
SIZES = [(1, 1), (31, 7), (33, 9), (48, 40)]          # all round the 32 x 8 tile
NAMES = ("image", "h0", "h1", "h2", "h3", "variance")
MT = 4


@pytest.fixture(scope="module")
def gpu_available():
    if pa.device_count() < 1:
        pytest.skip("no GPU")


def pt_camera(cam):
    c = pa.PtCamera()
    c.tan_half_fovy, c.aspect_ratio = float(cam["tan_half_fovy"]), float(cam["aspect_ratio"])
    for name in ("origin", "right", "up", "backward"):
        for k in range(3):
            getattr(c, name)[k] = float(cam[name][k])
    return c


def copy_camera(cam):
    return pa.PtCamera.from_buffer_copy(cam)


def device_step(color, p0, p1, p2, cur, hist, prev, rows, prev_index, alpha_min, max_history, sigma_plane, normal_cos_min,
                flags, min_temporal=None):
    """The two _motion_image forms with motion_model.model's signature."""
    kw = dict(alpha_min=alpha_min, max_history=max_history, sigma_plane=sigma_plane, normal_cos_min=normal_cos_min,
              demodulate=bool(flags & 1), same_primitive=bool(flags & 2))
    pc = pt_camera(prev) if hist is not None else None
    if min_temporal is None:
        return pa.temporal_motion_image(color, p0, p1, p2, pt_camera(cur), rows, prev_index, hist, pc, **kw)
    return pa.temporal_moments_motion_image(color, p0, p1, p2, pt_camera(cur), rows, prev_index, hist, pc,
                                            min_temporal=min_temporal, **kw)


def first_difference(got, want):
    g, w = (np.asarray(a).reshape(got.shape[0], got.shape[1], -1) for a in (got, want))
    bad = np.argwhere(~((dm.bits(g) == dm.bits(w)) | (np.isnan(g) & np.isnan(w))))
    y, x, k = bad[0]
    return f"{len(bad)} words differ; first at row {y}, x {x}, channel {k}: {g[y, x, k]!r} != {w[y, x, k]!r}"


def assert_step(got, want, what):
    assert len(got) == len(want)
    for name, g, w in zip(NAMES, got, want):
        assert dm.same_words(g, w), f"{what}, {name}: " + first_difference(g, w)


@pytest.fixture(scope="module")
def sequences():
    return {size: mm.make_sequence(*size) for size in SIZES}


@pytest.fixture(scope="module")
def modelled(sequences):
    """The model over the full-size sequence, once: {(flags, moments): outputs per frame}."""
    seq = sequences[(48, 40)]
    return {(flags, mt): mm.run_sequence(mm.model, seq, flags, min_temporal=mt) for flags in (0, 1, 2, 3) for mt in (None, MT)}


@pytest.mark.parametrize("width,height", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_the_sequence_equals_the_model(gpu_available, sequences, modelled, width, height):
    seq = sequences[(width, height)]
    for flags in (0, 1, 2, 3):
        for mt in (None, MT):
            want = modelled[(flags, mt)] if (width, height) == (48, 40) else mm.run_sequence(mm.model, seq, flags, min_temporal=mt)
            got = mm.run_sequence(device_step, seq, flags, min_temporal=mt)
            for k in range(mm.FRAMES):
                assert_step(got[k], want[k], f"{width}x{height}, flags {flags}, moments {mt}, frame {k}")
    if (width, height) == (48, 40):                 # history was used on the moved objects
        n = modelled[(3, None)][3][0][..., 3]
        for obj in (mm.TRANSLATING, mm.ROTATING):
            assert (n[mm.object_mask(seq[3][1], 3, obj)] == 4).sum() >= 16


def test_an_identity_table_gives_the_plain_forms(gpu_available):
    rows, prev_index = mm.identity_table(1000 + tm.WIDTH * tm.HEIGHT)      # svgf_model's lone ids are 1000 + pixel
    seq = sm.make_sequence()
    for flags in (0, 3):
        hist, hist4, prev = None, None, None
        for k, (cam, frame) in enumerate(seq):
            c, pc = pt_camera(cam), (pt_camera(prev) if prev is not None else None)
            kw = dict(demodulate=bool(flags & 1), same_primitive=bool(flags & 2), **tm.PARAMS)
            plain = pa.temporal_image(*frame, c, hist, pc, **kw)
            assert_step(pa.temporal_motion_image(*frame, c, rows, prev_index, hist, pc, **kw), plain, f"flags {flags}, frame {k}")
            plain4 = pa.temporal_moments_image(*frame, c, hist4, pc, min_temporal=MT, **kw)
            assert_step(pa.temporal_moments_motion_image(*frame, c, rows, prev_index, hist4, pc, min_temporal=MT, **kw), plain4,
                        f"moments, flags {flags}, frame {k}")
            hist, hist4, prev = plain[1:], plain4[1:5], cam
        assert (plain[0][..., 3] > 1).sum() > 100


def test_a_nan_row_an_unknown_id_an_infinite_history_and_a_camera_behind(gpu_available, sequences, modelled):
    seq = sequences[(48, 40)]
    for mt in (None, MT):
        flags = 1
        first = modelled[(flags, mt)][1]
        hist = first[1:5] if mt else first[1:4]
        cam, frame, (rows, prev_index) = seq[2]
        prev = seq[1][0]
        ok = tm.ok_mask(frame[0], frame[2], frame[3])

        def both(what, frame=frame, hist=hist, prev=prev, rows=rows, prev_index=prev_index):
            want = mm.model(*frame, cam, hist, prev, rows, prev_index, flags=flags, min_temporal=mt, **mm.PARAMS)
            got = device_step(*frame, cam, hist, prev, rows, prev_index, flags=flags, min_temporal=mt, **mm.PARAMS)
            assert_step(got, want, f"{what}, moments {mt}")
            return want

        base = both("the frame itself")
        # a NaN in one word of an entry: the pixels of that primitive restart
        bad = rows.copy()
        bad[mm.order(2)[mm.ROTATING], 2, 0] = F(np.nan)
        mask = mm.object_mask(frame, 2, mm.ROTATING) & ok
        want = both("a NaN row", rows=bad)
        assert (base[0][..., 3][mask] > 1).sum() >= 16 and np.all(want[0][..., 3][mask] == 1)
        # ids at and beyond prim_count: the load stays inside the table (the index is clamped) and the pixel restarts
        ids = mm.bits(frame[1][..., 3]).copy()
        far = ok & (np.arange(48)[None, :] % 2 == 0)
        beyond = np.where(np.arange(40) % 2 == 0, U(len(prev_index)), U(0xfffffffe)).astype(U)     # the first one, the last
        ids[far] = np.broadcast_to(beyond[:, None], ids.shape)[far]
        p0 = frame[1].copy()
        p0[..., 3] = ids.view(F)
        want = both("ids beyond the table", frame=(frame[0], p0, frame[2], frame[3]))
        assert far.sum() >= 16 and np.all(want[0][..., 3][far] == 1) and (want[0][..., 3][ok & ~far] > 1).any()
        # an infinite and a NaN history colour
        h0 = hist[0].copy()
        sel = (h0[..., 3] >= 1) & (np.arange(48)[None, :] % 3 == 0)
        h0[..., 1][sel] = F(np.inf)
        h0[..., 2][sel & (np.arange(40)[:, None] % 2 == 0)] = F(np.nan)
        assert sel.sum() >= 16
        both("an infinite history colour", hist=(h0,) + tuple(hist[1:]))
        # the previous camera behind the scene, looking away: z1 <= 0 everywhere
        behind = tm.camera((0.0, 1.0, -14.0), (0.0, 1.0, -20.0), 60.0, 1.2)
        want = both("the previous camera behind the scene", prev=behind)
        assert want[0][..., 3].max() == 1


# ---- on a context ----------------------------------------------------------------------------------------
PARAMS = dict(alpha_min=0.1, max_history=16, sigma_plane=0.05, normal_cos_min=0.9, demodulate=True, same_primitive=True)
MODEL_ARGS = (0.1, 16, 0.05, 0.9, 3)
VDN = dict(iterations=3, sigma_l=2.0, variance_floor=1e-6, sigma_plane=0.03, normal_power_log2=3, demodulate=True,
           same_primitive=False)
VDN_ARGS = (3, 2.0, 1e-6, 0.03, 3, 1)
CUBE, SPHERE = 6, 8                                  # the tall cube and the sphere of cornell_box.scene.json


def write_frames(tmp_path, scenes, count):
    """cornell_box with the tall cube translated and the sphere rotated a step per frame: the files' paths."""
    base = json.loads((scenes / "cornell_box.scene.json").read_text())
    assert base["objects"][CUBE]["type"] == "CUBE" and base["objects"][SPHERE]["type"] == "SPHERE"
    paths = []
    for k in range(count):
        d = json.loads(json.dumps(base))
        d["objects"][CUBE]["position"] = [base["objects"][CUBE]["position"][0] + 0.07 * k, base["objects"][CUBE]["position"][1],
                                          base["objects"][CUBE]["position"][2] + 0.04 * k]
        d["objects"][SPHERE]["rotation"] = [10.0 * k, 25.0 * k, 0.0]
        p = tmp_path / f"frame{k}.scene.json"
        p.write_text(json.dumps(d))
        paths.append(str(p))
    return paths


def moved_primitives(table):
    """The primitives whose map is not the identity."""
    rows, prev_index = table
    return np.flatnonzero((mm.bits(rows) != mm.bits(mm.identity_table(len(rows))[0])).any(axis=(1, 2)))


def orbit(cam):
    cam = copy_camera(cam)
    pa.camera_translate(cam, 0.03, 0.0, 0.0)
    pa.camera_rotate(cam, 0.0, -0.006)
    return cam


def test_moving_objects_equal_the_model_on_a_context(gpu_available, scenes, tmp_path):
    W = H = 64
    paths = write_frames(tmp_path, scenes, 4)
    pt, pv = pa.Pathtracer(W, H), pa.Pathtracer(W, H)
    hist, hist4, prev, cam = None, None, None, None
    for k, path in enumerate(paths):
        for p in (pt, pv):
            c = p.load_scene_moved(path)
            assert p.holds_motion() == (k > 0)
        cam = c if cam is None else orbit(cam)
        table = pt.motion_table()
        assert (table is None) == (k == 0)
        if k == 0:
            table = mm.identity_table(1)                # no history is held: nothing reads it
        else:
            moved = moved_primitives(table)
            assert len(moved) == 2 and np.array_equal(np.sort(table[1]), np.arange(len(table[1])))
            assert all(mm.same_words(a, b) for a, b in zip(table, pv.motion_table()))
        for p in (pt, pv):
            p.render(cam, 1, True)
        planes = pt.features(cam)["planes"]
        assert all(mm.same_words(a, b) for a, b in zip(planes, pv.features(cam)["planes"]))
        hdr, cur = pt.get_hdr_image_data(), tm.camera_of(cam)
        out = pt.temporal(**PARAMS)
        assert pt.history_used == (k > 0) and not pt.holds_motion()          # the pass consumed the table
        want = mm.model(hdr, *planes, cur, hist, prev if prev is not None else cur, *table, *MODEL_ARGS)
        assert dm.same_words(out, want[0]), f"frame {k}: " + first_difference(out, want[0])
        assert_step(pt.temporal_history()[:3], want[1:], f"frame {k}, the history")
        out4 = pv.temporal(variance=True, min_temporal=3, **PARAMS)
        assert pv.history_used == (k > 0)
        want4 = mm.model(hdr, *planes, cur, hist4, prev if prev is not None else cur, *table, *MODEL_ARGS, min_temporal=3)
        assert dm.same_words(out4, want4[0]) and dm.same_words(out4, out), f"frame {k}, moments: " + first_difference(out4, want4[0])
        assert_step(pv.temporal_history(), want4[1:5], f"frame {k}, the history with moments")
        var = pv.temporal_variance()
        assert dm.same_words(var, want4[5]), f"frame {k}, variance"
        filtered = pv.denoise(source="temporal", guide="variance", **VDN)
        fwant = sm.filter_model(out4, *planes, var, *VDN_ARGS)
        assert dm.same_words(filtered, fwant), f"frame {k}, filter: " + first_difference(filtered, fwant)
        if k > 0:                                       # the moved objects kept their history
            on = np.isin(mm.bits(planes[0][..., 3]), moved.astype(U)) & tm.ok_mask(hdr, planes[1], planes[2])
            assert on.sum() >= 64 and (out[..., 3][on] == k + 1).sum() * 2 > on.sum(), (k, np.bincount(out[..., 3][on].astype(int)))
        hist, hist4, prev = want[1:], want4[1:5], cur


def test_state_on_the_device(gpu_available, scenes, tmp_path):
    W = H = 48
    paths = write_frames(tmp_path, scenes, 4)
    pt, twin = pa.Pathtracer(W, H), pa.Pathtracer(W, H)

    def frame(p, cam):
        p.render(cam, 1, True)
        p.features(cam)
        return p.temporal(**PARAMS)

    cam = pt.load_scene(paths[0])
    twin.load_scene(paths[0])
    frame(pt, cam)
    frame(twin, cam)
    # two moves without a temporal pass between them: the history ends
    pt.load_scene_moved(paths[1])
    assert pt.holds_motion()
    pt.load_scene_moved(paths[2])
    assert not pt.holds_motion()
    frame(pt, cam)
    assert not pt.history_used
    # load_scene after a move: no table, no history
    pt.load_scene_moved(paths[3])
    assert pt.holds_motion()
    pt.load_scene(paths[3])
    assert not pt.holds_motion()
    frame(pt, cam)
    assert not pt.history_used
    # a move with previous = None and another object count is refused naming both counts, and changes nothing
    fewer = json.loads(open(paths[3]).read())
    del fewer["objects"][SPHERE]
    short = tmp_path / "fewer.scene.json"
    short.write_text(json.dumps(fewer))
    with pytest.raises(pa.PathtracerError) as e:
        pt.load_scene_moved(str(short))
    assert e.value.code == N.PT_ERR_ARG and "8 objects" in str(e.value) and "9" in str(e.value)
    # with the correspondences it is accepted: the object that left is nobody's previous one
    pt.load_scene_moved(str(short), previous=[0, 1, 2, 3, 4, 5, 6, 7])
    assert pt.holds_motion() and len(pt.motion_table()[1]) == 8
    frame(pt, cam)
    assert pt.history_used
    # and one that appears has no previous index
    pt.load_scene_moved(paths[3], previous=[0, 1, 2, 3, 4, 5, 6, 7, pa.NO_PREVIOUS])
    assert (pt.motion_table()[1] == pa.NO_PREVIOUS).sum() == 1
    frame(pt, cam)
    assert pt.history_used

    # a refused pt_set_scene_moved leaves the scene, the history and the table intact
    rng = twin.rng_state()                              # (the twin has rendered fewer frames: the same streams from here)
    for p in (pt, twin):
        p.load_scene(paths[0])
        p.set_rng_state(rng)
        frame(p, cam)
        p.load_scene_moved(paths[1])
    lib = N.hip()
    scene = pa.Scene(paths[2], W, H)
    nodes, prims = scene.bvh()
    n = len(prims)
    rows, prev_index = mm.identity_table(n)
    fp, up = N.C.POINTER(N.C.c_float), N.C.POINTER(N.C.c_uint32)
    args = (rows.ctypes.data_as(fp), prev_index.ctypes.data_as(up))
    leaf = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 0, 1 << 16)
    deep = bvh_edit.caterpillar([leaf] * 34, 34)
    dn = (pa.PtBvhNode * len(deep))()
    for i, (lo, hi, off, pca) in enumerate(deep):
        dn[i].aabb_min[:], dn[i].aabb_max[:], dn[i].offset, dn[i].primitive_count_axis = lo, hi, off, pca
    assert lib.pt_set_scene_moved(pt._ctx, dn, len(deep), prims, n, *args) == N.PT_ERR_DEPTH
    assert "depth" in lib.pt_last_error(pt._ctx).decode()
    bad = prev_index.copy()
    bad[1] = n                                          # neither 0xffffffff nor below the replaced scene's count
    assert lib.pt_set_scene_moved(pt._ctx, nodes, len(nodes), prims, n, rows.ctypes.data_as(fp), bad.ctypes.data_as(up)) == N.PT_ERR_ARG
    assert "primitive 1" in lib.pt_last_error(pt._ctx).decode()
    assert lib.pt_set_scene_moved(pt._ctx, nodes, len(nodes), prims, n, None, args[1]) == N.PT_ERR_ARG
    assert lib.pt_set_scene_moved(pt._ctx, nodes, 0, prims, n, *args) == N.PT_ERR_ARG
    assert pt.holds_motion()
    got, want = frame(pt, cam), frame(twin, cam)
    assert pt.history_used and twin.history_used
    assert dm.same_words(got, want), first_difference(got, want)
    assert_step(pt.temporal_history()[:3], twin.temporal_history()[:3], "the history after the refusals")
    # through the C ABI itself an accepted move does what the loader's does
    assert lib.pt_set_scene_moved(pt._ctx, nodes, len(nodes), prims, n, *args) == N.PT_OK
    assert pt.holds_motion()


def test_an_unchanged_sky_ends_nothing_and_another_one_ends_the_history(gpu_available, scenes, tmp_path):
    W = H = 48
    scene = scenes / "generated_scene.scene.json"                    # it has a sky, found beside the file
    assert json.loads(scene.read_text())["skybox"] == "skybox.hdr"
    pt = pa.Pathtracer(W, H)
    pt.load_scene(str(scene))
    cam = pt.load_scene(str(scene))         # loaded twice: the sky in use is the second handle with these pixels

    def frame():
        pt.render(cam, 1, True)
        pt.features(cam)
        pt.temporal(**PARAMS)
        return pt.history_used

    assert not frame()
    for _ in range(2):
        pt.load_scene_moved(str(scene))     # the same pixels: the sky keeps its handle, nothing is uploaded
        assert pt.holds_motion()
        assert frame()
    assert pt.history_lengths().max() == 3
    other = json.loads(scene.read_text())
    other["skybox"] = str(scenes / "checker.png")
    moved = tmp_path / "other_sky.scene.json"
    moved.write_text(json.dumps(other))
    pt.load_scene_moved(str(moved))         # a texture upload and another sky: the history ends as it did before
    assert not pt.holds_motion()
    assert not frame()


def tonemapped_mse(img, ref, mask):
    a, r = img[..., :3][mask].astype(np.float64) / 255.0, ref[..., :3][mask].astype(np.float64) / 255.0
    return float(np.mean((a - r) ** 2))


def tonemap(image):
    from oracle import pyoracle as po
    h, w = image.shape[:2]
    ldr = np.zeros((h, w, 4), dtype=np.uint8)
    po.lib().or_tonemap(po.fptr(np.ascontiguousarray(image)), w * h, 1, ldr.ctypes.data_as(N.C.POINTER(N.C.c_uint8)))
    return ldr


def test_it_keeps_history_on_a_moving_object(gpu_available, scenes, tmp_path):
    """Conditions, not tuned thresholds: after eight 1-spp frames of the cornell box with the tall cube translated
    and the sphere rotated every frame, on a slow orbit, the temporal image with motion is closer to a 1024-spp
    render of the last frame's scene and camera -- tonemapped MSE over the moved objects' hit, finite pixels -- than
    what the history restarted at every scene change gives (load_scene each frame: the last frame alone), and than
    camera-only reprojection through pt_temporal_image with SAME_PRIMITIVE off; and the mean history length on those
    pixels is above 1.  Measured on MI355X, over the 445 pixels of the two objects: 0.1750 with motion, 0.2510 restarted,
    0.2231 camera only; mean history length 6.96 (camera only 2.99)."""
    W = H = 64
    paths = write_frames(tmp_path, scenes, 8)
    params = dict(PARAMS, same_primitive=False)
    pt, plain, ref = pa.Pathtracer(W, H), pa.Pathtracer(W, H), pa.Pathtracer(W, H)
    cam, hist, prev = None, None, None
    for k, path in enumerate(paths):
        c = pt.load_scene_moved(path)
        plain.load_scene(path)
        cam = c if cam is None else orbit(cam)
        for p in (pt, plain):
            p.render(cam, 1, True)
            planes = p.features(cam)["planes"]
        out = pt.temporal(**params)
        restarted = plain.temporal(**params)
        assert pt.history_used == (k > 0) and not plain.history_used
        by_camera = pa.temporal_image(plain.get_hdr_image_data(), *planes, cam, hist, prev, **params)
        hist, prev = by_camera[1:], copy_camera(cam)
    ref.load_scene(paths[-1])
    ref.render(cam, 8, True, chunks=128)
    truth = ref.get_image_data()
    moved = moved_primitives(pt.motion_table())
    hdr = plain.get_hdr_image_data()
    mask = (np.isin(mm.bits(planes[0][..., 3]), moved.astype(U)) & tm.ok_mask(hdr, planes[1], planes[2])
            & np.isfinite(ref.get_hdr_image_data()[..., :3]).all(-1))
    with_motion = tonemapped_mse(pt.tonemap_temporal(), truth, mask)
    restart = tonemapped_mse(tonemap(restarted), truth, mask)
    camera_only = tonemapped_mse(tonemap(by_camera[0]), truth, mask)
    n = out[..., 3][mask].mean()
    print(f"tonemapped MSE over {int(mask.sum())} pixels of the moved objects: motion {with_motion:.6f}, restarted "
          f"{restart:.6f}, camera only {camera_only:.6f}; mean history length {n:.2f} "
          f"(camera only {by_camera[0][..., 3][mask].mean():.2f})")
    assert len(moved) == 2 and mask.sum() >= 100
    assert with_motion < restart
    assert with_motion < camera_only
    assert n > 1
