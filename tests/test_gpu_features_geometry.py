"""Normal, hit distance and position of the feature planes against a float64 closed form per shape.

The form takes the primitive the oracle names for the pixel (the twin scene of tests/test_gpu_features.py),
its inv_transform_rows, and the ray built from pixel_state and or_xorwow_uniform in camera_ray's float32
operations.  It is not the kernel's arithmetic (no stepwise rounding, another operation order), so the
comparison has a tolerance, and the tolerance is measured, not chosen: the same form evaluated in float32
and in float64 on the compared pixels, the largest difference, times 8 (the kernel's order differs from
the form's).  TOLERANCE below holds those values; test_tolerances_are_the_measured_ones recomputes them
without a GPU.  Pixels whose float64 |d . n| is below 0.1 (grazing hits, where a rounding of the ray moves
the hit point far) are left out, at most 5 % of the hit pixels.
"""
import ctypes as C

import numpy as np
import pytest

import pathtracercuda_amd as pa
from oracle import pyoracle as po
from test_gpu_features import first_hits

SPHERE, CYLINDER, DISK, CONE, PARABOLOID, QUAD, CUBE = range(7)
T_MIN = 0.001
GRAZING, GRAZING_CAP = 0.1, 0.05

CASES = {"cornell": ("cornell_box", 64, 64), "shapes": ("test_shapes", 96, 64)}
# 8 x the largest |float32 form - float64 form| over the compared pixels: (normal, distance, position),
# absolute, in scene units (the scenes' hit distances are 1 .. 30)
# measured: cornell 0.000968 / 0.000202 / 0.000199, shapes 0.0152 / 0.00168 / 0.00157 (the largest
# differences sit on the quadrics, where the root of the quadratic cancels), written rounded up
TOLERANCE = {"cornell": (9.7e-4, 2.1e-4, 2.0e-4), "shapes": (1.53e-2, 1.69e-3, 1.58e-3)}


def rays(osc, W, H):
    """Origin and direction (float32, H x W x 3) of every pixel's first-sample ray, in camera_ray's operations."""
    L = po.lib()
    F = np.float32
    u = np.zeros((H, W), dtype=F)
    v = np.zeros((H, W), dtype=F)
    for y in range(H):
        for x in range(W):
            st = po.pixel_state(W, x, y)
            u[y, x] = L.or_xorwow_uniform(C.byref(st))
            v[y, x] = L.or_xorwow_uniform(C.byref(st))
    xs, ys = np.meshgrid(np.arange(W, dtype=F), np.arange(H, dtype=F))
    u = (xs + u) / F(W)
    v = (ys + v) / F(H)
    cam = osc.camera
    llc, hor, ver = (np.array(list(a), dtype=F) for a in (cam.lowerLeftCorner, cam.horizontal, cam.vertical))
    d = (llc + u[..., None] * hor) + v[..., None] * ver
    l2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    d = (F(1) / np.sqrt(l2))[..., None] * d
    o = np.broadcast_to(np.array(list(cam.origin), dtype=F), d.shape)
    return o, d.astype(F)


def closed_form(dtype, rows, typ, o, d):
    """(normal, t, position) of rays o, d (n x 3) on the primitive with these inverse-transform rows."""
    T = dtype
    rows = np.asarray(rows, dtype=T)
    o, d = o.astype(T), d.astype(T)
    M, w = rows[:, :3], rows[:, 3]
    # (elementwise sums, not a BLAS product: the same roundings on every machine)
    lo = (o[:, 0:1] * M[:, 0] + o[:, 1:2] * M[:, 1]) + o[:, 2:3] * M[:, 2] + w
    ld = (d[:, 0:1] * M[:, 0] + d[:, 1:2] * M[:, 1]) + d[:, 2:3] * M[:, 2]
    one = T(1)
    if typ in (DISK, QUAD):
        t = -lo[:, 1] / ld[:, 1]
        nl = np.zeros_like(lo)
        nl[:, 1] = one
    elif typ == CUBE:
        with np.errstate(all="ignore"):
            a, b = (-one - lo) / ld, (one - lo) / ld
        near, far = np.minimum(a, b).max(1), np.maximum(a, b).min(1)
        t = np.where(near > T(T_MIN), near, far)
        lp = lo + t[:, None] * ld
        k = np.abs(lp).argmax(1)
        nl = np.zeros_like(lo)
        nl[np.arange(len(k)), k] = np.sign(lp[np.arange(len(k)), k])
    else:
        B = T({SPHERE: 1, CONE: -1}.get(typ, 0))
        Hc = T(-1 if typ == PARABOLOID else 0)
        J = T(-1 if typ in (SPHERE, CYLINDER) else 0)
        a = ld[:, 0] ** 2 + B * ld[:, 1] ** 2 + ld[:, 2] ** 2
        b = T(2) * (lo[:, 0] * ld[:, 0] + B * lo[:, 1] * ld[:, 1] + lo[:, 2] * ld[:, 2]) + Hc * ld[:, 1]
        c = lo[:, 0] ** 2 + B * lo[:, 1] ** 2 + lo[:, 2] ** 2 + Hc * lo[:, 1] + J
        with np.errstate(all="ignore"):
            rt = np.sqrt(np.maximum(b * b - T(4) * a * c, 0))
            q = np.where(b < 0, T(-0.5) * (b - rt), T(-0.5) * (b + rt))
            x0, x1 = q / a, c / q
        t0, t1 = np.minimum(x0, x1), np.maximum(x0, x1)
        if typ == SPHERE:
            t = np.where(t0 > T(T_MIN), t0, t1)
        else:
            h0 = ld[:, 1] * t0 + lo[:, 1]
            t = np.where((t0 > T(T_MIN)) & (h0 >= -one) & (h0 <= one), t0, t1)
        lp = lo + t[:, None] * ld
        if typ == SPHERE:
            nl = lp
        elif typ == CYLINDER:
            nl = lp * np.array([1, 0, 1], dtype=T)
        elif typ == CONE:
            nl = lp * np.array([2, -2, 2], dtype=T)
        else:
            nl = np.stack([T(2) * lp[:, 0], np.full(len(lp), -one, dtype=T), T(2) * lp[:, 2]], 1)
    n = (nl[:, 0:1] * M[0] + nl[:, 1:2] * M[1]) + nl[:, 2:3] * M[2]      # the transpose of the inverse
    n = n / np.sqrt((n * n).sum(1, keepdims=True))
    n = np.where(((d * n).sum(1) < 0)[:, None], n, -n)
    return n.astype(T), t.astype(T), (o + t[:, None] * d).astype(T)


def model(osc, W, H, dtype):
    """(hit mask, primitive, normal, t, position) over the frame."""
    n = osc.prim_count
    ids = first_hits(osc, [(i + 1, 0, 0) for i in range(n)], W, H, (1, 0, 1))[..., 0].astype(np.int64) - 1
    hit = ids >= 0
    o, d = rays(osc, W, H)
    nrm = np.zeros((H, W, 3), dtype=dtype)
    t = np.zeros((H, W), dtype=dtype)
    pos = np.zeros((H, W, 3), dtype=dtype)
    for i in np.unique(ids[hit]):
        m = ids == i
        prim = osc.prims[int(i)]
        rows = np.array([list(r) for r in prim.rows], dtype=np.float32)
        nrm[m], t[m], pos[m] = closed_form(dtype, rows, int(prim.type), o[m], d[m])
    return hit, ids, nrm, t, pos, d


_cache = {}


def measured(scenes, case):
    """The float64 form, the compared pixels, and 8 x the float32 form's largest differences from it."""
    if case not in _cache:
        name, W, H = CASES[case]
        osc = po.load_scene(scenes / f"{name}.scene.json", W, H)
        hit, ids, n64, t64, p64, d = model(osc, W, H, np.float64)
        _, _, n32, t32, p32, _ = model(osc, W, H, np.float32)
        grazing = hit & (np.abs((d.astype(np.float64) * n64).sum(-1)) < GRAZING)
        use = hit & ~grazing
        diff = tuple(8.0 * float(np.abs(a.astype(np.float64) - b)[use].max()) for a, b in ((n32, n64), (t32, t64), (p32, p64)))
        _cache[case] = (osc, hit, use, (n64, t64, p64), diff, float(grazing.sum()) / float(hit.sum()))
    return _cache[case]


@pytest.mark.parametrize("case", list(CASES))
def test_tolerances_are_the_measured_ones(scenes, case):
    osc, hit, use, _, diff, grazing = measured(scenes, case)
    print(f"{case}: {int(hit.sum())} hit pixels, {grazing:.2%} grazing; 8 x max |f32 - f64|: normal {diff[0]:.3g}, "
          f"t {diff[1]:.3g}, position {diff[2]:.3g}")
    assert grazing <= GRAZING_CAP
    # the written tolerance is the measured one rounded up, by 5 % at the most
    for got, written in zip(diff, TOLERANCE[case]):
        assert got <= written <= 1.05 * got, (got, written)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_normal_depth_position_against_the_closed_form(scenes, case):
    if pa.device_count() < 1:
        pytest.skip("no GPU")
    name, W, H = CASES[case]
    osc, hit, use, (n64, t64, p64), _, _ = measured(scenes, case)
    pt = pa.Pathtracer(W, H)
    f = pt.features(pt.load_scene(str(scenes / f"{name}.scene.json")))
    assert np.array_equal(f["hit"], hit)
    tol = TOLERANCE[case]
    err = (np.abs(f["normal"] - n64)[use].max(), np.abs(f["depth"] - t64)[use].max(), np.abs(f["position"] - p64)[use].max())
    print(f"{case}: max |gpu - f64 form| normal {err[0]:.3g} (allowed {tol[0]:.3g}), t {err[1]:.3g} ({tol[1]:.3g}), "
          f"position {err[2]:.3g} ({tol[2]:.3g}) over {int(use.sum())} pixels")
    assert err[0] <= tol[0] and err[1] <= tol[1] and err[2] <= tol[2]
