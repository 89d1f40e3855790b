"""Rule 9 of include/pt_hip.h, the guided upsampling onto supersampled planes, on the CPU: the two numpy restatements
of tests/upsample_resolve_model.py agree word for word, an analytic edge is antialiased to within the bounds derived
below, the seeded cases reach rule 8's rare branches inside the S x S blocks, and the Cornell box's silhouettes are
antialiased on inputs the oracle gives without a GPU."""
import numpy as np
import pytest

import upsample_model as um
import upsample_resolve_model as rm
from upsample_model import F, U, HIT, bits, same_words

EPS = 2.0 ** -24
SMALL_PAIRS = ((1, 1, 1, 1), (5, 3, 5, 3), (7, 5, 4, 3), (12, 9, 5, 4))


@pytest.mark.parametrize("flags", rm.FLAG_SETS)
@pytest.mark.parametrize("S", rm.FACTORS)
@pytest.mark.parametrize("sizes", SMALL_PAIRS, ids=lambda s: "%dx%d_from_%dx%d" % s)
def test_the_two_restatements_agree_word_for_word(sizes, S, flags):
    W, H, w, h = sizes
    lo, ss = rm.make_case(W, H, w, h, S, 23 + flags)
    sigma_plane, power = um.PARAM_SETS[flags]
    a, ca = rm.model(lo, ss, S, sigma_plane, power, flags)
    b, cb = rm.scalar(lo, ss, S, sigma_plane, power, flags)
    assert a.shape == b.shape == (H, W, 4)
    assert same_words(a, b), np.argwhere((bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b)))[:5]
    assert ca == cb
    assert np.all(a[..., 3] == 1)


def test_the_sum_runs_rows_outer_and_divides_by_the_block():
    # values whose float32 sum depends on the order: 2^24 absorbs a 1 added to it, and 1 + 1 first does not vanish
    img = np.zeros((2, 2, 4), dtype=F)
    img[0, 0, 0], img[0, 1, 0], img[1, 0, 0], img[1, 1, 0] = 2.0 ** 24, 1, -(2.0 ** 24), 1
    assert rm.box_mean(img, 2)[0, 0, 0] == F(0.25)               # ((2^24 + 1) - 2^24) + 1 = 1; columns outer gives 2
    ramp = np.arange(6 * 6 * 4, dtype=F).reshape(6, 6, 4)
    for S in (2, 3):
        want = ramp.reshape(6 // S, S, 6 // S, S, 4).astype(np.float64).mean(axis=(1, 3))
        assert np.array_equal(rm.box_mean(ramp, S)[..., :3], want[..., :3].astype(F))


# ---- an analytic edge -----------------------------------------------------------------------------------
L = np.array([[0.7, 0.4, 0.2], [0.1, 0.5, 0.9]], dtype=F)
ALBEDO = F(0.5)                                                    # a power of two: dividing and multiplying by it is exact
EDGES = ((0.83, 0.41, 14.37), (-0.29, 0.95, 7.913), (0.6, -0.77, 1.234))       # a x + b y > c, in output-pixel units


def edge_planes(X, Y, edge):
    """The planes of one plane facing the camera at the points (X, Y) (output-pixel units), id 1 where a x + b y > c."""
    a, b, c = edge
    ident = (a * X.astype(np.float64) + b * Y.astype(np.float64) > c).astype(U)
    n = X.shape
    p0 = np.full(n + (4,), ALBEDO, dtype=F)
    p0[..., 3] = ident.view(F)
    p1 = np.zeros(n + (4,), dtype=F)
    p1[..., 2], p1[..., 3] = 1, 4
    p2 = np.zeros(n + (4,), dtype=F)
    p2[..., 0], p2[..., 1] = F(0.1) * X.astype(F), F(0.1) * Y.astype(F)
    p2[..., 3] = np.full(n, HIT, dtype=U).view(F)
    return [np.ascontiguousarray(p, dtype=F) for p in (p0, p1, p2)], ident


def grid(n_y, n_x, per_pixel):
    """Centres of an n_y x n_x grid with `per_pixel` cells per output pixel, in output-pixel units (float64)."""
    y, x = np.mgrid[0:n_y, 0:n_x]
    return (x + 0.5) / per_pixel, (y + 0.5) / per_pixel


def coverage(W, H, edge):
    """The exact area of a x + b y > c inside every output pixel: the unit square clipped by the half-plane."""
    a, b, c = edge
    out = np.zeros((H, W))
    for Y in range(H):
        for X in range(W):
            poly = [(X, Y), (X + 1.0, Y), (X + 1.0, Y + 1.0), (X, Y + 1.0)]
            kept = []
            for k in range(4):
                p, q = poly[k], poly[(k + 1) % 4]
                dp, dq = a * p[0] + b * p[1] - c, a * q[0] + b * q[1] - c
                if dp > 0:
                    kept.append(p)
                if (dp > 0) != (dq > 0):
                    t = dp / (dp - dq)
                    kept.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
            area = 0.0
            for k in range(len(kept)):
                p, q = kept[k], kept[(k + 1) % len(kept)]
                area += p[0] * q[1] - q[0] * p[1]
            out[Y, X] = 0.5 * abs(area)
    return out


def analytic_frame(S, edge, W=24, H=20, w=12, h=10):
    """(lo, ss, one-sample planes, ids of the sub-pixels, coverage): the S-times ids at the sub-pixel centres, every
    low pixel of the colour of its own id (at its centre)."""
    xs, ys = grid(S * H, S * W, S)
    ss, id_ss = edge_planes(xs, ys, edge)
    x1, y1 = grid(H, W, 1)
    one, _ = edge_planes(x1, y1, edge)
    xl, yl = grid(h, w, 1)
    lo_planes, id_lo = edge_planes(xl * (W / w), yl * (H / h), edge)
    color = np.ones((h, w, 4), dtype=F)
    color[..., :3] = L[id_lo] * ALBEDO
    return [color] + lo_planes, ss, one, id_ss, coverage(W, H, edge)


def discrepancy(S):
    """|n / S^2 - area| for the centres of an S x S grid of cells against a half-plane.  A cell the line does not cross
    lies on its centre's side: no error.  A crossed cell whose centre is inside is at least half covered (the
    half-plane holds, with every point of the cell it misses, that point's mirror image in the centre), and at most
    half when the centre is outside: its error is at most half its area, 1 / (2 S^2).  A straight line meets at most
    2 S - 1 cells of an S x S grid (it crosses at most S - 1 inner lines of each direction)."""
    return (2 * S - 1) / (2.0 * S * S)


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("S", rm.FACTORS)
def test_a_straight_edge_is_antialiased_within_the_grids_discrepancy(S, edge):
    lo, ss, one, id_ss, cov = analytic_frame(S, edge)
    H, W = cov.shape
    stats = {}
    out, counts = rm.model(lo, ss, S, 0.005, 3, 3, stats)
    assert stats["guided"] == S * S * W * H and counts[1] == 0     # every sub-pixel finds a low pixel of its own id
    n1 = id_ss.reshape(H, S, W, S).sum(axis=(1, 3))
    edge_px = (n1 > 0) & (n1 < S * S)
    assert edge_px.sum() >= 12 and (cov[edge_px] > 0).all() and (cov[edge_px] < 1).all()
    L64 = L.astype(np.float64)
    # 1. the mix by the pixel's own sub-sample count.  I_q = (L / 2) / (1 / 2) = L exactly (D_q is a mean of equal
    # powers of two).  A sub-pixel is a convex combination of equal values, tests/test_upsample_rule.py's bound of 40
    # roundings (at most 12 taps: 12 products, 12 + 12 adds, a quotient and the product with D_p, with room), all terms
    # positive so the relative errors add; then S^2 - 1 adds of positive terms and one division: S^2 more.
    mix = (n1[..., None] * L64[1] + (S * S - n1)[..., None] * L64[0]) * 0.5 / (S * S)
    tol = (40 + S * S) * EPS * 1.01
    rel = np.abs(out[..., :3].astype(np.float64) - mix) / mix
    assert rel.max() <= tol, (rel.max(), tol)
    # 2. against the exact coverage, as a fraction of the step from L1 to L2 (per channel, the largest)
    step = np.abs(L64[1] - L64[0]) * 0.5
    truth = (cov[..., None] * L64[1] + (1 - cov)[..., None] * L64[0]) * 0.5
    err = (np.abs(out[..., :3].astype(np.float64) - truth) / step).max(-1)
    bound = discrepancy(S) + tol * float((L64.max() * 0.5 / step).max())
    assert err.max() <= bound, (err.max(), bound)
    # 3. rule 8's one sample per pixel is off by up to half the step, more than any S x S grid can be
    single, _ = um.model(lo, one, 0.005, 3, 3)
    err1 = (np.abs(single[..., :3].astype(np.float64) - truth) / step).max(-1)
    assert err1[edge_px].max() > bound, (err1[edge_px].max(), bound)
    assert err1[edge_px].max() > err[edge_px].max() and err1[edge_px].mean() > 1.5 * err[edge_px].mean()


# ---- the seeded cases -----------------------------------------------------------------------------------
# S -> the least number of output pixels (of 48 x 40 from 19 x 13) whose block is of mixed ids, holds a ring-2
# sub-pixel, holds a nearest sub-pixel
FLOORS = {2: dict(mixed=300, wide=10, nearest=10), 3: dict(mixed=300, wide=10, nearest=10), 4: dict(mixed=300, wide=10, nearest=10)}


@pytest.mark.parametrize("S", rm.FACTORS)
def test_the_seeded_cases_are_not_vacuous_and_the_counts_are_the_sub_pixels(S):
    W, H, w, h = 48, 40, 19, 13
    lo, ss = rm.make_case(W, H, w, h, S, 5)
    stats = {}
    out, counts = rm.model(lo, ss, S, 0.05, 2, 3, stats)
    blocks = rm.block_stats(ss[0], S, stats["wide_mask"], stats["nearest_mask"])
    for key, least in FLOORS[S].items():
        assert blocks[key] >= least, (key, blocks[key], least)
    # the unguided path (misses, emitters, guides that are not finite) occurs, and inside blocks that also hold guided
    # sub-pixels
    for key, least in dict(u_interpolated=100, u_nearest=20, u_miss=100, u_emitter=40, u_flags=20, u_id=10).items():
        assert stats[key] >= least, (key, stats[key], least)
    unguided = ~stats["guide_mask"].reshape(H, S, W, S)
    assert (unguided.any(axis=(1, 3)) & ~unguided.all(axis=(1, 3))).sum() >= 50
    # the counts are rule 8's at the S-times size, one per sub-pixel: more than the output pixels that hold one
    full, full_counts = um.model(lo, ss, 0.05, 2, 3)
    assert counts == full_counts == (int(stats["wide_mask"].sum()), int(stats["nearest_mask"].sum()))
    assert counts[0] > blocks["wide"] and counts[1] > blocks["nearest"]
    # a block of mixed ids is a mixture: some output pixel differs from every one of its sub-pixels
    assert same_words(out, rm.box_mean(full, S))
    mixed = blocks["mixed_mask"]
    sub = full.reshape(H, S, W, S, 4)[..., :3]
    differs = (sub != out[:, None, :, None, :3]).any(-1).all(axis=(1, 3))
    assert (differs & mixed).sum() >= FLOORS[S]["mixed"] // 2
    # a sub-pixel that is not finite makes its output pixel not finite
    bad = ~np.isfinite(sub).all(-1).all(axis=(1, 3))
    assert bad.sum() >= 5 and not np.isfinite(out[bad][..., :3]).all(-1).any()
    assert np.isfinite(out[~bad][..., :3]).all()


# ---- the Cornell box, without a GPU ---------------------------------------------------------------------
def oracle_planes(scene, W, H):
    """(oracle scene, planes) at W x H from tests/first_hit.py's twin scene: ids, albedo and the hit and emissive flags
    of each pixel's first ray, bit for bit what pt_render_features gives.  The oracle has no normals, positions or
    distances: N = (0, 0, 1), P = 0 and t = 1 everywhere, so every w_n and w_p is 1 and the id test alone decides --
    exact where the pixels of one id are coplanar (the six quads), an approximation on the two cubes and the sphere,
    whose faces the device keeps apart by their normals."""
    from first_hit import first_hits
    from oracle import pyoracle as po
    osc = po.load_scene(scene, W, H)
    n = osc.prim_count
    ids = first_hits(osc, [(i + 1, 0, 0) for i in range(n)], W, H, (1, 0, 1))[..., 0]
    albedo = first_hits(osc, [tuple(osc.prims[i].mat.baseColor) for i in range(n)], W, H, (1, 0, 1))[..., :3]
    index = np.where(ids > 0, ids.astype(np.int64) - 1, n)
    emissive = np.array([any(v > 0 for v in osc.prims[i].mat.emissive) for i in range(n)] + [False])
    flags = (np.where(ids > 0, HIT, 0) | np.where(emissive[index], um.EMISSIVE, 0)).astype(U)
    p0 = np.concatenate([albedo.astype(F), np.where(ids > 0, index, 0xffffffff).astype(U).view(F)[..., None]], -1)
    p1 = np.zeros((H, W, 4), dtype=F)
    p1[..., 2], p1[..., 3] = 1, 1
    p2 = np.zeros((H, W, 4), dtype=F)
    p2[..., 3] = flags.view(F)
    return osc, [np.ascontiguousarray(p, dtype=F) for p in (p0, p1, p2)]


def test_it_antialiases_on_the_cpu(scenes):
    """tests/test_gpu_upsample_resolve.py's test_it_antialiases with the oracle's renders (bit for bit the device's) and
    oracle_planes: cornell_box, output 64 x 64, low 32 x 32 at 256 spp, planes 128 x 128 (S = 2), reference 1,024 spp,
    tonemapped MSE.  Measured: 461 edge pixels; edge / all resolved 0.027733 / 0.017191, one sample 0.068548 / 0.021845,
    bilinear 0.027226 / 0.023312 (the device, with its own normals and positions: 0.027730 / 0.017070 and
    0.069084 / 0.022118)."""
    from oracle import pyoracle as po
    scene = scenes / "cornell_box.scene.json"
    S, Wo, Ho = 2, 64, 64
    olo, lo_planes = oracle_planes(scene, 32, 32)
    ohi, hi_planes = oracle_planes(scene, Wo, Ho)
    _, ss_planes = oracle_planes(scene, S * Wo, S * Ho)
    r = po.OracleRenderer(olo, 32, 32)
    r.render(olo.camera, 8, True, chunks=32)
    lows = [r.hdr()] + lo_planes
    r = po.OracleRenderer(ohi, Wo, Ho)
    r.render(ohi.camera, 8, True, chunks=128)
    ref = r.hdr()

    def tonemapped(img):
        x = np.maximum(img[..., :3].astype(np.float64), 0.0)
        return (x / (1.0 + x)) ** (1.0 / 2.2)

    resolved, _ = rm.model(lows, ss_planes, S, 0.005, 3, 3)
    single, _ = um.model(lows, hi_planes, 0.005, 3, 3)
    ids = bits(ss_planes[0][..., 3]).reshape(Ho, S, Wo, S)
    edge = (ids != ids[:, :1, :, :1]).any(axis=(1, 3))
    e = {name: (tonemapped(img) - tonemapped(ref)) ** 2 for name, img in
         (("resolved", resolved), ("one sample", single), ("bilinear", um.bilinear(lows[0], Wo, Ho)))}
    message = f"{int(edge.sum())} edge pixels; edge / all: " + ", ".join(f"{k} {v[edge].mean():.6f} / {v.mean():.6f}" for k, v in e.items())
    print(message)
    assert edge.sum() >= 200, message
    assert e["resolved"][edge].mean() < e["one sample"][edge].mean(), message
    assert e["resolved"].mean() <= e["one sample"].mean(), message
