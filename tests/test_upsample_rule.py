"""Rule 8 of include/pt_hip.h, the guided upsampling, on the CPU: the two numpy restatements of tests/upsample_model.py
agree word for word, the seeded cases reach every branch of the rule, and the properties the feature exists for
hold by construction."""
import numpy as np
import pytest

import upsample_model as um
from upsample_model import F, U, HIT, EMISSIVE, bits, same_words

EPS = 2.0 ** -24


@pytest.mark.parametrize("flags", (0, 1, 2, 3))
@pytest.mark.parametrize("sizes", um.SIZE_PAIRS, ids=lambda s: "%dx%d_from_%dx%d" % s)
def test_the_two_restatements_agree_word_for_word(sizes, flags):
    W, H, w, h = sizes
    lo, hi = um.make_case(W, H, w, h, 11 + flags)
    for sigma_plane, power in ((0.05, 2), um.PARAM_SETS[flags]):
        a, ca = um.model(lo, hi, sigma_plane, power, flags)
        b, cb = um.scalar(lo, hi, sigma_plane, power, flags)
        assert same_words(a, b), np.argwhere((bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b)))[:5]
        assert ca == cb
        assert np.all(a[..., 3] == 1)


# (high, low) -> the least number of high pixels at which each branch must occur under both flags
FLOORS = {
    (48, 40, 24, 20): dict(outside=100, not_kept=200, by_id=400, wide=20, nearest=30, u_outside=10, u_not_raw=20, u_kept=100,
                           u_flags=20, u_id=10, u_interpolated=100, u_nearest=20, u_miss=100, u_emitter=40, u_not_finite=10,
                           ring1=1000),
    (40, 24, 13, 8): dict(outside=100, not_kept=100, by_id=300, wide=5, nearest=10, u_outside=20, u_not_raw=10, u_kept=50,
                          u_flags=20, u_id=5, u_interpolated=50, u_nearest=10, u_miss=40, u_emitter=30, u_not_finite=4,
                          ring1=500, zero_b=50),
    (70, 45, 35, 23): dict(outside=100, not_kept=400, by_id=800, wide=30, nearest=50, u_outside=10, u_not_raw=30, u_kept=100,
                           u_flags=40, u_id=30, u_interpolated=150, u_nearest=40, u_miss=100, u_emitter=80, u_not_finite=16,
                           ring1=2000),
    (32, 8, 32, 8): dict(zero_b=200, wide=3, nearest=1, ring1=200),
}


@pytest.mark.parametrize("sizes", sorted(FLOORS), ids=lambda s: "%dx%d_from_%dx%d" % s)
def test_the_seeded_cases_are_not_vacuous(sizes):
    W, H, w, h = sizes
    lo, hi = um.make_case(W, H, w, h, 5)
    stats = {}
    um.model(lo, hi, 0.05, 2, 3, stats)
    for key, least in FLOORS[sizes].items():
        assert stats[key] >= least, (key, stats[key], least)
    # a high pixel over the middle of the block of low pixels that are not kept has 16 rejected taps
    if h >= 16:
        y, x = int(13.5 * H / h), int(6.5 * W / w)
        assert stats["nearest_mask"][y, x] or not stats["guide_mask"][y, x]
        assert stats["nearest_mask"][y - 1:y + 2, x - 1:x + 2].any()
    # without the id test nothing is rejected by it, and the plane and normal weights alone decide
    stats0 = {}
    um.model(lo, hi, 0.05, 2, 1, stats0)
    assert stats0["by_id"] == 0 and stats0["nearest"] <= stats["nearest"]


def analytic_frame(W=48, H=40, w=24, h=20):
    """One plane facing the camera, split into two primitives at high column 21 (inside low pixel 10's footprint); the
    demodulated colour is one constant per primitive, the high albedo a checker at high-pixel period.  A low pixel's
    own albedo is one sample of that checker (its first high pixel's), and its colour the constant times the mean albedo
    of its footprint on its primitive: what a render of many samples gives.  Returns (lo, hi, truth), truth in float64."""
    L = np.array([[0.7, 0.4, 0.2], [0.1, 0.5, 0.9]])

    def planes(X, Y, albedo):
        ident = (X >= 21).astype(U)
        n = X.shape
        p0 = np.concatenate([albedo.astype(F), ident.view(F)[..., None]], -1)
        p1 = np.zeros(n + (4,), dtype=F)
        p1[..., 2], p1[..., 3] = 1, 4
        p2 = np.zeros(n + (4,), dtype=F)
        p2[..., 0], p2[..., 1] = F(0.1) * X, F(0.1) * Y
        p2[..., 3] = np.full(n, HIT, dtype=U).view(F)
        return [np.ascontiguousarray(a, dtype=F) for a in (p0, p1, p2)], ident

    yh, xh = np.mgrid[0:H, 0:W]
    checker = np.where(((xh + yh) % 2 == 0)[..., None], [0.25, 0.5, 0.75], [0.75, 0.25, 0.5])
    hi, id_hi = planes(xh.astype(F), yh.astype(F), checker)
    yl, xl = np.mgrid[0:h, 0:w]
    X = ((xl.astype(F) + F(0.5)) * (F(W) / F(w)) - F(0.5)).astype(F)
    Y = ((yl.astype(F) + F(0.5)) * (F(H) / F(h)) - F(0.5)).astype(F)
    xn, yn = um.axis(W, w)[3], um.axis(H, h)[3]
    first_x, first_y = np.searchsorted(xn, np.arange(w)), np.searchsorted(yn, np.arange(h))
    lo_planes, id_lo = planes(X, Y, checker[first_y][:, first_x])
    color = np.ones((h, w, 4), dtype=F)
    color[..., :3] = (L[id_lo].astype(F) * um.footprint_divisor(lo_planes[0], hi[0], xn, yn, um.DEMODULATE)).astype(F)
    truth = L[id_hi] * hi[0][..., :3].astype(np.float64)
    return [color] + lo_planes, hi, truth


def test_high_resolution_albedo_comes_back_and_bilinear_cannot_bring_it():
    lo, hi, truth = analytic_frame()
    stats = {}
    out, counts = um.model(lo, hi, 0.005, 3, 3, stats)
    assert stats["guided"] == truth.shape[0] * truth.shape[1] and counts == (0, 0)
    # A convex combination of equal values.  I_q = (L D_q) / D_q: 2 roundings.  At most 12 taps: 12 products and 12 adds
    # into sumI on top of the weights' own error, which sumW's 12 adds share up to their own 12 roundings; the quotient
    # and the product with D_p: 2.  Every term is positive, so the relative errors add: 2 + 24 + 12 + 2 = 40 roundings
    # bound it with room, and the weights here (one plane, unit normals, b >= 1/16) are nowhere near underflow.
    tol = 40 * EPS * 1.01
    rel = np.abs(out[..., :3].astype(np.float64) - truth) / truth
    assert rel.max() <= tol, (rel.max(), tol)
    # the plain bilinear resampling of the same low image has no checker in it: it holds the mean albedo of every 2 x 2
    # block (1/2, 3/8, 5/8) where the pixel has 1/4, 1/2 or 3/4, off by a fifth at the least in two of the channels,
    # and mixes the two primitives across column 21
    plain = um.bilinear(lo[0], truth.shape[1], truth.shape[0])[..., :3].astype(np.float64)
    rel_plain = np.abs(plain - truth) / truth
    assert np.median(rel_plain.max(-1)) >= 0.2 - 1e-6
    assert rel_plain.max() > 1e4 * tol
    # and dividing a low pixel's colour by its own albedo, one sample of the checker, does not bring the constant back
    own = lo[0][..., :3] / lo[1][..., :3]
    assert np.abs(own / own[0, 0] - 1).max() > 0.2
    # without the id test the colours of the two primitives mix at the silhouette (same plane, same normal)
    mixed, _ = um.model(lo, hi, 0.005, 3, 1)
    rel_mixed = np.abs(mixed[..., :3].astype(np.float64) - truth) / truth
    assert rel_mixed[:, 19:23].max() > 0.05 and rel_mixed[:, :18].max() <= tol


def test_with_equal_sizes_it_is_the_input_to_within_four_roundings():
    lo, _ = um.make_case(48, 40, 48, 40, 5)
    stats = {}
    out, _ = um.model(lo, lo[1:], 0.005, 3, 3, stats)
    served = stats["ring1_mask"]                             # one tap of b = 1, the pixel itself, and three of b = 0
    assert served.sum() > 1500 and stats["zero_b"] > 1500
    got, want = out[served][..., :3].astype(np.float64), lo[0][served][..., :3].astype(np.float64)
    assert np.all(np.abs(got - want) <= 4 * EPS * 1.01 * np.abs(want))
    assert not same_words(out[served][..., :3], lo[0][served][..., :3])       # (wgt * I) / wgt rounds: not the identity


def test_a_pixel_that_is_not_kept_or_not_finite_reaches_no_guided_pixel():
    W, H, w, h = 48, 40, 24, 20
    lo, hi = um.make_case(W, H, w, h, 5)
    stats = {}
    out, _ = um.model(lo, hi, 0.05, 2, 3, stats)
    keep = um.dm.keep_mask(lo[0], lo[2], lo[3])
    assert (~keep).sum() > 50
    other = lo[0].copy()
    raw = np.isfinite(lo[0][..., :3]).all(-1)                # every low pixel that is not kept gets another colour:
    other[~keep & raw, :3] = F(12345.0)                      # a finite one stays finite, NaN and infinity change places
    other[~raw, :3] = np.where(np.isnan(lo[0][~raw, :3]), F(np.inf), F(np.nan))
    assert not keep[~raw].any() and (~keep & raw).sum() > 30 and (~raw).sum() > 20
    out2, _ = um.model((other,) + tuple(lo[1:]), hi, 0.05, 2, 3)
    served = stats["ring1_mask"] | stats["wide_mask"]        # guided, and a tap was accepted
    assert served.sum() > 1000
    assert np.array_equal(bits(out[served]), bits(out2[served]))
    assert np.isfinite(out[served][..., :3][np.isfinite(hi[0][served][..., :3]).all(-1)]).all()
    # and a colour that is not finite reaches no pixel through a tap: whatever was interpolated without a guide is finite
    fl = bits(hi[2][..., 3])
    guide = stats["guide_mask"]
    raw_near = np.isfinite(um.nearest(lo[0], W, H)[..., :3]).all(-1)
    assert np.isfinite(out[~guide & raw_near][..., :3]).all()
    # a kept pixel reaches no unguided one: with the kept colours changed, the pixels interpolated without a guide stay
    kept_other = lo[0].copy()
    kept_other[keep, :3] = F(777.0)
    out3, _ = um.model((kept_other,) + tuple(lo[1:]), hi, 0.05, 2, 3)
    kept_near = um.nearest(np.repeat(keep[..., None], 4, -1).astype(F), W, H)[..., 0] != 0
    assert (fl[~guide] & HIT).any() and (fl[~guide] & EMISSIVE).any()
    assert np.array_equal(bits(out[~guide & ~kept_near]), bits(out3[~guide & ~kept_near]))


def test_the_counts_are_the_pixels_that_took_those_branches():
    for W, H, w, h in ((48, 40, 24, 20), (40, 24, 13, 8)):
        lo, hi = um.make_case(W, H, w, h, 5)
        stats = {}
        out, counts = um.model(lo, hi, 0.05, 2, 3, stats)
        _, scalar_counts = um.scalar(lo, hi, 0.05, 2, 3)
        assert counts == scalar_counts == (int(stats["wide_mask"].sum()), int(stats["nearest_mask"].sum()))
        assert counts[0] > 0 and counts[1] > 0
        assert stats["guided"] == stats["ring1"] + counts[0] + counts[1]
        near = um.nearest(lo[0], W, H)
        assert same_words(out[stats["nearest_mask"]][..., :3], near[stats["nearest_mask"]][..., :3])


def test_the_tile_is_the_filters():
    assert (um.dm.TILE_W, um.dm.TILE_H) == (32, 8)
