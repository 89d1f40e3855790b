"""Rule 5 of include/pt_hip.h (the variance of an adaptive render's image) on the CPU: the two restatements of
tests/adaptive_variance_model.py against each other, the branches the seeded input must reach, the properties
of the rule, and what the window does for the filter.  tests/test_gpu_adaptive_variance.py holds the device
against the same model.
"""
import numpy as np
import pytest

import adaptive_variance_model as am
import svgf_model as sm
from adaptive_variance_model import F, U, DEMODULATE, SAME_PRIMITIVE, same_words
from test_adaptive_rule import unconverged

ALL_FLAGS = (0, DEMODULATE, SAME_PRIMITIVE, DEMODULATE | SAME_PRIMITIVE)


@pytest.fixture(scope="module")
def inputs():
    return am.make_inputs(am.WIDTH, am.HEIGHT, 1)


@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_the_two_forms_agree_word_for_word(flags):
    args = am.make_inputs(33, 19, 2)[:5]
    for min_batches, cos_min in ((8, 0.9), (2, 0.0), (255, 1.0)):
        a = am.model(*args, min_batches, 0.05, cos_min, flags)
        b = am.scalar(*args, min_batches, 0.05, cos_min, flags)
        assert same_words(a, b), (flags, min_batches, cos_min)


def test_se2_is_the_convergence_rules(inputs):
    """test_adaptive_rule.unconverged keeps its se2 to itself: its decision (se2 <= t * t, t = tolerance x (|mean| +
    floor)) must be the one this model's se2 gives, for every pixel at every tolerance of a sweep that moves t * t
    across the whole range of se2."""
    m1, m2, n = am.split_moments(inputs[4])
    fine = np.isfinite(m1) & np.isfinite(m2) & (n >= 2) & (n < 1000)
    m1, m2, n = m1[fine], m2[fine], n[fine]
    se2 = am.se2_of(m1, m2, n)
    assert se2.size > 1000 and (se2 > 0).sum() > 800
    flips = 0
    with np.errstate(all="ignore"):
        for tol in np.geomspace(1e-4, 4.0, 97):
            t = F(tol) * (np.abs(m1 / n.astype(F)) + F(0.01))
            mine = ~((se2 <= t * t) | ~np.isfinite(m2))
            theirs = unconverged(m1, m2, n, 2, float(tol), 0.01)
            assert np.array_equal(mine, theirs), tol
            flips += int(mine.sum())
    assert 0.1 * 97 * se2.size < flips < 0.9 * 97 * se2.size       # the sweep decides both ways


def test_every_branch_is_reached(inputs):
    color, p0, p1, p2, mom, cls = inputs
    flags = DEMODULATE | SAME_PRIMITIVE
    counts = {}
    var = am.model(color, p0, p1, p2, mom, flags=flags, counts=counts, **am.PARAMS)
    m1, m2, n = am.split_moments(mom)
    fl = am.bits(p2[..., 3])
    with np.errstate(all="ignore"):
        l = sm.lum((color[..., :3] / am.dm.divisor(p0, flags)).astype(F))
    reasons = {"miss": (fl & am.HIT) == 0, "emissive": (fl & am.EMISSIVE) != 0, "n0": n == 0, "n1": n == 1,
               "nan_m1": np.isnan(m1), "inf_m2": np.isinf(m2), "inf_l": ~np.isfinite(l)}
    total = np.sum([r.astype(int) for r in reasons.values()], axis=0)
    for name, r in reasons.items():
        counts["minus_one_" + name] = int((r & (total == 1) & (var == -1)).sum())
    assert np.array_equal(var == -1, total > 0)
    with np.errstate(all="ignore"):
        k = n.astype(F)
        raw = m2 - m1 * (m1 / k)
    has = var >= 0
    counts["ss_clamped"] = int((has & (raw < 0)).sum())
    counts["albedo0"] = int((has & (p0[..., :3] == 0).all(-1)).sum())
    counts["m2_3e38"] = int((has & (m2 == F(3e38))).sum())
    counts["n_max"] = int((has & (n == U(0xffffffff))).sum())
    print(counts)
    for name, c in counts.items():
        assert c >= 64, (name, c, counts)
    # the dark pixels are the generator's, and the model gives each of them its neighbourhood's spread
    dark = (cls == am.CLASSES.index("dark")) & has
    assert dark.sum() >= 64 and (var[dark] > 0).sum() >= 0.9 * dark.sum()
    # an m2 of 3e38 is a variance near 1e36 and stays finite: where the division by g * g overflows, clamp0 takes
    # it to 0 and a young pixel is left with its window
    huge = var[has & (m2 == F(3e38))]
    assert np.isfinite(huge).all() and (huge > 1e30).sum() >= 32


@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_with_min_batches_2_no_pixel_is_young_and_the_output_is_own(inputs, flags):
    color, p0, p1, p2, mom, _ = inputs
    counts = {}
    var = am.model(color, p0, p1, p2, mom, 2, 0.05, 0.9, flags, counts=counts)
    assert counts["young"] == 0 and counts["old"] > 1000
    m1, m2, n = am.split_moments(mom)
    with np.errstate(all="ignore"):
        D = am.dm.divisor(p0, flags)
        g = sm.lum(D) if flags & DEMODULATE else np.ones_like(m1)
        own = sm._clamp0(am.se2_of(m1, m2, n) / (g * g))
    assert same_words(var[var >= 0], own[var >= 0])


@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_scaling_every_call_by_4_scales_the_variance_by_16(inputs, flags):
    color, p0, p1, p2, mom, _ = inputs
    scaled_color = color.copy()
    scaled_color[..., :3] *= F(4)
    scaled = mom.copy()
    with np.errstate(all="ignore"):
        scaled[..., 0] *= F(4)
        scaled[..., 1] *= F(16)
    a = am.model(color, p0, p1, p2, mom, flags=flags, **am.PARAMS)
    b = am.model(scaled_color, p0, p1, p2, scaled, flags=flags, **am.PARAMS)
    # only powers of two are involved, so nothing rounds differently; a pixel whose scaled m2 overflows has none
    fits = np.isfinite(scaled[..., 1]) | ~np.isfinite(mom[..., 1])
    sel = (a >= 0) & np.isfinite(a) & fits
    assert sel.sum() > 1000 and (a[sel] > 0).sum() > 800
    assert same_words(b[sel], a[sel] * F(16))
    assert np.all(b[~fits] == -1) and (~fits).sum() >= 64


# ---- what the window is for -----------------------------------------------------------------------------
def speck_scene():
    """A flat grey wall, 24 x 16, bright and noisy, every pixel at 4 calls; in its middle a 3 x 3 speck whose calls
    all returned 0, so own = 0 exactly there.  Three pixels wide because rule 3 smooths the variance over 3 x 3
    before it forms a weight: a single dark pixel borrows from its neighbours there, the centre of this speck has
    nothing to borrow.  The 7 x 7 window reaches past the speck."""
    H, W = 16, 24
    rng = np.random.default_rng(9)
    y, x = np.mgrid[0:H, 0:W]
    p0 = np.zeros((H, W, 4), dtype=F)
    p0[..., :3] = F(0.5)
    p0[..., 3] = np.full((H, W), 7, dtype=U).view(F)
    p1 = np.zeros((H, W, 4), dtype=F)
    p1[..., 2], p1[..., 3] = F(1), F(4)
    p2 = np.zeros((H, W, 4), dtype=F)
    p2[..., 0], p2[..., 1] = F(0.1) * x.astype(F), F(0.1) * y.astype(F)
    p2[..., 3] = np.full((H, W), am.HIT, dtype=U).view(F)
    n = np.full((H, W), 4, dtype=U)
    accum, m1, m2 = np.zeros((H, W, 3), dtype=F), np.zeros((H, W), dtype=F), np.zeros((H, W), dtype=F)
    for _ in range(4):
        S = (F(0.5) * (F(1) + rng.normal(0, 0.4, (H, W, 1)).astype(F)) * np.ones(3, dtype=F)).astype(F)
        S[7:10, 11:14] = F(0)
        yl = sm.lum(S)
        accum, m1, m2 = accum + S, m1 + yl, m2 + yl * yl
    color = np.ones((H, W, 4), dtype=F)
    color[..., :3] = accum / F(4)
    return color, p0, p1, p2, np.stack([m1, m2, n.view(F)], -1).astype(F)


def test_the_window_pulls_a_dark_speck_to_its_neighbourhood():
    color, p0, p1, p2, mom = speck_scene()
    flags, floor = DEMODULATE, 1e-6
    fargs = dict(sigma_l=4.0, variance_floor=floor, sigma_plane=0.3, normal_power_log2=2, flags=flags)
    ring = np.ones((7, 7), dtype=bool)
    ring[2:5, 2:5] = False
    around = float(sm.lum(color[5:12, 9:16, :3])[ring].mean())
    assert color[7:10, 11:14, :3].max() == 0 and around > 0.4
    # min_batches above its n: the pixel is young, and the spread of its window stands in for its own 0
    var = am.model(color, p0, p1, p2, mom, 8, 0.3, 0.0, flags)
    assert var[8, 12] > 0.01
    one = sm.filter_model(color, p0, p1, p2, var, iterations=1, **fargs)
    full = sm.filter_model(color, p0, p1, p2, var, iterations=3, **fargs)
    print("with the window: first level", sm.lum(one[8, 12, :3]), "three levels", sm.lum(full[8, 12, :3]), "around", around)
    # the first level's 16 taps outside the speck carry 1 - (3/8 + 2/4)^2 = 0.234 of the kernel: with every colour weight
    # at 1 the centre would reach 0.234 of its surroundings, and it must get at least half of that; three levels reach
    # past the speck with most of the kernel
    assert sm.lum(one[8, 12, :3]) > 0.5 * 0.234 * around and sm.lum(full[8, 12, :3]) > 0.5 * around
    # min_batches = 2: own = 0 exactly there and in its 3 x 3, so den = variance_floor.  Of the first level's 25 taps
    # the 16 outside the speck are at least d away in luminance (checked below); each weighs at most
    # h_q / (1 + d * d / floor) < h_c * floor / (d * d) against the centre's own h_c, the largest of the kernel.
    # So the pixel moves by less than 16 * floor / (d * d) of the largest of them: one variance_floor-sized weight.
    var2 = am.model(color, p0, p1, p2, mom, 2, 0.3, 0.0, flags)
    assert np.all(var2[7:10, 11:14] == 0)
    near = sm.lum((color[6:11, 10:15, :3] / F(0.5)).astype(F))
    outside = np.ones((5, 5), dtype=bool)
    outside[1:4, 1:4] = False
    d, top = float(near[outside].min()), float(near[outside].max())
    assert d > 0.15
    one2 = sm.filter_model(color, p0, p1, p2, var2, iterations=1, **fargs)
    print("min_batches 2: first level", sm.lum(one2[8, 12, :3]), "bound", 16 * (floor / (d * d)) * top * 0.5)
    assert sm.lum(one2[8, 12, :3]) <= 16 * (floor / (d * d)) * top * 0.5
