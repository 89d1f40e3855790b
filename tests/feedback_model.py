"""The feedback of the filtered colour into the temporal history (rule 4 of include/pt_hip.h) restated in numpy
float32, twice, on top of svgf_model (imported, not copied), and a seeded four-frame sequence for it.

filter_feedback_model()   the variance-guided filter with feedback, whole-image arithmetic: the texel after
                          `level` iterations comes from svgf_model.filter_model's `levels`
filter_feedback_scalar()  the same pixel by pixel, written from the header independently: kept and fed are decided
                          per pixel here, and the texel after `level` iterations comes from svgf_model.filter_scalar
                          run for `level` iterations on the demodulated colour without the DEMODULATE bit (its
                          prepare then divides by 1 and its finish multiplies by 1: both exact)
run_chain()               frames chained: a moments step, the estimate, the filter with feedback; the next frame
                          reprojects the fed h0

tests/test_feedback_rule.py holds the two forms against each other word for word; tests/test_gpu_feedback.py
holds the device against the whole-image form.
"""
import numpy as np

import svgf_model as sm
import temporal_model as tm
from denoise_model import F, U, HIT, EMISSIVE, bits, same_words   # noqa: F401

DEMODULATE, SAME_PRIMITIVE = sm.DEMODULATE, sm.SAME_PRIMITIVE


def _finite(x):
    return (x - x) == 0


# ---- the filter with feedback, whole image ---------------------------------------------------------------
def fed_mask(I, v):
    """fed_p of the rule from the texel (I', v' or -1) of iteration level - 1."""
    with np.errstate(all="ignore"):
        return ~(v < 0) & _finite(I[..., 0]) & _finite(I[..., 1]) & _finite(I[..., 2])


def filter_feedback_model(color, plane0, plane1, plane2, variance, hist0, level, iterations, sigma_l, variance_floor,
                          sigma_plane, normal_power_log2, flags, stats=None):
    """Returns (out, h0): svgf_model.filter_model's image, and hist0 with the colours of the texel after `level`
    iterations where the pixel is fed; the n words are hist0's."""
    assert 1 <= level <= iterations
    levels = []
    out = sm.filter_model(color, plane0, plane1, plane2, variance, iterations, sigma_l, variance_floor, sigma_plane,
                          normal_power_log2, flags, levels=levels)
    I, v, _ = levels[level]
    fed = fed_mask(I, v)
    hist0 = np.ascontiguousarray(hist0, dtype=F)
    h0 = hist0.copy()
    h0[..., :3] = np.where(fed[..., None], I, hist0[..., :3])
    if stats is not None:
        stats.update(fed=int(fed.sum()), kept=int((~(v < 0)).sum()),
                     changed=int((fed & (bits(h0[..., :3]) != bits(hist0[..., :3])).any(-1)).sum()),
                     kept_not_finite=int((~(v < 0) & ~fed).sum()))
    return out, h0


# ---- the same, pixel by pixel ------------------------------------------------------------------------------
def filter_feedback_scalar(color, plane0, plane1, plane2, variance, hist0, level, iterations, sigma_l, variance_floor,
                           sigma_plane, normal_power_log2, flags, want_out=True):
    assert 1 <= level <= iterations
    color, plane0, plane1, plane2, hist0 = (np.ascontiguousarray(a, dtype=F) for a in (color, plane0, plane1, plane2, hist0))
    variance = np.ascontiguousarray(variance, dtype=F)
    H, W = color.shape[:2]
    lo = F(1.0 / 64.0)

    def finite(x):
        return bool((x - x) == 0)

    kept = np.zeros((H, W), dtype=bool)
    demod = color.copy()
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                fl = int(bits(plane2[y, x, 3:4])[0])
                ok = bool(fl & HIT) and not fl & EMISSIVE
                for img in (color, plane1, plane2):
                    for k in range(3):
                        ok = ok and finite(img[y, x, k])
                for k in range(3):
                    d = F(1)
                    if flags & DEMODULATE:
                        a = plane0[y, x, k]
                        d = a if a > lo else lo
                    demod[y, x, k] = color[y, x, k] / d
                I = demod[y, x]
                l = (F(0.2126) * I[0] + F(0.7152) * I[1]) + F(0.0722) * I[2]
                var = variance[y, x]
                kept[y, x] = ok and bool(var >= 0) and finite(var) and finite(l)
    # the texel's colour after `level` iterations: with the bit clear the filter divides and multiplies by 1
    texel = sm.filter_scalar(demod, plane0, plane1, plane2, variance, level, sigma_l, variance_floor, sigma_plane,
                             normal_power_log2, flags & ~DEMODULATE)
    h0 = hist0.copy()
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                if kept[y, x] and all(finite(texel[y, x, k]) for k in range(3)):
                    for k in range(3):
                        h0[y, x, k] = texel[y, x, k]
    out = None
    if want_out:
        out = sm.filter_scalar(color, plane0, plane1, plane2, variance, iterations, sigma_l, variance_floor, sigma_plane,
                               normal_power_log2, flags)
    return out, h0


# ---- chained frames -------------------------------------------------------------------------------------
VPARAMS = dict(sm.VPARAMS)


def run_chain(step, filt, seq, flags, level, iterations=3, min_temporal=4, params=None, vparams=None, stats=None, **kw):
    """Chain `step` (svgf_model.model / scalar or a device call of that signature) and `filt`
    (filter_feedback_model / _scalar or a device call of that signature) over a sequence: every frame is a
    moments step with the estimate, then the filter of the step's image with feedback into the step's h0; the
    next frame's history is (fed h0, h1, h2, h3).  level = 0: no feedback (the filter is not run; out is None).
    Returns per frame (image, fed h0, h1, h2, h3, variance, out, unfed h0)."""
    p = dict(tm.PARAMS if params is None else params)
    v = dict(VPARAMS if vparams is None else vparams)
    outs, hist, prev = [], None, None
    for cam, frame in seq:
        image, h0, h1, h2, h3, var = step(*frame, cam, hist, prev if prev is not None else cam, p["alpha_min"],
                                          p["max_history"], p["sigma_plane"], p["normal_cos_min"], flags, min_temporal)
        out, fed = None, h0
        if level:
            skw = dict(kw)
            if stats is not None:
                stats.append({})
                skw["stats"] = stats[-1]
            out, fed = filt(image, *frame[1:], var, h0, level, iterations, v["sigma_l"], v["variance_floor"],
                            v["sigma_plane"], v["normal_power_log2"], flags, **skw)
        outs.append((image, fed, h1, h2, h3, var, out, h0))
        hist, prev = (fed, h1, h2, h3), cam
    return outs


def make_sequence(width=tm.WIDTH, height=tm.HEIGHT, seed=1):
    """svgf_model.make_sequence's three frames and a fourth, from a camera one more step along the same path, with
    the same special pixels (colours of 3e38 and 1e20, primitive ids of their own)."""
    seq = sm.make_sequence(width, height, seed)
    cam = tm.camera((0.9, 1.0, 2.0), (0.3, 0.8, -3.0), 60.0, width / height)
    color, p0, p1, p2 = (a.copy() for a in tm.make_frame(width, height, cam, seed, 3))
    y, x = np.mgrid[0:height, 0:width]
    color[(x % 9 == 4) & (y % 8 == 1), :3] = F(3e38)
    color[(x % 9 == 7) & (y % 8 == 6), :3] = F(1e20)
    ids = bits(p0[..., 3]).copy()
    alone = (x % 10 == 2) & (y % 9 == 4) & (ids != U(0xffffffff))
    ids[alone] = (U(1000) + (y * width + x).astype(U))[alone]
    p0[..., 3] = ids.view(F)
    return seq + [(cam, (color, p0, p1, p2))]


def make_overflow_inputs(width, height, seed):
    """svgf_model.make_filter_inputs, and a kept pixel whose filtered colour is not finite.  The taps' weights
    h sum to 1 and every other factor is at most 1 for unit normals, so I' is a convex mean and a colour of 3e38
    alone never overflows it; with a normal of length 1.5 (an interpolated normal nobody normalised) the centre
    weight is (9/64) * 2.25^(2^normal_power_log2) > 1 and 3e38 times it is +inf.  Every pixel with a colour of 3e38 gets
    such a normal and an ordinary variance; without DEMODULATE it is kept where it is a hit that is not emissive.
    Returns make_filter_inputs' tuple and the mask of those pixels."""
    color, p0, p1, p2, var, cls = sm.make_filter_inputs(width, height, seed)
    big = (color[..., 0] == F(3e38)) & (color[..., 1] == F(3e38)) & (color[..., 2] == F(3e38))
    p1, var = p1.copy(), var.copy()
    p1[big, :3] = (p1[big, :3] * F(1.5)).astype(F)
    var[big] = F(0.01)
    return color, p0, p1, p2, var, cls, big
