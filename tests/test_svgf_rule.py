"""The rules of the per-pixel variance and the variance-guided filter (include/pt_hip.h) on the CPU: the two
numpy restatements of each (tests/svgf_model.py) against each other word for word, the colour of the moments
step against temporal_model.model, the identities the rules imply, that the seeded inputs hold every case,
and the filter's properties.  tests/test_gpu_svgf.py holds the device against the same models.
"""
import re

import numpy as np
import pytest

import denoise_model as dm
import pathtracercuda_amd as pa
import svgf_model as sm
import temporal_model as tm
from pathtracercuda_amd import _native as N

F = sm.F
NAMES = ("image", "h0", "h1", "h2", "h3", "variance")


def assert_same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert sm.same_words(g, w), f"{what}: {name} differs"


@pytest.fixture(scope="module")
def sequence():
    return sm.make_sequence()


# ---- the moments step and the estimate -----------------------------------------------------------------
@pytest.mark.parametrize("flags", (0, 1, 2, 3))
def test_model_equals_scalar_restatement(sequence, flags):
    mt = 4 if flags & 1 else 2
    a = sm.run_sequence(sm.model, sequence, flags, min_temporal=mt)
    b = sm.run_sequence(sm.scalar, sequence, flags, min_temporal=mt)
    for k in range(3):
        assert_same(a[k], b[k], f"flags {flags}, frame {k}")
    assert not sm.same_words(a[2][4], a[1][4])


def test_model_equals_scalar_on_small_images():
    for (w, h) in ((1, 1), (1, 7), (5, 1), (9, 6)):
        seq = sm.make_sequence(w, h, 10 * w + h)
        a, b = sm.run_sequence(sm.model, seq, 3), sm.run_sequence(sm.scalar, seq, 3)
        for k in range(3):
            assert_same(a[k], b[k], f"{w}x{h}, frame {k}")


@pytest.mark.parametrize("flags", (0, 1, 2, 3))
def test_colour_and_history_are_the_temporal_rules(sequence, flags):
    ours = sm.run_sequence(sm.model, sequence, flags)
    theirs = tm.run_sequence(tm.model, sequence, flags)
    for k in range(3):
        for name, g, w in zip(NAMES[:4], ours[k][:4], theirs[k]):
            assert sm.same_words(g, w), f"flags {flags}, frame {k}: {name} differs from temporal_model.model"


def test_a_camera_that_stands_still_gives_the_running_moments():
    cam = tm.cameras()[0]
    frames = [tm.make_frame(tm.WIDTH, tm.HEIGHT, cam, 5, k) for k in range(5)]
    ok = tm.ok_mask(frames[0][0], frames[0][2], frames[0][3])
    hist, m1, m2 = None, None, None
    for k, f in enumerate(frames, 1):
        out = sm.model(*f, cam, hist, cam, 0.0, 1000, 0.05, 0.9, 0, 4)
        with np.errstate(all="ignore"):
            l = sm.lum(f[0][..., :3])
            q = l * l
            m1 = l.copy() if m1 is None else (m1 + F(1.0 / k) * (l - m1)).astype(F)
            m2 = q.copy() if m2 is None else (m2 + F(1.0 / k) * (q - m2)).astype(F)
            v = m2 - m1 * m1
            v = np.where((v > 0) & np.isfinite(v), v, F(0)).astype(F)
        h3 = out[4]
        assert sm.same_words(h3[..., 0][ok], m1[ok]) and sm.same_words(h3[..., 1][ok], m2[ok])
        assert sm.same_words(h3[..., 2][ok], v[ok])
        assert np.all(h3[~ok] == np.array([0, 0, -1, 0], dtype=F))
        assert np.all(out[5][~ok] == -1)
        if k >= 4:                                      # the temporal estimate everywhere
            assert sm.same_words(out[5][ok], v[ok]) and (v[ok] > 0).sum() > ok.sum() // 2
        hist = out[1:5]
    assert ok.sum() > ok.size // 2


def test_a_constant_sequence_has_variance_zero():
    """The same frame again and again under a camera that stands still: m1 stays l and m2 stays l * l word for
    word (Hm + a * (x - Hm) with x == Hm), so the temporal variance m2 - m1 * m1 is +0 exactly in every frame,
    and the variance plane is +0 exactly as soon as it is the temporal one -- from the first frame with
    min_temporal = 1, from the fourth with 4.  (Before that the plane holds the spatial estimate, which is of
    the image's variation in space, not in time.)"""
    cam = tm.cameras()[0]
    frame = tm.make_frame(tm.WIDTH, tm.HEIGHT, cam, 5, 0)
    ok = tm.ok_mask(frame[0], frame[2], frame[3])
    with np.errstate(all="ignore"):
        l = sm.lum(frame[0][..., :3])
    ok &= np.isfinite(l * l)
    for mt in (1, 4):
        hist = None
        for k in range(1, 7):
            out = sm.model(*frame, cam, hist, cam, 0.0, 1000, 0.05, 0.9, 0, mt)
            assert np.all(sm.bits(out[4][..., 2][ok]) == 0), (mt, k)
            assert sm.same_words(out[4][..., 0][ok], l[ok])
            if k >= mt:
                assert np.all(sm.bits(out[5][ok]) == 0), (mt, k)
            else:
                assert (out[5][ok] > 0).sum() > ok.sum() // 2      # the spatial estimate of a noisy image
            assert np.all(out[5][out[1][..., 3] < 1] == -1)
            hist = out[1:5]
        assert (out[1][..., 3][ok] == 6).all()
    assert ok.sum() > ok.size // 2


def test_the_sequence_holds_every_case(sequence):
    stats = []
    sm.run_sequence(sm.model, sequence, 3, params=dict(tm.PARAMS, max_history=6), min_temporal=3, stats=stats)
    loose = []
    sm.run_sequence(sm.model, sequence, 1, min_temporal=3, stats=loose)
    for k, s in enumerate(stats):
        print(k, s)
    assert all(s["spatial"] > 0 for s in stats) and stats[0]["temporal"] == 0 and stats[2]["temporal"] > 0
    assert max(s["k1"] for s in stats) > 0
    assert max(s["restarted"] for s in stats[1:]) > 0
    for key in ("outside", "no_history", "by_id"):
        assert max(s[key] for s in stats) > 0, (key, stats)
    for key in ("by_normal", "by_plane"):
        assert max(s[key] for s in loose) > 0, (key, loose)


# ---- the filter ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", (0, 1, 2, 3))
def test_filter_model_equals_scalar_restatement(flags):
    color, p0, p1, p2, var, cls = sm.make_filter_inputs(23, 14, 40 + flags)
    assert set(np.unique(cls)) == set(range(len(sm.CLASSES)))
    a = sm.filter_model(color, p0, p1, p2, var, 3, flags=flags, **sm.VPARAMS)
    b = sm.filter_scalar(color, p0, p1, p2, var, 3, flags=flags, **sm.VPARAMS)
    assert sm.same_words(a, b)
    keep = sm.vkeep_mask(color, p0, p1, p2, var, flags)
    assert keep.sum() > keep.size // 2 and (sm.bits(a[..., :3]) != sm.bits(color[..., :3])).any(-1)[keep].mean() > 0.9


def test_the_keep_mask_follows_the_variance_classes_and_the_luminance():
    color, p0, p1, p2, var, cls = sm.make_filter_inputs(48, 40, 9)
    base = dm.keep_mask(color, p1, p2)
    for flags in (0, 1):
        keep = sm.vkeep_mask(color, p0, p1, p2, var, flags)
        for idx, name in enumerate(sm.CLASSES):
            sel = base & (cls == idx)
            assert sel.any(), name
            if name in ("inf", "nan", "negative"):
                assert not keep[sel].any(), name
        assert not (keep & ~base).any()
    # colours near 3e38: finite, so pt_denoise keeps them; divided by an albedo below 1 their luminance is not
    bright = base & (color[..., 0] == F(3e38)) & (cls <= 3) & (p0[..., :3] < F(0.85)).any(-1)
    assert bright.any() and not sm.vkeep_mask(color, p0, p1, p2, var, 1)[bright].any()


def test_a_pixel_that_is_not_kept_passes_through_and_reaches_nobody():
    color, p0, p1, p2, var, cls = sm.make_filter_inputs(48, 40, 11)
    keep = sm.vkeep_mask(color, p0, p1, p2, var, 1)
    out = sm.filter_model(color, p0, p1, p2, var, 4, flags=1, **sm.VPARAMS)
    assert np.array_equal(sm.bits(out[..., :3])[~keep], sm.bits(color[..., :3])[~keep]) and np.all(out[..., 3] == 1)
    assert np.isfinite(out[..., :3][keep]).all()
    # what a pixel that is not kept holds does not matter to anybody else
    other = color.copy()
    other[..., :3][~keep & np.isfinite(color[..., :3]).all(-1)] = F(123.0)
    var2 = np.where(keep, var, F(-3.0)).astype(F)            # (still not kept)
    assert np.array_equal(sm.vkeep_mask(other, p0, p1, p2, var2, 1), keep)
    out2 = sm.filter_model(other, p0, p1, p2, var2, 4, flags=1, **sm.VPARAMS)
    assert np.array_equal(sm.bits(out2[..., :3])[keep], sm.bits(out[..., :3])[keep])


def test_the_filtered_variance_never_exceeds_the_largest_in_reach():
    color, p0, p1, p2, var, cls = sm.make_filter_inputs(48, 40, 12)
    levels = []
    sm.filter_model(color, p0, p1, p2, var, 4, flags=1, levels=levels, **sm.VPARAMS)
    for i in range(4):
        (_, v, keep), (_, v2, _) = levels[i], levels[i + 1]
        s = 1 << i
        reach = np.full(v.shape, F(-1))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                reach = np.maximum(reach, dm._shift(v, s, dx, dy, F(-1)))
        # v' = sum(w^2 v) / (sum w)^2 <= max v, since sum(w^2) <= (sum w)^2; 25 roundings of 2^-24 each way
        assert np.all(v2[keep] <= reach[keep] * F(1 + 64 * 2.0 ** -24)), i
        assert np.all(v2[keep] >= 0) and np.array_equal(sm.bits(v2[~keep]), sm.bits(v[~keep]))


def flat_inputs(width, height, value=0.5):
    """One flat surface facing the camera: every geometric weight is exactly 1."""
    color = np.full((height, width, 4), F(value))
    p0 = np.ones((height, width, 4), dtype=F)
    p0[..., 3] = np.zeros((height, width), dtype=np.uint32).view(F)
    p1 = np.zeros((height, width, 4), dtype=F)
    p1[..., 2], p1[..., 3] = F(1), F(2)
    y, x = np.mgrid[0:height, 0:width]
    p2 = np.zeros((height, width, 4), dtype=F)
    p2[..., 0], p2[..., 1] = x.astype(F), y.astype(F)
    p2[..., 3] = np.full((height, width), sm.HIT, dtype=np.uint32).view(F)
    return color, p0, p1, p2


def test_the_colour_weight_is_one_over_one_plus_d2_over_sigma2_v():
    # two pixels side by side: p at luminance L, q at L + d, equal variances V, a negligible floor.  One
    # iteration gives I'_p = (h0 I_p + h1 w I_q) / (h0 + h1 w) with w = 1 / (1 + d^2 / (sigma^2 V)).
    sigma, V, d = 2.0, 0.01, 0.3
    color, p0, p1, p2 = flat_inputs(2, 1)
    color[0, 1, :3] = F(0.5 + d)
    var = np.full((1, 2), F(V))
    out = sm.filter_model(color, p0, p1, p2, var, 1, sigma, 1e-30, 0.05, 0, 0)
    w = 1.0 / (1.0 + d * d / (sigma * sigma * V))
    h0, h1 = (3 / 8) ** 2, (1 / 4) * (3 / 8)
    want = (h0 * 0.5 + h1 * w * (0.5 + d)) / (h0 + h1 * w)
    assert abs(float(out[0, 0, 0]) - want) < 1e-6 and w < 0.4


def outlier_inputs(own_variance):
    color, p0, p1, p2 = flat_inputs(9, 9)
    color[4, 4, :3] = F(50.0)
    var = np.full((9, 9), F(0.001))
    var[4, 4] = F(own_variance)
    return color, p0, p1, p2, var


def test_an_outlier_with_a_large_variance_is_pulled_to_its_neighbours_and_one_with_none_is_not():
    args = (3, 4.0, 1e-6, 0.05, 0, 0)
    noisy = sm.filter_model(*outlier_inputs(2500.0), *args)
    assert float(noisy[4, 4, 0]) < 25.0, noisy[4, 4]
    sure = sm.filter_model(*outlier_inputs(0.0), *args)
    assert float(sure[4, 4, 0]) > 49.0, sure[4, 4]
    # and a neighbour of the outlier that is sure of itself keeps away from it
    assert float(sure[4, 5, 0]) < 0.6


# ---- the header and the Python layer --------------------------------------------------------------------
def test_header_constants_and_defaults(root):
    text = (root / "include" / "pt_hip.h").read_text()

    def define(name):
        return re.search(rf"#define {name} (\S+)", text).group(1).rstrip("fu")

    assert int(define("PT_VARIANCE_DEFAULT_MIN_TEMPORAL")) == pa.VARIANCE_DEFAULTS["min_temporal"]
    d = pa.VDENOISE_DEFAULTS
    assert int(define("PT_VDENOISE_DEFAULT_ITERATIONS")) == d["iterations"]
    assert float(define("PT_VDENOISE_DEFAULT_SIGMA_L")) == d["sigma_l"]
    assert float(define("PT_VDENOISE_DEFAULT_VARIANCE_FLOOR")) == d["variance_floor"]
    assert float(define("PT_VDENOISE_DEFAULT_SIGMA_PLANE")) == d["sigma_plane"]
    assert int(define("PT_VDENOISE_DEFAULT_NORMAL_POWER_LOG2")) == d["normal_power_log2"]
    assert int(define("PT_VDENOISE_DEFAULT_FLAGS")) == (1 if d["demodulate"] else 0) | (2 if d["same_primitive"] else 0)


def test_python_refusals_name_the_field():
    nan = float("nan")
    for kw, field in ((dict(iterations=0), "iterations"), (dict(iterations=9), "iterations"), (dict(sigma_l=0.0), "sigma_l"),
                      (dict(sigma_l=2.0 ** 21), "sigma_l"), (dict(sigma_l=nan), "sigma_l"), (dict(variance_floor=0.0), "variance_floor"),
                      (dict(variance_floor=float("inf")), "variance_floor"), (dict(variance_floor=nan), "variance_floor"),
                      (dict(sigma_plane=1e-7), "sigma_plane"), (dict(sigma_plane=nan), "sigma_plane"),
                      (dict(normal_power_log2=8), "normal_power_log2"), (dict(staging=3), "staging")):
        with pytest.raises(pa.PathtracerError) as e:
            pa.vdenoise_params(**kw)
        assert e.value.code == N.PT_ERR_ARG and field in str(e.value), kw
    for bad in (0, 256, 2.5, nan):
        with pytest.raises(pa.PathtracerError) as e:
            pa.variance_params(bad)
        assert e.value.code == N.PT_ERR_ARG and "min_temporal" in str(e.value)
    p = pa.vdenoise_params()
    d = pa.VDENOISE_DEFAULTS
    assert (p.iterations, p.sigma_l, p.flags, p.staging) == (d["iterations"], d["sigma_l"], 1, 0)
    assert p.variance_floor == np.float32(d["variance_floor"]) and pa.variance_params().min_temporal == 4
