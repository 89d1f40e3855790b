"""The input sets of tests/dev_inputs.py (CPU): they are deterministic, every branch of every function
holds enough inputs, no tex2d input reads outside its texture, and the oracle's transcendentals stay
within measured distances of float64 over these same sets.  The GPU comparison over the sets is
tests/test_gpu_dev_functions.py."""
import numpy as np
import pytest

import dev_inputs as di
from oracle import pyoracle as po

F32 = np.float32


@pytest.mark.parametrize("op", sorted(di.BUILDERS))
def test_sets_are_deterministic_and_bounded(op):
    a, b = di.inputs(op), di.build(op)
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (op, k)
        assert a[k].tobytes() == b[k].tobytes(), f"{op}.{k}: two builds differ"
    assert 0 < di.count(op) <= di.MAX_INPUTS[op]
    assert len({v.size for v in a.values()}) == 1


@pytest.mark.parametrize("op", di.REGION_OPS)
def test_every_region_holds_enough_inputs(op):
    counts = {name: (int(mask.sum()), least) for name, (mask, least) in di.regions(op, di.inputs(op)).items()}
    short = {name: c for name, c in counts.items() if c[0] < c[1]}
    assert not short, f"{op}: regions with too few inputs (have, need): {short}"


def test_specials_cross_product_is_whole():
    assert len(set(di.SPECIAL_BITS.tolist())) == 16
    inp = di.inputs("atan2")
    pairs = set(zip(di.bits(inp["y"]).tolist(), di.bits(inp["x"]).tolist()))
    assert all((a, b) in pairs for a in di.SPECIAL_BITS.tolist() for b in di.SPECIAL_BITS.tolist())


def test_tex2d_taps_inside_and_forms_agree():
    di.check_tex2d_taps()


def test_tex2d_texture_table():
    texs = di.textures()
    assert [(t.shape[1], t.shape[0]) for t in texs] == list(di.TEX_SIZES)
    assert sum(bool(np.isinf(t).any()) for t in texs) == 1 and sum(bool(np.isnan(t).any()) for t in texs) == 1
    assert sum(bool((t < 0).any()) for t in texs) == 1
    for t in texs:
        ok = np.isfinite(t) & (t >= 0)
        assert t[ok].max() <= 60.0


@pytest.mark.parametrize("dev_op", list(di.DEVICE_OPS))
def test_fast_build_gives_the_same_words(dev_op):
    # the array entry points add loops only: liboracle_fast.so (bench.py's CPU baseline) keeps equal bits
    fast, plain = di.oracle_words(dev_op, fast=True), di.oracle_words(dev_op)
    differ = fast != plain
    if dev_op not in ("f2i_x86", "tonemap_pixel", "xorwow_init", "xorwow_skip", "xorwow_stream"):
        differ &= ~(np.isnan(fast.view(F32)) & np.isnan(plain.view(F32)))      # float words: equal, or both NaN
    assert not differ.any(), f"{dev_op}: {int(differ.sum())} words differ between the two builds of the oracle"


# ------------------------------------------------------------------------------------------------
# the oracle against float64
# ------------------------------------------------------------------------------------------------
# Measured over the sets above, rounded up to two significant digits.  "ulp": |oracle - float64| in ulp of
# the float64 result rounded to float32; "rel": |oracle - float64| / |float64|.  Only results that are
# normal floats count; on results in the denormal range (zero included) the absolute error must stay
# below 2^-149 times the ulp bound (for a relative bound: times the bound in units of 2^-24, and at
# least one 2^-149).  sin and cos are measured in ulp on the call sites' range [0, 2 pi]; beyond it, up to
# 65536, the three-part reduction is no longer exact near the zeros and the error is absolute.
BOUNDS = {
    "sin": {"ulp": 1.5, "abs_beyond_2pi": 9.6e-7},        # measured 1.487, 9.588e-7
    "cos": {"ulp": 14.0, "abs_beyond_2pi": 7.3e-7},       # measured 13.79 (beside the zeros at pi/2 and 3 pi/2), 7.227e-7
    "acos": {"ulp": 1.3},                                 # measured 1.260
    "atan2": {"ulp": 3.0},                                # measured 2.962
    "log": {"ulp": 0.81},                                 # measured 0.8021
    "exp": {"rel": 8.1e-8},                               # measured 8.015e-8
    "pow 2.2": {"rel": 8.0e-6},                           # measured 7.971e-6
    "pow 1/2.2": {"rel": 3.7e-6},                         # measured 3.638e-6
}
TINY = 2.0 ** -126


def float64_case(case):
    """(oracle float32 results, float64 results, mask of the inputs measured in ulp or relative terms,
    mask of those measured absolutely)."""
    with np.errstate(all="ignore"):
        if case in ("sin", "cos"):
            x = di.inputs("sincos_pos")["x"]
            got = po.dev_sincos(x)[0 if case == "sin" else 1]
            want = (np.sin if case == "sin" else np.cos)(x.astype(np.float64))
            return got, want, x <= di.K_TWO_PI, x > di.K_TWO_PI
        if case == "acos":
            x = di.inputs("acos")["x"]
            return po.dev_unary("acos", x), np.arccos(x.astype(np.float64)), None, None
        if case == "atan2":
            inp = di.inputs("atan2")
            return (po.dev_binary("atan2", inp["y"], inp["x"]),
                    np.arctan2(inp["y"].astype(np.float64), inp["x"].astype(np.float64)), None, None)
        if case == "log":
            x = di.inputs("log")["x"]
            return po.dev_unary("log", x), np.log(x.astype(np.float64)), None, None
        if case == "exp":
            x = di.inputs("exp")["x"]
            return po.dev_unary("exp", x), np.exp(x.astype(np.float64)), None, None
        yy = di.POW_Y[0 if case == "pow 2.2" else 1]
        inp = di.inputs("pow")
        m = inp["y"] == yy
        x, y = inp["x"][m], inp["y"][m]
        want = np.power(x.astype(np.float64), y.astype(np.float64))
        want[(x < 0) & ~np.isnan(x)] = np.nan          # pow_'s own rule: a negative base gives NaN (y != 0 here)
        return po.dev_binary("pow", x, y), want, None, None


@pytest.mark.parametrize("case", list(BOUNDS))
def test_oracle_against_float64(case):
    got, want, rel_mask, abs_mask = float64_case(case)
    with np.errstate(all="ignore"):
        want32 = want.astype(F32)
    everything = np.ones(got.size, dtype=bool)
    rel_mask = everything if rel_mask is None else rel_mask
    # NaNs and infinities at the same inputs as in float64 (rounded to float32), infinities of the same sign
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{case}: NaN at other inputs than float64"
    assert np.array_equal(np.isinf(got), np.isinf(want32)), f"{case}: infinity at other inputs than float64"
    inf = np.isinf(got)
    assert np.array_equal(np.signbit(got[inf]), np.signbit(want32[inf]))
    finite = np.isfinite(want32)
    normal = finite & (np.abs(want32) >= TINY)
    with np.errstate(all="ignore"):
        err = np.abs(got.astype(np.float64) - want)
    kind = "rel" if "rel" in BOUNDS[case] else "ulp"
    with np.errstate(all="ignore"):
        unit = np.abs(want) if kind == "rel" else np.spacing(np.abs(want32)).astype(np.float64)
    figures = {kind: float((err[normal & rel_mask] / unit[normal & rel_mask]).max())}
    if abs_mask is not None:
        figures["abs_beyond_2pi"] = float(err[finite & abs_mask].max())
    small = finite & ~normal & rel_mask
    figures["denormal range, in 2^-149"] = float(err[small].max() / 2.0 ** -149) if small.any() else 0.0
    print(f"{case}: " + ", ".join(f"{k} = {v:.4g}" for k, v in figures.items()))
    bound = BOUNDS[case]
    for k, b in bound.items():
        assert figures[k] <= b, f"{case}: {k} error {figures[k]:.4g} above the measured bound {b}"
    ulps = bound["ulp"] if kind == "ulp" else max(1.0, bound["rel"] * 2.0 ** 24)
    assert figures["denormal range, in 2^-149"] < ulps, f"{case}: denormal-range error {figures}"
