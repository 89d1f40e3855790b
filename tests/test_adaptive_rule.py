"""Adaptive sampling: the stop rule of pt_render_adaptive (include/pt_hip.h) restated in numpy float32
and driven by the CPU oracle.  No GPU here; tests/test_gpu_adaptive.py imports the restatement and
compares the device against it bit for bit.

How the oracle is driven: OracleRenderer.render(cam, spp, True) leaves each pixel's call colour sum S in
ref.accum while its RNG carries on, so every step renders ALL pixels one call, and the pixels the rule
left inactive get their RNG words put back (a numpy view of ref.rng).  The expected accumulation is
A_1 = S_1, A_k = S_k + A_{k-1} in float32 (trace.cu:196), the moments are the header's operations.
A render makes at most max_calls steps counted from the reset: a pixel that stopped and started again
ends below max_calls, and a render cut at 4 steps and continued to 8 is the 8-step render.
"""
import numpy as np
import pytest

from oracle import pyoracle as po

F = np.float32

# (scene, width, height, band_rows, row_offset, row_stride); widths and heights ragged on purpose
CASES = {
    "generated": ("generated_scene", 90, 52, 1, 0, 1),
    "shapes": ("test_shapes", 76, 44, 1, 0, 1),
    "cornell": ("cornell_box", 60, 44, 1, 0, 1),
    "banded": ("generated_scene", 90, 96, 8, 1, 2),
}
PARAMS = dict(spp=4, min_calls=2, max_calls=8, tolerance=0.2, floor=0.01)
# pixels ending at n = 2..8 and active pixels per step, from the oracle, for CASES under PARAMS
EXPECTED = {
    "generated": ([1747, 181, 168, 169, 197, 216, 2002], [4680, 4680, 2882, 2694, 2557, 2402, 2254, 2115]),
    "shapes": ([835, 271, 287, 127, 127, 147, 1550], [3344, 3344, 2372, 2124, 1895, 1828, 1797, 1753]),
    "cornell": ([1029, 26, 33, 44, 53, 84, 1371], [2640, 2640, 1371, 1455, 1508, 1552, 1585, 1611]),
    "banded": ([1951, 198, 154, 187, 169, 171, 1490], [4320, 4320, 2334, 2128, 1973, 1810, 1692, 1601]),
}


def luminance(S):
    return (F(0.2126) * S[..., 0] + F(0.7152) * S[..., 1]) + F(0.0722) * S[..., 2]


def unconverged(m1, m2, n, min_calls, tolerance, floor):
    """Pixels with their minimum of calls whose standard error is above the tolerance (pass 1)."""
    with np.errstate(all="ignore"):
        k = n.astype(F)
        mean = m1 / k
        ss = m2 - m1 * mean
        ss = np.where(ss < 0, F(0), ss)
        se2 = ss / (k * (k - F(1)))
        t = F(tolerance) * (np.abs(mean) + F(floor))
        conv = (se2 <= t * t) | ~np.isfinite(m2)
    if not tolerance > 0:
        conv = np.zeros_like(conv)          # tolerance 0 never converges
    return (n >= min_calls) & ~conv


def active_pixels(m1, m2, n, min_calls, max_calls, tolerance, floor):
    """The rule: below min_calls, or below max_calls with an unconverged pixel in the clipped 3x3."""
    flag = unconverged(m1, m2, n, min_calls, tolerance, floor)
    h, w = flag.shape
    pad = np.zeros((h + 2, w + 2), dtype=bool)
    pad[1:-1, 1:-1] = flag
    near = np.zeros_like(flag)
    for dy in range(3):
        for dx in range(3):
            near |= pad[dy:dy + h, dx:dx + w]
    return (n < min_calls) | ((n < max_calls) & near)


class AdaptiveOracle:
    """State of an adaptive render next to an OracleRenderer: accumulation, moments, counts."""

    def __init__(self, ref):
        self.ref = ref
        shape = (ref.rows, ref.width)
        self.accum = np.zeros(shape + (4,), dtype=F)
        self.m1 = np.zeros(shape, dtype=F)
        self.m2 = np.zeros(shape, dtype=F)
        self.n = np.zeros(shape, dtype=np.uint32)
        self.steps = []                      # active pixels of every step (call) so far

    def render(self, camera, spp, min_calls, max_calls, tolerance, floor=0.01, reset=True):
        ref = self.ref
        npix = ref.rows * ref.width
        words = np.frombuffer(ref.rng, dtype=np.uint32)[:6 * npix].reshape(ref.rows, ref.width, 6)
        fresh = np.zeros(self.n.shape, dtype=bool)
        if reset:
            self.m1[:] = 0
            self.m2[:] = 0
            self.n[:] = 0
            fresh[:] = True                  # the first call overwrites the accumulation value
            self.steps = []
        while len(self.steps) < max_calls:   # steps are counted from the reset, across continuations
            act = active_pixels(self.m1, self.m2, self.n, min_calls, max_calls, tolerance, floor)
            if not act.any():
                break
            saved = words.copy()
            ref.render(camera, spp, True)
            words[~act] = saved[~act]
            S = ref.accum[..., :3].copy()
            y = luminance(S)
            with np.errstate(all="ignore"):
                summed = np.where(fresh[..., None], S, S + self.accum[..., :3])
                self.accum[..., :3] = np.where(act[..., None], summed, self.accum[..., :3])
                self.accum[..., 3] = np.where(act, F(1), self.accum[..., 3])
                self.m1 = np.where(act, self.m1 + y, self.m1)
                self.m2 = np.where(act, self.m2 + y * y, self.m2)
            self.n = np.where(act, self.n + 1, self.n).astype(np.uint32)
            fresh &= ~act
            self.steps.append(int(act.sum()))
        return self

    def rng_array(self):
        return self.ref.rng_array()

    def moments(self):
        return np.stack([self.m1, self.m2, self.n.view(F)], axis=-1)


def make_oracle(scenes, case):
    name, W, H, band, off, stride = CASES[case]
    osc = po.load_scene(scenes / f"{name}.scene.json", W, H)
    return osc, po.OracleRenderer(osc, W, H, off, stride, band_rows=band)


_cache = {}


def expected(scenes, case):
    """The oracle's adaptive render of a case under PARAMS; computed once, never modified."""
    if case not in _cache:
        osc, ref = make_oracle(scenes, case)
        _cache[case] = (osc, AdaptiveOracle(ref).render(osc.camera, **PARAMS))
    return _cache[case]


def check_inputs(case, ad):
    """The conditions that make a case worth comparing: every path of the rule is taken."""
    npix = ad.n.size
    lo, hi = PARAMS["min_calls"], PARAMS["max_calls"]
    assert ad.n.min() >= lo and ad.n.max() <= hi
    assert (ad.n == lo).sum() >= 0.15 * npix, "too few pixels stop at min_calls"
    assert (ad.n == hi).sum() >= 0.25 * npix, "too few pixels reach max_calls"
    assert ((ad.n > lo) & (ad.n < hi)).sum() >= 0.08 * npix, "too few pixels stop in between"
    assert all(s % 64 for s in ad.steps), "a step without a partial last wave"
    assert ad.steps[:lo] == [npix] * lo
    assert sum(ad.steps) == int(ad.n.sum())
    if case == "cornell":
        assert any(b > a for a, b in zip(ad.steps[lo:], ad.steps[lo + 1:])), "no step reactivates pixels"


@pytest.mark.parametrize("case", list(CASES))
def test_rule_on_oracle(scenes, case):
    osc, ad = expected(scenes, case)
    check_inputs(case, ad)
    hist = [int((ad.n == k).sum()) for k in range(PARAMS["min_calls"], PARAMS["max_calls"] + 1)]
    assert (hist, ad.steps) == EXPECTED[case]
    # a stopped pixel holds what n plain calls leave: spot-check against the prefix of a plain render
    _, ref = make_oracle(scenes, case)
    ref.render(osc.camera, PARAMS["spp"], True, chunks=PARAMS["min_calls"])
    at_min = ad.n == PARAMS["min_calls"]
    assert np.array_equal(ad.accum[at_min].view(np.uint32), ref.accum[at_min].view(np.uint32))
    assert np.array_equal(ad.rng_array()[at_min], ref.rng_array()[at_min])


def test_tolerance_zero_is_the_plain_render(scenes):
    osc, ref = make_oracle(scenes, "cornell")
    p = dict(PARAMS, tolerance=0.0)
    ad = AdaptiveOracle(ref).render(osc.camera, **p)
    _, plain = make_oracle(scenes, "cornell")
    plain.render(osc.camera, p["spp"], True, chunks=p["max_calls"])
    assert (ad.n == p["max_calls"]).all()
    assert np.array_equal(ad.accum.view(np.uint32), plain.accum.view(np.uint32))
    assert np.array_equal(ad.rng_array(), plain.rng_array())


def test_python_interface():
    import ctypes as C
    import inspect

    import pathtracercuda_amd as pa
    from pathtracercuda_amd import _native as N
    sig = inspect.signature(pa.Pathtracer.render_adaptive)
    assert list(sig.parameters) == ["self", "camera", "spp", "min_calls", "max_calls", "tolerance", "floor", "reset"]
    assert sig.parameters["floor"].default == 0.01 and sig.parameters["reset"].default is True
    for name in ("moments", "sample_counts", "noise_map"):
        assert callable(getattr(pa.Pathtracer, name))
    assert C.sizeof(N.PtAdaptiveParams) == 24 and C.sizeof(N.PtAdaptiveResult) == 24
    # device groups are out of scope: the call raises before it reaches the native layer
    group = pa.Pathtracer.__new__(pa.Pathtracer)
    group._group, group._r = 1, None
    with pytest.raises(pa.PathtracerError) as e:
        group.render_adaptive(pa.PtCamera(), 4, 2, 8, 0.1)
    assert e.value.code == N.PT_ERR_STATE


def test_dilation_and_bounds():
    # one noisy pixel in a field of zero-variance ones keeps its 3x3 neighbourhood (clipped at the
    # corner) sampling; min_calls and max_calls bound every pixel whatever its noise
    m1 = np.zeros((5, 6), dtype=F)
    m2 = np.zeros((5, 6), dtype=F)
    n = np.full((5, 6), 3, dtype=np.uint32)
    m1[0, 0], m2[0, 0] = 3.0, 9.0            # calls 0, 0, 3: mean 1, far above a 10 % tolerance
    act = active_pixels(m1, m2, n, 2, 8, 0.1, 0.01)
    want = np.zeros((5, 6), dtype=bool)
    want[:2, :2] = True
    assert np.array_equal(act, want)
    assert active_pixels(m1, m2, np.full((5, 6), 1, dtype=np.uint32), 2, 8, 0.1, 0.01).all()
    assert not active_pixels(m1, m2, np.full((5, 6), 8, dtype=np.uint32), 2, 8, 0.1, 0.01).any()
    m2[3, 3] = np.inf                        # a non-finite pixel counts as converged
    m1[3, 3] = np.inf
    assert not active_pixels(m1, m2, n, 2, 8, 0.1, 0.01)[2:, 2:].any()
    assert active_pixels(m1, m2, n, 2, 8, 0.0, 0.01).all()      # tolerance 0 never converges
