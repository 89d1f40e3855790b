"""Input sets for the function-level comparison of the kernel's device functions with the oracle
(tests/test_dev_inputs.py on the CPU, tests/test_gpu_dev_functions.py on the GPU).

Every set is deterministic (fixed seeds, no clock) and has three parts: a strided sweep of bit patterns
over the whole range the function's call sites can pass, every float within 256 ulp of each constant
the function branches on, and a cross product of special values.  At most 2^22 inputs per operation
(tex2d: 2^18).  regions(op, inputs) names the branches of each function as numpy predicates restated
from csrc/pt_math.h, csrc/pt_dev_tex.h and csrc/pt_dev_tonemap.h; tests/test_dev_inputs.py asserts that
every region holds enough inputs.

Inputs are float32 arrays unless stated; float arithmetic in the predicates is float32 (numpy rounds
each operation once, as the kernel and the oracle do with contraction off).
"""
import functools
import pathlib

import numpy as np

from oracle import pyoracle as po

F32, U32, I64 = np.float32, np.uint32, np.int64
ULPS = 256                      # half-width of the neighbourhood of a branch constant

K_PI = F32(3.14159265358979323846)
K_TWO_PI = F32(2.0) * K_PI
K_FOPI = F32(1.27323954473516)
QNAN, QNAN_NEG = 0x7FC00000, 0xFFC00000
FLT_MAX_BITS, INF_BITS = 0x7F7FFFFF, 0x7F800000
# +-0, +-smallest denormal, +-largest denormal, +-smallest normal, +-1, +-FLT_MAX, +-inf, a quiet NaN of each sign
SPECIAL_BITS = np.array([s | m for m in (0, 1, 0x007FFFFF, 0x00800000, 0x3F800000, FLT_MAX_BITS, INF_BITS, QNAN)
                         for s in (0, 0x80000000)], dtype=U32)
MIN_REGION, MIN_LINE = 64, 4    # inputs a region must hold; a region that is one special-value line


def f32(bits):
    return np.ascontiguousarray(bits, dtype=U32).view(F32)


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(U32)


SPECIALS = f32(SPECIAL_BITS)


def sweep(lo_bits, hi_bits, count):
    """`count` bit patterns from lo_bits to hi_bits inclusive, evenly strided."""
    return f32(np.round(np.linspace(float(lo_bits), float(hi_bits), count)).astype(np.uint64).astype(U32))


def sweep_all(count):
    """Every class of float of both signs: bit patterns 0 .. 2^32 - 1, strided."""
    return sweep(0, 0xFFFFFFFF, count)


def near(values, k=ULPS):
    """Every float within k ulp of each value (steps through zero into the other sign)."""
    b = bits(np.atleast_1d(np.asarray(values, dtype=F32))).astype(I64)
    o = np.where(b < 2**31, b, 2**31 - b)                       # monotone in the float's value
    o = (o[:, None] + np.arange(-k, k + 1, dtype=I64)[None, :]).ravel()
    o = np.clip(o, -(INF_BITS - 0), INF_BITS)
    return f32(np.where(o >= 0, o, 2**31 - o).astype(U32))


def cat(*parts):
    return np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=F32).ravel() for p in parts]))


def cross(a, b):
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    return np.repeat(a, b.size), np.tile(b, a.size)


# ------------------------------------------------------------------------------------------------
# the sets
# ------------------------------------------------------------------------------------------------
def _sincos_pos():
    # The contract is x in [0, 65536] (pt_math.h); both call sites pass 2 pi u with u a curand_uniform
    # value in [2^-33, 1].  Inputs above 65536, negative inputs, infinities and NaN are outside the
    # contract (the oracle's pm_sinf returns early there, sincos_pos has no such line) and are left out.
    u = sweep(bits(F32(2.0**-33))[0], 0x3F800000, 1 << 19)
    draws = po.dev_xorwow_stream(1984, 1 << 20)[1]
    octants = near([F32(k * np.pi / 4) for k in range(9)])
    x = cat(K_TWO_PI * u, K_TWO_PI * draws, sweep(0, bits(F32(65536.0))[0], 1 << 19), octants,
            SPECIALS[(SPECIALS >= 0) & (SPECIALS <= 65536)])
    return {"x": x[(x >= 0) & (x <= F32(65536.0))]}


def _acos():
    mag = sweep(0, 0x3F800000, 1 << 18)                      # |x| <= 1, the range acos is defined on
    half = sweep(0x3F000000, 0x3F800000, 1 << 18)            # 0.5 <= |x| <= 1, the square-root ranges
    return {"x": cat(sweep_all(1 << 20), mag, -mag, half, -half,
                     near([0.5, -0.5, 1.0, -1.0, 1.0e-4, -1.0e-4, 0.0]), SPECIALS)}


def _atan2():
    rng = np.random.default_rng(20261)
    sy, sx = cross(SPECIALS, SPECIALS)
    rb = rng.integers(0, 2**32, size=(2, 1 << 21), dtype=np.uint64).astype(U32)
    nrm = rng.standard_normal(size=(2, 1 << 20)).astype(F32)
    ys, xs = [sy, f32(rb[0]), nrm[0]], [sx, f32(rb[1]), nrm[1]]
    # quotients within 256 ulp of atan_pos's two range constants: exact ones (x a power of two) and
    # rounded ones (x = 3, 7 / 5, ...), in every quadrant
    t = near([F32(0.4142135623730950), F32(2.414213562373095)])
    for xm in (2.0**-60, 2.0**-20, 1.0, 2.0**40, 3.0, 1.4, 1.0e-3, 12345.678):
        for sgy, sgx in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            ys.append(F32(sgy) * (t * F32(xm)))
            xs.append(np.full(t.size, sgx * xm, dtype=F32))
    # denormal quotients (2^-149 <= ay / ax < 2^-126) and quotients that overflow, finite arguments
    m = f32((rng.integers(0, 2**23, size=4096, dtype=np.uint64) | 0x3F800000).astype(U32))     # [1, 2)
    e = rng.integers(0, 23, size=4096)
    sg = np.where(rng.integers(0, 2, size=(2, 4096)) == 1, F32(-1), F32(1))
    ys += [sg[0] * np.ldexp(m, -110 - e).astype(F32), sg[0] * np.ldexp(m, 100 + e).astype(F32)]
    xs += [sg[1] * np.ldexp(m[::-1], 17).astype(F32), sg[1] * np.ldexp(m[::-1], -40).astype(F32)]
    # a denormal against a denormal, and against a normal
    d = f32(rng.integers(1, 2**23, size=(2, 4096), dtype=np.uint64).astype(U32))
    ys += [sg[0] * d[0], sg[0] * d[0]]
    xs += [sg[1] * d[1], sg[1] * np.ldexp(m, -120).astype(F32)]
    return {"y": cat(*ys), "x": cat(*xs)}


SQRT_HALF_BITS = 0x3F3504F3     # 0.707106781186547524f


def _log():
    # log_ is reached through pow_ alone, which passes positive finite x: zero, negatives, inf and NaN
    # are answered by pow_'s early returns and never reach it.
    parts = [sweep(1, FLT_MAX_BITS, 1 << 20)]
    for k in range(23):                                       # every denormal binade
        parts.append(sweep(1 << k, (2 << k) - 1, min(1 << k, 2048)))
    man = SQRT_HALF_BITS & 0x7FFFFF
    off = np.arange(-ULPS, ULPS + 1, dtype=I64)
    parts.append(f32(((np.arange(1, 255, dtype=I64)[:, None] << 23) + man + off[None, :]).ravel().astype(U32)))
    for s in range(1, 16):                                    # the same mantissa in denormals
        parts.append(f32((((man | 0x800000) >> s) + off).astype(U32)))
    parts.append(near([1.0, 0.5, 2.0]))
    parts.append(SPECIALS[(SPECIALS > 0) & np.isfinite(SPECIALS)])
    return {"x": cat(*parts)}


EXP_HI, EXP_LO = F32(88.7228391), F32(-103.972084)
LOG2E = F32(1.44269504088896341)


def _exp():
    ns = np.arange(-160, 131, dtype=np.float64)
    ties = near(((ns - 0.5) / float(LOG2E)).astype(F32))     # 1.4427 x + 0.5 within 256 ulp of an integer
    ties = ties[(ties > -110) & (ties < 90)]
    return {"x": cat(sweep(0, bits(F32(90.0))[0], 1 << 19), sweep(0x80000000, bits(F32(-110.0))[0], 1 << 19),
                     np.linspace(-110.0, 90.0, 1 << 19).astype(F32), near([EXP_HI, EXP_LO]), ties,
                     np.linspace(-103.98, -87.3, 1 << 17).astype(F32), SPECIALS)}


POW_Y = (F32(2.2), F32(1.0) / F32(2.2))    # Material.inl:30-32 and tonemap.cu:19-21


def _pow():
    base = cat(sweep_all(1 << 20), near([1.0, 0.0]), SPECIALS)
    xs, ys = [], []
    for y in POW_Y:
        xs.append(base)
        ys.append(np.full(base.size, y, dtype=F32))
    # the special-case lines only: other exponents against the specials and a thin sweep
    few = cat(SPECIALS, sweep_all(4096))
    sx, sy = cross(few, cat(f32([0, 0x80000000, QNAN, QNAN_NEG, INF_BITS, 0xFF800000]), [F32(-2.2)]))
    return {"x": cat(*xs, sx), "y": cat(*ys, sy)}


def _f2i():
    return {"x": cat(sweep_all(1 << 18), near([2.0**31, -2.0**31, 2.0**24, -2.0**24, 0.0, 1.0, -1.0, 255.0, 256.0]),
                     SPECIALS, np.arange(-300, 300, dtype=F32) * F32(0.75))}


TONEMAP_FRAMES = (0, 1, 2, 3, 7, 128, 1024, 2**24 + 1, 2**32 - 1)


def _tonemap():
    # r, g, b: accumulation words of every class, and non-negative ones (which tonemap to a colour); per
    # `frames` also the neighbourhood of -frames, where c + 1 crosses zero after the division
    common = cat(sweep_all(1 << 15), near([-1.0, 0.0]), SPECIALS)
    colour = cat(sweep(0, INF_BITS, 1 << 15), np.linspace(0.0, 4.0, 2048).astype(F32))
    out = {"r": [], "g": [], "b": [], "frames": []}
    for f in TONEMAP_FRAMES:
        with np.errstate(over="ignore"):
            scaled = colour * F32(max(f, 1))
        for a in (cat(common, near([-F32(f)])), scaled):
            n = a.size
            out["r"].append(a)
            out["g"].append(np.roll(a, n // 3))
            out["b"].append(np.roll(a, 2 * n // 3 + 1))
            out["frames"].append(np.full(n, f, dtype=U32))
    return {"r": cat(*out["r"]), "g": cat(*out["g"]), "b": cat(*out["b"]), "frames": np.concatenate(out["frames"])}


TEX_SIZES = ((1, 1), (1, 5), (5, 1), (2, 2), (7, 5), (512, 256))      # (width, height)
TEX_EDGE_OFFSETS_LARGE = (-256, -64, -16, -4, -2, -1, 0, 1, 2, 4, 16, 64, 256)


@functools.lru_cache(maxsize=None)
def textures():
    """(H, W, 4) float32 textures: seeded texels in [0, 60]; the 2x2 one has an inf texel, the 7x5 one a
    NaN texel, the 1x5 one a negative texel."""
    rng = np.random.default_rng(20262)
    out = []
    for w, h in TEX_SIZES:
        out.append((rng.random(size=(h, w, 4)) * 60.0).astype(F32))
    out[3][1, 0, 1] = np.inf
    out[4][2, 3, 0] = np.nan
    out[1][3, 0, 2] = -7.5
    for t in out:
        t.setflags(write=False)
    return tuple(out)


def _tex2d():
    big = cat([2.0**22, 2.0**22 + 0.25, 2.0**23, 2.0**23 - 0.5, 2.0**24, 1.0e9, 1.0e10], f32([FLT_MAX_BITS]))
    wild = cat(big, -big, f32([INF_BITS, 0xFF800000, QNAN, QNAN_NEG]))
    tex, us, vs = [], [], []

    def add(t, u, v):
        u, v = np.asarray(u, dtype=F32).ravel(), np.asarray(v, dtype=F32).ravel()
        assert u.size == v.size
        tex.append(np.full(u.size, t, dtype=U32))
        us.append(u)
        vs.append(v)

    for t, (w, h) in enumerate(TEX_SIZES):
        g = 160 if w > 16 else 48
        line = np.linspace(-3.0, 3.0, g).astype(F32)
        add(t, *cross(line, line))
        # every texel edge +-256 ulp, on both sides of [0, 1]: the edges of the texels (i / w) and of
        # the interpolation cells (i + 0.5) / w, where the tap index steps
        if w > 16:
            off = np.array(TEX_EDGE_OFFSETS_LARGE, dtype=I64)      # thinned to stay within 2^18 inputs
        else:
            off = np.arange(-ULPS, ULPS + 1, dtype=I64)
        for size, is_u in ((w, True), (h, False)):
            lo, hi = (-size, 2 * size) if size <= 16 else (-2, size + 2)
            k = np.arange(2 * lo, 2 * hi + 1, dtype=np.float64) / 2.0
            edges = (k / size).astype(F32)
            o = bits(edges).astype(I64)
            o = np.where(o < 2**31, o, 2**31 - o)[:, None] + off[None, :]
            e = f32(np.where(o >= 0, o, 2**31 - o).astype(U32)).ravel()
            other = np.resize(np.linspace(-0.3, 1.3, 37).astype(F32), e.size)
            add(t, e, other) if is_u else add(t, other, e)
        add(t, *cross(wild, wild))
        some = np.linspace(-1.25, 2.25, 29).astype(F32)
        add(t, *cross(wild, some))
        add(t, *cross(some, wild))
        add(t, *cross(SPECIALS, SPECIALS))
    return {"tex": np.concatenate(tex), "u": cat(*us), "v": cat(*vs)}


XORWOW_IDX = (0, 1, 2**31, 2**32 - 1985, 2**32 - 1)
XORWOW_HIGH = (0x0000000100000000, 0xDEADBEEF000007C0, 0xFFFFFFFFFFFFFFFF, 0x8000000000000000 | 1984)
XORWOW_SKIPS = (0, 1, 2, 1000, 65537)
XORWOW_STREAM = 1 << 18


def _xorwow_init():
    # initRandState passes (uint32)(1984 + idx); the 64-bit interface takes any seed
    low = [(1984 + i) & 0xFFFFFFFF for i in XORWOW_IDX]
    return {"seed": np.array(low + list(XORWOW_HIGH), dtype=np.uint64)}


def _xorwow_skip():
    seeds = _xorwow_init()["seed"]
    return {"seed": np.repeat(seeds, len(XORWOW_SKIPS)),
            "draws": np.tile(np.array(XORWOW_SKIPS, dtype=U32), seeds.size)}


def _xorwow_stream():
    return {"seed": np.array([1984, 1984 + 1919 + 1079 * 1920, XORWOW_HIGH[1], XORWOW_HIGH[2]], dtype=np.uint64)}


BUILDERS = {"sincos_pos": _sincos_pos, "acos": _acos, "atan2": _atan2, "log": _log, "exp": _exp, "pow": _pow,
            "f2i": _f2i, "tonemap": _tonemap, "tex2d": _tex2d, "xorwow_init": _xorwow_init,
            "xorwow_skip": _xorwow_skip, "xorwow_stream": _xorwow_stream}
MAX_INPUTS = {op: (1 << 18 if op == "tex2d" else 1 << 22) for op in BUILDERS}


def build(op):
    """The operation's inputs, built afresh: name -> array (read-only)."""
    out = BUILDERS[op]()
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def inputs(op):
    return build(op)


def count(op):
    return next(iter(inputs(op).values())).size


# ------------------------------------------------------------------------------------------------
# tex2d's tap indices, both forms
# ------------------------------------------------------------------------------------------------
def tex2d_taps(w, h, u, v):
    """(i0, i1, j0, j1) before wrap and clamp, then after them in the kernel's form (one conditional
    add) and in the oracle's form (modulo), for float32 u, v and int arrays w, h; and fy."""
    w, h = np.asarray(w, dtype=I64), np.asarray(h, dtype=I64)
    W, H = w.astype(F32), h.astype(F32)
    with np.errstate(all="ignore"):
        uw = u - np.floor(u)
        x = uw * W - F32(0.5)
        y = v * H - F32(0.5)
        fx, fy = np.floor(x), np.floor(y)
        okx = (fx > F32(-1.0e9)) & (fx < F32(1.0e9))
        oky = (fy > F32(-1.0e9)) & (fy < F32(1.0e9))
        i0 = np.where(okx, np.where(okx, fx, 0).astype(I64), 0)
        j0 = np.where(oky, np.where(oky, fy, 0).astype(I64), np.where(fy > 0, h, -1))
    i1, j1 = i0 + 1, j0 + 1
    raw = (i0, i1, j0, j1)
    cj0, cj1 = np.clip(j0, 0, h - 1), np.clip(j1, 0, h - 1)
    kernel = (np.where(i0 < 0, i0 + w, i0), np.where(i1 >= w, i1 - w, i1), cj0, cj1)
    # C's % truncates towards zero
    cmod = lambda a: np.fmod(np.fmod(a, w) + w, w)
    oracle = (cmod(i0), cmod(i1), cj0, cj1)
    return raw, kernel, oracle, fy


def check_tex2d_taps():
    """Every tap of every tex2d input lies inside its texture, in the kernel's form and the oracle's,
    and the two forms pick the same texels.  The GPU test calls this before it starts the device tool."""
    inp = inputs("tex2d")
    assert int(inp["tex"].max()) < len(TEX_SIZES)
    wh = np.array(TEX_SIZES, dtype=np.int64)[inp["tex"]]
    w, h = wh[:, 0], wh[:, 1]
    _, kernel, oracle, _ = tex2d_taps(w, h, inp["u"], inp["v"])
    for form, taps in (("kernel", kernel), ("oracle", oracle)):
        for name, t, size in zip(("i0", "i1", "j0", "j1"), taps, (w, w, h, h)):
            bad = np.flatnonzero((t < 0) | (t >= size))
            assert bad.size == 0, (f"tex2d {form} form: {name} outside the texture at {bad.size} inputs, first "
                                   f"u = {inp['u'][bad[0]]!r}, v = {inp['v'][bad[0]]!r}, texture {inp['tex'][bad[0]]}")
    for name, a, b in zip(("i0", "i1", "j0", "j1"), kernel, oracle):
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, (f"tex2d: the conditional add and the modulo disagree on {name} at {bad.size} inputs, first "
                               f"u = {inp['u'][bad[0]]!r}, v = {inp['v'][bad[0]]!r}, texture {inp['tex'][bad[0]]}")


# ------------------------------------------------------------------------------------------------
# regions: name -> (mask over the inputs, least count)
# ------------------------------------------------------------------------------------------------
def _atan_pos_ranges(q):
    big = q > F32(2.414213562373095)
    mid = ~big & (q > F32(0.4142135623730950))
    return big, mid, ~big & ~mid & ~np.isnan(q)


def regions(op, inp):
    R = {}
    with np.errstate(all="ignore"):
        if op == "sincos_pos":
            j = (inp["x"] * K_FOPI).astype(np.int32)
            for k in range(8):
                R[f"octant {k}"] = (j & 7) == k
        elif op == "acos":
            x = inp["x"]
            inside = (x >= -1) & (x <= 1)
            lo, hi = inside & (x < F32(-0.5)), inside & (x > F32(0.5))
            a = np.where(lo | hi, np.sqrt(F32(0.5) * (F32(1.0) - np.abs(x))), np.abs(x))      # asin_core's argument
            R["NaN"] = np.isnan(x)
            R["|x| > 1"] = ~inside & ~np.isnan(x)
            R["x < -0.5"], R["x > 0.5"] = lo, hi
            R["-0.5 <= x < 0"] = inside & ~lo & (x < 0)
            R["0 <= x <= 0.5"] = inside & ~hi & ~(x < 0)
            R["asin_core a < 1e-4"] = inside & (a < F32(1.0e-4))
            R["asin_core polynomial"] = inside & ~(a < F32(1.0e-4))
            # asin_core's a > 0.5 range is not reached from acos_: sqrt(0.5 (1 - |x|)) <= 0.5 for |x| > 0.5
        elif op == "atan2":
            y, x = inp["y"], inp["x"]
            nan = np.isnan(x) | np.isnan(y)
            y0 = ~nan & (y == 0)
            x0 = ~nan & ~y0 & (x == 0)
            ax, ay = np.abs(x), np.abs(y)
            xinf = ~nan & ~y0 & ~x0 & np.isinf(ax)
            gen = ~nan & ~y0 & ~x0 & ~xinf
            q = ay / ax
            big, mid, small = _atan_pos_ranges(q)
            R["NaN argument"] = (nan, MIN_REGION)
            R["y == 0, x sign set"] = (y0 & np.signbit(x), MIN_LINE)
            R["y == 0, x sign clear"] = (y0 & ~np.signbit(x), MIN_LINE)
            R["x == 0"] = (x0, MIN_LINE)
            R["x infinite, y infinite"] = (xinf & np.isinf(ay), MIN_LINE)
            R["x infinite, y finite"] = (xinf & ~np.isinf(ay), MIN_LINE)
            R["atan_pos q > 2.414"], R["atan_pos 0.414 < q <= 2.414"], R["atan_pos q <= 0.414"] = gen & big, gen & mid, gen & small
            R["quotient denormal"] = gen & (q > 0) & (q < F32(2.0**-126))
            R["quotient zero (underflow)"] = gen & (q == 0)
            R["quotient infinite (overflow)"] = gen & np.isinf(q)
            R["x < 0"], R["y < 0"] = gen & (x < 0), gen & (y < 0)
        elif op == "log":
            b = bits(inp["x"])
            den = (b >> 23) == 0
            xs = np.where(den, inp["x"] * F32(8388608.0), inp["x"])
            m = f32((bits(xs) & U32(0x807FFFFF)) | U32(0x3F000000))
            low = m < F32(0.707106781186547524)
            R["denormal"], R["mantissa < sqrt(1/2)"], R["mantissa >= sqrt(1/2)"] = den, low, ~low
            R["denormal, mantissa < sqrt(1/2)"], R["denormal, mantissa >= sqrt(1/2)"] = den & low, den & ~low
        elif op == "exp":
            x = inp["x"]
            hi, lo = x > EXP_HI, x < EXP_LO
            body = ~hi & ~lo & ~np.isnan(x)
            z = np.floor(LOG2E * x + F32(0.5))
            n = np.where(body, z, 0).astype(I64)
            R["x > 88.72"], R["x < -103.97"] = hi, lo
            R["n odd"], R["n even"], R["n negative"] = body & (n % 2 == 1), body & (n % 2 == 0), body & (n < 0)
            e = np.exp(x.astype(np.float64))
            R["denormal result"] = body & (e > 0) & (e < 2.0**-126)
        elif op == "pow":
            x, y = inp["x"], inp["y"]
            nan = np.isnan(x) | np.isnan(y)
            one = ~nan & ((y == 0) | (x == 1))
            zero = ~nan & ~one & (x == 0)
            neg = ~nan & ~one & ~zero & (x < 0)
            inf = ~nan & ~one & ~zero & ~neg & np.isinf(x)
            gen = ~nan & ~one & ~zero & ~neg & ~inf
            R["NaN argument"] = (nan, MIN_REGION)
            R["y == 0 or x == 1"] = (one, MIN_LINE)
            R["x == 0"] = (zero, MIN_LINE)
            R["x < 0"] = (neg, MIN_REGION)
            R["x infinite"] = (inf, MIN_LINE)
            p = np.power(np.where(gen, x, 1).astype(np.float64), y.astype(np.float64))
            for yy, name in zip(POW_Y, ("2.2", "1/2.2")):
                R[f"general, y = {name}"] = gen & (y == yy)
            R["general, denormal result, y = 2.2"] = gen & (y == POW_Y[0]) & (p > 0) & (p < 2.0**-126)
            R["general, denormal base"] = gen & (x < F32(2.0**-126))
        elif op == "f2i":
            x = inp["x"]
            inside = (x > F32(-2147483904.0)) & (x < F32(2147483648.0))
            R["out of range"], R["in range"] = ~inside, inside
            R["out of range, not NaN"] = ~inside & ~np.isnan(x)
        elif op == "tonemap":
            fr = inp["frames"].astype(F32)
            nanline = np.zeros(fr.size, dtype=bool)
            for k in "rgb":
                c = (F32(1.0) / fr) * inp[k]
                c = (F32(1.0) / (c + F32(1.0))) * c
                nanline |= np.isnan(c) | (c < 0)             # pow_ of a NaN or of a negative base is NaN
            R["NaN channel"] = nanline
            R["no NaN channel"] = ~nanline
            for f in TONEMAP_FRAMES:
                R[f"frames = {f}"] = inp["frames"] == f
        elif op == "tex2d":
            wh = np.array(TEX_SIZES, dtype=I64)[inp["tex"]]
            w, h = wh[:, 0], wh[:, 1]
            raw, _, _, fy = tex2d_taps(w, h, inp["u"], inp["v"])
            i0, i1, j0, j1 = raw
            R["column wrap, left"], R["column wrap, right"] = i0 < 0, i1 >= w
            R["row clamp, low"], R["row clamp, high"] = j0 < 0, j1 > h - 1
            R["fy >= 1e9"] = ~(fy < F32(1.0e9)) & (fy > 0)
            R["fy <= -1e9"] = ~(fy > F32(-1.0e9)) & ~(fy > 0) & ~np.isnan(fy)
            R["NaN u"], R["NaN v"] = np.isnan(inp["u"]), np.isnan(inp["v"])
            R["width 1"], R["height 1"] = w == 1, h == 1
        else:
            raise KeyError(op)
    return {k: (v if isinstance(v, tuple) else (v, MIN_REGION)) for k, v in R.items()}


REGION_OPS = ("sincos_pos", "acos", "atan2", "log", "exp", "pow", "f2i", "tonemap", "tex2d")


def regions_at(op, inp, index):
    """For a failure message: the names of the regions input `index` falls in."""
    sub = {k: np.ascontiguousarray(v[index:index + 1]) for k, v in inp.items()}
    return [name for name, (mask, _) in regions(op, sub).items() if mask[0]]


# ------------------------------------------------------------------------------------------------
# the oracle over the sets, and the files tools/dev_functions.hip reads and writes
# ------------------------------------------------------------------------------------------------
# device operation -> (input set, input file, planes of the input file, output file)
DEVICE_OPS = {
    "sincos_pos": ("sincos_pos", "sincos_pos.in", ("x",), "sincos_pos.out"),
    "acos_": ("acos", "acos.in", ("x",), "acos_.out"),
    "acos_sel": ("acos", "acos.in", ("x",), "acos_sel.out"),
    "atan2_": ("atan2", "atan2.in", ("y", "x"), "atan2_.out"),
    "atan2_sel": ("atan2", "atan2.in", ("y", "x"), "atan2_sel.out"),
    "log_": ("log", "log.in", ("x",), "log_.out"),
    "exp_": ("exp", "exp.in", ("x",), "exp_.out"),
    "pow_": ("pow", "pow.in", ("x", "y"), "pow_.out"),
    "f2i_x86": ("f2i", "f2i.in", ("x",), "f2i_x86.out"),
    "tonemap_pixel": ("tonemap", "tonemap.in", ("r", "g", "b", "frames"), "tonemap_pixel.out"),
    "tex2d": ("tex2d", "tex2d.in", ("tex", "u", "v"), "tex2d.out"),
    "xorwow_init": ("xorwow_init", "xorwow_init.in", None, "xorwow_init.out"),
    "xorwow_skip": ("xorwow_skip", "xorwow_skip.in", None, "xorwow_skip.out"),
    "xorwow_stream": ("xorwow_stream", "xorwow_stream.in", None, "xorwow_stream.out"),
}


def _seed_words(seeds):
    return (seeds & np.uint64(0xFFFFFFFF)).astype(U32), (seeds >> np.uint64(32)).astype(U32)


def write_inputs(directory):
    """The files of tools/dev_functions.hip's header comment."""
    d = pathlib.Path(directory)
    done = set()
    for _, (name, fname, planes, _) in DEVICE_OPS.items():
        if fname in done:
            continue
        done.add(fname)
        inp = inputs(name)
        if planes is not None:
            words = np.concatenate([np.ascontiguousarray(inp[p]).view(U32) for p in planes])
        elif name == "xorwow_stream":
            lo, hi = _seed_words(inp["seed"])
            words = np.concatenate([np.array([XORWOW_STREAM], dtype=U32), np.stack([lo, hi], axis=1).ravel()])
        else:
            lo, hi = _seed_words(inp["seed"])
            words = np.concatenate([lo, hi] + ([inp["draws"]] if name == "xorwow_skip" else []))
        words.astype("<u4").tofile(d / fname)
    texs = textures()
    head = [len(texs)] + [s for t in texs for s in (t.shape[1], t.shape[0])]
    np.concatenate([np.array(head, dtype=U32)] + [t.ravel().view(U32) for t in texs]).astype("<u4").tofile(d / "tex2d.tab")


def read_output(directory, dev_op):
    return np.fromfile(pathlib.Path(directory) / DEVICE_OPS[dev_op][3], dtype="<u4").astype(U32)


@functools.lru_cache(maxsize=None)
def oracle_words(dev_op, fast=False):
    """The oracle's result words in the layout of the device operation's output file (fast: from the -O3
    build of the oracle)."""
    name = DEVICE_OPS[dev_op][0]
    inp = inputs(name)
    if dev_op == "sincos_pos":
        return np.concatenate([bits(a) for a in po.dev_sincos(inp["x"], fast=fast)])
    if name in ("acos", "log", "exp"):
        return bits(po.dev_unary(name, inp["x"], fast=fast))
    if name == "atan2":
        return bits(po.dev_binary("atan2", inp["y"], inp["x"], fast=fast))
    if name == "pow":
        return bits(po.dev_binary("pow", inp["x"], inp["y"], fast=fast))
    if name == "f2i":
        return po.dev_f2i(inp["x"], fast=fast).view(U32)
    if name == "tonemap":
        out = np.empty((inp["r"].size, 4), dtype=np.uint8)
        rgb = np.stack([inp["r"], inp["g"], inp["b"]], axis=1)
        for f in TONEMAP_FRAMES:
            m = inp["frames"] == f
            out[m] = po.dev_tonemap(rgb[m], f, fast=fast)
        return np.ascontiguousarray(out).view("<u4").ravel().astype(U32)
    if name == "tex2d":
        return bits(po.dev_tex2d(textures(), inp["tex"], inp["u"], inp["v"], fast=fast)).ravel()
    if name == "xorwow_init":
        return po.dev_xorwow_init(inp["seed"], fast=fast).ravel()
    if name == "xorwow_skip":
        return po.dev_xorwow_skip(inp["seed"], inp["draws"], fast=fast).ravel()
    if name == "xorwow_stream":
        parts = []
        for s in inp["seed"]:
            nxt, uni = po.dev_xorwow_stream(int(s), XORWOW_STREAM, fast=fast)
            parts += [nxt, bits(uni)]
        return np.concatenate(parts)
    raise KeyError(dev_op)
