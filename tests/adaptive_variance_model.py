"""Rule 5 of include/pt_hip.h, "the variance of an adaptive render's image", restated in numpy float32 twice,
and seeded inputs for it.

model()    whole-image arithmetic (one shifted copy per tap), with svgf_model's helpers where they fit
scalar()   the same pixel by pixel with np.float32 scalars, written from the header independently

tests/test_adaptive_variance_rule.py holds the two against each other word for word;
tests/test_gpu_adaptive_variance.py holds the device against model().

Images are height x width x 4 float32 as in denoise_model; `moments` is height x width x 3 float32 as
Pathtracer.moments() returns it (m1, m2, n as uint32 bits); a variance is height x width float32.
"""
import numpy as np

import denoise_model as dm
import svgf_model as sm
import temporal_model as tm
from denoise_model import F, U, HIT, EMISSIVE, bits, same_words   # noqa: F401

DEMODULATE, SAME_PRIMITIVE = 1, 2
RADIUS = 3
# the parameters of the branch test: every one of the five tap tests rejects something under them
PARAMS = dict(min_batches=8, sigma_plane=0.05, normal_cos_min=0.9)
WIDTH, HEIGHT = 48, 40


def split_moments(moments):
    m = np.ascontiguousarray(moments, dtype=F)
    return m[..., 0], m[..., 1], bits(m[..., 2])


def se2_of(m1, m2, n):
    """The batch-means variance of the mean: adapt_flag_kernel's operations up to se2."""
    with np.errstate(all="ignore"):
        k = n.astype(F)
        mean = m1 / k
        ss = m2 - m1 * mean
        ss = np.where(ss < 0, F(0), ss)
        return (ss / (k * (k - F(1)))).astype(F)


# ---- whole image ----------------------------------------------------------------------------------------
def model(color, plane0, plane1, plane2, moments, min_batches, sigma_plane, normal_cos_min, flags, counts=None):
    color, plane0, plane1, plane2 = (np.ascontiguousarray(a, dtype=F) for a in (color, plane0, plane1, plane2))
    m1, m2, n = split_moments(moments)
    Hh, Ww = color.shape[:2]
    ids = bits(plane0[..., 3])
    Nn, t, P = plane1[..., :3], plane1[..., 3], plane2[..., :3]
    fl = bits(plane2[..., 3])
    D = dm.divisor(plane0, flags)
    with np.errstate(all="ignore"):
        I = (color[..., :3] / D).astype(F)
        l = sm.lum(I)
        g = sm.lum(D) if flags & DEMODULATE else np.ones((Hh, Ww), dtype=F)
        ok = ((fl & HIT) != 0) & ((fl & EMISSIVE) == 0) & sm._finite(l) & tm._finite3(plane1) & tm._finite3(plane2)
        has = ok & (n >= 2) & sm._finite(m1) & sm._finite(m2)
        own = sm._clamp0(se2_of(m1, m2, n) / (g * g))
        young = has & (n < U(min_batches))
        yy, xx = np.mgrid[0:Hh, 0:Ww]
        c = dict(old=int((has & ~young).sum()), young=int(young.sum()), outside=0, not_ok=0, by_normal=0, by_plane=0, by_id=0)
        m = F(sigma_plane) * t
        mm = m * m
        k, s1, s2 = (np.zeros((Hh, Ww), dtype=F) for _ in range(3))
        met = {name: np.zeros((Hh, Ww), dtype=bool) for name in ("outside", "not_ok", "by_normal", "by_plane", "by_id")}
        for dy in range(-RADIUS, RADIUS + 1):
            for dx in range(-RADIUS, RADIUS + 1):
                inside = (xx + dx >= 0) & (xx + dx < Ww) & (yy + dy >= 0) & (yy + dy < Hh)
                lq, okq = sm._clip_shift(l, dx, dy), sm._clip_shift(ok, dx, dy)
                Nq, idq, Pq = sm._clip_shift(Nn, dx, dy), sm._clip_shift(ids, dx, dy), sm._clip_shift(P, dx, dy)
                gq = tm._dot(Nn, (Pq - P).astype(F))
                reasons = [("outside", ~inside), ("not_ok", ~okq), ("by_normal", tm._dot(Nn, Nq) < F(normal_cos_min)),
                           ("by_plane", ~(gq * gq <= mm)),
                           ("by_id", (idq != ids) if flags & SAME_PRIMITIVE else np.zeros((Hh, Ww), dtype=bool))]
                skip = np.zeros((Hh, Ww), dtype=bool)
                if dx or dy:
                    for name, r in reasons:
                        met[name] |= young & ~skip & r                # the taps this test is the first to reject
                        skip |= r
                k = np.where(skip, k, k + F(1))
                s1 = np.where(skip, s1, s1 + lq)
                s2 = np.where(skip, s2, s2 + lq * lq)
        mean = s1 / k
        vs = sm._clamp0(s2 / k - mean * mean)
        var = np.where(~has, F(-1), np.where(young, np.where(vs > own, vs, own), own)).astype(F)
    c.update({name: int(mask.sum()) for name, mask in met.items()})       # young pixels with such a tap
    c.update(vs_wins=int((young & (vs > own)).sum()), own_wins=int((young & ~(vs > own)).sum()),
             centre_alone=int((young & (k == 1)).sum()), dark=int((young & (own == 0) & (vs > 0)).sum()))
    if counts is not None:
        counts.update(c)
    return var


# ---- pixel by pixel -------------------------------------------------------------------------------------
def scalar(color, plane0, plane1, plane2, moments, min_batches, sigma_plane, normal_cos_min, flags):
    color, plane0, plane1, plane2 = (np.ascontiguousarray(a, dtype=F) for a in (color, plane0, plane1, plane2))
    mom = np.ascontiguousarray(moments, dtype=F)
    H, W = color.shape[:2]
    one, lo, zero = F(1), F(1.0 / 64.0), F(0)

    def finite(x):
        return bool((x - x) == 0)

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    def lum3(c):
        return (F(0.2126) * c[0] + F(0.7152) * c[1]) + F(0.0722) * c[2]

    def clamp0(v):
        return v if (v > 0 and finite(v)) else zero

    L = np.zeros((H, W), dtype=F)
    OK = np.zeros((H, W), dtype=bool)
    G = np.ones((H, W), dtype=F)
    var = np.zeros((H, W), dtype=F)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                Dp = [one, one, one]
                if flags & DEMODULATE:
                    Dp = [plane0[y, x, j] if plane0[y, x, j] > lo else lo for j in range(3)]
                    G[y, x] = lum3(Dp)
                L[y, x] = lum3([color[y, x, j] / Dp[j] for j in range(3)])
                fl = int(bits(plane2[y, x, 3:4])[0])
                ok = bool(fl & HIT) and not fl & EMISSIVE and finite(L[y, x])
                for j in range(3):
                    ok = ok and finite(plane1[y, x, j]) and finite(plane2[y, x, j])
                OK[y, x] = ok
        for y in range(H):
            for x in range(W):
                m1, m2, n = mom[y, x, 0], mom[y, x, 1], int(bits(mom[y, x, 2:3])[0])
                if not OK[y, x] or n < 2 or not finite(m1) or not finite(m2):
                    var[y, x] = F(-1)
                    continue
                k = F(n)
                mean = m1 / k
                ss = m2 - m1 * mean
                if ss < 0:
                    ss = zero
                se2 = ss / (k * (k - one))
                own = clamp0(se2 / (G[y, x] * G[y, x]))
                if n >= min_batches:
                    var[y, x] = own
                    continue
                Np, Pp = plane1[y, x, :3], plane2[y, x, :3]
                m = F(sigma_plane) * plane1[y, x, 3]
                cnt, s1, s2 = zero, zero, zero
                for dy in range(-3, 4):
                    for dx in range(-3, 4):
                        qx, qy = x + dx, y + dy
                        if dx != 0 or dy != 0:
                            if qx < 0 or qx >= W or qy < 0 or qy >= H or not OK[qy, qx]:
                                continue
                            if dot(Np, plane1[qy, qx, :3]) < F(normal_cos_min):
                                continue
                            gq = dot(Np, [plane2[qy, qx, j] - Pp[j] for j in range(3)])
                            if not gq * gq <= m * m:
                                continue
                            if flags & SAME_PRIMITIVE and bits(plane0[qy, qx, 3:4])[0] != bits(plane0[y, x, 3:4])[0]:
                                continue
                        lq = L[qy, qx]
                        cnt, s1, s2 = cnt + one, s1 + lq, s2 + lq * lq
                mean = s1 / cnt
                vs = clamp0(s2 / cnt - mean * mean)
                var[y, x] = vs if vs > own else own
    return var


# ---- inputs ---------------------------------------------------------------------------------------------
CLASSES = ("ordinary", "emissive", "n0", "n1", "nan_m1", "inf_m2", "inf_l", "ss_negative", "dark", "albedo0", "m2_3e38",
           "n_max", "alone")
SHARE = 0.042           # of every class but the first


def make_inputs(width, height, seed):
    """denoise_model.make_inputs' planes (stripes of ids, antiparallel normals, a sloped plane, misses) with an
    adaptive render made over them: per pixel n calls, each call's colour sum drawn around a smooth signal, the
    accumulation their float32 sum in call order and m1, m2 the sums of their luminance and its square, so the
    colour accum / n and the moments describe the same calls.  About half of the ordinary pixels have fewer than
    8 calls.  Then one class of CLASSES per pixel (seeded; a miss stays a miss).  Returns
    (color, plane0, plane1, plane2, moments, classes) with color = accum / max(n, 1)."""
    _, p0, p1, p2 = dm.make_inputs(width, height, seed)
    p0, p1, p2 = p0.copy(), p1.copy(), p2.copy()
    rng = np.random.default_rng([seed, 555])
    H, W = height, width
    y, x = np.mgrid[0:H, 0:W]
    # make_inputs' own emissive region, zero albedos and NaN normals are replaced by the classes below
    fl = bits(p2[..., 3]).copy()
    miss = (fl & HIT) == 0
    fl[~miss] = HIT
    p1[..., 0] = np.where(np.isnan(p1[..., 0]), F(0.3), p1[..., 0])
    alb = (F(0.2) + F(0.8) * rng.random((H, W, 3), dtype=F)).astype(F)
    alb[miss] = F(0)
    pick = rng.random((H, W))
    cls = np.zeros((H, W), dtype=np.int64)
    for idx in range(1, len(CLASSES)):
        cls[(pick >= SHARE * (idx - 1)) & (pick < SHARE * idx)] = idx
    for idx in range(1, len(CLASSES)):                     # every class at a fixed place too, whatever the size
        if idx < W * H:
            cls.flat[(idx * 7) % (W * H)] = idx
    cls[miss] = 0
    is_ = {name: cls == k for k, name in enumerate(CLASSES)}
    n = np.where(rng.random((H, W)) < 0.5, rng.integers(2, 8, (H, W)), rng.integers(8, 17, (H, W))).astype(U)
    n[is_["n0"]], n[is_["n1"]] = 0, 1
    n[is_["dark"]] = rng.integers(2, 5, (H, W)).astype(U)[is_["dark"]]
    n[is_["alone"]] = rng.integers(2, 8, (H, W)).astype(U)[is_["alone"]]
    alb[is_["albedo0"]] = F(0)
    signal = F(0.5) + F(0.25) * np.sin(x / F(6)).astype(F) + F(0.25) * np.cos(y / F(5)).astype(F)
    accum = np.zeros((H, W, 3), dtype=F)
    m1, m2 = np.zeros((H, W), dtype=F), np.zeros((H, W), dtype=F)
    shown = np.where(alb > 0, alb, F(0.05))               # a black albedo still reflects something here: D is 1/64 there
    for call in range(16):
        S = (shown * (signal[..., None] * (F(1) + rng.normal(0, 0.3, (H, W, 3)).astype(F)))).astype(F)
        S[is_["dark"]] = F(0)                              # every call of a dark pixel returned the same value
        yl = sm.lum(S)
        act = call < n
        accum = np.where(act[..., None], accum + S, accum).astype(F)
        m1 = np.where(act, m1 + yl, m1).astype(F)
        m2 = np.where(act, m2 + yl * yl, m2).astype(F)
    fl[is_["emissive"]] = HIT | EMISSIVE
    m1[is_["nan_m1"]] = F(np.nan)
    m2[is_["inf_m2"]] = F(np.inf)
    accum[is_["inf_l"], 1] = F(np.inf)
    with np.errstate(all="ignore"):
        under = (m1 * (m1 / np.maximum(n, 1).astype(F)) * F(0.99)).astype(F)
    m2[is_["ss_negative"]] = under[is_["ss_negative"]]
    m2[is_["m2_3e38"]] = F(3e38)
    n[is_["n_max"]] = U(0xffffffff)
    ids = bits(p0[..., 3]).copy()
    ids[is_["alone"]] = (U(100000) + (y * W + x).astype(U))[is_["alone"]]
    p0[..., :3] = alb
    p0[..., 3] = ids.view(F)
    p2[..., 3] = fl.view(F)
    with np.errstate(all="ignore"):
        color = np.ones((H, W, 4), dtype=F)
        color[..., :3] = accum / np.maximum(n, 1).astype(F)[..., None]
    moments = np.stack([m1, m2, n.view(F)], -1)
    return tuple(np.ascontiguousarray(a, dtype=F) for a in (color, p0, p1, p2, moments)) + (cls,)
