"""The three rules of "per-pixel variance from the temporal history, and the variance-guided filter"
(include/pt_hip.h) restated in numpy float32, each twice, and seeded inputs for them.

model()          the temporal step with moments and the variance estimate, whole-image arithmetic
scalar()         the same pixel by pixel with np.float32 scalars, written from the header independently
filter_model()   the variance-guided a-trous filter, whole-image arithmetic (one shifted copy per tap)
filter_scalar()  the same pixel by pixel

tests/test_svgf_rule.py holds each pair against each other word for word and the colour of model() against
temporal_model.model(); tests/test_gpu_svgf.py holds the device against model() and filter_model().

Images are height x width x 4 float32 as in temporal_model / denoise_model; the moments plane h3 is
(m1, m2, v, 0); a variance is height x width float32.
"""
import numpy as np

import denoise_model as dm
import temporal_model as tm
from denoise_model import F, U, HIT, EMISSIVE, bits, same_words   # noqa: F401

DEMODULATE, SAME_PRIMITIVE = 1, 2
RADIUS = 3
BIG = F(2.0 ** 60)
K3 = (F(0.5), F(0.25))
VPARAMS = dict(sigma_l=1.5, variance_floor=1e-6, sigma_plane=0.05, normal_power_log2=2)


def lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def _finite(x):
    return (x - x) == 0


def _clamp0(v):
    return np.where((v > 0) & _finite(v), v, F(0)).astype(F)


# ---- 1 + 2: the step with moments and the estimate, whole image ----------------------------------------
def model(color, plane0, plane1, plane2, cur, hist, prev, alpha_min, max_history, sigma_plane, normal_cos_min, flags,
          min_temporal=4, stats=None):
    """One step.  hist = (h0, h1, h2, h3) or None.  Returns (image, h0, h1, h2, h3, variance)."""
    color, plane0, plane1, plane2 = (np.ascontiguousarray(a, dtype=F) for a in (color, plane0, plane1, plane2))
    Hh, Ww = color.shape[:2]
    C, A, ids = color[..., :3], plane0[..., :3], bits(plane0[..., 3])
    Nn, t, P = plane1[..., :3], plane1[..., 3], plane2[..., :3]
    ok = tm.ok_mask(color, plane1, plane2)
    lo = F(1.0 / 64.0)
    D = np.where(A > lo, A, lo).astype(F) if flags & DEMODULATE else np.ones_like(A)
    mh = F(max_history)
    counts = dict(restarted=0, have=0)
    with np.errstate(all="ignore"):
        Icur = (C / D).astype(F)
        l = lum(Icur)
        q = l * l
        I, n, m1, m2 = Icur, np.ones((Hh, Ww), dtype=F), l, q
        if hist is not None:
            h0, h1, h2, h3 = (np.ascontiguousarray(a, dtype=F) for a in hist)
            yy, xx = np.mgrid[0:Hh, 0:Ww]
            W, H = F(Ww), F(Hh)
            su0, sv0, z0 = tm._project(cur, P)
            su1, sv1, z1 = tm._project(prev, P)
            fx = xx.astype(F) + (su1 - su0) * W
            fy = yy.astype(F) + (sv1 - sv0) * H
            reproj = (z0 > 0) & (z1 > 0) & (fx > F(-1)) & (fx < W) & (fy > F(-1)) & (fy < H)
            live = reproj & ok
            fxs, fys = np.where(live, fx, F(0)), np.where(live, fy, F(0))
            flx, fly = np.floor(fxs), np.floor(fys)
            ax, ay = fxs - flx, fys - fly
            x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
            m = F(sigma_plane) * t
            mm = m * m
            sumW = np.zeros((Hh, Ww), dtype=F)
            sumI = np.zeros((Hh, Ww, 3), dtype=F)
            sumM1, sumM2 = np.zeros((Hh, Ww), dtype=F), np.zeros((Hh, Ww), dtype=F)
            nh = np.full((Hh, Ww), mh, dtype=F)
            for i, j in ((0, 0), (1, 0), (0, 1), (1, 1)):
                w = (ax if i else F(1) - ax) * (ay if j else F(1) - ay)
                qx, qy = x0 + i, y0 + j
                inside = (qx >= 0) & (qx < Ww) & (qy >= 0) & (qy < Hh)
                cx, cy = np.clip(qx, 0, Ww - 1), np.clip(qy, 0, Hh - 1)
                Iq, nq = h0[cy, cx, :3], h0[cy, cx, 3]
                Nq, idq, Pq = h1[cy, cx, :3], bits(h1[..., 3])[cy, cx], h2[cy, cx, :3]
                g = tm._dot(Nn, (Pq - P).astype(F))
                skip = ~(w > 0) | ~inside | (nq < F(1)) | ~tm._finite3(Iq) | (tm._dot(Nn, Nq) < F(normal_cos_min)) | ~(g * g <= mm)
                if flags & SAME_PRIMITIVE:
                    skip = skip | (idq != ids)
                sumW = np.where(skip, sumW, sumW + w)
                sumI = np.where(skip[..., None], sumI, sumI + w[..., None] * Iq)
                sumM1 = np.where(skip, sumM1, sumM1 + w * h3[cy, cx, 0])
                sumM2 = np.where(skip, sumM2, sumM2 + w * h3[cy, cx, 1])
                nh = np.where(skip, nh, np.where(nq < nh, nq, nh))
            have = live & (sumW >= lo)
            Hc = sumI / sumW[..., None]
            Hm1, Hm2 = sumM1 / sumW, sumM2 / sumW
            nn = nh + F(1)
            nn = np.where(nn < mh, nn, mh)
            a = F(1) / nn
            a = np.where(a > F(alpha_min), a, F(alpha_min))
            I = np.where(have[..., None], Hc + a[..., None] * (Icur - Hc), Icur).astype(F)
            n = np.where(have, nn, F(1)).astype(F)
            m1 = np.where(have, Hm1 + a * (l - Hm1), l).astype(F)
            m2 = np.where(have, Hm2 + a * (q - Hm2), q).astype(F)
            counts["have"] = int(have.sum())
            counts["restarted"] = int((have & ~(_finite(m1) & _finite(m2))).sum())
        restart = ~(_finite(m1) & _finite(m2))
        m1, m2 = np.where(restart, l, m1).astype(F), np.where(restart, q, m2).astype(F)
        v = _clamp0(m2 - m1 * m1)
        image = np.zeros((Hh, Ww, 4), dtype=F)
        image[..., :3] = np.where(ok[..., None], I * D, C)
        image[..., 3] = np.where(ok, n, F(0))
        o0 = np.zeros((Hh, Ww, 4), dtype=F)
        o0[..., :3] = np.where(ok[..., None], I, C)
        o0[..., 3] = image[..., 3]
        o3 = np.zeros((Hh, Ww, 4), dtype=F)
        o3[..., 0], o3[..., 1] = np.where(ok, m1, F(0)), np.where(ok, m2, F(0))
        o3[..., 2] = np.where(ok, v, F(-1))
    o1 = np.concatenate([Nn, plane0[..., 3:4]], -1).astype(F)
    o2 = np.concatenate([P, t[..., None]], -1).astype(F)
    var = variance_model(o0, o1, o2, o3, sigma_plane, normal_cos_min, flags, min_temporal, counts)
    if stats is not None:
        stats.update(counts)
    return image, o0, o1, o2, o3, var


def _clip_shift(a, dx, dy):
    """a[clip(y + dy), clip(x + dx)]: the load behind a clamped index."""
    h, w = a.shape[:2]
    yy = np.clip(np.arange(h) + dy, 0, h - 1)
    xx = np.clip(np.arange(w) + dx, 0, w - 1)
    return a[yy][:, xx]


def variance_model(h0, h1, h2, h3, sigma_plane, normal_cos_min, flags, min_temporal, counts=None):
    Hh, Ww = h0.shape[:2]
    I, n = h0[..., :3], h0[..., 3]
    Nn, ids, P, t = h1[..., :3], bits(h1[..., 3]), h2[..., :3], h2[..., 3]
    mt = F(min_temporal)
    yy, xx = np.mgrid[0:Hh, 0:Ww]
    spatial = (n >= F(1)) & ~(n >= mt)
    c = dict(spatial=int(spatial.sum()), temporal=int((n >= mt).sum()), outside=0, no_history=0, by_normal=0, by_plane=0,
             by_id=0)
    with np.errstate(all="ignore"):
        m = F(sigma_plane) * t
        mm = m * m
        k, s1, s2 = (np.zeros((Hh, Ww), dtype=F) for _ in range(3))
        for dy in range(-RADIUS, RADIUS + 1):
            for dx in range(-RADIUS, RADIUS + 1):
                inside = (xx + dx >= 0) & (xx + dx < Ww) & (yy + dy >= 0) & (yy + dy < Hh)
                Iq, nq = _clip_shift(I, dx, dy), _clip_shift(n, dx, dy)
                Nq, idq, Pq = _clip_shift(Nn, dx, dy), _clip_shift(ids, dx, dy), _clip_shift(P, dx, dy)
                g = tm._dot(Nn, (Pq - P).astype(F))
                reasons = [("outside", ~inside), ("no_history", nq < F(1)), ("by_normal", tm._dot(Nn, Nq) < F(normal_cos_min)),
                           ("by_plane", ~(g * g <= mm)),
                           ("by_id", (idq != ids) if flags & SAME_PRIMITIVE else np.zeros((Hh, Ww), dtype=bool))]
                skip = np.zeros((Hh, Ww), dtype=bool)
                if dx or dy:
                    for name, r in reasons:
                        c[name] += int((spatial & ~skip & r).sum())
                        skip |= r
                lq = lum(Iq)
                k = np.where(skip, k, k + F(1))
                s1 = np.where(skip, s1, s1 + lq)
                s2 = np.where(skip, s2, s2 + lq * lq)
        mean = s1 / k
        vs = _clamp0(s2 / k - mean * mean)
        var = np.where(n < F(1), F(-1), np.where(n >= mt, h3[..., 2], vs * (mt / n))).astype(F)
    c["k1"] = int((spatial & (k == 1)).sum())
    if counts is not None:
        counts.update(c)
    return var


# ---- 1 + 2, pixel by pixel ------------------------------------------------------------------------------
def scalar(color, plane0, plane1, plane2, cur, hist, prev, alpha_min, max_history, sigma_plane, normal_cos_min, flags,
           min_temporal=4):
    color, plane0, plane1, plane2 = (np.ascontiguousarray(a, dtype=F) for a in (color, plane0, plane1, plane2))
    Hh, Ww = color.shape[:2]
    one, half, lo, zero = F(1), F(0.5), F(1.0 / 64.0), F(0)
    W, H, mh = F(Ww), F(Hh), F(max_history)
    image, o0, o1, o2, o3 = (np.zeros((Hh, Ww, 4), dtype=F) for _ in range(5))
    var = np.zeros((Hh, Ww), dtype=F)

    def finite(x):
        return bool((x - x) == 0)

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    def lum3(c):
        return (F(0.2126) * c[0] + F(0.7152) * c[1]) + F(0.0722) * c[2]

    def clamp0(v):
        return v if (v > 0 and finite(v)) else zero

    def project(cam, p):
        e = [p[k] - cam["origin"][k] for k in range(3)]
        z = -dot(e, cam["backward"])
        hh = F(cam["tan_half_fovy"])
        hw = F(cam["aspect_ratio"]) * hh
        return ((dot(e, cam["right"]) / z) / hw) * half + half, ((dot(e, cam["up"]) / z) / hh) * half + half, z

    with np.errstate(all="ignore"):
        for y in range(Hh):
            for x in range(Ww):
                c, Np, Pp, tp = color[y, x, :3], plane1[y, x, :3], plane2[y, x, :3], plane1[y, x, 3]
                o1[y, x, :3], o1[y, x, 3] = Np, plane0[y, x, 3]
                o2[y, x, :3], o2[y, x, 3] = Pp, tp
                ok = bool(int(bits(plane2[y, x, 3:4])[0]) & HIT)
                for v in (c, Np, Pp):
                    for k in range(3):
                        ok = ok and finite(v[k])
                if not ok:
                    image[y, x, :3] = o0[y, x, :3] = c
                    o3[y, x, 2] = F(-1)
                    continue
                D = [one, one, one]
                if flags & DEMODULATE:
                    D = [plane0[y, x, k] if plane0[y, x, k] > lo else lo for k in range(3)]
                Icur = [c[k] / D[k] for k in range(3)]
                l = lum3(Icur)
                q = l * l
                I, n, m1, m2 = Icur, one, l, q
                if hist is not None:
                    h0, h1, h2, h3 = hist
                    su0, sv0, z0 = project(cur, Pp)
                    su1, sv1, z1 = project(prev, Pp)
                    fx = F(x) + (su1 - su0) * W
                    fy = F(y) + (sv1 - sv0) * H
                    if z0 > 0 and z1 > 0 and fx > -one and fx < W and fy > -one and fy < H:
                        flx, fly = np.floor(fx), np.floor(fy)
                        ax, ay = fx - flx, fy - fly
                        x0, y0 = int(flx), int(fly)
                        m = F(sigma_plane) * tp
                        sumW, sumI, nh, sM1, sM2 = zero, [zero, zero, zero], mh, zero, zero
                        for j in (0, 1):
                            for i in (0, 1):
                                w = (ax if i else one - ax) * (ay if j else one - ay)
                                qx, qy = x0 + i, y0 + j
                                if not w > 0 or qx < 0 or qx >= Ww or qy < 0 or qy >= Hh:
                                    continue
                                Iq, nq = h0[qy, qx, :3], F(h0[qy, qx, 3])
                                if nq < one or not all(finite(F(v)) for v in Iq):
                                    continue
                                if flags & SAME_PRIMITIVE and bits(h1[qy, qx, 3:4])[0] != bits(plane0[y, x, 3:4])[0]:
                                    continue
                                if dot(Np, h1[qy, qx, :3]) < F(normal_cos_min):
                                    continue
                                g = dot(Np, [F(h2[qy, qx, k]) - Pp[k] for k in range(3)])
                                if not g * g <= m * m:
                                    continue
                                sumW = sumW + w
                                sumI = [sumI[k] + w * F(Iq[k]) for k in range(3)]
                                sM1 = sM1 + w * F(h3[qy, qx, 0])
                                sM2 = sM2 + w * F(h3[qy, qx, 1])
                                nh = nq if nq < nh else nh
                        if sumW >= lo:
                            Hc = [sumI[k] / sumW for k in range(3)]
                            Hm1, Hm2 = sM1 / sumW, sM2 / sumW
                            n = nh + one
                            n = n if n < mh else mh
                            a = one / n
                            a = a if a > F(alpha_min) else F(alpha_min)
                            I = [Hc[k] + a * (Icur[k] - Hc[k]) for k in range(3)]
                            m1 = Hm1 + a * (l - Hm1)
                            m2 = Hm2 + a * (q - Hm2)
                if not (finite(m1) and finite(m2)):
                    m1, m2 = l, q
                for k in range(3):
                    image[y, x, k] = I[k] * D[k]
                    o0[y, x, k] = I[k]
                image[y, x, 3] = o0[y, x, 3] = n
                o3[y, x, 0], o3[y, x, 1], o3[y, x, 2] = m1, m2, clamp0(m2 - m1 * m1)
        mt = F(min_temporal)
        for y in range(Hh):
            for x in range(Ww):
                n = o0[y, x, 3]
                if n < one:
                    var[y, x] = F(-1)
                elif n >= mt:
                    var[y, x] = o3[y, x, 2]
                else:
                    Np, Pp = o1[y, x, :3], o2[y, x, :3]
                    m = F(sigma_plane) * o2[y, x, 3]
                    k, s1, s2 = zero, zero, zero
                    for dy in range(-3, 4):
                        for dx in range(-3, 4):
                            qx, qy = x + dx, y + dy
                            if dx != 0 or dy != 0:
                                if qx < 0 or qx >= Ww or qy < 0 or qy >= Hh or o0[qy, qx, 3] < one:
                                    continue
                                if dot(Np, o1[qy, qx, :3]) < F(normal_cos_min):
                                    continue
                                g = dot(Np, [o2[qy, qx, j] - Pp[j] for j in range(3)])
                                if not g * g <= m * m:
                                    continue
                                if flags & SAME_PRIMITIVE and bits(o1[qy, qx, 3:4])[0] != bits(o1[y, x, 3:4])[0]:
                                    continue
                            lq = lum3(o0[qy, qx, :3])
                            k, s1, s2 = k + one, s1 + lq, s2 + lq * lq
                    mean = s1 / k
                    var[y, x] = clamp0(s2 / k - mean * mean) * (mt / n)
    return image, o0, o1, o2, o3, var


def run_sequence(step, seq, flags, params=None, min_temporal=4, stats=None):
    """temporal_model.run_sequence with the four-plane history and the variance."""
    p = dict(tm.PARAMS if params is None else params)
    outs, hist, prev = [], None, None
    for cam, frame in seq:
        kw = {}
        if stats is not None:
            stats.append({})
            kw["stats"] = stats[-1]
        out = step(*frame, cam, hist, prev if prev is not None else cam, p["alpha_min"], p["max_history"], p["sigma_plane"],
                   p["normal_cos_min"], flags, min_temporal, **kw)
        outs.append(out)
        hist, prev = out[1:5], cam
    return outs


def make_sequence(width=tm.WIDTH, height=tm.HEIGHT, seed=1):
    """temporal_model.make_sequence, then colours near 3e38 in the later frames: their luminance squared (and,
    divided by an albedo below 1, the colour itself) overflows, so the blended moments restart.  And pixels with
    a primitive id of their own in every frame: under SAME_PRIMITIVE nothing around them, in the history or in
    the window, is the same surface, so their history stays young and their window holds the centre alone."""
    seq = tm.make_sequence(width, height, seed)
    y, x = np.mgrid[0:height, 0:width]
    alone = (x % 10 == 2) & (y % 9 == 4)
    out = []
    for k, (cam, (color, p0, p1, p2)) in enumerate(seq):
        color, p0 = color.copy(), p0.copy()
        if k >= 1:
            color[(x % 9 == 4) & (y % 8 == 1), :3] = F(3e38)
            color[(x % 9 == 7) & (y % 8 == 6), :3] = F(1e20)
        ids = bits(p0[..., 3]).copy()
        hit = ids != U(0xffffffff)
        ids[alone & hit] = (U(1000) + (y * width + x).astype(U))[alone & hit]
        p0[..., 3] = ids.view(F)
        out.append((cam, (color, p0, p1, p2)))
    return out


# ---- 3: the variance-guided filter ----------------------------------------------------------------------
def vkeep_mask(color, plane0, plane1, plane2, variance, flags):
    with np.errstate(all="ignore"):
        I = (color[..., :3].astype(F) / dm.divisor(plane0, flags)).astype(F)
        var = np.ascontiguousarray(variance, dtype=F)
        return dm.keep_mask(color, plane1, plane2) & (var >= 0) & _finite(var) & _finite(lum(I))


def filter_model(color, plane0, plane1, plane2, variance, iterations, sigma_l, variance_floor, sigma_plane,
                 normal_power_log2, flags, levels=None):
    """Returns the filtered image; `levels` (a list) receives (I, v, keep) before the first and after every
    iteration."""
    color, plane0, plane1, plane2 = (np.ascontiguousarray(a, dtype=F) for a in (color, plane0, plane1, plane2))
    var = np.ascontiguousarray(variance, dtype=F)
    C = color[..., :3]
    ids = bits(plane0[..., 3])
    Nn, t, P = plane1[..., :3], plane1[..., 3], plane2[..., :3]
    D = dm.divisor(plane0, flags)
    keep = vkeep_mask(color, plane0, plane1, plane2, var, flags)
    sl2 = F(sigma_l) * F(sigma_l)
    with np.errstate(all="ignore"):
        I = (C / D).astype(F)
        v = np.where(keep, np.where(var < BIG, var, BIG), F(-1)).astype(F)
        if levels is not None:
            levels.append((I.copy(), v.copy(), keep.copy()))
        m = F(sigma_plane) * t
        mm = m * m
        for i in range(iterations):
            s = 1 << i
            sumG, sumV = np.zeros(t.shape, dtype=F), np.zeros(t.shape, dtype=F)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    vq = dm._shift(v, 1, dx, dy, F(-1))
                    skip = vq < 0
                    g = K3[abs(dx)] * K3[abs(dy)]
                    sumG = np.where(skip, sumG, sumG + g)
                    sumV = np.where(skip, sumV, sumV + g * vq)
            vg = sumV / sumG
            den = sl2 * vg + F(variance_floor)
            lp = lum(I)
            sumW, sumV2 = np.zeros(t.shape, dtype=F), np.zeros(t.shape, dtype=F)
            sumI = np.zeros(C.shape, dtype=F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    vq = dm._shift(v, s, dx, dy, F(-1))
                    skip = vq < 0
                    if flags & SAME_PRIMITIVE:
                        skip = skip | (dm._shift(ids, s, dx, dy) != ids)
                    Nq, Pq, Iq = dm._shift(Nn, s, dx, dy), dm._shift(P, s, dx, dy), dm._shift(I, s, dx, dy)
                    h = dm.K[abs(dx)] * dm.K[abs(dy)]
                    c = (Nn[..., 0] * Nq[..., 0] + Nn[..., 1] * Nq[..., 1]) + Nn[..., 2] * Nq[..., 2]
                    c = np.where(c > 0, c, F(0))
                    for _ in range(normal_power_log2):
                        c = c * c
                    e = Pq - P
                    g = (Nn[..., 0] * e[..., 0] + Nn[..., 1] * e[..., 1]) + Nn[..., 2] * e[..., 2]
                    wp = F(1) / (F(1) + (g * g) / mm)
                    d = lum(Iq) - lp
                    wc = F(1) / (F(1) + (d * d) / den)
                    w = ((h * c) * wp) * wc
                    sumW = np.where(skip, sumW, sumW + w)
                    sumI = np.where(skip[..., None], sumI, sumI + w[..., None] * Iq)
                    sumV2 = np.where(skip, sumV2, sumV2 + (w * w) * vq)
            kept = ~(v < 0)
            I = np.where(kept[..., None], sumI / sumW[..., None], I).astype(F)
            v = np.where(kept, sumV2 / (sumW * sumW), v).astype(F)
            if levels is not None:
                levels.append((I.copy(), v.copy(), kept.copy()))
        out = np.ones(color.shape, dtype=F)
        out[..., :3] = np.where((~(v < 0))[..., None], I * D, C)
    return out


def filter_scalar(color, plane0, plane1, plane2, variance, iterations, sigma_l, variance_floor, sigma_plane,
                  normal_power_log2, flags):
    color, plane0, plane1, plane2 = (np.ascontiguousarray(a, dtype=F) for a in (color, plane0, plane1, plane2))
    variance = np.ascontiguousarray(variance, dtype=F)
    H, W = color.shape[:2]
    one, lo = F(1), F(1.0 / 64.0)

    def finite(x):
        return bool((x - x) == 0)

    def lum3(c):
        return (F(0.2126) * c[0] + F(0.7152) * c[1]) + F(0.0722) * c[2]

    D = np.ones((H, W, 3), dtype=F)
    T = np.zeros((H, W, 4), dtype=F)                 # the texel (I, v or -1)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                fl = int(bits(plane2[y, x, 3:4])[0])
                ok = bool(fl & HIT) and not fl & EMISSIVE
                for img in (color, plane1, plane2):
                    for k in range(3):
                        ok = ok and finite(img[y, x, k])
                for k in range(3):
                    if flags & DEMODULATE:
                        a = plane0[y, x, k]
                        D[y, x, k] = a if a > lo else lo
                    T[y, x, k] = color[y, x, k] / D[y, x, k]
                var = variance[y, x]
                ok = ok and bool(var >= 0) and finite(var) and finite(lum3(T[y, x, :3]))
                T[y, x, 3] = (var if var < BIG else BIG) if ok else F(-1)
        sl2 = F(sigma_l) * F(sigma_l)
        for i in range(iterations):
            s = 1 << i
            nxt = T.copy()
            for y in range(H):
                for x in range(W):
                    if T[y, x, 3] < 0:
                        continue
                    sumG, sumV = F(0), F(0)
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            qx, qy = x + dx, y + dy
                            if qx < 0 or qx >= W or qy < 0 or qy >= H or T[qy, qx, 3] < 0:
                                continue
                            g = K3[abs(dx)] * K3[abs(dy)]
                            sumG = sumG + g
                            sumV = sumV + g * T[qy, qx, 3]
                    den = sl2 * (sumV / sumG) + F(variance_floor)
                    Np, Pp, Ip = plane1[y, x, :3], plane2[y, x, :3], T[y, x, :3]
                    lp = lum3(Ip)
                    m = F(sigma_plane) * plane1[y, x, 3]
                    mm = m * m
                    sumW, sumV2, sumI = F(0), F(0), [F(0), F(0), F(0)]
                    for dy in (-2, -1, 0, 1, 2):
                        for dx in (-2, -1, 0, 1, 2):
                            qx, qy = x + s * dx, y + s * dy
                            if qx < 0 or qx >= W or qy < 0 or qy >= H or T[qy, qx, 3] < 0:
                                continue
                            if flags & SAME_PRIMITIVE and bits(plane0[qy, qx, 3:4])[0] != bits(plane0[y, x, 3:4])[0]:
                                continue
                            Nq, Pq, Iq = plane1[qy, qx, :3], plane2[qy, qx, :3], T[qy, qx, :3]
                            h = dm.K[abs(dx)] * dm.K[abs(dy)]
                            c = (Np[0] * Nq[0] + Np[1] * Nq[1]) + Np[2] * Nq[2]
                            c = c if c > 0 else F(0)
                            for _ in range(normal_power_log2):
                                c = c * c
                            e = [Pq[k] - Pp[k] for k in range(3)]
                            g = (Np[0] * e[0] + Np[1] * e[1]) + Np[2] * e[2]
                            wp = one / (one + (g * g) / mm)
                            d = lum3(Iq) - lp
                            wc = one / (one + (d * d) / den)
                            w = ((h * c) * wp) * wc
                            sumW = sumW + w
                            sumV2 = sumV2 + (w * w) * T[qy, qx, 3]
                            for k in range(3):
                                sumI[k] = sumI[k] + w * Iq[k]
                    for k in range(3):
                        nxt[y, x, k] = sumI[k] / sumW
                    nxt[y, x, 3] = sumV2 / (sumW * sumW)
            T = nxt
        out = np.ones((H, W, 4), dtype=F)
        for y in range(H):
            for x in range(W):
                for k in range(3):
                    out[y, x, k] = color[y, x, k] if T[y, x, 3] < 0 else T[y, x, k] * D[y, x, k]
    return out


CLASSES = ("zero", "tiny", "ordinary", "huge", "inf", "nan", "negative")


def make_filter_inputs(width, height, seed):
    """denoise_model.make_inputs with colours near 3e38 added (their demodulated luminance, or its square,
    overflows) and a seeded variance plane that holds every class of CLASSES.  Returns
    (color, plane0, plane1, plane2, variance, classes) with classes = the index into CLASSES per pixel."""
    color, p0, p1, p2 = dm.make_inputs(width, height, seed)
    rng = np.random.default_rng([seed, 77])
    y, x = np.mgrid[0:height, 0:width]
    color = color.copy()
    color[(x % 19 == 11) & (y % 11 == 4), :3] = F(3e38)
    cls = np.full((height, width), 2, dtype=np.int64)
    pick = rng.random((height, width))
    bands = {0: (0.0, 0.06), 1: (0.06, 0.12), 3: (0.12, 0.15), 4: (0.15, 0.18), 5: (0.18, 0.21), 6: (0.21, 0.24)}
    for idx, (lo, hi) in bands.items():
        cls[(pick >= lo) & (pick < hi)] = idx
    for idx in (0, 1, 3, 4, 5, 6):                     # every class at a fixed place too, whatever the size
        if idx < width * height:
            cls.flat[(idx * 5) % (width * height)] = idx
    ordinary = (F(0.02) * rng.random((height, width), dtype=F) ** 2).astype(F)
    values = [np.zeros_like(ordinary), np.full_like(ordinary, F(1e-30)), ordinary, np.full_like(ordinary, F(1e30)),
              np.full_like(ordinary, F(np.inf)), np.full_like(ordinary, F(np.nan)), np.full_like(ordinary, F(-0.01))]
    var = np.choose(cls, values).astype(F)
    return color, p0, p1, p2, np.ascontiguousarray(var), cls
