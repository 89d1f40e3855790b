"""Rule 8 of include/pt_hip.h, the guided upsampling, restated in numpy float32 twice, and seeded inputs for it.

model()    whole-image arithmetic (one gathered copy of the low image per tap, the skips as selects)
scalar()   the same pixel by pixel with np.float32 scalars, written from the header independently

tests/test_upsample_rule.py holds the two against each other word for word; tests/test_gpu_upsample.py holds the
device against model().

Images are height x width x 4 float32 as in denoise_model.  `lo` = (color, plane0, plane1, plane2) of the low image,
`hi` = (plane0, plane1, plane2) of the high one.  Both return (out, (count_wide, count_nearest)).
"""
import numpy as np

import denoise_model as dm
from denoise_model import F, U, HIT, EMISSIVE, bits, same_words   # noqa: F401

DEMODULATE, SAME_PRIMITIVE = 1, 2
# (high width, high height, low width, low height): around the tile, odd against even, ratios 1, 2, about 3, and 4
SIZE_PAIRS = ((1, 1, 1, 1), (2, 2, 1, 1), (31, 7, 16, 4), (33, 9, 17, 5), (32, 8, 32, 8), (48, 40, 24, 20),
              (64, 16, 16, 4), (40, 24, 13, 8), (70, 45, 35, 23))
PARAM_SETS = ((0.005, 0), (0.005, 7), (0.3, 0), (0.3, 7))          # sigma_plane, normal_power_log2


def _finite(a):
    with np.errstate(all="ignore"):
        a = np.asarray(a, dtype=F)
        return (a - a) == 0


def _finite3(img):
    return _finite(img[..., 0]) & _finite(img[..., 1]) & _finite(img[..., 2])


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def axis(n_hi, n_lo):
    """u, floor(u) as int, u - floor(u) and the nearest low index along one axis, in the rule's operations."""
    s = F(n_lo) / F(n_hi)
    x = np.arange(n_hi).astype(F)
    c = ((x + F(0.5)) * s).astype(F)
    u = (c - F(0.5)).astype(F)
    f0 = np.floor(u).astype(F)
    return u, f0.astype(np.int64), (u - f0).astype(F), np.minimum(c.astype(np.int64), n_lo - 1)


def footprint_divisor(l0, h0, xn, yn, flags):
    """D_q: the mean of the high pixels' divisors over q's footprint (the high pixels whose nearest low pixel is q) on
    q's primitive, summed row by row; q's own divisor where no high pixel of the footprint has its id, and 1 without
    DEMODULATE."""
    own = dm.divisor(l0, flags)
    if not flags & DEMODULATE:
        return own
    h, w = l0.shape[:2]
    Dp = dm.divisor(h0, flags)
    qi = (yn[:, None] * w + xn[None, :]).ravel()                  # raster order of the high pixels: y outer, x inner
    member = bits(h0[..., 3]).ravel() == bits(l0[..., 3]).ravel()[qi]
    S = np.zeros((h * w, 3), dtype=F)
    n = np.zeros(h * w, dtype=np.int64)
    np.add.at(S, qi[member], Dp.reshape(-1, 3)[member])           # unbuffered: one float32 add per member, in this order
    np.add.at(n, qi[member], 1)
    with np.errstate(all="ignore"):
        mean = (S / n.astype(F)[:, None]).astype(F).reshape(h, w, 3)
    return np.where((n > 0).reshape(h, w, 1), mean, own).astype(F)


# ---- whole image ----------------------------------------------------------------------------------------
def model(lo, hi, sigma_plane, normal_power_log2, flags, stats=None):
    color, l0, l1, l2 = (np.ascontiguousarray(a, dtype=F) for a in lo)
    h0, h1, h2 = (np.ascontiguousarray(a, dtype=F) for a in hi)
    h, w = color.shape[:2]
    H, W = h0.shape[:2]
    u, x0, fx, xn = axis(W, w)
    v, y0, fy, yn = axis(H, h)
    keep = dm.keep_mask(color, l1, l2)
    raw = _finite3(color)
    idq_all, flq_all = bits(l0[..., 3]), bits(l2[..., 3])
    idp, flp = bits(h0[..., 3]), bits(h2[..., 3])
    Dq = footprint_divisor(l0, h0, xn, yn, flags)
    Np, Pp, tp = h1[..., :3], h2[..., :3], h1[..., 3]
    guide = ((flp & HIT) != 0) & ((flp & EMISSIVE) == 0) & _finite3(h1) & _finite3(h2)
    Dp = dm.divisor(h0, flags)
    met = {k: np.zeros((H, W), dtype=bool) for k in ("outside", "not_kept", "by_id", "zero_b", "u_outside", "u_not_raw",
                                                      "u_kept", "u_flags", "u_id", "u_accepted")}
    with np.errstate(all="ignore"):
        Iq_all = (color[..., :3] / Dq).astype(F)
        m = F(sigma_plane) * tp
        mm = m * m

        def gather(qx, qy):
            cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            inside = ((qy >= 0) & (qy < h))[:, None] & ((qx >= 0) & (qx < w))[None, :]
            return inside, (lambda a: a[cy][:, cx])

        def guided(taps, note):
            sumW = np.zeros((H, W), dtype=F)
            sumI = np.zeros((H, W, 3), dtype=F)
            for qx, qy, b in taps:
                inside, at = gather(qx, qy)
                reasons = [("outside", ~inside), ("not_kept", ~at(keep)),
                           ("by_id", (at(idq_all) != idp) if flags & SAME_PRIMITIVE else np.zeros((H, W), dtype=bool))]
                skip = np.zeros((H, W), dtype=bool)
                for name, r in reasons:
                    if note:
                        met[name] |= guide & ~skip & r
                    skip |= r
                if note:
                    met["zero_b"] |= guide & ~skip & (b == 0)
                Nq, Pq, Iq = at(l1[..., :3]), at(l2[..., :3]), at(Iq_all)
                c = _dot(Np, Nq)
                c = np.where(c > 0, c, F(0))
                for _ in range(normal_power_log2):
                    c = c * c
                g = _dot(Np, (Pq - Pp).astype(F))
                wp = F(1) / (F(1) + (g * g) / mm)
                wgt = ((b * c) * wp).astype(F)
                sumW = np.where(skip, sumW, sumW + wgt).astype(F)
                sumI = np.where(skip[..., None], sumI, sumI + wgt[..., None] * Iq).astype(F)
            return sumW, sumI

        one = F(1)
        ring1 = [(x0 + i, y0 + j, ((fx if i else one - fx)[None, :] * (fy if j else one - fy)[:, None]).astype(F))
                 for j in (0, 1) for i in (0, 1)]
        ring2 = []
        for dy in (-1, 0, 1, 2):
            for dx in (-1, 0, 1, 2):
                if dx in (0, 1) and dy in (0, 1):
                    continue
                ex, ey = ((x0 + dx).astype(F) - u).astype(F), ((y0 + dy).astype(F) - v).astype(F)
                ring2.append((x0 + dx, y0 + dy, (one / (one + ((ex * ex)[None, :] + (ey * ey)[:, None]))).astype(F)))
        W1, I1 = guided(ring1, True)
        W2, I2 = guided(ring2, False)
        have1 = _finite(W1) & (W1 > 0)
        have2 = _finite(W2) & (W2 > 0)
        near = color[yn][:, xn][..., :3]
        g1 = ((I1 / W1[..., None]) * Dp).astype(F)
        g2 = ((I2 / W2[..., None]) * Dp).astype(F)
        out_g = np.where(have1[..., None], g1, np.where(have2[..., None], g2, near))
        # without a guide: ring 1 on the raw colour
        sumB = np.zeros((H, W), dtype=F)
        sumC = np.zeros((H, W, 3), dtype=F)
        emit = (flp & EMISSIVE) != 0
        for qx, qy, b in ring1:
            inside, at = gather(qx, qy)
            reasons = [("u_outside", ~inside), ("u_not_raw", ~at(raw)), ("u_kept", at(keep)), ("u_flags", at(flq_all) != flp),
                       ("u_id", emit & (at(idq_all) != idp))]
            skip = np.zeros((H, W), dtype=bool)
            for name, r in reasons:
                met[name] |= ~guide & ~skip & r
                skip |= r
            met["u_accepted"] |= ~guide & ~skip
            sumB = np.where(skip, sumB, sumB + b).astype(F)
            sumC = np.where(skip[..., None], sumC, sumC + b[..., None] * at(color[..., :3])).astype(F)
        haveU = _finite(sumB) & (sumB > 0)
        out_u = np.where(haveU[..., None], (sumC / sumB[..., None]).astype(F), near)
        out = np.ones((H, W, 4), dtype=F)
        out[..., :3] = np.where(guide[..., None], out_g, out_u)
    wide, nearest = guide & ~have1 & have2, guide & ~have1 & ~have2
    if stats is not None:
        stats.update({k: int(a.sum()) for k, a in met.items()})
        stats.update(guided=int(guide.sum()), ring1=int((guide & have1).sum()), wide=int(wide.sum()), nearest=int(nearest.sum()),
                     unguided=int((~guide).sum()), u_interpolated=int((~guide & haveU).sum()),
                     u_nearest=int((~guide & ~haveU).sum()), guide_mask=guide, ring1_mask=guide & have1, wide_mask=wide,
                     nearest_mask=nearest, u_miss=int((~guide & (flp == 0)).sum()), u_emitter=int((~guide & emit).sum()),
                     u_not_finite=int((~guide & ~emit & (flp != 0)).sum()))
    return out, (int(wide.sum()), int(nearest.sum()))


# ---- pixel by pixel -------------------------------------------------------------------------------------
def scalar(lo, hi, sigma_plane, normal_power_log2, flags):
    color, l0, l1, l2 = (np.ascontiguousarray(a, dtype=F) for a in lo)
    h0, h1, h2 = (np.ascontiguousarray(a, dtype=F) for a in hi)
    h, w = color.shape[:2]
    H, W = h0.shape[:2]
    one, half, floor_a = F(1), F(0.5), F(1.0 / 64.0)

    def finite(x):
        return bool((x - x) == 0)

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    def divisor(a):
        return [(a[k] if a[k] > floor_a else floor_a) if flags & DEMODULATE else one for k in range(3)]

    lid, lfl, hid, hfl = bits(l0[..., 3]), bits(l2[..., 3]), bits(h0[..., 3]), bits(h2[..., 3])
    KEEP = np.zeros((h, w), dtype=bool)
    RAW = np.zeros((h, w), dtype=bool)
    I = np.zeros((h, w, 3), dtype=F)
    out = np.ones((H, W, 4), dtype=F)
    counts = [0, 0]
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                RAW[y, x] = all(finite(color[y, x, k]) for k in range(3))
                fl = int(lfl[y, x])
                KEEP[y, x] = (bool(fl & HIT) and not fl & EMISSIVE and RAW[y, x]
                              and all(finite(l1[y, x, k]) and finite(l2[y, x, k]) for k in range(3)))
        sx, sy = F(w) / F(W), F(h) / F(H)
        # D_q: the mean of the divisors of the high pixels of q's footprint that carry q's id, in raster order
        S = np.zeros((h, w, 3), dtype=F)
        members = np.zeros((h, w), dtype=np.int64)
        if flags & DEMODULATE:
            for y in range(H):
                qy = min(int((F(y) + half) * sy), h - 1)
                for x in range(W):
                    qx = min(int((F(x) + half) * sx), w - 1)
                    if hid[y, x] == lid[qy, qx]:
                        Dp = divisor(h0[y, x])
                        for k in range(3):
                            S[qy, qx, k] = S[qy, qx, k] + Dp[k]
                        members[qy, qx] += 1
        for y in range(h):
            for x in range(w):
                D = divisor(l0[y, x])
                if members[y, x]:
                    D = [S[y, x, k] / F(members[y, x]) for k in range(3)]
                for k in range(3):
                    I[y, x, k] = color[y, x, k] / D[k]
        for y in range(H):
            cv = (F(y) + half) * sy
            v = cv - half
            y0 = int(np.floor(v))
            fy = v - F(y0)
            yn = min(int(cv), h - 1)
            for x in range(W):
                cu = (F(x) + half) * sx
                u = cu - half
                x0 = int(np.floor(u))
                fx = u - F(x0)
                xn = min(int(cu), w - 1)
                fl = int(hfl[y, x])
                Np, Pp = h1[y, x, :3], h2[y, x, :3]
                guide = bool(fl & HIT) and not fl & EMISSIVE and all(finite(Np[k]) and finite(Pp[k]) for k in range(3))
                result = None
                if guide:
                    m = F(sigma_plane) * h1[y, x, 3]
                    mm = m * m
                    Dp = divisor(h0[y, x])
                    for ring in (1, 2):
                        sumW, sumI = F(0), [F(0), F(0), F(0)]
                        offsets = ((0, 0), (1, 0), (0, 1), (1, 1)) if ring == 1 else \
                            tuple((dx, dy) for dy in (-1, 0, 1, 2) for dx in (-1, 0, 1, 2) if not (dx in (0, 1) and dy in (0, 1)))
                        for dx, dy in offsets:
                            qx, qy = x0 + dx, y0 + dy
                            if qx < 0 or qx >= w or qy < 0 or qy >= h or not KEEP[qy, qx]:
                                continue
                            if flags & SAME_PRIMITIVE and lid[qy, qx] != hid[y, x]:
                                continue
                            if ring == 1:
                                b = (fx if dx else one - fx) * (fy if dy else one - fy)
                            else:
                                ex, ey = F(qx) - u, F(qy) - v
                                b = one / (one + (ex * ex + ey * ey))
                            Nq, Pq = l1[qy, qx, :3], l2[qy, qx, :3]
                            c = dot(Np, Nq)
                            c = c if c > 0 else F(0)
                            for _ in range(normal_power_log2):
                                c = c * c
                            g = dot(Np, [Pq[k] - Pp[k] for k in range(3)])
                            wp = one / (one + (g * g) / mm)
                            wgt = (b * c) * wp
                            sumW = sumW + wgt
                            for k in range(3):
                                sumI[k] = sumI[k] + wgt * I[qy, qx, k]
                        if finite(sumW) and sumW > 0:
                            result = [(sumI[k] / sumW) * Dp[k] for k in range(3)]
                            if ring == 2:
                                counts[0] += 1
                            break
                    if result is None:
                        counts[1] += 1
                else:
                    sumB, sumC = F(0), [F(0), F(0), F(0)]
                    for dy in (0, 1):
                        for dx in (0, 1):
                            qx, qy = x0 + dx, y0 + dy
                            if qx < 0 or qx >= w or qy < 0 or qy >= h or not RAW[qy, qx] or KEEP[qy, qx]:
                                continue
                            if int(lfl[qy, qx]) != fl or (fl & EMISSIVE and lid[qy, qx] != hid[y, x]):
                                continue
                            b = (fx if dx else one - fx) * (fy if dy else one - fy)
                            sumB = sumB + b
                            for k in range(3):
                                sumC[k] = sumC[k] + b * color[qy, qx, k]
                    if finite(sumB) and sumB > 0:
                        result = [sumC[k] / sumB for k in range(3)]
                if result is None:
                    result = [color[yn, xn, k] for k in range(3)]
                for k in range(3):
                    out[y, x, k] = result[k]
    return out, (counts[0], counts[1])


# ---- inputs ---------------------------------------------------------------------------------------------
def _surface(X, Y, rng, special):
    """The planes of one image whose pixel centres lie at (X, Y) in high-pixel units: surfaces in stripes six high
    pixels wide and five high (so low and high pixels of one place carry one id), one stripe in three facing the
    other way, a region of misses and an emissive region; then, where `special`, by pixel position: albedo 0 and
    below 1/64, a NaN normal, t = 0 and ids that match nothing."""
    Hn, Wn = X.shape
    yi, xi = np.mgrid[0:Hn, 0:Wn]
    ident = (np.floor(X / 6) + 3 * np.floor(Y / 5)).astype(np.int64).astype(U)
    nrm = np.zeros((Hn, Wn, 3), dtype=F)
    base = np.array([0.3, 0.5, 0.8], dtype=F)
    nrm[:] = base / F(np.sqrt(np.sum(base.astype(np.float64) ** 2)))
    nrm[..., 0] += F(0.02) * (ident % 5).astype(F)
    nrm = (nrm / np.sqrt((nrm * nrm).sum(-1, keepdims=True))).astype(F)
    nrm[(ident % 3) == 1] *= F(-1)
    t = (F(3) + F(0.05) * X + F(0.02) * Y).astype(F)
    pos = np.stack([F(0.1) * X, F(0.1) * Y, F(0.01) * (ident % 7).astype(F) + rng.normal(0, 0.002, (Hn, Wn)).astype(F)],
                   -1).astype(F)
    alb = (F(0.2) + F(0.8) * rng.random((Hn, Wn, 3), dtype=F)).astype(F)
    flags = np.full((Hn, Wn), HIT, dtype=U)
    miss = (np.floor(X) % 16 >= 12) & (np.floor(Y) % 12 >= 8)
    flags[miss] = 0
    flags[(np.floor(X) % 16 < 3) & (np.floor(Y) % 12 >= 9)] = HIT | EMISSIVE
    if special:
        alb[(xi % 11 == 3) & (yi % 7 == 2)] = F(0)
        alb[(xi % 11 == 5) & (yi % 7 == 4)] = F(1.0 / 128.0)
        nrm[(xi % 17 == 9) & (yi % 10 == 6), 0] = F(np.nan)
        nrm[(xi % 19 == 4) & (yi % 11 == 3), 1] = F(np.inf)
        t[(xi % 13 == 2) & (yi % 9 == 1)] = F(0)
        ident[(xi % 23 == 7) & (yi % 5 == 0)] = U(0x7fffffff)
    ident[miss] = U(0xffffffff)
    for a in (alb, nrm, pos):
        a[miss] = F(0)
    t[miss] = F(0)
    return (np.concatenate([alb, ident.view(F)[..., None]], -1), np.concatenate([nrm, t[..., None]], -1),
            np.concatenate([pos, flags.view(F)[..., None]], -1))


def make_case(W, H, w, h, seed):
    """Seeded (lo, hi) of one scene seen at both sizes, with every case the rule distinguishes.  Low pixels: noisy
    colour over a smooth signal, NaN, +inf and -inf colours, NaN and infinite normals, misses and emitters beside kept
    pixels, and a block of pixels that are not kept (16 rejected taps for the high pixels above its middle).  High
    pixels: NaN and infinite normals, albedo 0, t = 0, ids that never match."""
    rng = np.random.default_rng(seed)
    yh, xh = np.mgrid[0:H, 0:W]
    hi = _surface(xh.astype(F), yh.astype(F), rng, True)
    yl, xl = np.mgrid[0:h, 0:w]
    X = ((xl.astype(F) + F(0.5)) * (F(W) / F(w)) - F(0.5)).astype(F)
    Y = ((yl.astype(F) + F(0.5)) * (F(H) / F(h)) - F(0.5)).astype(F)
    l0, l1, l2 = _surface(X, Y, rng, True)
    signal = F(0.5) + F(0.25) * np.sin(X / F(6)).astype(F) + F(0.25) * np.cos(Y / F(5)).astype(F)
    col = (l0[..., :3] * (signal[..., None] + rng.normal(0, 0.15, (h, w, 3)).astype(F))).astype(F)
    col[(xl % 13 == 6) & (yl % 9 == 3)] = F(np.nan)
    col[(xl % 13 == 8) & (yl % 9 == 5), 1] = F(np.inf)
    col[(xl % 13 == 10) & (yl % 9 == 7), 2] = F(-np.inf)
    block = (xl >= 4) & (xl < 9) & (yl >= 11) & (yl < 16)          # 5 x 5 low pixels, none of them kept
    col[block, 0] = F(np.nan)
    color = np.concatenate([col, np.ones((h, w, 1), dtype=F)], -1)
    c = lambda a: np.ascontiguousarray(a, dtype=F)                  # noqa: E731
    return (c(color), c(l0), c(l1), c(l2)), tuple(c(a) for a in hi)


def bilinear(color, W, H):
    """The plain bilinear resampling of a low image to W x H (rule 8's coordinates, clamped at the border, no guide)."""
    color = np.ascontiguousarray(color, dtype=F)
    h, w = color.shape[:2]
    _, x0, fx, _ = axis(W, w)
    _, y0, fy, _ = axis(H, h)
    xa, xb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1)
    ya, yb = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    fx, fy = fx[None, :, None], fy[:, None, None]
    top = color[ya][:, xa] * (1 - fx) + color[ya][:, xb] * fx
    bot = color[yb][:, xa] * (1 - fx) + color[yb][:, xb] * fx
    return (top * (1 - fy) + bot * fy).astype(F)


def nearest(color, W, H):
    color = np.ascontiguousarray(color, dtype=F)
    h, w = color.shape[:2]
    return color[axis(H, h)[3]][:, axis(W, w)[3]]
