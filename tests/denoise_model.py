"""The a-trous filter rule of include/pt_hip.h restated in numpy float32, twice, and seeded inputs for it.

model()   whole-image arithmetic: one shifted copy of the image per tap, the taps in the rule's order
          (dy outer, dx inner), every operation a separate float32 rounding (numpy never contracts)
scalar()  the same rule pixel by pixel with np.float32 scalars, written from the header independently of
          model(); tests/test_denoise_rule.py holds the two against each other word for word, and
          tests/test_gpu_denoise.py holds the device against model()

Images are height x width x 4 float32: colour (w ignored) and the three feature planes
(albedo + primitive bits, normal + t, position + flag bits).
"""
import numpy as np

F = np.float32
U = np.uint32
HIT, EMISSIVE = 1, 2
DEMODULATE, SAME_PRIMITIVE = 1, 2
K = (F(3.0 / 8.0), F(1.0 / 4.0), F(1.0 / 16.0))
TILE_W, TILE_H = 32, 8                    # PT_DENOISE_TILE_W / _H (tests/test_denoise_rule.py checks them)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(U)


def keep_mask(color, plane1, plane2):
    fl = bits(plane2[..., 3])
    with np.errstate(all="ignore"):
        fin = np.ones(fl.shape, dtype=bool)
        for img in (color, plane1, plane2):
            for k in range(3):
                x = img[..., k].astype(F)
                fin &= (x - x) == 0
    return ((fl & HIT) != 0) & ((fl & EMISSIVE) == 0) & fin


def divisor(plane0, flags):
    A = plane0[..., :3].astype(F)
    if not flags & DEMODULATE:
        return np.ones_like(A)
    lo = F(1.0 / 64.0)
    return np.where(A > lo, A, lo).astype(F)


def _shift(a, s, dx, dy, fill=0):
    """a[y + s dy, x + s dx], `fill` outside."""
    h, w = a.shape[:2]
    r = 2 * s
    pad = np.full((h + 2 * r, w + 2 * r) + a.shape[2:], fill, dtype=a.dtype)
    pad[r:r + h, r:r + w] = a
    return pad[r + s * dy:r + s * dy + h, r + s * dx:r + s * dx + w]


def model(color, plane0, plane1, plane2, iterations, sigma_color, sigma_plane, normal_power_log2, flags):
    color, plane0, plane1, plane2 = (np.ascontiguousarray(a, dtype=F) for a in (color, plane0, plane1, plane2))
    C = color[..., :3]
    ids = bits(plane0[..., 3])
    Nn, t, P = plane1[..., :3], plane1[..., 3], plane2[..., :3]
    keep = keep_mask(color, plane1, plane2)
    D = divisor(plane0, flags)
    with np.errstate(all="ignore"):
        I = (C / D).astype(F)
        for i in range(iterations):
            s = 1 << i
            sigma = F(sigma_color) * F(1.0 / s)
            ss = sigma * sigma
            m = F(sigma_plane) * t
            mm = m * m
            sumW = np.zeros(t.shape, dtype=F)
            sumI = np.zeros(C.shape, dtype=F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    kq = _shift(keep, s, dx, dy, False)
                    skip = ~kq
                    if flags & SAME_PRIMITIVE:
                        skip = skip | (_shift(ids, s, dx, dy) != ids)
                    Nq, Pq, Iq = _shift(Nn, s, dx, dy), _shift(P, s, dx, dy), _shift(I, s, dx, dy)
                    h = K[abs(dx)] * K[abs(dy)]
                    c = (Nn[..., 0] * Nq[..., 0] + Nn[..., 1] * Nq[..., 1]) + Nn[..., 2] * Nq[..., 2]
                    c = np.where(c > 0, c, F(0))
                    for _ in range(normal_power_log2):
                        c = c * c
                    e = Pq - P
                    g = (Nn[..., 0] * e[..., 0] + Nn[..., 1] * e[..., 1]) + Nn[..., 2] * e[..., 2]
                    wp = F(1) / (F(1) + (g * g) / mm)
                    d = Iq - I
                    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                    wc = F(1) / (F(1) + d2 / ss)
                    w = ((h * c) * wp) * wc
                    sumW = np.where(skip, sumW, sumW + w)
                    sumI = np.where(skip[..., None], sumI, sumI + w[..., None] * Iq)
            I = np.where(keep[..., None], sumI / sumW[..., None], I).astype(F)
        out = np.ones(color.shape, dtype=F)
        out[..., :3] = np.where(keep[..., None], I * D, C)
    return out


def scalar(color, plane0, plane1, plane2, iterations, sigma_color, sigma_plane, normal_power_log2, flags):
    """The rule pixel by pixel (small images only)."""
    color, plane0, plane1, plane2 = (np.ascontiguousarray(a, dtype=F) for a in (color, plane0, plane1, plane2))
    H, W = color.shape[:2]
    one, lo = F(1), F(1.0 / 64.0)

    def finite(x):
        return (x - x) == 0

    keep = np.zeros((H, W), dtype=bool)
    D = np.ones((H, W, 3), dtype=F)
    I = np.zeros((H, W, 3), dtype=F)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                fl = int(bits(plane2[y, x, 3:4])[0])
                ok = bool(fl & HIT) and not fl & EMISSIVE
                for img in (color, plane1, plane2):
                    for k in range(3):
                        ok = ok and bool(finite(img[y, x, k]))
                keep[y, x] = ok
                for k in range(3):
                    if flags & DEMODULATE:
                        a = plane0[y, x, k]
                        D[y, x, k] = a if a > lo else lo
                    I[y, x, k] = color[y, x, k] / D[y, x, k]
        for i in range(iterations):
            s = 1 << i
            sigma = F(sigma_color) * F(2.0 ** -i)
            ss = sigma * sigma
            nxt = I.copy()
            for y in range(H):
                for x in range(W):
                    if not keep[y, x]:
                        continue
                    Np, Pp, Ip = plane1[y, x, :3], plane2[y, x, :3], I[y, x]
                    m = F(sigma_plane) * plane1[y, x, 3]
                    mm = m * m
                    sumW = F(0)
                    sumI = [F(0), F(0), F(0)]
                    for dy in (-2, -1, 0, 1, 2):
                        for dx in (-2, -1, 0, 1, 2):
                            qx, qy = x + s * dx, y + s * dy
                            if qx < 0 or qx >= W or qy < 0 or qy >= H or not keep[qy, qx]:
                                continue
                            if flags & SAME_PRIMITIVE and bits(plane0[qy, qx, 3:4])[0] != bits(plane0[y, x, 3:4])[0]:
                                continue
                            Nq, Pq, Iq = plane1[qy, qx, :3], plane2[qy, qx, :3], I[qy, qx]
                            h = K[abs(dx)] * K[abs(dy)]
                            c = (Np[0] * Nq[0] + Np[1] * Nq[1]) + Np[2] * Nq[2]
                            c = c if c > 0 else F(0)
                            for _ in range(normal_power_log2):
                                c = c * c
                            e = [Pq[k] - Pp[k] for k in range(3)]
                            g = (Np[0] * e[0] + Np[1] * e[1]) + Np[2] * e[2]
                            wp = one / (one + (g * g) / mm)
                            d = [Iq[k] - Ip[k] for k in range(3)]
                            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                            wc = one / (one + d2 / ss)
                            w = ((h * c) * wp) * wc
                            sumW = sumW + w
                            for k in range(3):
                                sumI[k] = sumI[k] + w * Iq[k]
                    for k in range(3):
                        nxt[y, x, k] = sumI[k] / sumW
            I = nxt
        out = np.ones((H, W, 4), dtype=F)
        for y in range(H):
            for x in range(W):
                for k in range(3):
                    out[y, x, k] = I[y, x, k] * D[y, x, k] if keep[y, x] else color[y, x, k]
    return out


def same_words(a, b):
    """Words equal, or both NaN."""
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def make_inputs(width, height, seed):
    """Seeded inputs with every case the rule distinguishes: surfaces in vertical stripes four pixels
    wide (neighbouring pixels with different ids), one stripe in three facing the other way (antiparallel
    normals), noisy colour over a smooth signal; then, by position, a region of misses, an emissive
    region, albedo 0 and albedo below 1/64, NaN, +inf and -inf colours and a NaN normal.  The special
    pixels are sparse, so more than half of any image is kept.  Returns (color, plane0, plane1, plane2)."""
    rng = np.random.default_rng(seed)
    H, W = height, width
    y, x = np.mgrid[0:H, 0:W]
    ident = (x // 4 + 3 * (y // 5)).astype(U)
    nrm = np.zeros((H, W, 3), dtype=F)
    base = np.array([0.3, 0.5, 0.8], dtype=F)
    base = base / F(np.sqrt(np.sum(base.astype(np.float64) ** 2)))
    nrm[:] = base
    nrm[..., 0] += (F(0.02) * (ident % 5).astype(F))
    nrm = (nrm / np.sqrt((nrm * nrm).sum(-1, keepdims=True))).astype(F)
    nrm[(ident % 3) == 1] *= F(-1)
    t = (F(3) + F(0.05) * x.astype(F) + F(0.02) * y.astype(F)).astype(F)
    pos = np.stack([F(0.1) * x.astype(F), F(0.1) * y.astype(F),
                    F(0.01) * (ident % 7).astype(F) + rng.normal(0, 0.002, (H, W)).astype(F)], -1).astype(F)
    alb = (F(0.2) + F(0.8) * rng.random((H, W, 3), dtype=F)).astype(F)
    alb[(x % 11 == 3) & (y % 7 == 2)] = F(0)
    alb[(x % 11 == 5) & (y % 7 == 4)] = F(1.0 / 128.0)
    signal = F(0.5) + F(0.25) * np.sin(x / F(6)).astype(F) + F(0.25) * np.cos(y / F(5)).astype(F)
    col = (alb * (signal[..., None] + rng.normal(0, 0.15, (H, W, 3)).astype(F))).astype(F)
    flags = np.full((H, W), HIT, dtype=U)
    miss = (x % 16 >= 13) & (y % 12 >= 9)
    flags[miss] = 0
    flags[(x % 16 < 2) & (y % 12 >= 10)] = HIT | EMISSIVE
    col[(x % 13 == 6) & (y % 9 == 3)] = F(np.nan)
    col[(x % 13 == 8) & (y % 9 == 5), 1] = F(np.inf)
    col[(x % 13 == 10) & (y % 9 == 7), 2] = F(-np.inf)
    nrm[(x % 17 == 9) & (y % 10 == 6), 0] = F(np.nan)
    ident = ident.copy()
    ident[miss] = U(0xffffffff)
    for a in (alb, nrm, pos):
        a[miss] = F(0)
    t = t.copy()
    t[miss] = F(0)
    color = np.concatenate([col, np.ones((H, W, 1), dtype=F)], -1)
    plane0 = np.concatenate([alb, ident.view(F)[..., None]], -1)
    plane1 = np.concatenate([nrm, t[..., None]], -1)
    plane2 = np.concatenate([pos, flags.view(F)[..., None]], -1)
    return tuple(np.ascontiguousarray(a, dtype=F) for a in (color, plane0, plane1, plane2))


def vacuity(color, plane1, plane2, out):
    """The conditions that make a comparison worth making, as (kept share, changed share of the kept,
    every non-kept pixel equals its input)."""
    keep = keep_mask(color, plane1, plane2)
    changed = (bits(out[..., :3]) != bits(color[..., :3])).any(-1)
    untouched = bool(np.all(bits(out[..., :3])[~keep] == bits(color[..., :3])[~keep]))
    kept = int(keep.sum())
    return kept / keep.size, (int((changed & keep).sum()) / kept if kept else 0.0), untouched
