"""Rule 6 of include/pt_hip.h, "despike", restated in numpy float32 twice, and seeded inputs for it.

model()    whole-image arithmetic (one shifted copy per tap, the insertion into top[] as four selects)
scalar()   the same pixel by pixel with np.float32 scalars and a Python list for top[], written from the header
           independently

tests/test_despike_rule.py holds the two against each other word for word; tests/test_gpu_despike.py holds the
device against model().

Images are height x width x 4 float32 as in denoise_model.  Both return (out, count).
"""
import numpy as np

import denoise_model as dm
import svgf_model as sm
import temporal_model as tm
from denoise_model import F, U, HIT, EMISSIVE, bits, same_words   # noqa: F401

DEMODULATE, SAME_PRIMITIVE = 1, 2
# the parameters of the size and flag tests: every one of the five tap tests rejects something under them on
# make_case's 48 x 40 image, and its planted spikes are spikes
PARAMS = dict(radius=2, rank=2, factor=2.0, floor=0.05, min_neighbors=2, sigma_plane=0.05, normal_cos_min=0.9)
SIZES = ((1, 1), (1, 7), (7, 1), (31, 7), (32, 8), (33, 9), (48, 40), (65, 17))      # width, height
SPIKE = F(64)


# ---- whole image ----------------------------------------------------------------------------------------
def model(color, plane0, plane1, plane2, radius, rank, factor, floor, min_neighbors, sigma_plane, normal_cos_min, flags,
          stats=None):
    color, plane0, plane1, plane2 = (np.ascontiguousarray(a, dtype=F) for a in (color, plane0, plane1, plane2))
    Hh, Ww = color.shape[:2]
    C = color[..., :3]
    ids = bits(plane0[..., 3])
    Nn, t, P = plane1[..., :3], plane1[..., 3], plane2[..., :3]
    fl = bits(plane2[..., 3])
    D = dm.divisor(plane0, flags)
    yy, xx = np.mgrid[0:Hh, 0:Ww]
    with np.errstate(all="ignore"):
        I = (C / D).astype(F)
        l = sm.lum(I)
        ok = ((fl & HIT) != 0) & ((fl & EMISSIVE) == 0) & sm._finite(l) & tm._finite3(plane1) & tm._finite3(plane2)
        m = F(sigma_plane) * t
        mm = m * m
        top = [np.full((Hh, Ww), -np.inf, dtype=F) for _ in range(4)]
        k = np.zeros((Hh, Ww), dtype=np.int64)
        met = {name: np.zeros((Hh, Ww), dtype=bool) for name in ("outside", "not_ok", "by_normal", "by_plane", "by_id")}
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                if dx == 0 and dy == 0:
                    continue
                inside = (xx + dx >= 0) & (xx + dx < Ww) & (yy + dy >= 0) & (yy + dy < Hh)
                lq, okq = sm._clip_shift(l, dx, dy), sm._clip_shift(ok, dx, dy)
                Nq, idq, Pq = sm._clip_shift(Nn, dx, dy), sm._clip_shift(ids, dx, dy), sm._clip_shift(P, dx, dy)
                g = tm._dot(Nn, (Pq - P).astype(F))
                reasons = [("outside", ~inside), ("not_ok", ~okq), ("by_normal", tm._dot(Nn, Nq) < F(normal_cos_min)),
                           ("by_plane", ~(g * g <= mm)),
                           ("by_id", (idq != ids) if flags & SAME_PRIMITIVE else np.zeros((Hh, Ww), dtype=bool))]
                skip = np.zeros((Hh, Ww), dtype=bool)
                for name, r in reasons:
                    met[name] |= ok & ~skip & r                       # the taps this test is the first to reject
                    skip |= r
                k = np.where(skip, k, k + 1)
                v = lq
                for j in range(4):
                    up = v > top[j]
                    new_top, down = np.where(up, v, top[j]), np.where(up, top[j], v)
                    top[j] = np.where(skip, top[j], new_top).astype(F)
                    v = down
        M = top[rank - 1]
        limit = (F(factor) * M + F(floor)).astype(F)
        spike = ok & (k >= min_neighbors) & (limit >= 0) & (l > limit)
        s = (limit / l).astype(F)
        clamped = ((I * s[..., None]) * D).astype(F)
        out = np.ones(color.shape, dtype=F)
        out[..., :3] = np.where(spike[..., None], clamped, C)
    if stats is not None:
        stats.update({name: int(mask.sum()) for name, mask in met.items()})
        stats.update(ok=int(ok.sum()), spikes=int(spike.sum()), few=int((ok & (k < min_neighbors)).sum()),
                     s_min=float(s[spike].min()) if spike.any() else None,
                     s_max=float(s[spike].max()) if spike.any() else None, spike_mask=spike, ok_mask=ok)
    return out, int(spike.sum())


# ---- pixel by pixel -------------------------------------------------------------------------------------
def scalar(color, plane0, plane1, plane2, radius, rank, factor, floor, min_neighbors, sigma_plane, normal_cos_min, flags):
    color, plane0, plane1, plane2 = (np.ascontiguousarray(a, dtype=F) for a in (color, plane0, plane1, plane2))
    H, W = color.shape[:2]
    one, lo = F(1), F(1.0 / 64.0)

    def finite(x):
        return bool((x - x) == 0)

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    L = np.zeros((H, W), dtype=F)
    OK = np.zeros((H, W), dtype=bool)
    Dv = np.ones((H, W, 3), dtype=F)
    Iv = np.zeros((H, W, 3), dtype=F)
    out = np.ones((H, W, 4), dtype=F)
    count = 0
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                for j in range(3):
                    if flags & DEMODULATE:
                        a = plane0[y, x, j]
                        Dv[y, x, j] = a if a > lo else lo
                    Iv[y, x, j] = color[y, x, j] / Dv[y, x, j]
                L[y, x] = (F(0.2126) * Iv[y, x, 0] + F(0.7152) * Iv[y, x, 1]) + F(0.0722) * Iv[y, x, 2]
                fl = int(bits(plane2[y, x, 3:4])[0])
                ok = bool(fl & HIT) and not fl & EMISSIVE and finite(L[y, x])
                for j in range(3):
                    ok = ok and finite(plane1[y, x, j]) and finite(plane2[y, x, j])
                OK[y, x] = ok
        for y in range(H):
            for x in range(W):
                out[y, x, :3] = color[y, x, :3]
                if not OK[y, x]:
                    continue
                Np, Pp = plane1[y, x, :3], plane2[y, x, :3]
                m = F(sigma_plane) * plane1[y, x, 3]
                top = [F(-np.inf)] * 4
                k = 0
                for dy in range(-radius, radius + 1):
                    for dx in range(-radius, radius + 1):
                        qx, qy = x + dx, y + dy
                        if dx == 0 and dy == 0:
                            continue
                        if qx < 0 or qx >= W or qy < 0 or qy >= H or not OK[qy, qx]:
                            continue
                        if dot(Np, plane1[qy, qx, :3]) < F(normal_cos_min):
                            continue
                        g = dot(Np, [plane2[qy, qx, j] - Pp[j] for j in range(3)])
                        if not g * g <= m * m:
                            continue
                        if flags & SAME_PRIMITIVE and bits(plane0[qy, qx, 3:4])[0] != bits(plane0[y, x, 3:4])[0]:
                            continue
                        k += 1
                        v = L[qy, qx]
                        for j in range(4):
                            if v > top[j]:
                                v, top[j] = top[j], v
                if k < min_neighbors:
                    continue
                limit = F(factor) * top[rank - 1] + F(floor)
                if limit >= 0 and L[y, x] > limit:
                    s = limit / L[y, x]
                    for j in range(3):
                        out[y, x, j] = (Iv[y, x, j] * s) * Dv[y, x, j]
                    count += 1
    return out, count


# ---- inputs ---------------------------------------------------------------------------------------------
def make_case(width, height, seed):
    """denoise_model.make_inputs (misses, emissive, NaN, +-inf, id stripes, antiparallel normals) with isolated
    planted spikes: the colour times 64 where (7 x + 13 y) % 29 == 5 (no two of them within three pixels of each
    other) and at the centre pixel, so that the smallest images have one too."""
    color, p0, p1, p2 = dm.make_inputs(width, height, seed)
    color = color.copy()
    y, x = np.mgrid[0:height, 0:width]
    planted = ((7 * x + 13 * y) % 29 == 5) | ((x == width // 2) & (y == height // 2))
    with np.errstate(all="ignore"):
        color[planted, :3] = np.abs(color[planted, :3]) * SPIKE
    return color, p0, p1, p2


def flat_inputs(width, height, value=0.25):
    """One surface facing the camera: every pixel ok, the same id, normal and depth, grey albedo 0.5 and the colour
    `value` in every channel.  What the planted cases of tests/test_despike_rule.py are written into."""
    y, x = np.mgrid[0:height, 0:width]
    color = np.full((height, width, 4), value, dtype=F)
    color[..., 3] = 1
    p0 = np.full((height, width, 4), 0.5, dtype=F)
    p0[..., 3] = np.full((height, width), 7, dtype=U).view(F)
    p1 = np.zeros((height, width, 4), dtype=F)
    p1[..., 2] = 1
    p1[..., 3] = 4
    p2 = np.zeros((height, width, 4), dtype=F)
    p2[..., 0], p2[..., 1] = F(0.1) * x.astype(F), F(0.1) * y.astype(F)
    p2[..., 3] = np.full((height, width), HIT, dtype=U).view(F)
    return tuple(np.ascontiguousarray(a, dtype=F) for a in (color, p0, p1, p2))


def window_offers(width, height, radius):
    """The most taps a pixel's window has inside the image."""
    return min(2 * radius + 1, width) * min(2 * radius + 1, height) - 1
