"""The temporal reprojection rule of include/pt_hip.h restated in numpy float32, twice, and seeded inputs for it.

model()   whole-image arithmetic: one gather of the previous history per tap, the taps in the rule's order,
          every operation a separate float32 rounding (numpy never contracts)
scalar()  the same rule pixel by pixel with np.float32 scalars, written from the header independently of
          model(); tests/test_temporal_rule.py holds the two against each other word for word, and
          tests/test_gpu_temporal.py holds the device against model()

Images are height x width x 4 float32: colour (w ignored), the three feature planes (albedo + primitive
bits, normal + t, position + flag bits) and the three history planes ((I, n), (N, id bits), (P, t)).
A camera is a dict of float32 values: tan_half_fovy, aspect_ratio, origin, right, up, backward.
"""
import numpy as np

from denoise_model import F, U, HIT, EMISSIVE, bits, same_words   # noqa: F401  (same_words is reused by the tests)

DEMODULATE, SAME_PRIMITIVE = 1, 2
PARAMS = dict(alpha_min=0.1, max_history=6, sigma_plane=0.05, normal_cos_min=0.9)


# ---- cameras ----------------------------------------------------------------------------------------
def camera(position, look_at, fovy_degrees=60.0, aspect=1.2, up=(0.0, 1.0, 0.0)):
    """A pinhole camera in float32 (any orthonormal frame serves the rule; this one looks down -backward)."""
    p, a, u = (np.asarray(v, dtype=np.float64) for v in (position, look_at, up))
    b = p - a
    b /= np.linalg.norm(b)
    r = np.cross(u, b)
    r /= np.linalg.norm(r)
    return {"tan_half_fovy": F(np.tan(np.radians(fovy_degrees) / 2)), "aspect_ratio": F(aspect), "origin": p.astype(F),
            "right": r.astype(F), "up": np.cross(b, r).astype(F), "backward": b.astype(F)}


def camera_of(c):
    """The same dict from a pt_camera (ctypes)."""
    return {"tan_half_fovy": F(c.tan_half_fovy), "aspect_ratio": F(c.aspect_ratio),
            "origin": np.array(list(c.origin), dtype=F), "right": np.array(list(c.right), dtype=F),
            "up": np.array(list(c.up), dtype=F), "backward": np.array(list(c.backward), dtype=F)}


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _project(cam, P):
    e = (P - cam["origin"]).astype(F)
    z = -_dot(e, cam["backward"])
    hh = F(cam["tan_half_fovy"])
    hw = F(cam["aspect_ratio"]) * hh
    su = ((_dot(e, cam["right"]) / z) / hw) * F(0.5) + F(0.5)
    sv = ((_dot(e, cam["up"]) / z) / hh) * F(0.5) + F(0.5)
    return su, sv, z


def _finite3(a):
    with np.errstate(all="ignore"):
        x = a[..., :3].astype(F)
        return ((x - x) == 0).all(-1)


def ok_mask(color, plane1, plane2):
    return ((bits(plane2[..., 3]) & HIT) != 0) & _finite3(color) & _finite3(plane1) & _finite3(plane2)


# ---- the rule, whole image --------------------------------------------------------------------------
def model(color, plane0, plane1, plane2, cur, hist, prev, alpha_min, max_history, sigma_plane, normal_cos_min, flags,
          stats=None):
    """One step.  hist = (h0, h1, h2) or None.  Returns (image, h0, h1, h2).  `stats` (a dict) receives the
    counts tests/test_temporal_rule.py's vacuity conditions are about."""
    color, plane0, plane1, plane2 = (np.ascontiguousarray(a, dtype=F) for a in (color, plane0, plane1, plane2))
    Hh, Ww = color.shape[:2]
    C, A, ids = color[..., :3], plane0[..., :3], bits(plane0[..., 3])
    Nn, t, P = plane1[..., :3], plane1[..., 3], plane2[..., :3]
    ok = ok_mask(color, plane1, plane2)
    lo = F(1.0 / 64.0)
    D = np.where(A > lo, A, lo).astype(F) if flags & DEMODULATE else np.ones_like(A)
    mh = F(max_history)
    with np.errstate(all="ignore"):
        Icur = (C / D).astype(F)
        I, n = Icur, np.ones((Hh, Ww), dtype=F)
        counts = dict(hits=int(ok.sum()), have=0, taps4=0, taps13=0, taps0=0, outside=0, by_id=0, no_history=0,
                      by_normal=0, by_plane=0, not_finite=0)
        if hist is not None:
            h0, h1, h2 = (np.ascontiguousarray(a, dtype=F) for a in hist)
            yy, xx = np.mgrid[0:Hh, 0:Ww]
            W, H = F(Ww), F(Hh)
            su0, sv0, z0 = _project(cur, P)
            su1, sv1, z1 = _project(prev, P)
            fx = xx.astype(F) + (su1 - su0) * W
            fy = yy.astype(F) + (sv1 - sv0) * H
            reproj = (z0 > 0) & (z1 > 0) & (fx > F(-1)) & (fx < W) & (fy > F(-1)) & (fy < H)
            live = reproj & ok                                   # only these pixels' taps mean anything
            fxs, fys = np.where(live, fx, F(0)), np.where(live, fy, F(0))
            flx, fly = np.floor(fxs), np.floor(fys)
            ax, ay = fxs - flx, fys - fly
            x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
            m = F(sigma_plane) * t
            mm = m * m
            sumW = np.zeros((Hh, Ww), dtype=F)
            sumI = np.zeros((Hh, Ww, 3), dtype=F)
            nh = np.full((Hh, Ww), mh, dtype=F)
            taken = np.zeros((Hh, Ww), dtype=np.int64)
            for i, j in ((0, 0), (1, 0), (0, 1), (1, 1)):
                w = (ax if i else F(1) - ax) * (ay if j else F(1) - ay)
                qx, qy = x0 + i, y0 + j
                inside = (qx >= 0) & (qx < Ww) & (qy >= 0) & (qy < Hh)
                cx, cy = np.clip(qx, 0, Ww - 1), np.clip(qy, 0, Hh - 1)
                Iq, nq = h0[cy, cx, :3], h0[cy, cx, 3]
                Nq, idq, Pq = h1[cy, cx, :3], bits(h1[..., 3])[cy, cx], h2[cy, cx, :3]
                g = _dot(Nn, (Pq - P).astype(F))
                reasons = [("weight", ~(w > 0)), ("outside", ~inside), ("no_history", nq < F(1)), ("not_finite", ~_finite3(Iq)),
                           ("by_id", (idq != ids) if flags & SAME_PRIMITIVE else np.zeros((Hh, Ww), dtype=bool)),
                           ("by_normal", _dot(Nn, Nq) < F(normal_cos_min)), ("by_plane", ~(g * g <= mm))]
                skip = np.zeros((Hh, Ww), dtype=bool)
                for name, r in reasons:                          # the first reason of the rule's list that holds
                    if name in counts:
                        counts[name] += int((live & ~skip & r).sum())
                    skip |= r
                sumW = np.where(skip, sumW, sumW + w)
                sumI = np.where(skip[..., None], sumI, sumI + w[..., None] * Iq)
                nh = np.where(skip, nh, np.where(nq < nh, nq, nh))
                taken += (live & ~skip)
            have = live & (sumW >= lo)
            Hc = sumI / sumW[..., None]
            nn = nh + F(1)
            nn = np.where(nn < mh, nn, mh)
            a = F(1) / nn
            a = np.where(a > F(alpha_min), a, F(alpha_min))
            I = np.where(have[..., None], Hc + a[..., None] * (Icur - Hc), Icur).astype(F)
            n = np.where(have, nn, F(1)).astype(F)
            counts.update(have=int(have.sum()), taps4=int((live & (taken == 4)).sum()),
                          taps13=int((live & (taken >= 1) & (taken <= 3)).sum()), taps0=int((ok & (taken == 0)).sum()))
        if stats is not None:
            stats.update(counts)
        image = np.zeros((Hh, Ww, 4), dtype=F)
        image[..., :3] = np.where(ok[..., None], I * D, C)
        image[..., 3] = np.where(ok, n, F(0))
        o0 = np.zeros((Hh, Ww, 4), dtype=F)
        o0[..., :3] = np.where(ok[..., None], I, C)
        o0[..., 3] = image[..., 3]
    o1 = np.concatenate([Nn, plane0[..., 3:4]], -1).astype(F)
    o2 = np.concatenate([P, t[..., None]], -1).astype(F)
    return image, o0, o1, o2


# ---- the rule, pixel by pixel -----------------------------------------------------------------------
def scalar(color, plane0, plane1, plane2, cur, hist, prev, alpha_min, max_history, sigma_plane, normal_cos_min, flags):
    """The rule pixel by pixel (small images only)."""
    color, plane0, plane1, plane2 = (np.ascontiguousarray(a, dtype=F) for a in (color, plane0, plane1, plane2))
    Hh, Ww = color.shape[:2]
    one, half, lo = F(1), F(0.5), F(1.0 / 64.0)
    W, H, mh = F(Ww), F(Hh), F(max_history)
    image, o0 = np.zeros((Hh, Ww, 4), dtype=F), np.zeros((Hh, Ww, 4), dtype=F)
    o1, o2 = np.zeros((Hh, Ww, 4), dtype=F), np.zeros((Hh, Ww, 4), dtype=F)

    def finite(x):
        return (x - x) == 0

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

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
                        ok = ok and bool(finite(v[k]))
                if not ok:
                    image[y, x, :3] = o0[y, x, :3] = c
                    continue
                D = [one, one, one]
                if flags & DEMODULATE:
                    D = [plane0[y, x, k] if plane0[y, x, k] > lo else lo for k in range(3)]
                Icur = [c[k] / D[k] for k in range(3)]
                I, n = Icur, one
                if hist is not None:
                    h0, h1, h2 = hist
                    su0, sv0, z0 = project(cur, Pp)
                    su1, sv1, z1 = project(prev, Pp)
                    fx = F(x) + (su1 - su0) * W
                    fy = F(y) + (sv1 - sv0) * H
                    if z0 > 0 and z1 > 0 and fx > -one and fx < W and fy > -one and fy < H:
                        flx, fly = np.floor(fx), np.floor(fy)
                        ax, ay = fx - flx, fy - fly
                        x0, y0 = int(flx), int(fly)
                        m = F(sigma_plane) * tp
                        sumW, sumI, nh = F(0), [F(0), F(0), F(0)], mh
                        for j in (0, 1):
                            for i in (0, 1):
                                w = (ax if i else one - ax) * (ay if j else one - ay)
                                qx, qy = x0 + i, y0 + j
                                if not w > 0 or qx < 0 or qx >= Ww or qy < 0 or qy >= Hh:
                                    continue
                                Iq, nq = h0[qy, qx, :3], F(h0[qy, qx, 3])
                                if nq < one or not all(bool(finite(F(v))) for v in Iq):
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
                                nh = nq if nq < nh else nh
                        if sumW >= lo:
                            Hc = [sumI[k] / sumW for k in range(3)]
                            n = nh + one
                            n = n if n < mh else mh
                            a = one / n
                            a = a if a > F(alpha_min) else F(alpha_min)
                            I = [Hc[k] + a * (Icur[k] - Hc[k]) for k in range(3)]
                for k in range(3):
                    image[y, x, k] = I[k] * D[k]
                    o0[y, x, k] = I[k]
                image[y, x, 3] = o0[y, x, 3] = n
    return image, o0, o1, o2


# ---- seeded inputs ----------------------------------------------------------------------------------
WIDTH, HEIGHT = 48, 40


def cameras(aspect=1.2):
    """Three cameras moving to the right past the slab: the wall behind its left edge comes into view."""
    return [camera((0.3 * k, 1.0, 2.0), (0.1 * k, 0.8, -3.0), 60.0, aspect) for k in range(3)]


def camera_behind():
    """Behind the back wall, looking away from the scene: every point of it has z1 <= 0."""
    return camera((0.0, 1.0, -8.0), (0.0, 1.0, -12.0))


def make_frame(width, height, cam, seed, frame=0):
    """One frame of the analytic scene -- floor y = 0 (|x| < 6), back wall z = -6 (0 <= y < 4), slab z = -3
    (|x| < 0.8, 0 <= y < 1.6), the slab's top third emissive -- seen through `cam`: every pixel's ray goes
    through a jittered point of the pixel (the jitter is seeded by `seed` alone: the same in every frame),
    the planes hold its closest hit in float32, the colour is albedo x a smooth irradiance plus noise seeded
    by (seed, frame).  Then the special pixels of denoise_model.make_inputs, by position: albedo 0 and below
    1/64, NaN, +inf and -inf colours and a NaN normal.  Returns (color, plane0, plane1, plane2)."""
    Hh, Ww = height, width
    jit = np.random.default_rng(seed).random((Hh, Ww, 2))
    rng = np.random.default_rng([seed, frame])
    y, x = np.mgrid[0:Hh, 0:Ww]
    o = cam["origin"].astype(np.float64)
    hh = float(cam["tan_half_fovy"])
    hw = float(cam["aspect_ratio"]) * hh
    sx = ((x + jit[..., 0]) / Ww * 2 - 1) * hw
    sy = ((y + jit[..., 1]) / Hh * 2 - 1) * hh
    d = (sx[..., None] * cam["right"].astype(np.float64) + sy[..., None] * cam["up"].astype(np.float64)
         - cam["backward"].astype(np.float64))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    best = np.full((Hh, Ww), np.inf)
    ident = np.full((Hh, Ww), 0xffffffff, dtype=U)
    nrm = np.zeros((Hh, Ww, 3))
    surfaces = [(0, 1, 0.0, (0, 1, 0), lambda p: np.abs(p[..., 0]) < 6),
                (1, 2, -6.0, (0, 0, 1), lambda p: (p[..., 1] >= 0) & (p[..., 1] < 4)),
                (2, 2, -3.0, (0, 0, 1), lambda p: (np.abs(p[..., 0]) < 0.8) & (p[..., 1] >= 0) & (p[..., 1] < 1.6))]
    with np.errstate(all="ignore"):
        for sid, axis, value, normal, within in surfaces:
            tt = (value - o[axis]) / d[..., axis]
            p = o + tt[..., None] * d
            hit = (tt > 1e-4) & (tt < best) & within(p)
            best = np.where(hit, tt, best)
            ident[hit] = sid
            nrm[hit] = normal
    hit = np.isfinite(best)
    t = np.where(hit, best, 0).astype(F)
    pos = np.where(hit[..., None], o + np.where(hit, best, 0)[..., None] * d, 0).astype(F)
    nrm = nrm.astype(F)
    base = np.array([[0.7, 0.6, 0.5], [0.3, 0.5, 0.8], [0.8, 0.3, 0.2]], dtype=F)
    alb = np.where(hit[..., None], base[np.minimum(ident, 2)], 0).astype(F)
    alb = (alb * (F(0.8) + F(0.2) * np.sin(pos[..., 0:1] * F(3)) * np.cos(pos[..., 1:2] * F(2) + pos[..., 2:3]))).astype(F)
    alb[(x % 11 == 3) & (y % 7 == 2) & hit] = F(0)
    alb[(x % 11 == 5) & (y % 7 == 4) & hit] = F(1.0 / 128.0)
    signal = (F(0.6) + F(0.3) * np.sin(pos[..., 0] * F(1.5)) * np.cos(pos[..., 2] * F(0.7))).astype(F)
    col = (alb * (signal[..., None] + rng.normal(0, 0.15, (Hh, Ww, 3)).astype(F))).astype(F)
    flags = np.where(hit, HIT, 0).astype(U)
    emissive = hit & (ident == 2) & (pos[..., 1] > F(1.1))
    flags[emissive] |= EMISSIVE
    col[emissive] = F(4.0)
    col[~hit] = F(0.05)
    col[(x % 13 == 6) & (y % 9 == 3)] = F(np.nan)
    col[(x % 13 == 8) & (y % 9 == 5), 1] = F(np.inf)
    col[(x % 13 == 10) & (y % 9 == 7), 2] = F(-np.inf)
    nrm[(x % 17 == 9) & (y % 10 == 6) & hit, 0] = F(np.nan)
    color = np.concatenate([col, np.ones((Hh, Ww, 1), dtype=F)], -1)
    plane0 = np.concatenate([alb, ident.view(F)[..., None]], -1)
    plane1 = np.concatenate([nrm, t[..., None]], -1)
    plane2 = np.concatenate([pos, flags.view(F)[..., None]], -1)
    return tuple(np.ascontiguousarray(a, dtype=F) for a in (color, plane0, plane1, plane2))


def make_sequence(width=WIDTH, height=HEIGHT, seed=1):
    """[(camera, (color, plane0, plane1, plane2))] for the three cameras, at the image's own aspect ratio."""
    cams = cameras(width / height)
    return [(c, make_frame(width, height, c, seed, k)) for k, c in enumerate(cams)]


def run_sequence(step, seq, flags, params=None, stats=None):
    """Chain `step` (model, scalar, or a device call of the same signature) over a sequence; returns every
    frame's (image, h0, h1, h2)."""
    p = dict(PARAMS if params is None else params)
    outs, hist, prev = [], None, None
    for k, (cam, frame) in enumerate(seq):
        kw = {}
        if stats is not None:
            stats.append({})
            kw["stats"] = stats[-1]
        out = step(*frame, cam, hist, prev if prev is not None else cam, p["alpha_min"], p["max_history"], p["sigma_plane"],
                   p["normal_cos_min"], flags, **kw)
        outs.append(out)
        hist, prev = out[1:], cam
    return outs
