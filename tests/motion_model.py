"""Rule 7 of include/pt_hip.h -- the temporal step (and the step with moments) across a scene whose objects moved --
restated in numpy float32, twice, pth_motion_table (include/pt_host.h) restated in float64, and a seeded analytic
sequence with moving objects.

model()        whole-image arithmetic, every operation a separate float32 rounding
scalar()       the same rule pixel by pixel with np.float32 scalars, written from the header independently of model()
table_model()  the per-object maps from two sets of world->object rows, float64 operation by operation

tests/test_motion_rule.py holds model() against scalar() word for word and both against temporal_model / svgf_model
under an identity table; tests/test_gpu_motion.py holds the device against model().

Images are height x width x 4 float32 as in temporal_model; a motion table is (rows, prev_index): count x 3 x 4
float32 and count uint32, one entry per primitive of the current scene; NONE = "was not there".
"""
import numpy as np

import svgf_model as sm
import temporal_model as tm
from denoise_model import F, U, HIT, EMISSIVE, bits, same_words   # noqa: F401

DEMODULATE, SAME_PRIMITIVE = 1, 2
NONE = U(0xffffffff)
PARAMS = dict(tm.PARAMS)


def identity_table(count):
    rows = np.zeros((count, 3, 4), dtype=F)
    rows[:, 0, 0] = rows[:, 1, 1] = rows[:, 2, 2] = F(1)
    return rows, np.arange(count, dtype=U)


# ---- pth_motion_table, float64 ------------------------------------------------------------------------
def table_model(prev_rows, cur_rows):
    """prev_rows, cur_rows: count x 3 x 4 float32 world->object rows [A | b] of the same objects in two scenes.
    Returns (rows float32 count x 3 x 4, valid bool count) in pt_host.h's operation order."""
    a = np.asarray(prev_rows, dtype=F).astype(np.float64).reshape(-1, 3, 4)
    c = np.asarray(cur_rows, dtype=F).astype(np.float64).reshape(-1, 3, 4)
    n = a.shape[0]
    out = np.zeros((n, 3, 4), dtype=F)
    with np.errstate(all="ignore"):
        def A(r, k):
            return a[:, r, k]
        co = [[A(1, 1) * A(2, 2) - A(1, 2) * A(2, 1), A(1, 2) * A(2, 0) - A(1, 0) * A(2, 2), A(1, 0) * A(2, 1) - A(1, 1) * A(2, 0)],
              [A(0, 2) * A(2, 1) - A(0, 1) * A(2, 2), A(0, 0) * A(2, 2) - A(0, 2) * A(2, 0), A(0, 1) * A(2, 0) - A(0, 0) * A(2, 1)],
              [A(0, 1) * A(1, 2) - A(0, 2) * A(1, 1), A(0, 2) * A(1, 0) - A(0, 0) * A(1, 2), A(0, 0) * A(1, 1) - A(0, 1) * A(1, 0)]]
        det = (A(0, 0) * co[0][0] + A(0, 1) * co[0][1]) + A(0, 2) * co[0][2]
        inv = [[co[k][r] / det for k in range(3)] for r in range(3)]
        d = [c[:, k, 3] - a[:, k, 3] for k in range(3)]
        for r in range(3):
            for k in range(3):
                out[:, r, k] = ((inv[r][0] * c[:, 0, k] + inv[r][1] * c[:, 1, k]) + inv[r][2] * c[:, 2, k]).astype(F)
            out[:, r, 3] = ((inv[r][0] * d[0] + inv[r][1] * d[1]) + inv[r][2] * d[2]).astype(F)
    return out, np.isfinite(out).all(axis=(1, 2))


# ---- the rule, whole image --------------------------------------------------------------------------
def model(color, plane0, plane1, plane2, cur, hist, prev, rows, prev_index, alpha_min, max_history, sigma_plane,
          normal_cos_min, flags, min_temporal=None, stats=None):
    """One step under rule 7.  hist = (h0, h1, h2) or None: returns (image, h0, h1, h2).  With min_temporal given the
    step carries moments: hist = (h0, h1, h2, h3) or None, returns (image, h0, h1, h2, h3, variance).  `stats` (a
    dict) receives the counts tests/test_motion_rule.py's vacuity conditions are about."""
    moments = min_temporal is not None
    color, plane0, plane1, plane2 = (np.ascontiguousarray(a, dtype=F) for a in (color, plane0, plane1, plane2))
    rows = np.ascontiguousarray(rows, dtype=F).reshape(-1, 3, 4)
    prev_index = np.ascontiguousarray(prev_index, dtype=U)
    Hh, Ww = color.shape[:2]
    C, A, ids = color[..., :3], plane0[..., :3], bits(plane0[..., 3])
    Nn, t, P = plane1[..., :3], plane1[..., 3], plane2[..., :3]
    ok = tm.ok_mask(color, plane1, plane2)
    lo = F(1.0 / 64.0)
    D = np.where(A > lo, A, lo).astype(F) if flags & DEMODULATE else np.ones_like(A)
    mh = F(max_history)
    counts = dict(normal_differs=0, plane_differs=0, id_differs=0, appearing=0, leaves=0, have=0, unknown_id=0)
    with np.errstate(all="ignore"):
        Icur = (C / D).astype(F)
        l = sm.lum(Icur)
        q = l * l
        I, n, m1, m2 = Icur, np.ones((Hh, Ww), dtype=F), l, q
        if hist is not None:
            hs = [np.ascontiguousarray(a, dtype=F) for a in hist]
            h0, h1, h2 = hs[:3]
            h3 = hs[3] if moments else np.zeros_like(h0)
            known = ids < U(prev_index.size)
            ci = np.where(known, ids, U(0)).astype(np.int64)                 # clamped before the load
            T = rows[ci]
            pid = np.where(known, prev_index[ci], NONE)
            Pm = np.stack([((T[..., r, 0] * P[..., 0] + T[..., r, 1] * P[..., 1]) + T[..., r, 2] * P[..., 2]) + T[..., r, 3]
                           for r in range(3)], -1).astype(F)
            Nm = np.stack([(T[..., r, 0] * Nn[..., 0] + T[..., r, 1] * Nn[..., 1]) + T[..., r, 2] * Nn[..., 2]
                           for r in range(3)], -1).astype(F)
            yy, xx = np.mgrid[0:Hh, 0:Ww]
            W, H = F(Ww), F(Hh)
            su0, sv0, z0 = tm._project(cur, P)
            su1, sv1, z1 = tm._project(prev, Pm)
            fx = xx.astype(F) + (su1 - su0) * W
            fy = yy.astype(F) + (sv1 - sv0) * H
            inside_image = (fx > F(-1)) & (fx < W) & (fy > F(-1)) & (fy < H)
            reproj = (z0 > 0) & (z1 > 0) & inside_image & (pid != NONE)
            live = reproj & ok
            counts["appearing"] = int((ok & known & (pid == NONE)).sum())
            counts["unknown_id"] = int((ok & ~known).sum())
            counts["leaves"] = int((ok & (pid != NONE) & (z0 > 0) & (z1 > 0) & ~inside_image).sum())
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
            dn, dp, di = (np.zeros((Hh, Ww), dtype=bool) for _ in range(3))
            for i, j in ((0, 0), (1, 0), (0, 1), (1, 1)):
                w = (ax if i else F(1) - ax) * (ay if j else F(1) - ay)
                qx, qy = x0 + i, y0 + j
                inside = (qx >= 0) & (qx < Ww) & (qy >= 0) & (qy < Hh)
                cx, cy = np.clip(qx, 0, Ww - 1), np.clip(qy, 0, Hh - 1)
                Iq, nq = h0[cy, cx, :3], h0[cy, cx, 3]
                Nq, idq, Pq = h1[cy, cx, :3], bits(h1[..., 3])[cy, cx], h2[cy, cx, :3]
                g = tm._dot(Nm, (Pq - Pm).astype(F))
                by_normal = tm._dot(Nm, Nq) < F(normal_cos_min)
                by_plane = ~(g * g <= mm)
                by_id = idq != pid
                skip = ~(w > 0) | ~inside | (nq < F(1)) | ~tm._finite3(Iq) | by_normal | by_plane
                if flags & SAME_PRIMITIVE:
                    skip = skip | by_id
                # what the camera-only rule would have said of the same tap, for the vacuity counts
                tap = live & (w > 0) & inside & (nq >= F(1))
                g3 = tm._dot(Nm, (Pq - P).astype(F))
                dn |= tap & (by_normal != (tm._dot(Nn, Nq) < F(normal_cos_min)))
                dp |= tap & (by_plane != ~(g3 * g3 <= mm))
                di |= tap & (by_id != (idq != ids))
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
            counts.update(normal_differs=int(dn.sum()), plane_differs=int(dp.sum()), id_differs=int(di.sum()),
                          have=int(have.sum()))
        restart = ~(sm._finite(m1) & sm._finite(m2))
        m1, m2 = np.where(restart, l, m1).astype(F), np.where(restart, q, m2).astype(F)
        v = sm._clamp0(m2 - m1 * m1)
        image = np.zeros((Hh, Ww, 4), dtype=F)
        image[..., :3] = np.where(ok[..., None], I * D, C)
        image[..., 3] = np.where(ok, n, F(0))
        o0 = np.zeros((Hh, Ww, 4), dtype=F)
        o0[..., :3] = np.where(ok[..., None], I, C)
        o0[..., 3] = image[..., 3]
        o3 = np.zeros((Hh, Ww, 4), dtype=F)
        o3[..., 0], o3[..., 1] = np.where(ok, m1, F(0)), np.where(ok, m2, F(0))
        o3[..., 2] = np.where(ok, v, F(-1))
    o1 = np.concatenate([Nn, plane0[..., 3:4]], -1).astype(F)          # the current scene's words
    o2 = np.concatenate([P, t[..., None]], -1).astype(F)
    if stats is not None:
        stats.update(counts)
    if not moments:
        return image, o0, o1, o2
    return image, o0, o1, o2, o3, sm.variance_model(o0, o1, o2, o3, sigma_plane, normal_cos_min, flags, min_temporal)


# ---- the rule, pixel by pixel -----------------------------------------------------------------------
def scalar(color, plane0, plane1, plane2, cur, hist, prev, rows, prev_index, alpha_min, max_history, sigma_plane,
           normal_cos_min, flags, min_temporal=None):
    """The rule pixel by pixel (small images only); the variance estimate, which rule 7 does not change, is
    svgf_model.scalar's and is taken from there by the tests."""
    moments = min_temporal is not None
    color, plane0, plane1, plane2 = (np.ascontiguousarray(a, dtype=F) for a in (color, plane0, plane1, plane2))
    table = np.ascontiguousarray(rows, dtype=F).reshape(-1, 12)
    prev_index = np.ascontiguousarray(prev_index, dtype=U)
    count = int(prev_index.size)
    Hh, Ww = color.shape[:2]
    one, half, lo, zero = F(1), F(0.5), F(1.0 / 64.0), F(0)
    W, H, mh = F(Ww), F(Hh), F(max_history)
    image, o0, o1, o2, o3 = (np.zeros((Hh, Ww, 4), dtype=F) for _ in range(5))

    def finite(x):
        return bool((x - x) == 0)

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
                        ok = ok and finite(v[k])
                if not ok:
                    image[y, x, :3] = o0[y, x, :3] = c
                    o3[y, x, 2] = F(-1)
                    continue
                D = [one, one, one]
                if flags & DEMODULATE:
                    D = [plane0[y, x, k] if plane0[y, x, k] > lo else lo for k in range(3)]
                Icur = [c[k] / D[k] for k in range(3)]
                l = (F(0.2126) * Icur[0] + F(0.7152) * Icur[1]) + F(0.0722) * Icur[2]
                q = l * l
                I, n, m1, m2 = Icur, one, l, q
                if hist is not None:
                    h0, h1, h2 = hist[:3]
                    i = int(bits(plane0[y, x, 3:4])[0])
                    pid = int(prev_index[i]) if i < count else int(NONE)
                    Tr = table[i if i < count else 0]
                    Pm = [((Tr[4 * r] * Pp[0] + Tr[4 * r + 1] * Pp[1]) + Tr[4 * r + 2] * Pp[2]) + Tr[4 * r + 3] for r in range(3)]
                    Nm = [(Tr[4 * r] * Np[0] + Tr[4 * r + 1] * Np[1]) + Tr[4 * r + 2] * Np[2] for r in range(3)]
                    su0, sv0, z0 = project(cur, Pp)
                    su1, sv1, z1 = project(prev, Pm)
                    fx = F(x) + (su1 - su0) * W
                    fy = F(y) + (sv1 - sv0) * H
                    if z0 > 0 and z1 > 0 and fx > -one and fx < W and fy > -one and fy < H and pid != int(NONE):
                        flx, fly = np.floor(fx), np.floor(fy)
                        ax, ay = fx - flx, fy - fly
                        x0, y0 = int(flx), int(fly)
                        m = F(sigma_plane) * tp
                        sumW, sumI, nh, sM1, sM2 = zero, [zero, zero, zero], mh, zero, zero
                        for jj in (0, 1):
                            for ii in (0, 1):
                                w = (ax if ii else one - ax) * (ay if jj else one - ay)
                                qx, qy = x0 + ii, y0 + jj
                                if not w > 0 or qx < 0 or qx >= Ww or qy < 0 or qy >= Hh:
                                    continue
                                Iq, nq = h0[qy, qx, :3], F(h0[qy, qx, 3])
                                if nq < one or not all(finite(F(v)) for v in Iq):
                                    continue
                                if flags & SAME_PRIMITIVE and int(bits(h1[qy, qx, 3:4])[0]) != pid:
                                    continue
                                if dot(Nm, h1[qy, qx, :3]) < F(normal_cos_min):
                                    continue
                                g = dot(Nm, [F(h2[qy, qx, k]) - Pm[k] for k in range(3)])
                                if not g * g <= m * m:
                                    continue
                                sumW = sumW + w
                                sumI = [sumI[k] + w * F(Iq[k]) for k in range(3)]
                                if moments:
                                    sM1 = sM1 + w * F(hist[3][qy, qx, 0])
                                    sM2 = sM2 + w * F(hist[3][qy, qx, 1])
                                nh = nq if nq < nh else nh
                        if sumW >= lo:
                            Hc = [sumI[k] / sumW for k in range(3)]
                            n = nh + one
                            n = n if n < mh else mh
                            a = one / n
                            a = a if a > F(alpha_min) else F(alpha_min)
                            I = [Hc[k] + a * (Icur[k] - Hc[k]) for k in range(3)]
                            if moments:
                                Hm1, Hm2 = sM1 / sumW, sM2 / sumW
                                m1 = Hm1 + a * (l - Hm1)
                                m2 = Hm2 + a * (q - Hm2)
                if not (finite(m1) and finite(m2)):
                    m1, m2 = l, q
                for k in range(3):
                    image[y, x, k] = I[k] * D[k]
                    o0[y, x, k] = I[k]
                image[y, x, 3] = o0[y, x, 3] = n
                d = m2 - m1 * m1
                o3[y, x, 0], o3[y, x, 1], o3[y, x, 2] = m1, m2, (d if (d > 0 and finite(d)) else zero)
    if not moments:
        return image, o0, o1, o2
    return image, o0, o1, o2, o3


# ---- the seeded sequence ------------------------------------------------------------------------------
WIDTH, HEIGHT = tm.WIDTH, tm.HEIGHT
FRAMES = 5
GROUND, STILL, TRANSLATING, ROTATING, APPEARING = range(5)      # the objects, by their index in frames 0 .. 3
APPEARS_IN = 3
PERMUTATION = (3, 0, 4, 1, 2)     # frame 4: object k is primitive PERMUTATION[k]


def _rot_y(deg):
    a = np.radians(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def _rot_x(deg):
    a = np.radians(deg)
    return np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])


def objects(frame):
    """The scene of a frame: per object (shape, size, R, centre) -- object space -> world is R p + centre; a quad
    lies in its z = 0 plane with half sizes `size` and normal +z, a sphere has radius `size`."""
    k = frame
    out = [("quad", (6.0, 6.0), _rot_x(-90.0), np.array([0.0, 0.0, -3.0])),                      # the ground, normal +y
           ("sphere", 0.7, np.eye(3), np.array([-2.1, 0.7, -3.6])),                               # still
           ("quad", (0.6, 0.7), np.eye(3), np.array([-0.9 + 0.3 * k, 0.8, -3.4 + 0.3 * k])),     # translates, also towards the eye
           ("quad", (0.8, 0.8), _rot_y(-60.0 + 30.0 * k), np.array([1.7, 0.9, -3.4]))]           # rotates about its own y axis
    if k >= APPEARS_IN:
        out.append(("sphere", 0.5, np.eye(3), np.array([0.3, 0.5, -1.6])))
    return out


def inv_rows(objs):
    """World -> object rows [R^T | -R^T c] in float32, as a scene's primitives carry them."""
    return np.stack([np.concatenate([R.T, -(R.T @ c)[:, None]], 1) for _, _, R, c in objs]).astype(F)


def order(frame):
    """Primitive index of every object of the frame."""
    n = len(objects(frame))
    return list(PERMUTATION[:n]) if frame == FRAMES - 1 else list(range(n))


def table(frame):
    """The motion table of `frame` against frame - 1, per primitive of `frame`: (rows, prev_index).  The maps are
    table_model's of the float32 rows; the appearing object has no previous index in the frame it appears in."""
    cur, prv = objects(frame), objects(frame - 1)
    rc = inv_rows(cur)
    rp = np.concatenate([inv_rows(prv), rc[len(prv):]])               # (a new object's own rows: the entry is not used)
    t, valid = table_model(rp, rc)
    assert valid.all()
    oc, op = order(frame), order(frame - 1)
    rows = np.zeros((len(cur), 3, 4), dtype=F)
    prev_index = np.full(len(cur), NONE, dtype=U)
    for k in range(len(cur)):
        rows[oc[k]] = t[k]
        if k < len(prv):
            prev_index[oc[k]] = op[k]
    return rows, prev_index


def cameras(aspect=1.2):
    """An orbit about the objects, 5 degrees a frame."""
    out = []
    for k in range(FRAMES):
        a = np.radians(-10.0 + 5.0 * k)
        out.append(tm.camera((5.2 * np.sin(a), 1.4, -3.2 + 5.2 * np.cos(a)), (0.0, 0.7, -3.2), 60.0, aspect))
    return out


def make_frame(width, height, cam, seed, frame):
    """One frame, in temporal_model.make_frame's style: a jittered ray per pixel (the jitter seeded by `seed` alone),
    its closest hit among the frame's objects in float32 planes, colour = albedo x a smooth irradiance + noise seeded
    by (seed, frame), the still sphere's top emissive, and the same special pixels by position."""
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
    obj = np.full((Hh, Ww), -1, dtype=np.int64)
    nrm = np.zeros((Hh, Ww, 3))
    prim = order(frame)
    with np.errstate(all="ignore"):
        for k, (shape, size, R, c) in enumerate(objects(frame)):
            oo, dd = (o - c) @ R, d @ R                                  # R^T (o - c), R^T d
            if shape == "quad":
                tt = -oo[2] / dd[..., 2]
                p = oo + tt[..., None] * dd
                hit = (np.abs(p[..., 0]) < size[0]) & (np.abs(p[..., 1]) < size[1])
                nl = np.broadcast_to(np.array([0.0, 0.0, 1.0]), p.shape)
            else:
                b = dd @ oo
                disc = b * b - (oo @ oo - size * size)
                tt = -b - np.sqrt(disc)
                p = oo + tt[..., None] * dd
                hit = disc > 0
                nl = p / size
            hit = hit & (tt > 1e-4) & (tt < best)
            best = np.where(hit, tt, best)
            ident[hit] = prim[k]
            obj[hit] = k
            nrm[hit] = (nl @ R.T)[hit]
    hit = np.isfinite(best)
    t = np.where(hit, best, 0).astype(F)
    pos = np.where(hit[..., None], o + np.where(hit, best, 0)[..., None] * d, 0).astype(F)
    nrm = nrm.astype(F)
    base = np.array([[0.7, 0.6, 0.5], [0.3, 0.5, 0.8], [0.8, 0.3, 0.2], [0.3, 0.7, 0.3], [0.7, 0.7, 0.2]], dtype=F)
    alb = np.where(hit[..., None], base[np.maximum(obj, 0)], 0).astype(F)
    alb = (alb * (F(0.8) + F(0.2) * np.sin(pos[..., 0:1] * F(3)) * np.cos(pos[..., 1:2] * F(2) + pos[..., 2:3]))).astype(F)
    alb[(x % 11 == 3) & (y % 7 == 2) & hit] = F(0)
    alb[(x % 11 == 5) & (y % 7 == 4) & hit] = F(1.0 / 128.0)
    signal = (F(0.6) + F(0.3) * np.sin(pos[..., 0] * F(1.5)) * np.cos(pos[..., 2] * F(0.7))).astype(F)
    col = (alb * (signal[..., None] + rng.normal(0, 0.15, (Hh, Ww, 3)).astype(F))).astype(F)
    flags = np.where(hit, HIT, 0).astype(U)
    emissive = hit & (obj == STILL) & (pos[..., 1] > F(1.1))
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
    """[(camera, (color, plane0, plane1, plane2), (rows, prev_index))] for the five frames; frame 0's table is the
    identity (no history is held then, so nothing reads it)."""
    cams = cameras(width / height)
    out = []
    for k, c in enumerate(cams):
        tab = table(k) if k else identity_table(len(objects(0)))
        out.append((c, make_frame(width, height, c, seed, k), tab))
    return out


def object_mask(frame_planes, frame, obj):
    """The pixels of a frame that hit object `obj`."""
    return bits(frame_planes[1][..., 3]) == U(order(frame)[obj])


def run_sequence(step, seq, flags, params=None, min_temporal=None, stats=None):
    """Chain `step` (model, scalar, or a device call of the same signature) over a sequence; returns every frame's
    outputs."""
    p = dict(PARAMS if params is None else params)
    outs, hist, prev = [], None, None
    for cam, frame, (rows, prev_index) in seq:
        kw = {}
        if stats is not None:
            stats.append({})
            kw["stats"] = stats[-1]
        if min_temporal is not None:
            kw["min_temporal"] = min_temporal
        out = step(*frame, cam, hist, prev if prev is not None else cam, rows, prev_index, p["alpha_min"], p["max_history"],
                   p["sigma_plane"], p["normal_cos_min"], flags, **kw)
        outs.append(out)
        hist, prev = out[1:5] if min_temporal is not None else out[1:4], cam
    return outs
