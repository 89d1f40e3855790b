// Temporal reprojection (pt_temporal, pt_temporal_image; the rule is written out in include/pt_hip.h and
// restated in tests/temporal_model.py), and the same step across a scene whose objects moved (rule 7:
// pt_temporal_motion_image, pt_temporal after pt_set_scene_moved; tests/motion_model.py).  Part of the trace kernel's single translation unit: included by
// pt_kernels.hip inside its anonymous namespace after pt_dev_denoise.h; not a standalone header.
// Nothing here is used by trace_kernel, and no existing kernel or parameter struct changes.
#pragma once

// One step.  The previous history (ph0..2, null when there is none) is only read, the new one (h0..2) and
// the image only written: the caller alternates two history sets, so this frame's planes become the next
// frame's "previous" without a copy.  Its own argument struct, as the feature pass.
struct TemporalArgs {
    const float4* color;        // C
    const float4* plane0;       // (A, id)
    const float4* plane1;       // (N, t)
    const float4* plane2;       // (P, flags)
    const float4* ph0;          // previous (I, n), or null
    const float4* ph1;          // previous (N, id)
    const float4* ph2;          // previous (P, t)
    float4* image;              // (I * D, n)
    float4* h0;
    float4* h1;
    float4* h2;
    uint32_t width, height;
    float alphaMin, maxHistory, sigmaPlane, normalCosMin;
    uint32_t flags;
    pt_camera cur, prev;
};

struct TpProjection {
    float su, sv, z;
};

// project(cam, P) of the rule, in its operation order
PT_DEV TpProjection tp_project(const pt_camera& cam, float px, float py, float pz)
{
    const float ex = px - cam.origin[0], ey = py - cam.origin[1], ez = pz - cam.origin[2];
    const float z = -((ex * cam.backward[0] + ey * cam.backward[1]) + ez * cam.backward[2]);
    const float hh = cam.tan_half_fovy;
    const float hw = cam.aspect_ratio * hh;
    const float r = (ex * cam.right[0] + ey * cam.right[1]) + ez * cam.right[2];
    const float u = (ex * cam.up[0] + ey * cam.up[1]) + ez * cam.up[2];
    TpProjection o;
    o.su = ((r / z) / hw) * 0.5f + 0.5f;
    o.sv = ((u / z) / hh) * 0.5f + 0.5f;
    o.z = z;
    return o;
}

// A workgroup of 256 lanes takes the denoiser's tile of 32 x 8 pixels, one pixel per lane: 64 B read and
// 64 B written per pixel in float4 rows a wave reads whole, and up to four taps of 48 B that neighbouring
// lanes share (a tile's taps are a shifted tile: the caches serve them, so nothing is staged in LDS).
__global__ void __launch_bounds__(256) temporal_kernel(TemporalArgs A)
{
    const uint32_t lx = threadIdx.x & (kDnTileW - 1u), ly = threadIdx.x / kDnTileW;
    const uint32_t x = blockIdx.x * kDnTileW + lx, y = blockIdx.y * kDnTileH + ly;
    if (x >= A.width || y >= A.height) return;
    const size_t pi = (size_t)y * A.width + x;
    const float4 c = A.color[pi], a = A.plane0[pi], n4 = A.plane1[pi], p4 = A.plane2[pi];
    A.h1[pi] = make_float4(n4.x, n4.y, n4.z, a.w);
    A.h2[pi] = make_float4(p4.x, p4.y, p4.z, n4.w);
    const bool ok = (__float_as_uint(p4.w) & PT_FEATURE_HIT) && dn_finite(c.x) && dn_finite(c.y) && dn_finite(c.z) &&
                    dn_finite(n4.x) && dn_finite(n4.y) && dn_finite(n4.z) && dn_finite(p4.x) && dn_finite(p4.y) &&
                    dn_finite(p4.z);
    if (!ok) {
        const float4 o = make_float4(c.x, c.y, c.z, 0.0f);
        A.image[pi] = o;
        A.h0[pi] = o;
        return;
    }
    const f3 D = dn_divisor(a, (A.flags & PT_TEMPORAL_DEMODULATE) ? PT_DENOISE_DEMODULATE : 0u);
    const f3 Icur = mk(c.x / D.x, c.y / D.y, c.z / D.z);
    f3 I = Icur;
    float n = 1.0f;
    if (A.ph0) {
        const float W = (float)A.width, H = (float)A.height;
        const TpProjection p0 = tp_project(A.cur, p4.x, p4.y, p4.z);
        const TpProjection p1 = tp_project(A.prev, p4.x, p4.y, p4.z);
        const float fx = (float)(int32_t)x + (p1.su - p0.su) * W;
        const float fy = (float)(int32_t)y + (p1.sv - p0.sv) * H;
        const bool reproj = p0.z > 0.0f && p1.z > 0.0f && fx > -1.0f && fx < W && fy > -1.0f && fy < H;
        if (reproj) {
            const float flx = floorf(fx), fly = floorf(fy);
            const float ax = fx - flx, ay = fy - fly;
            const int32_t x0 = (int32_t)flx, y0 = (int32_t)fly;       // -1 .. width - 1, -1 .. height - 1
            const int32_t Wi = (int32_t)A.width, Hi = (int32_t)A.height;
            const float m = A.sigmaPlane * n4.w;
            const float mm = m * m;
            float sumW = 0.0f, nh = A.maxHistory;
            f3 sumI = mk(0.0f, 0.0f, 0.0f);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = k & 1, j = k >> 1;
                const float w = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
                const int32_t qx = x0 + i, qy = y0 + j;
                const bool inside = qx >= 0 && qx < Wi && qy >= 0 && qy < Hi;
                const size_t qi = inside ? (size_t)qy * A.width + (uint32_t)qx : pi;
                const float4 Iq = A.ph0[qi], Nq = A.ph1[qi], Pq = A.ph2[qi];
                const float cs = (n4.x * Nq.x + n4.y * Nq.y) + n4.z * Nq.z;
                const float ex = Pq.x - p4.x, ey = Pq.y - p4.y, ez = Pq.z - p4.z;
                const float g = (n4.x * ex + n4.y * ey) + n4.z * ez;
                const bool skip = !(w > 0.0f) || !inside || Iq.w < 1.0f || !dn_finite(Iq.x) || !dn_finite(Iq.y) ||
                                  !dn_finite(Iq.z) ||
                                  ((A.flags & PT_TEMPORAL_SAME_PRIMITIVE) && __float_as_uint(Nq.w) != __float_as_uint(a.w)) ||
                                  cs < A.normalCosMin || !(g * g <= mm);
                const float nW = sumW + w;
                const float nx = sumI.x + w * Iq.x, ny = sumI.y + w * Iq.y, nz = sumI.z + w * Iq.z;
                const float nn = Iq.w < nh ? Iq.w : nh;
                sumW = skip ? sumW : nW;
                sumI.x = skip ? sumI.x : nx;
                sumI.y = skip ? sumI.y : ny;
                sumI.z = skip ? sumI.z : nz;
                nh = skip ? nh : nn;
            }
            if (sumW >= 1.0f / 64.0f) {
                const f3 Hc = mk(sumI.x / sumW, sumI.y / sumW, sumI.z / sumW);
                n = nh + 1.0f;
                n = n < A.maxHistory ? n : A.maxHistory;
                float al = 1.0f / n;
                al = al > A.alphaMin ? al : A.alphaMin;
                I = mk(Hc.x + al * (Icur.x - Hc.x), Hc.y + al * (Icur.y - Hc.y), Hc.z + al * (Icur.z - Hc.z));
            }
        }
    }
    A.image[pi] = make_float4(I.x * D.x, I.y * D.y, I.z * D.z, n);
    A.h0[pi] = make_float4(I.x, I.y, I.z, n);
}

// ---------------------------------------------------------------------------------------------
// Rule 7: the same step when the objects moved between the history's scene and this one.  The motion table
// holds four float4 per primitive of the current scene: the rows of T_i, then (prev_index bits, 0, 0, 0), so
// an entry is four whole 16 B loads.  Neighbouring lanes mostly share the primitive, so the gather is a few
// 64 B lines per wave and the caches serve it; nothing is staged in LDS.  A second kernel rather than a
// template parameter of temporal_kernel, so that kernel's code object and name stay what they were.
// ---------------------------------------------------------------------------------------------
struct MotionTable {
    const float4* entries;      // [primCount][4]
    uint32_t primCount;         // >= 1
};

// What rule 7 puts on the p side of the taps: the point and the normal moved into the history's scene, and
// the primitive's index there (0xffffffff: take no history).
struct TpMoved {
    float px, py, pz, nx, ny, nz;
    uint32_t prevId;
};

PT_DEV TpMoved tp_move(const MotionTable& T, uint32_t id, const float4 n4, const float4 p4)
{
    const bool known = id < T.primCount;
    const size_t e = 4u * (size_t)(known ? id : 0u);          // clamped before the load, as the taps' indices
    const float4 r0 = T.entries[e], r1 = T.entries[e + 1], r2 = T.entries[e + 2], r3 = T.entries[e + 3];
    TpMoved o;
    o.px = ((r0.x * p4.x + r0.y * p4.y) + r0.z * p4.z) + r0.w;
    o.py = ((r1.x * p4.x + r1.y * p4.y) + r1.z * p4.z) + r1.w;
    o.pz = ((r2.x * p4.x + r2.y * p4.y) + r2.z * p4.z) + r2.w;
    o.nx = (r0.x * n4.x + r0.y * n4.y) + r0.z * n4.z;
    o.ny = (r1.x * n4.x + r1.y * n4.y) + r1.z * n4.z;
    o.nz = (r2.x * n4.x + r2.y * n4.y) + r2.z * n4.z;
    o.prevId = known ? __float_as_uint(r3.x) : 0xffffffffu;
    return o;
}

struct TemporalMotionArgs {
    TemporalArgs T;
    MotionTable motion;         // read only where T.ph0 is set
};

__global__ void __launch_bounds__(256) temporal_motion_kernel(TemporalMotionArgs B)
{
    const TemporalArgs& A = B.T;
    const uint32_t lx = threadIdx.x & (kDnTileW - 1u), ly = threadIdx.x / kDnTileW;
    const uint32_t x = blockIdx.x * kDnTileW + lx, y = blockIdx.y * kDnTileH + ly;
    if (x >= A.width || y >= A.height) return;
    const size_t pi = (size_t)y * A.width + x;
    const float4 c = A.color[pi], a = A.plane0[pi], n4 = A.plane1[pi], p4 = A.plane2[pi];
    A.h1[pi] = make_float4(n4.x, n4.y, n4.z, a.w);           // the current scene's: the new history is of it
    A.h2[pi] = make_float4(p4.x, p4.y, p4.z, n4.w);
    const bool ok = (__float_as_uint(p4.w) & PT_FEATURE_HIT) && dn_finite(c.x) && dn_finite(c.y) && dn_finite(c.z) &&
                    dn_finite(n4.x) && dn_finite(n4.y) && dn_finite(n4.z) && dn_finite(p4.x) && dn_finite(p4.y) &&
                    dn_finite(p4.z);
    if (!ok) {
        const float4 o = make_float4(c.x, c.y, c.z, 0.0f);
        A.image[pi] = o;
        A.h0[pi] = o;
        return;
    }
    const f3 D = dn_divisor(a, (A.flags & PT_TEMPORAL_DEMODULATE) ? PT_DENOISE_DEMODULATE : 0u);
    const f3 Icur = mk(c.x / D.x, c.y / D.y, c.z / D.z);
    f3 I = Icur;
    float n = 1.0f;
    if (A.ph0) {
        const float W = (float)A.width, H = (float)A.height;
        const TpMoved mv = tp_move(B.motion, __float_as_uint(a.w), n4, p4);
        const TpProjection p0 = tp_project(A.cur, p4.x, p4.y, p4.z);
        const TpProjection p1 = tp_project(A.prev, mv.px, mv.py, mv.pz);
        const float fx = (float)(int32_t)x + (p1.su - p0.su) * W;
        const float fy = (float)(int32_t)y + (p1.sv - p0.sv) * H;
        const bool reproj = p0.z > 0.0f && p1.z > 0.0f && fx > -1.0f && fx < W && fy > -1.0f && fy < H &&
                            mv.prevId != 0xffffffffu;
        if (reproj) {
            const float flx = floorf(fx), fly = floorf(fy);
            const float ax = fx - flx, ay = fy - fly;
            const int32_t x0 = (int32_t)flx, y0 = (int32_t)fly;       // -1 .. width - 1, -1 .. height - 1
            const int32_t Wi = (int32_t)A.width, Hi = (int32_t)A.height;
            const float m = A.sigmaPlane * n4.w;
            const float mm = m * m;
            float sumW = 0.0f, nh = A.maxHistory;
            f3 sumI = mk(0.0f, 0.0f, 0.0f);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = k & 1, j = k >> 1;
                const float w = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
                const int32_t qx = x0 + i, qy = y0 + j;
                const bool inside = qx >= 0 && qx < Wi && qy >= 0 && qy < Hi;
                const size_t qi = inside ? (size_t)qy * A.width + (uint32_t)qx : pi;
                const float4 Iq = A.ph0[qi], Nq = A.ph1[qi], Pq = A.ph2[qi];
                const float cs = (mv.nx * Nq.x + mv.ny * Nq.y) + mv.nz * Nq.z;
                const float ex = Pq.x - mv.px, ey = Pq.y - mv.py, ez = Pq.z - mv.pz;
                const float g = (mv.nx * ex + mv.ny * ey) + mv.nz * ez;
                const bool skip = !(w > 0.0f) || !inside || Iq.w < 1.0f || !dn_finite(Iq.x) || !dn_finite(Iq.y) ||
                                  !dn_finite(Iq.z) ||
                                  ((A.flags & PT_TEMPORAL_SAME_PRIMITIVE) && __float_as_uint(Nq.w) != mv.prevId) ||
                                  cs < A.normalCosMin || !(g * g <= mm);
                const float nW = sumW + w;
                const float nx = sumI.x + w * Iq.x, ny = sumI.y + w * Iq.y, nz = sumI.z + w * Iq.z;
                const float nn = Iq.w < nh ? Iq.w : nh;
                sumW = skip ? sumW : nW;
                sumI.x = skip ? sumI.x : nx;
                sumI.y = skip ? sumI.y : ny;
                sumI.z = skip ? sumI.z : nz;
                nh = skip ? nh : nn;
            }
            if (sumW >= 1.0f / 64.0f) {
                const f3 Hc = mk(sumI.x / sumW, sumI.y / sumW, sumI.z / sumW);
                n = nh + 1.0f;
                n = n < A.maxHistory ? n : A.maxHistory;
                float al = 1.0f / n;
                al = al > A.alphaMin ? al : A.alphaMin;
                I = mk(Hc.x + al * (Icur.x - Hc.x), Hc.y + al * (Icur.y - Hc.y), Hc.z + al * (Icur.z - Hc.z));
            }
        }
    }
    A.image[pi] = make_float4(I.x * D.x, I.y * D.y, I.z * D.z, n);
    A.h0[pi] = make_float4(I.x, I.y, I.z, n);
}
