// Per-pixel variance from the temporal history and the variance-guided a-trous filter (pt_temporal_moments,
// pt_denoise_variance and their _image forms; the rules are written out in include/pt_hip.h and restated in
// tests/svgf_model.py), and the feedback of the filtered colour into the history (pt_denoise_variance_feedback;
// tests/feedback_model.py).  Part of the trace kernel's single translation unit: included by pt_kernels.hip
// inside its anonymous namespace after pt_dev_temporal.h; not a standalone header.
// Nothing here is used by an existing kernel, and no existing kernel or parameter struct changes.
#pragma once

PT_DEV float sv_lum(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }
PT_DEV float sv_clamp0(float v) { return (v > 0.0f && dn_finite(v)) ? v : 0.0f; }

// ---------------------------------------------------------------------------------------------
// 1. The temporal step with moments: temporal_kernel's operations on the colour, in its order, with the
// two moment sums riding on the same taps.  A second kernel rather than a template parameter of
// temporal_kernel, so that kernel's code object and name stay what they were.
// ---------------------------------------------------------------------------------------------
struct MomentsArgs {
    TemporalArgs T;
    const float4* ph3;          // previous (m1, m2, v, 0); read only where T.ph0 is set
    float4* h3;
};

__global__ void __launch_bounds__(256) temporal_moments_kernel(MomentsArgs M)
{
    const TemporalArgs& A = M.T;
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
        M.h3[pi] = make_float4(0.0f, 0.0f, -1.0f, 0.0f);
        return;
    }
    const f3 D = dn_divisor(a, (A.flags & PT_TEMPORAL_DEMODULATE) ? PT_DENOISE_DEMODULATE : 0u);
    const f3 Icur = mk(c.x / D.x, c.y / D.y, c.z / D.z);
    const float l = sv_lum(Icur.x, Icur.y, Icur.z);
    const float q = l * l;
    f3 I = Icur;
    float n = 1.0f, m1 = l, m2 = q;
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
            float sumW = 0.0f, nh = A.maxHistory, sumM1 = 0.0f, sumM2 = 0.0f;
            f3 sumI = mk(0.0f, 0.0f, 0.0f);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = k & 1, j = k >> 1;
                const float w = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
                const int32_t qx = x0 + i, qy = y0 + j;
                const bool inside = qx >= 0 && qx < Wi && qy >= 0 && qy < Hi;
                const size_t qi = inside ? (size_t)qy * A.width + (uint32_t)qx : pi;
                const float4 Iq = A.ph0[qi], Nq = A.ph1[qi], Pq = A.ph2[qi], Mq = M.ph3[qi];
                const float cs = (n4.x * Nq.x + n4.y * Nq.y) + n4.z * Nq.z;
                const float ex = Pq.x - p4.x, ey = Pq.y - p4.y, ez = Pq.z - p4.z;
                const float g = (n4.x * ex + n4.y * ey) + n4.z * ez;
                const bool skip = !(w > 0.0f) || !inside || Iq.w < 1.0f || !dn_finite(Iq.x) || !dn_finite(Iq.y) ||
                                  !dn_finite(Iq.z) ||
                                  ((A.flags & PT_TEMPORAL_SAME_PRIMITIVE) && __float_as_uint(Nq.w) != __float_as_uint(a.w)) ||
                                  cs < A.normalCosMin || !(g * g <= mm);
                const float nW = sumW + w;
                const float nx = sumI.x + w * Iq.x, ny = sumI.y + w * Iq.y, nz = sumI.z + w * Iq.z;
                const float n1 = sumM1 + w * Mq.x, n2 = sumM2 + w * Mq.y;
                const float nn = Iq.w < nh ? Iq.w : nh;
                sumW = skip ? sumW : nW;
                sumI.x = skip ? sumI.x : nx;
                sumI.y = skip ? sumI.y : ny;
                sumI.z = skip ? sumI.z : nz;
                sumM1 = skip ? sumM1 : n1;
                sumM2 = skip ? sumM2 : n2;
                nh = skip ? nh : nn;
            }
            if (sumW >= 1.0f / 64.0f) {
                const f3 Hc = mk(sumI.x / sumW, sumI.y / sumW, sumI.z / sumW);
                const float Hm1 = sumM1 / sumW, Hm2 = sumM2 / sumW;
                n = nh + 1.0f;
                n = n < A.maxHistory ? n : A.maxHistory;
                float al = 1.0f / n;
                al = al > A.alphaMin ? al : A.alphaMin;
                I = mk(Hc.x + al * (Icur.x - Hc.x), Hc.y + al * (Icur.y - Hc.y), Hc.z + al * (Icur.z - Hc.z));
                m1 = Hm1 + al * (l - Hm1);
                m2 = Hm2 + al * (q - Hm2);
            }
        }
    }
    const bool restart = !dn_finite(m1) || !dn_finite(m2);
    m1 = restart ? l : m1;
    m2 = restart ? q : m2;
    A.image[pi] = make_float4(I.x * D.x, I.y * D.y, I.z * D.z, n);
    A.h0[pi] = make_float4(I.x, I.y, I.z, n);
    M.h3[pi] = make_float4(m1, m2, sv_clamp0(m2 - m1 * m1), 0.0f);
}

// The same step under rule 7 (pt_dev_temporal.h): temporal_motion_kernel's substitution on the p side of the
// taps, the moment sums riding on the same taps.  Again a kernel of its own.
struct MomentsMotionArgs {
    MomentsArgs M;
    MotionTable motion;         // read only where M.T.ph0 is set
};

__global__ void __launch_bounds__(256) temporal_moments_motion_kernel(MomentsMotionArgs B)
{
    const MomentsArgs& M = B.M;
    const TemporalArgs& A = M.T;
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
        M.h3[pi] = make_float4(0.0f, 0.0f, -1.0f, 0.0f);
        return;
    }
    const f3 D = dn_divisor(a, (A.flags & PT_TEMPORAL_DEMODULATE) ? PT_DENOISE_DEMODULATE : 0u);
    const f3 Icur = mk(c.x / D.x, c.y / D.y, c.z / D.z);
    const float l = sv_lum(Icur.x, Icur.y, Icur.z);
    const float q = l * l;
    f3 I = Icur;
    float n = 1.0f, m1 = l, m2 = q;
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
            float sumW = 0.0f, nh = A.maxHistory, sumM1 = 0.0f, sumM2 = 0.0f;
            f3 sumI = mk(0.0f, 0.0f, 0.0f);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = k & 1, j = k >> 1;
                const float w = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
                const int32_t qx = x0 + i, qy = y0 + j;
                const bool inside = qx >= 0 && qx < Wi && qy >= 0 && qy < Hi;
                const size_t qi = inside ? (size_t)qy * A.width + (uint32_t)qx : pi;
                const float4 Iq = A.ph0[qi], Nq = A.ph1[qi], Pq = A.ph2[qi], Mq = M.ph3[qi];
                const float cs = (mv.nx * Nq.x + mv.ny * Nq.y) + mv.nz * Nq.z;
                const float ex = Pq.x - mv.px, ey = Pq.y - mv.py, ez = Pq.z - mv.pz;
                const float g = (mv.nx * ex + mv.ny * ey) + mv.nz * ez;
                const bool skip = !(w > 0.0f) || !inside || Iq.w < 1.0f || !dn_finite(Iq.x) || !dn_finite(Iq.y) ||
                                  !dn_finite(Iq.z) ||
                                  ((A.flags & PT_TEMPORAL_SAME_PRIMITIVE) && __float_as_uint(Nq.w) != mv.prevId) ||
                                  cs < A.normalCosMin || !(g * g <= mm);
                const float nW = sumW + w;
                const float nx = sumI.x + w * Iq.x, ny = sumI.y + w * Iq.y, nz = sumI.z + w * Iq.z;
                const float n1 = sumM1 + w * Mq.x, n2 = sumM2 + w * Mq.y;
                const float nn = Iq.w < nh ? Iq.w : nh;
                sumW = skip ? sumW : nW;
                sumI.x = skip ? sumI.x : nx;
                sumI.y = skip ? sumI.y : ny;
                sumI.z = skip ? sumI.z : nz;
                sumM1 = skip ? sumM1 : n1;
                sumM2 = skip ? sumM2 : n2;
                nh = skip ? nh : nn;
            }
            if (sumW >= 1.0f / 64.0f) {
                const f3 Hc = mk(sumI.x / sumW, sumI.y / sumW, sumI.z / sumW);
                const float Hm1 = sumM1 / sumW, Hm2 = sumM2 / sumW;
                n = nh + 1.0f;
                n = n < A.maxHistory ? n : A.maxHistory;
                float al = 1.0f / n;
                al = al > A.alphaMin ? al : A.alphaMin;
                I = mk(Hc.x + al * (Icur.x - Hc.x), Hc.y + al * (Icur.y - Hc.y), Hc.z + al * (Icur.z - Hc.z));
                m1 = Hm1 + al * (l - Hm1);
                m2 = Hm2 + al * (q - Hm2);
            }
        }
    }
    const bool restart = !dn_finite(m1) || !dn_finite(m2);
    m1 = restart ? l : m1;
    m2 = restart ? q : m2;
    A.image[pi] = make_float4(I.x * D.x, I.y * D.y, I.z * D.z, n);
    A.h0[pi] = make_float4(I.x, I.y, I.z, n);
    M.h3[pi] = make_float4(m1, m2, sv_clamp0(m2 - m1 * m1), 0.0f);
}

// ---------------------------------------------------------------------------------------------
// 2. The variance estimate over the new history.  The temporal tile, one pixel per lane; only a young pixel
// walks the 7 x 7 window, a row of seven taps of 48 B in flight at a time (the caches serve the overlap).
// ---------------------------------------------------------------------------------------------
struct VarianceArgs {
    const float4* h0;           // new (I, n)
    const float4* h1;           // new (N, id)
    const float4* h2;           // new (P, t)
    const float4* h3;           // new (m1, m2, v, 0)
    float* var;
    uint32_t width, height;
    float minTemporal, sigmaPlane, normalCosMin;
    uint32_t flags;
};

__global__ void __launch_bounds__(256) variance_kernel(VarianceArgs A)
{
    const uint32_t lx = threadIdx.x & (kDnTileW - 1u), ly = threadIdx.x / kDnTileW;
    const uint32_t x = blockIdx.x * kDnTileW + lx, y = blockIdx.y * kDnTileH + ly;
    if (x >= A.width || y >= A.height) return;
    const size_t pi = (size_t)y * A.width + x;
    const float4 Ip = A.h0[pi];
    if (Ip.w < 1.0f) {
        A.var[pi] = -1.0f;
        return;
    }
    if (Ip.w >= A.minTemporal) {
        A.var[pi] = A.h3[pi].z;
        return;
    }
    const float4 Np = A.h1[pi], Pp = A.h2[pi];
    const int32_t W = (int32_t)A.width, H = (int32_t)A.height;
    const float m = A.sigmaPlane * Pp.w;
    const float mm = m * m;
    float k = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll 1
    for (int dy = -3; dy <= 3; ++dy) {
#pragma unroll
        for (int dx = -3; dx <= 3; ++dx) {
            const int32_t qx = (int32_t)x + dx, qy = (int32_t)y + dy;
            const bool inside = qx >= 0 && qx < W && qy >= 0 && qy < H;
            const size_t qi = inside ? (size_t)qy * A.width + (uint32_t)qx : pi;
            const float4 Iq = A.h0[qi], Nq = A.h1[qi], Pq = A.h2[qi];
            const float cs = (Np.x * Nq.x + Np.y * Nq.y) + Np.z * Nq.z;
            const float ex = Pq.x - Pp.x, ey = Pq.y - Pp.y, ez = Pq.z - Pp.z;
            const float g = (Np.x * ex + Np.y * ey) + Np.z * ez;
            const bool centre = dx == 0 && dy == 0;
            const bool skip = !centre && (!inside || Iq.w < 1.0f || cs < A.normalCosMin || !(g * g <= mm) ||
                                          ((A.flags & PT_TEMPORAL_SAME_PRIMITIVE) &&
                                           __float_as_uint(Nq.w) != __float_as_uint(Np.w)));
            const float lq = sv_lum(Iq.x, Iq.y, Iq.z);
            const float nk = k + 1.0f, n1 = s1 + lq, n2 = s2 + lq * lq;
            k = skip ? k : nk;
            s1 = skip ? s1 : n1;
            s2 = skip ? s2 : n2;
        }
    }
    const float mean = s1 / k;
    const float vs = sv_clamp0(s2 / k - mean * mean);
    A.var[pi] = vs * (A.minTemporal / Ip.w);
}

// ---------------------------------------------------------------------------------------------
// 3. The variance-guided filter: dn_prepare / dn_iter / dn_finish with the texel's w holding the variance
// (or -1 for a pixel that is not kept) instead of the 0 / 1 keep word.  g0 and g1 are dn_prepare's.
// ---------------------------------------------------------------------------------------------
struct VDenoiseArgs {
    DenoiseArgs D;              // ss is not used
    const float* var;           // prepare's input
    float sl2;                  // sigma_l * sigma_l
    float floorV;               // variance_floor
};

__global__ void __launch_bounds__(256) vdn_prepare_kernel(VDenoiseArgs V)
{
    const DenoiseArgs& A = V.D;
    const size_t npix = (size_t)A.width * A.height;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const float4 c = A.color[i], a = A.plane0[i], n = A.plane1[i], p = A.plane2[i];
    const float var = V.var[i];
    const uint32_t fl = __float_as_uint(p.w);
    const f3 D = dn_divisor(a, A.flags);
    const f3 I = mk(c.x / D.x, c.y / D.y, c.z / D.z);
    const bool keep = (fl & PT_FEATURE_HIT) && !(fl & PT_FEATURE_EMISSIVE) && dn_finite(c.x) && dn_finite(c.y) &&
                      dn_finite(c.z) && dn_finite(n.x) && dn_finite(n.y) && dn_finite(n.z) && dn_finite(p.x) &&
                      dn_finite(p.y) && dn_finite(p.z) && var >= 0.0f && dn_finite(var) &&
                      dn_finite(sv_lum(I.x, I.y, I.z));
    const float big = 1152921504606846976.0f;             // 2^60
    const float v = var < big ? var : big;
    A.dst[i] = make_float4(I.x, I.y, I.z, keep ? v : -1.0f);
    A.g0[i] = make_float4(n.x, n.y, n.z, a.w);
    A.g1[i] = make_float4(p.x, p.y, p.z, n.w);
}

// One of the 25 taps, in the rule's operation order; the caller has marked a tap outside the image as not
// kept.
PT_DEV void vdn_tap(const VDenoiseArgs& V, float h, float lp, float den, const float4 Np, const float4 Pp, float mm,
                    const float4 Iq, const float4 Nq, const float4 Pq, float& sumW, f3& sumI, float& sumV2)
{
    const DenoiseArgs& A = V.D;
    const bool skip = Iq.w < 0.0f ||
                      ((A.flags & PT_DENOISE_SAME_PRIMITIVE) && __float_as_uint(Nq.w) != __float_as_uint(Np.w));
    float c = (Np.x * Nq.x + Np.y * Nq.y) + Np.z * Nq.z;
    c = c > 0.0f ? c : 0.0f;
    for (uint32_t k = 0; k < A.normalPower; ++k) c = c * c;
    const float ex = Pq.x - Pp.x, ey = Pq.y - Pp.y, ez = Pq.z - Pp.z;
    const float g = (Np.x * ex + Np.y * ey) + Np.z * ez;
    const float wp = 1.0f / (1.0f + (g * g) / mm);
    const float d = sv_lum(Iq.x, Iq.y, Iq.z) - lp;
    const float wc = 1.0f / (1.0f + (d * d) / den);
    const float w = ((h * c) * wp) * wc;
    const float nW = sumW + w;
    const float nx = sumI.x + w * Iq.x, ny = sumI.y + w * Iq.y, nz = sumI.z + w * Iq.z;
    const float nV = sumV2 + (w * w) * Iq.w;
    sumW = skip ? sumW : nW;
    sumI.x = skip ? sumI.x : nx;
    sumI.y = skip ? sumI.y : ny;
    sumI.z = skip ? sumI.z : nz;
    sumV2 = skip ? sumV2 : nV;
}

// dn_iter_kernel's tile, staging and tap order (see there).  The 3 x 3 variance filter is at unit spacing:
// inside the staged halo of 2 s >= 2 texels, or nine 16 B loads through the caches.
template <bool STAGED>
__global__ void __launch_bounds__(256, 4) vdn_iter_kernel(VDenoiseArgs V)
{
    const DenoiseArgs& A = V.D;
    const uint32_t lx = threadIdx.x & (kDnTileW - 1u), ly = threadIdx.x / kDnTileW;
    const uint32_t x0 = blockIdx.x * kDnTileW, y0 = blockIdx.y * kDnTileH;
    const uint32_t x = x0 + lx, y = y0 + ly;
    const int32_t s = (int32_t)A.step;
    const int32_t W = (int32_t)A.width, H = (int32_t)A.height;
    const uint32_t RW = kDnTileW + 4u * A.step, RH = kDnTileH + 4u * A.step, RN = RW * RH;
    if (STAGED) {
        float4* sI = lds4;
        float4* sN = lds4 + RN;
        float4* sP = lds4 + 2u * RN;
        const int32_t gx0 = (int32_t)x0 - 2 * s, gy0 = (int32_t)y0 - 2 * s;
        for (uint32_t k = threadIdx.x; k < RN; k += 256u) {
            const uint32_t ry = k / RW, rx = k - ry * RW;
            const int32_t gx = gx0 + (int32_t)rx, gy = gy0 + (int32_t)ry;
            float4 vi = make_float4(0.0f, 0.0f, 0.0f, -1.0f), vn = make_float4(0.0f, 0.0f, 0.0f, 0.0f), vp = vn;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const size_t gi = (size_t)gy * A.width + (uint32_t)gx;
                vi = A.src[gi];
                vn = A.g0[gi];
                vp = A.g1[gi];
            }
            sI[k] = vi;
            sN[k] = vn;
            sP[k] = vp;
        }
        __syncthreads();
    }
    if (x >= A.width || y >= A.height) return;
    const size_t pi = (size_t)y * A.width + x;
    const uint32_t cIdx = (ly + 2u * A.step) * RW + (lx + 2u * A.step);    // the pixel's texel in the staged region
    const float4 Ip = STAGED ? lds4[cIdx] : A.src[pi];
    if (Ip.w < 0.0f) {                                   // not kept: handed on unchanged
        A.dst[pi] = Ip;
        return;
    }
    float sumG = 0.0f, sumV = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const float g = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
            float vq;
            if (STAGED) {
                vq = lds4[(uint32_t)((int32_t)cIdx + dy * (int32_t)RW + dx)].w;
            } else {
                const int32_t qx = (int32_t)x + dx, qy = (int32_t)y + dy;
                const bool inside = qx >= 0 && qx < W && qy >= 0 && qy < H;
                vq = A.src[inside ? (size_t)qy * A.width + (uint32_t)qx : pi].w;
                vq = inside ? vq : -1.0f;
            }
            const bool skip = vq < 0.0f;
            const float nG = sumG + g, nV = sumV + g * vq;
            sumG = skip ? sumG : nG;
            sumV = skip ? sumV : nV;
        }
    }
    const float vg = sumV / sumG;
    const float den = V.sl2 * vg + V.floorV;
    const float lp = sv_lum(Ip.x, Ip.y, Ip.z);
    const float4 Np = STAGED ? lds4[RN + cIdx] : A.g0[pi];
    const float4 Pp = STAGED ? lds4[2u * RN + cIdx] : A.g1[pi];
    const float m = A.sigmaPlane * Pp.w;
    const float mm = m * m;
    const float kk[3] = {3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    float sumW = 0.0f, sumV2 = 0.0f;
    f3 sumI = mk(0.0f, 0.0f, 0.0f);
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
        const int ady = dy < 0 ? -dy : dy;
        const float ky = ady == 0 ? kk[0] : (ady == 1 ? kk[1] : kk[2]);
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const float h = kk[dx < 0 ? -dx : dx] * ky;
            float4 Iq, Nq, Pq;
            if (STAGED) {
                const uint32_t qi = (uint32_t)((int32_t)cIdx + dy * s * (int32_t)RW + dx * s);
                Iq = lds4[qi];
                Nq = lds4[RN + qi];
                Pq = lds4[2u * RN + qi];
            } else {
                const int32_t qx = (int32_t)x + dx * s, qy = (int32_t)y + dy * s;
                const bool inside = qx >= 0 && qx < W && qy >= 0 && qy < H;
                const size_t qi = inside ? (size_t)qy * A.width + (uint32_t)qx : pi;
                Iq = A.src[qi];
                Nq = A.g0[qi];
                Pq = A.g1[qi];
                if (!inside) Iq.w = -1.0f;               // skipped, as a texel that is not kept
            }
            vdn_tap(V, h, lp, den, Np, Pp, mm, Iq, Nq, Pq, sumW, sumI, sumV2);
        }
    }
    A.dst[pi] = make_float4(sumI.x / sumW, sumI.y / sumW, sumI.z / sumW, sumV2 / (sumW * sumW));
}

__global__ void __launch_bounds__(256) vdn_finish_kernel(VDenoiseArgs V)
{
    const DenoiseArgs& A = V.D;
    const size_t npix = (size_t)A.width * A.height;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const float4 c = A.color[i], I = A.src[i];
    const f3 D = dn_divisor(A.plane0[i], A.flags);
    const bool keep = !(I.w < 0.0f);
    A.dst[i] = make_float4(keep ? I.x * D.x : c.x, keep ? I.y * D.y : c.y, keep ? I.z * D.z : c.z, 1.0f);
}

// ---------------------------------------------------------------------------------------------
// 4. The feedback: the texel iteration L - 1 wrote becomes the colour the next frame reprojects.  Flat, one
// pixel per lane, two 16 B loads and one unconditional 16 B store; the history length is the word that was
// there.  A kernel of its own after the iteration, so vdn_iter_kernel's code objects stay what they were.
// ---------------------------------------------------------------------------------------------
struct FeedbackArgs {
    const float4* texel;        // the buffer iteration L - 1 wrote: (I', v') or w < 0
    float4* h0;                 // the history's (I, n) the last moments step wrote
    size_t npix;
};

__global__ void __launch_bounds__(256) vdn_feedback_kernel(FeedbackArgs A)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.npix) return;
    const float4 T = A.texel[i], h = A.h0[i];
    const bool fed = !(T.w < 0.0f) && dn_finite(T.x) && dn_finite(T.y) && dn_finite(T.z);
    A.h0[i] = make_float4(fed ? T.x : h.x, fed ? T.y : h.y, fed ? T.z : h.z, h.w);
}
