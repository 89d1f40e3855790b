// The variance of an adaptive render's image from its own per-pixel moments (pt_denoise_adaptive,
// pt_adaptive_variance_image; rule 5 of include/pt_hip.h, restated in tests/adaptive_variance_model.py).
// Part of the trace kernel's single translation unit: included by pt_kernels.hip inside its anonymous
// namespace after pt_dev_svgf.h; not a standalone header.
// Nothing here is used by an existing kernel, and no existing kernel or parameter struct changes.
#pragma once

struct AVarianceArgs {
    const float4* color;        // C = accumulation / n
    const float4* plane0;       // (A, id)
    const float4* plane1;       // (N, t)
    const float4* plane2;       // (P, flags)
    const uint32_t* mom;        // [3][pixels]: m1, m2 (float bits), n -- the context's adMom layout
    float4* t0;                 // (N, l), l = NaN where the pixel is not ok
    float4* t1;                 // (P, id)
    float* var;
    uint32_t width, height;
    uint32_t minBatches;
    float sigmaPlane, normalCosMin;
    uint32_t flags;
};

// ---------------------------------------------------------------------------------------------
// 1. Everything of the rule that needs the pixel alone (operations 1 to 7): var = -1 or `own`, and the two
// float4 a window tap needs, 32 B instead of the 64 B of the colour and the three planes.  "Not ok" travels
// as a luminance that is not finite, which an ok pixel never has, so the id keeps all of its 32 bits.
// Flat, one pixel per lane.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) avar_prepare_kernel(AVarianceArgs A)
{
    const size_t npix = (size_t)A.width * A.height;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const float4 c = A.color[i], a = A.plane0[i], n4 = A.plane1[i], p4 = A.plane2[i];
    const float m1 = __uint_as_float(A.mom[i]), m2 = __uint_as_float(A.mom[npix + i]);
    const uint32_t n = A.mom[2 * npix + i];
    const uint32_t fl = __float_as_uint(p4.w);
    const f3 D = dn_divisor(a, A.flags);
    const float l = sv_lum(c.x / D.x, c.y / D.y, c.z / D.z);
    const float g = (A.flags & PT_DENOISE_DEMODULATE) ? sv_lum(D.x, D.y, D.z) : 1.0f;
    const bool ok = (fl & PT_FEATURE_HIT) && !(fl & PT_FEATURE_EMISSIVE) && dn_finite(l) && dn_finite(n4.x) &&
                    dn_finite(n4.y) && dn_finite(n4.z) && dn_finite(p4.x) && dn_finite(p4.y) && dn_finite(p4.z);
    // adapt_flag_kernel's operations on the same words, up to se2
    const float k = (float)n;
    const float mean = m1 / k;
    float ss = m2 - m1 * mean;
    if (ss < 0.0f) ss = 0.0f;
    const float se2 = ss / (k * (k - 1.0f));
    const float own = sv_clamp0(se2 / (g * g));
    const bool has = ok && n >= 2u && dn_finite(m1) && dn_finite(m2);
    A.var[i] = has ? own : -1.0f;
    A.t0[i] = make_float4(n4.x, n4.y, n4.z, ok ? l : __uint_as_float(0x7fc00000u));
    A.t1[i] = make_float4(p4.x, p4.y, p4.z, a.w);
}

// ---------------------------------------------------------------------------------------------
// 2. The window of a young pixel (operations 8 to 10), over what the prepare kernel wrote; a pixel that is
// not young keeps the word it has.  The filter's 32 x 8 tile, one pixel per lane.  How many pixels walk depends
// on the render and on min_batches: none to all of those with a variance.
// STAGED: the tile and its halo of 3, 38 x 14 texels of 32 B = 17,024 B of LDS (and 16 B of votes), are copied first
// (a texel outside the image as not ok), so each texel is fetched once per workgroup and not once per tap; a tile
// without a young pixel copies nothing.
// Unstaged: a row of seven taps of 32 B in flight at a time, through the caches.  The same operations either
// way, so the same words.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kAvHalo = 3u;
constexpr uint32_t kAvRW = kDnTileW + 2u * kAvHalo, kAvRH = kDnTileH + 2u * kAvHalo, kAvRN = kAvRW * kAvRH;

template <bool STAGED>
__global__ void __launch_bounds__(256) adaptive_variance_kernel(AVarianceArgs A)
{
    const uint32_t lx = threadIdx.x & (kDnTileW - 1u), ly = threadIdx.x / kDnTileW;
    const uint32_t x0 = blockIdx.x * kDnTileW, y0 = blockIdx.y * kDnTileH;
    const uint32_t x = x0 + lx, y = y0 + ly;
    const int32_t W = (int32_t)A.width, H = (int32_t)A.height;
    const size_t npix = (size_t)A.width * A.height;
    const size_t pi = (size_t)y * A.width + x;
    float own = -1.0f;
    bool young = false;
    if (x < A.width && y < A.height) {
        own = A.var[pi];
        young = !(own < 0.0f) && A.mom[2 * npix + pi] < A.minBatches;
    }
    if (STAGED) {
        // a tile without a young pixel stages nothing: one vote per wave, gathered through four words behind the region
        uint32_t* votes = reinterpret_cast<uint32_t*>(lds4 + 2u * kAvRN);
        const uint32_t vote = __any(young ? 1 : 0) ? 1u : 0u;
        if ((threadIdx.x & 63u) == 0u) votes[threadIdx.x >> 6] = vote;
        __syncthreads();
        if ((votes[0] | votes[1] | votes[2] | votes[3]) == 0u) return;
        const int32_t gx0 = (int32_t)x0 - (int32_t)kAvHalo, gy0 = (int32_t)y0 - (int32_t)kAvHalo;
        for (uint32_t k = threadIdx.x; k < kAvRN; k += 256u) {
            const uint32_t ry = k / kAvRW, rx = k - ry * kAvRW;
            const int32_t gx = gx0 + (int32_t)rx, gy = gy0 + (int32_t)ry;
            float4 v0 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0x7fc00000u)), v1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const size_t gi = (size_t)gy * A.width + (uint32_t)gx;
                v0 = A.t0[gi];
                v1 = A.t1[gi];
            }
            lds4[k] = v0;
            lds4[kAvRN + k] = v1;
        }
        __syncthreads();
    }
    if (!young) return;                                  // the word the prepare kernel wrote stands
    const uint32_t cIdx = (ly + kAvHalo) * kAvRW + (lx + kAvHalo);        // the pixel's texel in the staged region
    const float4 Np = STAGED ? lds4[cIdx] : A.t0[pi];
    const float4 Pp = STAGED ? lds4[kAvRN + cIdx] : A.t1[pi];
    const float m = A.sigmaPlane * A.plane1[pi].w;
    const float mm = m * m;
    float k = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll 1
    for (int dy = -3; dy <= 3; ++dy) {
#pragma unroll
        for (int dx = -3; dx <= 3; ++dx) {
            float4 Nq, Pq;
            bool inside = true;                          // a staged texel outside the image is not ok
            if (STAGED) {
                const uint32_t qi = (uint32_t)((int32_t)cIdx + dy * (int32_t)kAvRW + dx);
                Nq = lds4[qi];
                Pq = lds4[kAvRN + qi];
            } else {
                const int32_t qx = (int32_t)x + dx, qy = (int32_t)y + dy;
                inside = qx >= 0 && qx < W && qy >= 0 && qy < H;
                const size_t qi = inside ? (size_t)qy * A.width + (uint32_t)qx : pi;
                Nq = A.t0[qi];
                Pq = A.t1[qi];
            }
            const float cs = (Np.x * Nq.x + Np.y * Nq.y) + Np.z * Nq.z;
            const float ex = Pq.x - Pp.x, ey = Pq.y - Pp.y, ez = Pq.z - Pp.z;
            const float g = (Np.x * ex + Np.y * ey) + Np.z * ez;
            const bool centre = dx == 0 && dy == 0;
            const bool skip = !centre && (!inside || !dn_finite(Nq.w) || cs < A.normalCosMin || !(g * g <= mm) ||
                                          ((A.flags & PT_DENOISE_SAME_PRIMITIVE) &&
                                           __float_as_uint(Pq.w) != __float_as_uint(Pp.w)));
            const float lq = Nq.w;
            const float nk = k + 1.0f, n1 = s1 + lq, n2 = s2 + lq * lq;
            k = skip ? k : nk;
            s1 = skip ? s1 : n1;
            s2 = skip ? s2 : n2;
        }
    }
    const float mean = s1 / k;
    const float vs = sv_clamp0(s2 / k - mean * mean);
    A.var[pi] = vs > own ? vs : own;
}
