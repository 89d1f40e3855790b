// First-hit feature pass and the edge-avoiding a-trous filter (pt_render_features, pt_denoise,
// pt_denoise_image; the rule is written out in include/pt_hip.h and restated in tests/denoise_model.py).
// Part of the trace kernel's single translation unit: included by pt_kernels.hip inside its anonymous
// namespace after pt_dev_fold.h; not a standalone header.  Nothing here is used by trace_kernel.
#pragma once

// ---------------------------------------------------------------------------------------------
// Feature pass: one wave = one 8x8 tile, one lane = one pixel, four tiles per workgroup; the
// workgroup's dynamic LDS is four wave stacks of stackDepth x 64 u32 (traverse's layout).
// Its own parameter struct: TraceParams does not grow (kernel arguments cost the trace kernel).
// ---------------------------------------------------------------------------------------------
struct FeatureParams {
    float4* planes;             // 3 planes of rows x width
    const float4* nodes;
    const float4* prims;
    const float4* mats;
    const DevTex* textures;
    uint32_t width, rows, rowOffset, rowStride, bandShift;
    float fwidth, fheight;
    uint32_t tilesX, tiles;
    uint32_t stackDepth, slabFast;
    DevCamera cam;
};

__global__ void __launch_bounds__(256) features_kernel(FeatureParams P)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t tile = blockIdx.x * 4u + wave;
    if (tile >= P.tiles) return;
    const uint32_t ty = tile / P.tilesX, tx = tile - ty * P.tilesX;
    const uint32_t x = tx * 8u + (lane & 7u), ly = ty * 8u + (lane >> 3);
    if (x >= P.width || ly >= P.rows) return;
    const size_t npix = (size_t)P.rows * P.width;
    const size_t li = (size_t)ly * P.width + x;
    const uint32_t y = global_row(ly, P.rowOffset, P.rowStride, P.bandShift);
    // the pixel's first sample of a reset render: initRandState's state (init_rng_kernel), then the two
    // uniforms of camera_ray, x then y, in camera_ray's operations
    Xorwow rng = xorwow_init((uint64_t)(uint32_t)(1984u + (x + y * P.width)));
    const float fx = (float)(int32_t)x, fy = (float)(int32_t)y;
    const float u = (fx + uniform(rng)) / P.fwidth;
    const float v = (fy + uniform(rng)) / P.fheight;
    const f3 o = P.cam.origin;
    const f3 d = normalize(add(add(P.cam.llc, scale(u, P.cam.horizontal)), scale(v, P.cam.vertical)));
    uint32_t* stack = reinterpret_cast<uint32_t*>(lds4) + wave * (P.stackDepth * 64u) + lane;
    Counters cnt = {};
    float t;
    const uint32_t e = traverse<false, 1>(P.nodes, P.prims, stack, o, d, P.slabFast != 0, t, cnt);
    float4 f0 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xffffffffu));
    float4 f1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 f2q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (e != 0xffffffffu) {
        const float4 m0 = P.mats[3 * e + 0];
        const float4 m1 = P.mats[3 * e + 1];
        const float4 m2 = P.mats[3 * e + 2];
        const float4 q0 = P.prims[4 * e + 0];
        const float4 q1 = P.prims[4 * e + 1];
        const float4 q2 = P.prims[4 * e + 2];
        const uint32_t ptype = __float_as_uint(P.prims[4 * e + 3].x);
        const uint32_t texIdx = __float_as_uint(m2.x);
        const Surface sf = surface_of(q0, q1, q2, ptype, o, d, t, texIdx != 0);
        f3 base = mk(m0.x, m0.y, m0.z);
        if (texIdx != 0) {                                                        // as shade forms it
            const f3 tap = tex2d(P.textures[texIdx - 1], sf.u, sf.v);
            base = mk(pow_(tap.x, 2.2f), pow_(tap.y, 2.2f), pow_(tap.z, 2.2f));
        }
        const bool emissive = m1.x != 0.0f || m1.y != 0.0f || m1.z != 0.0f;
        f0 = make_float4(base.x, base.y, base.z, __uint_as_float(e));
        f1 = make_float4(sf.n.x, sf.n.y, sf.n.z, t);
        f2q = make_float4(sf.p.x, sf.p.y, sf.p.z, __uint_as_float(PT_FEATURE_HIT | (emissive ? PT_FEATURE_EMISSIVE : 0u)));
    }
    P.planes[li] = f0;
    P.planes[npix + li] = f1;
    P.planes[2 * npix + li] = f2q;
}

// The context's image in the HDR read-out's units: accumulation * inv (inv = 1 / max(frames, 1)), or
// with `calls` accumulation / n per pixel (pt_read_adaptive_hdr's arithmetic).
__global__ void __launch_bounds__(256) dn_color_kernel(float4* __restrict__ out, const float4* __restrict__ accum,
                                                       const uint32_t* __restrict__ calls, size_t npix, float inv)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const float4 a = accum[i];
    if (calls) {
        const uint32_t c = calls[i];
        const float n = (float)(c > 1u ? c : 1u);
        out[i] = make_float4(a.x / n, a.y / n, a.z / n, a.w / n);
    } else {
        out[i] = make_float4(a.x * inv, a.y * inv, a.z * inv, a.w * inv);
    }
}

// ---------------------------------------------------------------------------------------------
// The filter.  Prepare repacks what a tap needs into three float4 per pixel, so an iteration reads
// 48 B per tap: I = (colour / D, keep as 0 / 1), G0 = (N, id bits), G1 = (P, t).
// ---------------------------------------------------------------------------------------------
struct DenoiseArgs {
    const float4* color;        // C
    const float4* plane0;       // (A, id)
    const float4* plane1;       // (N, t)
    const float4* plane2;       // (P, flags)
    float4* g0;                 // (N, id)
    float4* g1;                 // (P, t)
    const float4* src;          // iteration input  (I, keep)
    float4* dst;                // iteration output / prepare's I / finish's out
    uint32_t width, height;
    uint32_t step;              // s
    float ss;                   // sigma_i * sigma_i
    float sigmaPlane;
    uint32_t normalPower;
    uint32_t flags;
};

PT_DEV bool dn_finite(float x) { return x - x == 0.0f; }

PT_DEV f3 dn_divisor(const float4 a, uint32_t flags)
{
    if (!(flags & PT_DENOISE_DEMODULATE)) return mk(1.0f, 1.0f, 1.0f);
    const float lo = 1.0f / 64.0f;
    return mk(a.x > lo ? a.x : lo, a.y > lo ? a.y : lo, a.z > lo ? a.z : lo);
}

__global__ void __launch_bounds__(256) dn_prepare_kernel(DenoiseArgs A)
{
    const size_t npix = (size_t)A.width * A.height;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const float4 c = A.color[i], a = A.plane0[i], n = A.plane1[i], p = A.plane2[i];
    const uint32_t fl = __float_as_uint(p.w);
    const bool keep = (fl & PT_FEATURE_HIT) && !(fl & PT_FEATURE_EMISSIVE) && dn_finite(c.x) && dn_finite(c.y) &&
                      dn_finite(c.z) && dn_finite(n.x) && dn_finite(n.y) && dn_finite(n.z) && dn_finite(p.x) &&
                      dn_finite(p.y) && dn_finite(p.z);
    const f3 D = dn_divisor(a, A.flags);
    A.dst[i] = make_float4(c.x / D.x, c.y / D.y, c.z / D.z, __uint_as_float(keep ? 1u : 0u));
    A.g0[i] = make_float4(n.x, n.y, n.z, a.w);
    A.g1[i] = make_float4(p.x, p.y, p.z, n.w);
}

// One tap of the rule (pt_hip.h), in its operation order.  Returns nothing for a skipped tap: the
// caller selects.
PT_DEV void dn_tap(const DenoiseArgs& A, float h, const float4 Ip, const float4 Np, const float4 Pp, float mm,
                   const float4 Iq, const float4 Nq, const float4 Pq, float& sumW, f3& sumI)
{
    const bool skip = __float_as_uint(Iq.w) == 0u ||
                      ((A.flags & PT_DENOISE_SAME_PRIMITIVE) && __float_as_uint(Nq.w) != __float_as_uint(Np.w));
    float c = (Np.x * Nq.x + Np.y * Nq.y) + Np.z * Nq.z;
    c = c > 0.0f ? c : 0.0f;
    for (uint32_t k = 0; k < A.normalPower; ++k) c = c * c;
    const float ex = Pq.x - Pp.x, ey = Pq.y - Pp.y, ez = Pq.z - Pp.z;
    const float g = (Np.x * ex + Np.y * ey) + Np.z * ez;
    const float wp = 1.0f / (1.0f + (g * g) / mm);
    const float dr = Iq.x - Ip.x, dg = Iq.y - Ip.y, db = Iq.z - Ip.z;
    const float d2 = (dr * dr + dg * dg) + db * db;
    const float wc = 1.0f / (1.0f + d2 / A.ss);
    const float w = ((h * c) * wp) * wc;
    const float nW = sumW + w;
    const float nx = sumI.x + w * Iq.x, ny = sumI.y + w * Iq.y, nz = sumI.z + w * Iq.z;
    sumW = skip ? sumW : nW;
    sumI.x = skip ? sumI.x : nx;
    sumI.y = skip ? sumI.y : ny;
    sumI.z = skip ? sumI.z : nz;
}

// One iteration.  A workgroup of 256 lanes takes a tile of 32 x 8 pixels, one pixel per lane.
// STAGED: the tile and its halo of 2 s pixels, (32 + 4 s) x (8 + 4 s) texels of 48 B, are copied to LDS
// first (texels outside the image as not kept), so each global texel is fetched once per workgroup and
// not once per tap: 20.3 KB at s = 1, 30 KB at s = 2, 54 KB at s = 4 (two workgroups per CU); s >= 8
// would need 120 KB and its taps share no cache lines anyway.  Unstaged: the taps are read through the
// caches.  Same operations either way, so the same words.
constexpr uint32_t kDnTileW = PT_DENOISE_TILE_W, kDnTileH = PT_DENOISE_TILE_H;
static_assert(kDnTileW * kDnTileH == 256, "one pixel per lane");

template <bool STAGED>
__global__ void __launch_bounds__(256, 4) dn_iter_kernel(DenoiseArgs A)
{
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
            float4 vi = make_float4(0.0f, 0.0f, 0.0f, 0.0f), vn = vi, vp = vi;
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
    if (__float_as_uint(Ip.w) == 0u) {                   // not kept: handed on unchanged
        A.dst[pi] = Ip;
        return;
    }
    const float4 Np = STAGED ? lds4[RN + cIdx] : A.g0[pi];
    const float4 Pp = STAGED ? lds4[2u * RN + cIdx] : A.g1[pi];
    const float m = A.sigmaPlane * Pp.w;
    const float mm = m * m;
    const float kk[3] = {3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    float sumW = 0.0f;
    f3 sumI = mk(0.0f, 0.0f, 0.0f);
    // a row of five taps (60 registers of loads) in flight at a time: all 25 at once took 234 VGPRs and
    // left two waves per SIMD to hide the loads of a bandwidth-bound kernel
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
                if (!inside) Iq.w = 0.0f;                // skipped, as a texel that is not kept
            }
            dn_tap(A, h, Ip, Np, Pp, mm, Iq, Nq, Pq, sumW, sumI);
        }
    }
    A.dst[pi] = make_float4(sumI.x / sumW, sumI.y / sumW, sumI.z / sumW, Ip.w);
}

__global__ void __launch_bounds__(256) dn_finish_kernel(DenoiseArgs A)
{
    const size_t npix = (size_t)A.width * A.height;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const float4 c = A.color[i], I = A.src[i];
    const f3 D = dn_divisor(A.plane0[i], A.flags);
    const bool keep = __float_as_uint(I.w) != 0u;
    A.dst[i] = make_float4(keep ? I.x * D.x : c.x, keep ? I.y * D.y : c.y, keep ? I.z * D.z : c.z, 1.0f);
}

// pt_tonemap's arithmetic with divisor 1 over a float4 image.
__global__ void __launch_bounds__(256) tonemap_denoised_kernel(uchar4* out, const float4* img, size_t npix)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    out[i] = tonemap_pixel(img[i], 1u);
}
