// Guided upsampling of a low-resolution image to the full frame (pt_upsample, pt_upsample_image; rule 8 of
// include/pt_hip.h, restated in tests/upsample_model.py).
// Part of the trace kernel's single translation unit: included by pt_kernels.hip inside its anonymous
// namespace after pt_dev_despike.h; not a standalone header.
// Nothing here is used by an existing kernel, and no existing kernel or parameter struct changes.
#pragma once

struct UpsampleArgs {
    const float4* color;        // low C
    const float4* lo0;          // low (A, id)
    const float4* lo1;          // low (N, t)
    const float4* lo2;          // low (P, flags)
    float4* t0;                 // low (I where kept, else C; class)
    float4* t1;                 // low (N, id)
    float4* t2;                 // low (P, flags)
    const float4* hi0;          // high (A, id)
    const float4* hi1;          // high (N, t)
    const float4* hi2;          // high (P, flags)
    float4* out;                // high
    uint32_t* counts;           // two words, zeroed before the launch: ring 2, nearest
    uint32_t w, h, W, H;
    float sigmaPlane;
    uint32_t normalPower;
    uint32_t flags;
};

constexpr uint32_t kUsKept = 1u, kUsRaw = 2u;   // a low texel's class: kept; finite but not kept; 0 = neither

// u, the high pixel centre x in low pixel units (the rule's operations; v likewise), and the nearest low index
PT_DEV float us_coord(uint32_t x, float s) { return ((float)x + 0.5f) * s - 0.5f; }
PT_DEV int32_t us_nearest(uint32_t x, float s, int32_t n) { return min((int32_t)(((float)x + 0.5f) * s), n - 1); }

// ---------------------------------------------------------------------------------------------
// 1. What a tap needs, 48 B instead of the 64 B of the colour and the three planes: a kept texel is only ever read
// for I and a texel that is not kept only for C, so one float4 holds either, with the class beside it.
// The divisor of a low pixel is the mean of the high pixels' divisors over its footprint (the high pixels whose
// nearest low pixel it is) on its primitive: its own albedo is one sample of a texture that its colour averages.
// The candidates are a rectangle one high pixel wider than the footprint on every side, membership is the rule's own
// test, so the bounds decide nothing; they are whole numbers formed in 64 bits.
// Flat, one low pixel per lane.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) upsample_prepare_kernel(UpsampleArgs A)
{
    const size_t npix = (size_t)A.w * A.h;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const float4 c = A.color[i], a = A.lo0[i], n = A.lo1[i], p = A.lo2[i];
    const uint32_t fl = __float_as_uint(p.w);
    const bool raw = dn_finite(c.x) && dn_finite(c.y) && dn_finite(c.z);
    const bool keep = (fl & PT_FEATURE_HIT) && !(fl & PT_FEATURE_EMISSIVE) && raw && dn_finite(n.x) && dn_finite(n.y) &&
                      dn_finite(n.z) && dn_finite(p.x) && dn_finite(p.y) && dn_finite(p.z);
    f3 D = dn_divisor(a, A.flags);
    if (keep && (A.flags & PT_DENOISE_DEMODULATE)) {
        const uint32_t qy = (uint32_t)(i / A.w), qx = (uint32_t)(i - (size_t)qy * A.w);
        const float sx = (float)A.w / (float)A.W, sy = (float)A.h / (float)A.H;
        const uint64_t ax = (uint64_t)qx * A.W / A.w, bx = ((uint64_t)(qx + 1u) * A.W - 1u) / A.w + 1u;
        const uint64_t ay = (uint64_t)qy * A.H / A.h, by = ((uint64_t)(qy + 1u) * A.H - 1u) / A.h + 1u;
        const uint32_t xa = (uint32_t)(ax > 0u ? ax - 1u : 0u), xb = (uint32_t)(bx < A.W ? bx : A.W - 1u);
        const uint32_t ya = (uint32_t)(ay > 0u ? ay - 1u : 0u), yb = (uint32_t)(by < A.H ? by : A.H - 1u);
        f3 S = mk(0.0f, 0.0f, 0.0f);
        uint32_t members = 0u;
        for (uint32_t y = ya; y <= yb; ++y) {
            const bool row = us_nearest(y, sy, (int32_t)A.h) == (int32_t)qy;
            for (uint32_t x = xa; x <= xb; ++x) {
                const float4 ap = A.hi0[(size_t)y * A.W + x];
                const bool in = row && us_nearest(x, sx, (int32_t)A.w) == (int32_t)qx &&
                                __float_as_uint(ap.w) == __float_as_uint(a.w);
                const f3 Dp = dn_divisor(ap, A.flags);
                S.x = in ? S.x + Dp.x : S.x;
                S.y = in ? S.y + Dp.y : S.y;
                S.z = in ? S.z + Dp.z : S.z;
                members = in ? members + 1u : members;
            }
        }
        const float fn = (float)members;
        D = members != 0u ? mk(S.x / fn, S.y / fn, S.z / fn) : D;
    }
    const uint32_t cls = keep ? kUsKept : (raw ? kUsRaw : 0u);
    A.t0[i] = make_float4(keep ? c.x / D.x : c.x, keep ? c.y / D.y : c.y, keep ? c.z / D.z : c.z, __uint_as_float(cls));
    A.t1[i] = make_float4(n.x, n.y, n.z, a.w);
    A.t2[i] = p;
}

// One guided tap in the rule's operation order: the sums move only where the tap is not skipped.
PT_DEV void us_tap(const UpsampleArgs& A, float b, bool inside, const float4 Np, const float4 Pp, uint32_t idp, float mm,
                   const float4 Iq, const float4 Nq, const float4 Pq, float& sumW, f3& sumI)
{
    const bool skip = !inside || __float_as_uint(Iq.w) != kUsKept ||
                      ((A.flags & PT_DENOISE_SAME_PRIMITIVE) && __float_as_uint(Nq.w) != idp);
    float c = (Np.x * Nq.x + Np.y * Nq.y) + Np.z * Nq.z;
    c = c > 0.0f ? c : 0.0f;
    for (uint32_t k = 0; k < A.normalPower; ++k) c = c * c;
    const float ex = Pq.x - Pp.x, ey = Pq.y - Pp.y, ez = Pq.z - Pp.z;
    const float g = (Np.x * ex + Np.y * ey) + Np.z * ez;
    const float wp = 1.0f / (1.0f + (g * g) / mm);
    const float wgt = (b * c) * wp;
    const float nW = sumW + wgt;
    const float nx = sumI.x + wgt * Iq.x, ny = sumI.y + wgt * Iq.y, nz = sumI.z + wgt * Iq.z;
    sumW = skip ? sumW : nW;
    sumI.x = skip ? sumI.x : nx;
    sumI.y = skip ? sumI.y : ny;
    sumI.z = skip ? sumI.z : nz;
}

// ---------------------------------------------------------------------------------------------
// 2. One high pixel per lane on the filter's 32 x 8 tile.  u and v do not decrease with x and y (every operation
// that forms them is monotone), so the ring-1 taps of a tile lie in the low rectangle from (floor u, floor v) of its
// first pixel to (floor u + 1, floor v + 1) of its last pixel inside the image: at most 32 sx + 3 by 8 sy + 3 texels,
// 35 x 11 at sx = sy = 1.
// STAGED: that rectangle is copied to LDS first (a texel outside the low image as class 0, which every tap skips),
// 385 texels of 48 B = 18,480 B at the most behind 32 B for the counts, so each low texel is fetched once per
// workgroup and not once per lane that reaches it (16 times at a ratio of 2 by 2).  Adjacent lanes read the same or
// adjacent 16-byte texels of one row.  A rectangle that did not fit (none does: see above) would be read through the
// caches, never past the allocation.  Unstaged: the taps are read through the caches.  The same operations either
// way, so the same words.
// Ring 2 and the nearest pixel are rare and always go through the caches.  A lane outside the image computes its
// tile's last pixel again and stores and counts nothing.
// The two counts: one ballot per wave, summed over the workgroup's four waves in LDS, then at most one atomic add
// each; integer adds commute, so the counts are the same in any order.
// The per-pixel body below (from the loads of Ap, Np, Pp to the nearest-pixel fallback) has a second copy,
// us_resolve_pixel in pt_dev_upsample_resolve.h, which must stay operation for operation the same: a change to one
// needs the other.  tests/test_gpu_upsample_resolve.py holds them together (the box mean of this kernel's image).
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kUsMaxRN = (kDnTileW + 3u) * (kDnTileH + 3u);
constexpr uint32_t kUsCountF4 = 2u;             // 8 words ahead of the staged texels: 4 waves x 2 counts

template <bool STAGED>
__global__ void __launch_bounds__(256) upsample_kernel(UpsampleArgs A)
{
    const uint32_t lx = threadIdx.x & (kDnTileW - 1u), ly = threadIdx.x / kDnTileW;
    const uint32_t X0 = blockIdx.x * kDnTileW, Y0 = blockIdx.y * kDnTileH;
    const uint32_t X1 = min(X0 + kDnTileW - 1u, A.W - 1u), Y1 = min(Y0 + kDnTileH - 1u, A.H - 1u);
    const bool inb = X0 + lx < A.W && Y0 + ly < A.H;
    const uint32_t x = min(X0 + lx, X1), y = min(Y0 + ly, Y1);
    const int32_t w = (int32_t)A.w, h = (int32_t)A.h;
    const float sx = (float)A.w / (float)A.W, sy = (float)A.h / (float)A.H;
    // the tile's low rectangle (uniform)
    const int32_t gx0 = (int32_t)floorf(us_coord(X0, sx)), gy0 = (int32_t)floorf(us_coord(Y0, sy));
    const uint32_t RW = (uint32_t)((int32_t)floorf(us_coord(X1, sx)) + 2 - gx0);
    const uint32_t RH = (uint32_t)((int32_t)floorf(us_coord(Y1, sy)) + 2 - gy0);
    const uint32_t RN = RW * RH;
    const bool staged = STAGED && RN <= kUsMaxRN;
    float4* const sT = lds4 + kUsCountF4;
    if (staged) {
        for (uint32_t k = threadIdx.x; k < RN; k += 256u) {
            const uint32_t ry = k / RW, rx = k - ry * RW;
            const int32_t gx = gx0 + (int32_t)rx, gy = gy0 + (int32_t)ry;
            float4 v0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), v1 = v0, v2 = v0;
            if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
                const size_t gi = (size_t)gy * A.w + (uint32_t)gx;
                v0 = A.t0[gi];
                v1 = A.t1[gi];
                v2 = A.t2[gi];
            }
            sT[k] = v0;
            sT[RN + k] = v1;
            sT[2u * RN + k] = v2;
        }
        __syncthreads();
    }
    const size_t pi = (size_t)y * A.W + x;
    const float4 Ap = A.hi0[pi], Np = A.hi1[pi], Pp = A.hi2[pi];
    const uint32_t idp = __float_as_uint(Ap.w), flp = __float_as_uint(Pp.w);
    const float u = us_coord(x, sx), v = us_coord(y, sy);
    const float fu = floorf(u), fv = floorf(v);
    const float fx = u - fu, fy = v - fv;
    const int32_t x0 = (int32_t)fu, y0 = (int32_t)fv;
    const bool guide = (flp & PT_FEATURE_HIT) && !(flp & PT_FEATURE_EMISSIVE) && dn_finite(Np.x) && dn_finite(Np.y) &&
                       dn_finite(Np.z) && dn_finite(Pp.x) && dn_finite(Pp.y) && dn_finite(Pp.z);
    const float m = A.sigmaPlane * Np.w;
    const float mm = m * m;
    float sumW = 0.0f, sumB = 0.0f;
    f3 sumI = mk(0.0f, 0.0f, 0.0f), sumC = mk(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int32_t j = 0; j < 2; ++j) {
#pragma unroll
        for (int32_t i = 0; i < 2; ++i) {
            const int32_t qx = x0 + i, qy = y0 + j;
            const bool inside = qx >= 0 && qx < w && qy >= 0 && qy < h;
            float4 Iq, Nq, Pq;
            if (staged) {
                const uint32_t k = (uint32_t)(qy - gy0) * RW + (uint32_t)(qx - gx0);
                Iq = sT[k];
                Nq = sT[RN + k];
                Pq = sT[2u * RN + k];
            } else {
                const size_t qi = (size_t)min(max(qy, 0), h - 1) * A.w + (uint32_t)min(max(qx, 0), w - 1);
                Iq = A.t0[qi];
                Nq = A.t1[qi];
                Pq = A.t2[qi];
            }
            const float b = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy);
            us_tap(A, b, inside, Np, Pp, idp, mm, Iq, Nq, Pq, sumW, sumI);
            // the same tap for a pixel without a guide: the raw colour under b alone
            const bool skipU = !inside || __float_as_uint(Iq.w) != kUsRaw || __float_as_uint(Pq.w) != flp ||
                               ((flp & PT_FEATURE_EMISSIVE) && __float_as_uint(Nq.w) != idp);
            const float nB = sumB + b;
            const float cx = sumC.x + b * Iq.x, cy = sumC.y + b * Iq.y, cz = sumC.z + b * Iq.z;
            sumB = skipU ? sumB : nB;
            sumC.x = skipU ? sumC.x : cx;
            sumC.y = skipU ? sumC.y : cy;
            sumC.z = skipU ? sumC.z : cz;
        }
    }
    bool wide = false, nearest = false;
    float ox, oy, oz;
    if (guide) {
        bool have = dn_finite(sumW) && sumW > 0.0f;
        if (!have) {
            sumW = 0.0f;
            sumI = mk(0.0f, 0.0f, 0.0f);
#pragma unroll 1
            for (int32_t dy = -1; dy <= 2; ++dy) {
#pragma unroll
                for (int32_t dx = -1; dx <= 2; ++dx) {
                    if ((dx == 0 || dx == 1) && (dy == 0 || dy == 1)) continue;      // ring 1 (uniform)
                    const int32_t qx = x0 + dx, qy = y0 + dy;
                    const bool inside = qx >= 0 && qx < w && qy >= 0 && qy < h;
                    const size_t qi = (size_t)min(max(qy, 0), h - 1) * A.w + (uint32_t)min(max(qx, 0), w - 1);
                    const float ex = (float)qx - u, ey = (float)qy - v;
                    const float b = 1.0f / (1.0f + (ex * ex + ey * ey));
                    us_tap(A, b, inside, Np, Pp, idp, mm, A.t0[qi], A.t1[qi], A.t2[qi], sumW, sumI);
                }
            }
            have = dn_finite(sumW) && sumW > 0.0f;
            wide = have;
            nearest = !have;
        }
        const f3 D = dn_divisor(Ap, A.flags);
        ox = (sumI.x / sumW) * D.x;
        oy = (sumI.y / sumW) * D.y;
        oz = (sumI.z / sumW) * D.z;
    } else {
        nearest = !(dn_finite(sumB) && sumB > 0.0f);       // (not counted: see below)
        ox = sumC.x / sumB;
        oy = sumC.y / sumB;
        oz = sumC.z / sumB;
    }
    if (nearest) {
        const int32_t xn = us_nearest(x, sx, w), yn = us_nearest(y, sy, h);
        const float4 c = A.color[(size_t)yn * A.w + (uint32_t)xn];
        ox = c.x;
        oy = c.y;
        oz = c.z;
    }
    if (inb) A.out[pi] = make_float4(ox, oy, oz, 1.0f);
    // the counts are of guided pixels inside the image
    uint32_t* const votes = reinterpret_cast<uint32_t*>(lds4);
    const unsigned long long nWide = __ballot(inb && wide ? 1 : 0), nNear = __ballot(inb && guide && nearest ? 1 : 0);
    if ((threadIdx.x & 63u) == 0u) {
        votes[2u * (threadIdx.x >> 6)] = (uint32_t)__popcll(nWide);
        votes[2u * (threadIdx.x >> 6) + 1u] = (uint32_t)__popcll(nNear);
    }
    __syncthreads();
    if (threadIdx.x < 2u) {
        const uint32_t n = (votes[threadIdx.x] + votes[2u + threadIdx.x]) + (votes[4u + threadIdx.x] + votes[6u + threadIdx.x]);
        if (n != 0u) atomicAdd(A.counts + threadIdx.x, n);
    }
}
