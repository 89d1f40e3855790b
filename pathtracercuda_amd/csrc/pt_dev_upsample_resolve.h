// Guided upsampling onto supersampled feature planes, resolved to the output size in the same pass
// (pt_upsample_resolve, pt_upsample_resolve_image; rule 9 of include/pt_hip.h, restated in
// tests/upsample_resolve_model.py).
// Part of the trace kernel's single translation unit: included by pt_kernels.hip inside its anonymous
// namespace after pt_dev_upsample.h; not a standalone header.
// Nothing here is used by an existing kernel, and no existing kernel or parameter struct changes.
#pragma once

struct UpsampleResolveArgs {
    UpsampleArgs U;             // rule 8's arguments at the S-times size: U.W = S * OW, U.H = S * OH; U.out is not used
    float4* out;                // OW x OH
    uint32_t OW, OH, S;
};

// Rule 8 for the one pixel (x, y) of the S-times frame, in upsample_kernel's operation order (its taps through us_tap
// and the same helpers).  ST = the tile's staged low rectangle (origin gx0, gy0; RW wide, RN texels) or null.
// This is a second copy of upsample_kernel's per-pixel body in pt_dev_upsample.h (that kernel may not change, so the
// body could not be shared): the two must stay operation for operation the same, and a change to one needs the other.
// tests/test_gpu_upsample_resolve.py compares this kernel with the box mean of that kernel's image, word for word.
PT_DEV f3 us_resolve_pixel(const UpsampleArgs& A, uint32_t x, uint32_t y, float sx, float sy, const float4* ST, int32_t gx0,
                           int32_t gy0, uint32_t RW, uint32_t RN, bool& wide, bool& near)
{
    const int32_t w = (int32_t)A.w, h = (int32_t)A.h;
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
            if (ST) {
                const uint32_t k = (uint32_t)(qy - gy0) * RW + (uint32_t)(qx - gx0);
                Iq = ST[k];
                Nq = ST[RN + k];
                Pq = ST[2u * RN + k];
            } else {
                const size_t qi = (size_t)min(max(qy, 0), h - 1) * A.w + (uint32_t)min(max(qx, 0), w - 1);
                Iq = A.t0[qi];
                Nq = A.t1[qi];
                Pq = A.t2[qi];
            }
            const float b = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy);
            us_tap(A, b, inside, Np, Pp, idp, mm, Iq, Nq, Pq, sumW, sumI);
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
    bool nearest = false;
    wide = false;
    f3 o;
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
        o = mk((sumI.x / sumW) * D.x, (sumI.y / sumW) * D.y, (sumI.z / sumW) * D.z);
    } else {
        nearest = !(dn_finite(sumB) && sumB > 0.0f);       // (not counted, as in rule 8)
        o = mk(sumC.x / sumB, sumC.y / sumB, sumC.z / sumB);
    }
    if (nearest) {
        const int32_t xn = us_nearest(x, sx, w), yn = us_nearest(y, sy, h);
        const float4 c = A.color[(size_t)yn * A.w + (uint32_t)xn];
        o = mk(c.x, c.y, c.z);
    }
    near = guide && nearest;
    return o;
}

// ---------------------------------------------------------------------------------------------
// One output pixel per lane on the filter's 32 x 8 tile; the lane walks its S x S pixels of the S-times frame, rows
// outer, and adds their rule-8 results in that order (the rule's order, so the words do not depend on the launch).
// The tile covers the S-times pixels S X0 .. S X1 + S - 1.  Their u differ by less than 32 S (w / (S W)) <= 32, so the
// floors differ by at most 32 and the ring-1 rectangle is at most 34 x 10 texels: inside rule 8's 35 x 11, and the same
// LDS (18,480 B behind the counts).  It is the rectangle an S = 1 tile has at the ratio w / W, to within the half
// S-times pixel by which the first and last centres move outwards.
// STAGED: as upsample_kernel.  A rectangle that did not fit (none does in exact arithmetic; the float32 coordinates
// of a frame wider than 2^24 are not exact) is read through the caches, never past the allocation.
// A lane outside the image computes its tile's last pixel again and stores and counts nothing.
// The counts are per S-times pixel: one ballot per wave and sub-pixel, added in a wave-uniform register, then LDS and
// at most one atomic add each per workgroup.
// ---------------------------------------------------------------------------------------------
template <bool STAGED>
__global__ void __launch_bounds__(256) upsample_resolve_kernel(UpsampleResolveArgs R)
{
    const UpsampleArgs& A = R.U;
    const uint32_t S = R.S;
    const uint32_t lx = threadIdx.x & (kDnTileW - 1u), ly = threadIdx.x / kDnTileW;
    const uint32_t X0 = blockIdx.x * kDnTileW, Y0 = blockIdx.y * kDnTileH;
    const uint32_t X1 = min(X0 + kDnTileW - 1u, R.OW - 1u), Y1 = min(Y0 + kDnTileH - 1u, R.OH - 1u);
    const bool inb = X0 + lx < R.OW && Y0 + ly < R.OH;
    const uint32_t X = min(X0 + lx, X1), Y = min(Y0 + ly, Y1);
    const int32_t w = (int32_t)A.w, h = (int32_t)A.h;
    const float sx = (float)A.w / (float)A.W, sy = (float)A.h / (float)A.H;
    // the tile's low rectangle (uniform)
    const int32_t gx0 = (int32_t)floorf(us_coord(S * X0, sx)), gy0 = (int32_t)floorf(us_coord(S * Y0, sy));
    const uint32_t RW = (uint32_t)((int32_t)floorf(us_coord(S * X1 + S - 1u, sx)) + 2 - gx0);
    const uint32_t RH = (uint32_t)((int32_t)floorf(us_coord(S * Y1 + S - 1u, sy)) + 2 - gy0);
    const uint32_t RN = RW * RH;
    const bool staged = STAGED && RW <= kDnTileW + 3u && RH <= kDnTileH + 3u;
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
    f3 sum = mk(0.0f, 0.0f, 0.0f);
    uint32_t nWide = 0u, nNear = 0u;                       // wave-uniform
#pragma unroll 1
    for (uint32_t j = 0; j < S; ++j) {
#pragma unroll 1
        for (uint32_t i = 0; i < S; ++i) {
            bool wide, near;
            const f3 o = us_resolve_pixel(A, S * X + i, S * Y + j, sx, sy, staged ? sT : nullptr, gx0, gy0, RW, RN, wide, near);
            sum.x = sum.x + o.x;
            sum.y = sum.y + o.y;
            sum.z = sum.z + o.z;
            nWide += (uint32_t)__popcll(__ballot(inb && wide ? 1 : 0));
            nNear += (uint32_t)__popcll(__ballot(inb && near ? 1 : 0));
        }
    }
    const float n = (float)(S * S);
    if (inb) R.out[(size_t)Y * R.OW + X] = make_float4(sum.x / n, sum.y / n, sum.z / n, 1.0f);
    uint32_t* const votes = reinterpret_cast<uint32_t*>(lds4);
    if ((threadIdx.x & 63u) == 0u) {
        votes[2u * (threadIdx.x >> 6)] = nWide;
        votes[2u * (threadIdx.x >> 6) + 1u] = nNear;
    }
    __syncthreads();
    if (threadIdx.x < 2u) {
        const uint32_t c = (votes[threadIdx.x] + votes[2u + threadIdx.x]) + (votes[4u + threadIdx.x] + votes[6u + threadIdx.x]);
        if (c != 0u) atomicAdd(A.counts + threadIdx.x, c);
    }
}
