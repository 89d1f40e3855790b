// Despike: the same-surface firefly clamp ahead of the filters (pt_despike, pt_despike_image; rule 6 of
// include/pt_hip.h, restated in tests/despike_model.py).
// Part of the trace kernel's single translation unit: included by pt_kernels.hip inside its anonymous
// namespace after pt_dev_adaptive_variance.h; not a standalone header.
// Nothing here is used by an existing kernel, and no existing kernel or parameter struct changes.
#pragma once

struct DespikeArgs {
    const float4* color;        // C
    const float4* plane0;       // (A, id)
    const float4* plane1;       // (N, t)
    const float4* plane2;       // (P, flags)
    float4* t0;                 // (N, l), l = NaN where the pixel is not ok
    float4* t1;                 // (P, id)
    float4* out;
    uint32_t* count;            // one word, zeroed before the launch
    uint32_t width, height;
    uint32_t radius, rank;
    float factor, floor;
    uint32_t minNeighbors;
    float sigmaPlane, normalCosMin;
    uint32_t flags;
};

// ---------------------------------------------------------------------------------------------
// 1. What a tap needs, 32 B instead of the 64 B of the colour and the three planes: (N, l) and (P, id).  "Not ok"
// travels as a luminance that is not finite, which an ok pixel never has (the layout of avar_prepare_kernel).
// Flat, one pixel per lane.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) despike_prepare_kernel(DespikeArgs A)
{
    const size_t npix = (size_t)A.width * A.height;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const float4 c = A.color[i], a = A.plane0[i], n4 = A.plane1[i], p4 = A.plane2[i];
    const uint32_t fl = __float_as_uint(p4.w);
    const f3 D = dn_divisor(a, A.flags);
    const float l = sv_lum(c.x / D.x, c.y / D.y, c.z / D.z);
    const bool ok = (fl & PT_FEATURE_HIT) && !(fl & PT_FEATURE_EMISSIVE) && dn_finite(l) && dn_finite(n4.x) &&
                    dn_finite(n4.y) && dn_finite(n4.z) && dn_finite(p4.x) && dn_finite(p4.y) && dn_finite(p4.z);
    A.t0[i] = make_float4(n4.x, n4.y, n4.z, ok ? l : __uint_as_float(0x7fc00000u));
    A.t1[i] = make_float4(p4.x, p4.y, p4.z, a.w);
}

// One compare-and-swap step of the insertion into top[]: after it `hi` is the larger (strictly: an equal value
// stays where it is) and `v` the one handed down.
PT_DEV void ds_step(float& v, float& hi)
{
    const bool up = v > hi;
    const float down = up ? hi : v;
    hi = up ? v : hi;
    v = down;
}

// ---------------------------------------------------------------------------------------------
// 2. The window, the limit and the clamp, over what the flat pass wrote.  The filter's 32 x 8 tile, one pixel per
// lane.  top[0..3] are four registers: every tap runs the four compare-and-select steps, and M is picked by
// selects, so neither `rank` nor a loop index ever indexes an array (no scratch).
// STAGED: the tile and its halo of `radius`, at most 38 x 14 texels of 32 B = 17,024 B of LDS (and 16 B of votes
// behind the largest region), are copied first (a texel outside the image as not ok), so each texel is fetched once
// per workgroup and not once per tap.  Adjacent lanes read adjacent 16-byte texels of one row: the b128 reads of a
// quarter-wave cover all 64 banks once, as the filter's staged form.  A tile without an ok pixel copies nothing.
// Unstaged: the taps are read through the caches.  The same operations either way, so the same words.
// The spikes are counted with one ballot and at most one atomic add per wave; integer adds commute, so the
// count is the same in any order.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kDsMaxRadius = 3u;
constexpr uint32_t kDsMaxRN = (kDnTileW + 2u * kDsMaxRadius) * (kDnTileH + 2u * kDsMaxRadius);

template <bool STAGED>
__global__ void __launch_bounds__(256) despike_kernel(DespikeArgs A)
{
    const uint32_t lx = threadIdx.x & (kDnTileW - 1u), ly = threadIdx.x / kDnTileW;
    const uint32_t x0 = blockIdx.x * kDnTileW, y0 = blockIdx.y * kDnTileH;
    const uint32_t x = x0 + lx, y = y0 + ly;
    const int32_t W = (int32_t)A.width, H = (int32_t)A.height;
    const int32_t R = (int32_t)A.radius;
    const uint32_t RW = kDnTileW + 2u * A.radius, RH = kDnTileH + 2u * A.radius, RN = RW * RH;
    const bool inb = x < A.width && y < A.height;
    const size_t pi = inb ? (size_t)y * A.width + x : 0;       // a lane outside the image loads pixel 0 and stores nothing
    const float4 c = A.color[pi];
    const float4 Np = A.t0[pi];
    const bool ok = inb && dn_finite(Np.w);
    bool live = true;                                          // the workgroup has an ok pixel (uniform)
    if (STAGED) {
        uint32_t* votes = reinterpret_cast<uint32_t*>(lds4 + 2u * kDsMaxRN);
        const uint32_t vote = __any(ok ? 1 : 0) ? 1u : 0u;
        if ((threadIdx.x & 63u) == 0u) votes[threadIdx.x >> 6] = vote;
        __syncthreads();
        live = (votes[0] | votes[1] | votes[2] | votes[3]) != 0u;
        if (live) {
            const int32_t gx0 = (int32_t)x0 - R, gy0 = (int32_t)y0 - R;
            for (uint32_t k = threadIdx.x; k < RN; k += 256u) {
                const uint32_t ry = k / RW, rx = k - ry * RW;
                const int32_t gx = gx0 + (int32_t)rx, gy = gy0 + (int32_t)ry;
                float4 v0 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0x7fc00000u)), v1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                    const size_t gi = (size_t)gy * A.width + (uint32_t)gx;
                    v0 = A.t0[gi];
                    v1 = A.t1[gi];
                }
                lds4[k] = v0;
                lds4[RN + k] = v1;
            }
            __syncthreads();
        }
    }
    float ox = c.x, oy = c.y, oz = c.z;
    bool spike = false;
    if (ok && live) {
        const uint32_t cIdx = (ly + A.radius) * RW + (lx + A.radius);     // the pixel's texel in the staged region
        const float4 Pp = STAGED ? lds4[RN + cIdx] : A.t1[pi];
        const float m = A.sigmaPlane * A.plane1[pi].w;
        const float mm = m * m;
        const float ninf = __uint_as_float(0xff800000u);
        float top0 = ninf, top1 = ninf, top2 = ninf, top3 = ninf;
        uint32_t k = 0u;
#pragma unroll 1
        for (int32_t dy = -R; dy <= R; ++dy) {
#pragma unroll 1
            for (int32_t dx = -R; dx <= R; ++dx) {
                float4 Nq, Pq;
                bool inside = true;                          // a staged texel outside the image is not ok
                if (STAGED) {
                    const uint32_t qi = (uint32_t)((int32_t)cIdx + dy * (int32_t)RW + dx);
                    Nq = lds4[qi];
                    Pq = lds4[RN + qi];
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
                const bool skip = centre || !inside || !dn_finite(Nq.w) || cs < A.normalCosMin || !(g * g <= mm) ||
                                  ((A.flags & PT_DENOISE_SAME_PRIMITIVE) && __float_as_uint(Pq.w) != __float_as_uint(Pp.w));
                float v = Nq.w, n0 = top0, n1 = top1, n2 = top2, n3 = top3;
                ds_step(v, n0);
                ds_step(v, n1);
                ds_step(v, n2);
                ds_step(v, n3);
                k = skip ? k : k + 1u;
                top0 = skip ? top0 : n0;
                top1 = skip ? top1 : n1;
                top2 = skip ? top2 : n2;
                top3 = skip ? top3 : n3;
            }
        }
        const float M = A.rank == 1u ? top0 : (A.rank == 2u ? top1 : (A.rank == 3u ? top2 : top3));
        const float limit = A.factor * M + A.floor;
        const float lp = Np.w;
        spike = k >= A.minNeighbors && limit >= 0.0f && lp > limit;
        const f3 D = dn_divisor(A.plane0[pi], A.flags);
        const float s = limit / lp;
        const float sx = ((c.x / D.x) * s) * D.x, sy = ((c.y / D.y) * s) * D.y, sz = ((c.z / D.z) * s) * D.z;
        ox = spike ? sx : ox;
        oy = spike ? sy : oy;
        oz = spike ? sz : oz;
    }
    if (inb) A.out[pi] = make_float4(ox, oy, oz, 1.0f);
    const unsigned long long spikes = __ballot(spike ? 1 : 0);
    if ((threadIdx.x & 63u) == 0u && spikes != 0ull) atomicAdd(A.count, (uint32_t)__popcll(spikes));
}
