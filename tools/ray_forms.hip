// The slab test, the child-pair test and the object-space transform of the trace kernel, form against form
// (on the GPU).
//
// The reference forms are the packed-FP32 ones the kernel had before they were rewritten with plain FP32
// instructions: slab_lo_x, cb_pair and to_local as they stood, on register pairs (v_pk_add_f32 /
// v_pk_mul_f32), kept here word for word under the names ref_*.  The forms under test are the shipped ones:
// this file includes the kernel's own headers in the kernel's order and is built with the kernel's
// code-generation flags (Makefile, HIPCODEGEN) into pathtracercuda_amd/lib/ray_forms.  Inputs are made on the
// device from the case index, both forms run in the same thread, and the differing output words are counted
// on the device; tests/test_gpu_ray_forms.py asserts the counts.
//
//   ray_forms [--mutate]
//
// Cases (S = the 25 values +-0, +-2^-149, +-2^-127, +-2^-126, +-2^-125, +-0.001, +-1, +-3, +-2^125, +-2^127,
// +-FLT_MAX, +-inf, NaN):
//   slab      one axis at a time, (box low, box high, origin, reciprocal) over the whole of S^4, the other two
//             axes benign seeded values: 3 x 25^4 cases; lo and X of the per-ray form and of the all-fast form
//   cb_pair   2^20 seeded records and rays (one direction component in sixteen is zero), t_max by case index
//             from {FLT_MAX, 1, 0.001, 0, NaN}; the six fields of ChildPair, per-ray and all-fast form
//   to_local  every pair of the 18 input words (12 row words, 6 ray words) over S^2, the rest seeded:
//             153 x 25^2 cases; then 2^20 seeded cases; the six words of LocalRay
// --mutate evaluates one product of the form under test with an FMA (a copy of the form, in this file): the
// negative control of the comparison -- it must find differences.
// Prints one JSON line {"slab": {"cases": n, "diff_words": d}, "cb_pair": ..., "to_local": ..., "mutate": b}.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <cmath>

#include "../pathtracercuda_amd/csrc/pt_math.h"
#include "../pathtracercuda_amd/csrc/pt_leaf_forms.h"
#include "../include/pt_hip.h"

using namespace pt;

namespace {

#include "../pathtracercuda_amd/csrc/pt_dev_scene.h"
#include "../pathtracercuda_amd/csrc/pt_dev_walk.h"     // (the later headers of the kernel hold none of the three)

#define CHECK(call)                                                                                   \
    do {                                                                                              \
        const hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) {                                                                       \
            fprintf(stderr, "ray_forms: %s: %s\n", #call, hipGetErrorString(e_));                     \
            exit(1);                                                                                  \
        }                                                                                             \
    } while (0)

// ---- the reference: the packed forms, word for word ------------------------------------------------
typedef float rf2v __attribute__((ext_vector_type(2)));   // lowers to v_pk_{add,mul}_f32 on gfx950

PT_DEV rf2v rf2(float a, float b) { return (rf2v){a, b}; }

struct RefSlabRay {
    rf2v ox2, oy2, oz2, ix2, iy2, iz2;
    f3 o;
    float ix, iy, iz;
    bool fast;
};

template <bool ALLFAST = false>
PT_DEV float ref_slab_lo_x(const RefSlabRay& R, rf2v bx, rf2v by, rf2v bz, float tMin, float& X)
{
    if (ALLFAST || R.fast) {
        const rf2v tx = (bx - R.ox2) * R.ix2;
        const rf2v ty = (by - R.oy2) * R.iy2;
        const rf2v tz = (bz - R.oz2) * R.iz2;
        X = __builtin_fminf(__builtin_fmaxf(tx.x, tx.y), __builtin_fminf(__builtin_fmaxf(ty.x, ty.y), __builtin_fmaxf(tz.x, tz.y)));
        return __builtin_fmaxf(__builtin_fmaxf(tMin, __builtin_fminf(tx.x, tx.y)),
                               __builtin_fmaxf(__builtin_fminf(ty.x, ty.y), __builtin_fminf(tz.x, tz.y)));
    }
    float lo = tMin, hi = __builtin_inff();
    const float inv[3] = {R.ix, R.iy, R.iz};
    const float org[3] = {R.o.x, R.o.y, R.o.z};
    const rf2v b[3] = {bx, by, bz};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float t0 = (b[k].x - org[k]) * inv[k], t1 = (b[k].y - org[k]) * inv[k];
        if (inv[k] < 0.0f) { const float tmp = t0; t0 = t1; t1 = tmp; }
        lo = t0 > lo ? t0 : lo;
        hi = t1 < hi ? t1 : hi;
    }
    X = hi;
    return lo;
}

// The mutated copy of the form under test (--mutate): the plain-FP32 fast branch with the first product
// as one FMA, (b - o) * i = fma(b, i, -(o * i)).
template <bool ALLFAST = false>
PT_DEV float mut_slab_lo_x(const RefSlabRay& R, rf2v bx, rf2v by, rf2v bz, float tMin, float& X)
{
    if (ALLFAST || R.fast) {
        const float tx0 = __builtin_fmaf(bx.x, R.ix, -(R.o.x * R.ix)), tx1 = (bx.y - R.o.x) * R.ix;
        const float ty0 = (by.x - R.o.y) * R.iy, ty1 = (by.y - R.o.y) * R.iy;
        const float tz0 = (bz.x - R.o.z) * R.iz, tz1 = (bz.y - R.o.z) * R.iz;
        X = __builtin_fminf(__builtin_fmaxf(tx0, tx1), __builtin_fminf(__builtin_fmaxf(ty0, ty1), __builtin_fmaxf(tz0, tz1)));
        return __builtin_fmaxf(__builtin_fmaxf(tMin, __builtin_fminf(tx0, tx1)),
                               __builtin_fmaxf(__builtin_fminf(ty0, ty1), __builtin_fminf(tz0, tz1)));
    }
    return ref_slab_lo_x<false>(R, bx, by, bz, tMin, X);
}

// cb_pair as it stood; MUT only swaps the slab test for its mutated copy.
template <bool ALLFAST = false, bool MUT = false>
PT_DEV ChildPair ref_cb_pair(const float4& Q0, const float4& Q1, const float4& Q2, const float4& Q3, const RefSlabRay& R,
                             uint32_t negMask, float tMin, float tMax)
{
    float XL, XR;
    const float loL = MUT ? mut_slab_lo_x<ALLFAST>(R, rf2(Q0.x, Q0.y), rf2(Q0.z, Q0.w), rf2(Q1.x, Q1.y), tMin, XL)
                          : ref_slab_lo_x<ALLFAST>(R, rf2(Q0.x, Q0.y), rf2(Q0.z, Q0.w), rf2(Q1.x, Q1.y), tMin, XL);
    const float loR = MUT ? mut_slab_lo_x<ALLFAST>(R, rf2(Q2.x, Q2.y), rf2(Q2.z, Q2.w), rf2(Q1.z, Q1.w), tMin, XR)
                          : ref_slab_lo_x<ALLFAST>(R, rf2(Q2.x, Q2.y), rf2(Q2.z, Q2.w), rf2(Q1.z, Q1.w), tMin, XR);
    const bool isNeg = (negMask & __float_as_uint(Q3.z)) != 0u;
    const uint32_t wL = __float_as_uint(Q3.x), wR = __float_as_uint(Q3.y);
    const bool hL = XL > loL && !(tMax <= loL);   // (a NaN t_max passes: slab_pass_all)
    const bool hR = XR > loR && !(tMax <= loR);
    const bool takeL = hL && (!hR || !isNeg);
    ChildPair c;
    c.push = hL && hR;
    c.any = hL || hR;
    c.wNext = takeL ? wL : wR;
    c.loNext = takeL ? loL : loR;
    c.wF = isNeg ? wL : wR;
    c.loF = isNeg ? loL : loR;
    return c;
}

PT_DEV LocalRay ref_to_local(const float4& P0, const float4& P1, const float4& r2, f3 o, f3 d)
{
    LocalRay l;
    rf2v oxy = rf2(P0.x, P0.y) * rf2(o.x, o.x);
    oxy = oxy + rf2(P0.z, P0.w) * rf2(o.y, o.y);
    oxy = oxy + rf2(P1.x, P1.y) * rf2(o.z, o.z);
    oxy = oxy + rf2(P1.z, P1.w);
    rf2v dxy = rf2(P0.x, P0.y) * rf2(d.x, d.x);
    dxy = dxy + rf2(P0.z, P0.w) * rf2(d.y, d.y);
    dxy = dxy + rf2(P1.x, P1.y) * rf2(d.z, d.z);
    l.o.x = oxy.x;
    l.o.y = oxy.y;
    l.o.z = (o.x * r2.x + o.y * r2.y + o.z * r2.z) + r2.w;
    l.d.x = dxy.x;
    l.d.y = dxy.y;
    l.d.z = d.x * r2.x + d.y * r2.y + d.z * r2.z;
    return l;
}

// The mutated copy of the form under test (--mutate): the first product of the local origin's x as an FMA.
PT_DEV LocalRay mut_to_local(const float4& P0, const float4& P1, const float4& r2, f3 o, f3 d)
{
    LocalRay l = to_local(P0, P1, r2, o, d);
    l.o.x = (__builtin_fmaf(P0.x, o.x, P0.z * o.y) + P1.x * o.z) + P1.z;
    return l;
}

// ---- the forms under test: the shipped headers' ----------------------------------------------------
PT_DEV SlabRay shipped_ray(const RefSlabRay& r)
{
    SlabRay R;
    R.o = r.o;
    R.ix = r.ix;
    R.iy = r.iy;
    R.iz = r.iz;
    R.fast = r.fast;
    return R;
}

template <bool ALLFAST>
PT_DEV float shipped_slab(const RefSlabRay& r, rf2v bx, rf2v by, rf2v bz, float tMin, float& X)
{
    return slab_lo_x<ALLFAST>(shipped_ray(r), bx.x, bx.y, by.x, by.y, bz.x, bz.y, tMin, X);
}

// ---- inputs from the case index --------------------------------------------------------------------
PT_DEV uint32_t mix(uint32_t h)
{
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}

// the k-th seeded number of case `idx` of part `part`, uniform in [lo, hi)
PT_DEV float seeded(uint32_t part, uint32_t idx, uint32_t k, float lo, float hi)
{
    const uint32_t h = mix(mix(idx * 0x9E3779B9u + part) + k * 0x7F4A7C15u);
    return lo + (hi - lo) * ((float)(h >> 8) * 0x1p-24f);
}

constexpr uint32_t kS = 25;

PT_DEV float special(uint32_t k)
{
    const uint32_t mag[12] = {0x00000000u, 0x00000001u, 0x00400000u, 0x00800000u, 0x01000000u, 0x3a83126fu,
                              0x3f800000u, 0x40400000u, 0x7e000000u, 0x7f000000u, 0x7f7fffffu, 0x7f800000u};
    if (k == 24u) return __uint_as_float(0x7fc00000u);
    return __uint_as_float(mag[k >> 1] | ((k & 1u) << 31));
}

PT_DEV RefSlabRay make_ray(f3 o, float ix, float iy, float iz)
{
    RefSlabRay R;
    R.o = o;
    R.ix = ix;
    R.iy = iy;
    R.iz = iz;
    R.fast = slab_fast_ray(true, o, ix, iy, iz);
    R.ox2 = rf2(o.x, o.x);
    R.oy2 = rf2(o.y, o.y);
    R.oz2 = rf2(o.z, o.z);
    R.ix2 = rf2(ix, ix);
    R.iy2 = rf2(iy, iy);
    R.iz2 = rf2(iz, iz);
    return R;
}

PT_DEV uint32_t differs(float a, float b) { return __float_as_uint(a) != __float_as_uint(b) ? 1u : 0u; }

// diff[0] += n; diff[3] (the cases run, counted on the device too) += 1, once per wave
PT_DEV void count(unsigned long long* diff, uint32_t n)
{
    if (n) atomicAdd(diff, (unsigned long long)n);
    const unsigned long long m = __ballot(1);
    if ((threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)m) - 1)) atomicAdd(diff + 3, (unsigned long long)__popcll(m));
}

constexpr uint32_t kSlabCases = 3u * kS * kS * kS * kS;
constexpr uint32_t kPairCases = 1u << 20;
constexpr uint32_t kLocalPairs = 153u * kS * kS;
constexpr uint32_t kLocalCases = kLocalPairs + (1u << 20);

template <bool MUT>
__global__ void __launch_bounds__(256) slab_kernel(unsigned long long* diff)
{
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= kSlabCases) return;
    const uint32_t axis = idx / (kS * kS * kS * kS);
    uint32_t r = idx % (kS * kS * kS * kS);
    float lo[3], hi[3], org[3], inv[3];
#pragma unroll
    for (uint32_t a = 0; a < 3; ++a) {
        lo[a] = seeded(0, idx, 4 * a, -2.0f, 0.0f);
        hi[a] = seeded(0, idx, 4 * a + 1, 0.0f, 2.0f);
        org[a] = seeded(0, idx, 4 * a + 2, -1.0f, 1.0f);
        const float m = seeded(0, idx, 4 * a + 3, -4.0f, 4.0f);
        inv[a] = m < 0.0f ? m - 0.5f : m + 0.5f;
        if (a == axis) {
            lo[a] = special(r % kS); r /= kS;
            hi[a] = special(r % kS); r /= kS;
            org[a] = special(r % kS); r /= kS;
            inv[a] = special(r % kS);
        }
    }
    const RefSlabRay R = make_ray(mk(org[0], org[1], org[2]), inv[0], inv[1], inv[2]);
    const rf2v bx = rf2(lo[0], hi[0]), by = rf2(lo[1], hi[1]), bz = rf2(lo[2], hi[2]);
    const float tMin = 0.001f;
    float Xr, Xt, Xrf, Xtf;
    const float lr = ref_slab_lo_x<false>(R, bx, by, bz, tMin, Xr);
    const float lrf = ref_slab_lo_x<true>(R, bx, by, bz, tMin, Xrf);
    const float lt = MUT ? mut_slab_lo_x<false>(R, bx, by, bz, tMin, Xt) : shipped_slab<false>(R, bx, by, bz, tMin, Xt);
    const float ltf = MUT ? mut_slab_lo_x<true>(R, bx, by, bz, tMin, Xtf) : shipped_slab<true>(R, bx, by, bz, tMin, Xtf);
    count(diff, differs(lr, lt) + differs(Xr, Xt) + differs(lrf, ltf) + differs(Xrf, Xtf));
}

PT_DEV uint32_t pair_differs(const ChildPair& a, const ChildPair& b)
{
    return (a.push != b.push ? 1u : 0u) + (a.any != b.any ? 1u : 0u) + (a.wNext != b.wNext ? 1u : 0u) +
           (a.wF != b.wF ? 1u : 0u) + differs(a.loNext, b.loNext) + differs(a.loF, b.loF);
}

template <bool MUT>
__global__ void __launch_bounds__(256) pair_kernel(unsigned long long* diff)
{
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= kPairCases) return;
    float b[12];
#pragma unroll
    for (uint32_t k = 0; k < 6; ++k) {            // six (low, high) slabs: L xyz, R xyz
        const float c = seeded(1, idx, 2 * k, -10.0f, 10.0f), e = seeded(1, idx, 2 * k + 1, 0.0f, 6.0f);
        b[2 * k] = c - e;
        b[2 * k + 1] = c + e;
    }
    const float4 Q0 = make_float4(b[0], b[1], b[2], b[3]), Q1 = make_float4(b[4], b[5], b[10], b[11]);
    const float4 Q2 = make_float4(b[6], b[7], b[8], b[9]);
    const uint32_t h = mix(idx ^ 0x51ED270Bu);
    const float4 Q3 = make_float4(__uint_as_float(mix(h)), __uint_as_float(mix(h + 1u)), __uint_as_float(1u << (h % 3u)),
                                  __uint_as_float(mix(h + 2u)));
    const f3 o = mk(seeded(1, idx, 12, -12.0f, 12.0f), seeded(1, idx, 13, -12.0f, 12.0f), seeded(1, idx, 14, -12.0f, 12.0f));
    f3 d = mk(seeded(1, idx, 15, -1.0f, 1.0f), seeded(1, idx, 16, -1.0f, 1.0f), seeded(1, idx, 17, -1.0f, 1.0f));
    if ((idx & 15u) == 15u) {                     // an axis-aligned ray: an infinite reciprocal, the exact form
        const uint32_t z = (idx >> 4) % 3u;
        if (z == 0u) d.x = 0.0f;
        if (z == 1u) d.y = 0.0f;
        if (z == 2u) d.z = 0.0f;
    }
    const RefSlabRay R = make_ray(o, 1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    const uint32_t negMask = (d.x < 0.0f ? 1u : 0u) | (d.y < 0.0f ? 2u : 0u) | (d.z < 0.0f ? 4u : 0u);
    const float tMaxOf[5] = {kFltMax, 1.0f, 0.001f, 0.0f, __uint_as_float(0x7fc00000u)};
    const float tMin = 0.001f, tMax = tMaxOf[idx % 5u];
    const ChildPair r0 = ref_cb_pair<false>(Q0, Q1, Q2, Q3, R, negMask, tMin, tMax);
    const ChildPair r1 = ref_cb_pair<true>(Q0, Q1, Q2, Q3, R, negMask, tMin, tMax);
    const SlabRay T = shipped_ray(R);
    const ChildPair t0 = MUT ? ref_cb_pair<false, true>(Q0, Q1, Q2, Q3, R, negMask, tMin, tMax)
                             : cb_pair<false>(Q0, Q1, Q2, Q3, T, negMask, tMin, tMax);
    const ChildPair t1 = MUT ? ref_cb_pair<true, true>(Q0, Q1, Q2, Q3, R, negMask, tMin, tMax)
                             : cb_pair<true>(Q0, Q1, Q2, Q3, T, negMask, tMin, tMax);
    count(diff, pair_differs(r0, t0) + pair_differs(r1, t1));
}

template <bool MUT>
__global__ void __launch_bounds__(256) local_kernel(unsigned long long* diff)
{
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= kLocalCases) return;
    float w[18];                                  // 12 row words (P0, P1, row 2), origin, direction
#pragma unroll
    for (uint32_t k = 0; k < 18; ++k) w[k] = seeded(2, idx, k, -8.0f, 8.0f);
    if (idx < kLocalPairs) {
        uint32_t p = idx / (kS * kS), i = 0, n = 17;   // pair number p -> words i < j
        while (p >= n) { p -= n; ++i; --n; }
        const uint32_t j = i + 1u + p;
        const float vi = special(idx % kS), vj = special((idx / kS) % kS);
#pragma unroll
        for (uint32_t k = 0; k < 18; ++k) w[k] = k == i ? vi : (k == j ? vj : w[k]);
    }
    const float4 P0 = make_float4(w[0], w[1], w[2], w[3]), P1 = make_float4(w[4], w[5], w[6], w[7]);
    const float4 r2 = make_float4(w[8], w[9], w[10], w[11]);
    const f3 o = mk(w[12], w[13], w[14]), d = mk(w[15], w[16], w[17]);
    const LocalRay r = ref_to_local(P0, P1, r2, o, d);
    const LocalRay t = MUT ? mut_to_local(P0, P1, r2, o, d) : to_local(P0, P1, r2, o, d);
    count(diff, differs(r.o.x, t.o.x) + differs(r.o.y, t.o.y) + differs(r.o.z, t.o.z) + differs(r.d.x, t.d.x) +
                    differs(r.d.y, t.d.y) + differs(r.d.z, t.d.z));
}

}  // namespace

int main(int argc, char** argv)
{
    bool mutate = false;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--mutate")) mutate = true;
        else {
            fprintf(stderr, "usage: ray_forms [--mutate]\n");
            return 1;
        }
    }
    unsigned long long* ddiff;
    unsigned long long hdiff[6] = {0, 0, 0, 0, 0, 0};     // differing words of the three parts, then their cases
    CHECK(hipMalloc(&ddiff, sizeof(hdiff)));
    CHECK(hipMemset(ddiff, 0, sizeof(hdiff)));
    const auto blocks = [](uint32_t n) { return dim3((n + 255u) / 256u); };
    if (mutate) {
        hipLaunchKernelGGL(slab_kernel<true>, blocks(kSlabCases), dim3(256), 0, 0, ddiff + 0);
        hipLaunchKernelGGL(pair_kernel<true>, blocks(kPairCases), dim3(256), 0, 0, ddiff + 1);
        hipLaunchKernelGGL(local_kernel<true>, blocks(kLocalCases), dim3(256), 0, 0, ddiff + 2);
    } else {
        hipLaunchKernelGGL(slab_kernel<false>, blocks(kSlabCases), dim3(256), 0, 0, ddiff + 0);
        hipLaunchKernelGGL(pair_kernel<false>, blocks(kPairCases), dim3(256), 0, 0, ddiff + 1);
        hipLaunchKernelGGL(local_kernel<false>, blocks(kLocalCases), dim3(256), 0, 0, ddiff + 2);
    }
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(hdiff, ddiff, sizeof(hdiff), hipMemcpyDeviceToHost));
    CHECK(hipFree(ddiff));
    printf("{\"slab\": {\"cases\": %llu, \"diff_words\": %llu}, \"cb_pair\": {\"cases\": %llu, \"diff_words\": %llu}, "
           "\"to_local\": {\"cases\": %llu, \"diff_words\": %llu}, \"mutate\": %s}\n",
           hdiff[3], hdiff[0], hdiff[4], hdiff[1], hdiff[5], hdiff[2], mutate ? "true" : "false");
    return 0;
}
