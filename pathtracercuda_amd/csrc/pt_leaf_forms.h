// pt_leaf_forms.h -- the cube leaf test in its two forms and the quadric constants of a record.
// The kernel runs the exact form; the fast form is kept with its host check and its measurements
// (a consistent 0.5 % that did not clear the headline's acceptance rule).
//
// Plain C++ that compiles for the device (included by pt_kernels.hip after pt_math.h) and for the
// host (tools/leaf_forms_check.cpp compares the two cube forms over a directed grid and 10^8 random
// cases; pt_set_scene takes the quadric constants from here).  On the device 1/x is rcp_rn (exact
// form) or its fast sequence rcp_fast (fast form, inside the guard's range); both are the correctly
// rounded reciprocal (tools/fp_exhaustive.hip), which on the host is 1.0f / x.
#pragma once

#if defined(__HIPCC__)
#define PT_LF __device__ __forceinline__
#define PT_LF_HD __host__ __device__ inline
#define PT_LF_RCP(x) rcp_rn(x)
#define PT_LF_RCP_FAST(x) rcp_fast(x)
#else
#define PT_LF static inline
#define PT_LF_HD static inline
#define PT_LF_RCP(x) (1.0f / (x))
#define PT_LF_RCP_FAST(x) (1.0f / (x))
#endif

namespace pt {

// Quadric coefficients that vary among the four quadric shapes (Hittable.inl:152,176,242,273):
// B (the y^2 term), H (the y term) and J (the constant); A = C = 1, the rest are 0.  Per-primitive
// constants: pt_set_scene writes them into words y, z, w of the record's fourth quad and
// quadric_roots reads them there.  Planes and cubes get zeros (never read).
PT_LF_HD void quadric_consts(unsigned type, float& B, float& Hc, float& J)
{
    // SPHERE = 0, CYLINDER = 1, DISK = 2, CONE = 3, PARABOLOID = 4, QUAD = 5, CUBE = 6
    B = type == 0u ? 1.0f : (type == 3u ? -1.0f : 0.0f);
    Hc = type == 4u ? -1.0f : 0.0f;
    J = (type == 0u || type == 1u) ? -1.0f : 0.0f;
}

// Exact form of the unit cube's slab test, for any ray: the reference's loop as written
// (Hittable.inl:331-358, AABB.inl:46-69).  o, d: the ray in the cube's local space.
PT_LF bool cube_hit_exact(float ox, float oy, float oz, float dx, float dy, float dz, float tMin, float tMax,
                          float& tOut)
{
    float lo = tMin, hi = tMax;
    const float o[3] = {ox, oy, oz};
    const float d[3] = {dx, dy, dz};
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int a = 0; a < 3; ++a) {
        const float invD = PT_LF_RCP(d[a]);
        float t0 = (-1.0f - o[a]) * invD;
        float t1 = (1.0f - o[a]) * invD;
        if (invD < 0.0f) { const float tmp = t0; t0 = t1; t1 = tmp; }
        lo = t0 > lo ? t0 : lo;
        hi = t1 < hi ? t1 : hi;
    }
    if (hi <= lo) return false;
    tOut = lo;
    return true;
}

// The lane's half of the fast form's guard (the wave takes the fast form only when every lane in the
// test passes): every local direction component has a magnitude in [2^-125, 2^125] (rcp_fast's
// range; this excludes +-0, denormals, inf and NaN), the local origin is finite, t_max is not NaN
// and t_min is positive (it is the constant 0.001 at every call site, so that term folds away).
// min3/max3 of the magnitudes drop a NaN operand, so NaNs are caught by two unordered compares,
// which also take t_max along; one sum stands for the three origin components (finite only if all
// are; a sum of finite ones that overflows or cancels only sends the wave to the exact form).
PT_LF bool cube_fast_ok(float ox, float oy, float oz, float dx, float dy, float dz, float tMin, float tMax)
{
    const float ax = __builtin_fabsf(dx), ay = __builtin_fabsf(dy), az = __builtin_fabsf(dz);
    const float mn = __builtin_fminf(__builtin_fminf(ax, ay), az);
    const float mx = __builtin_fmaxf(__builtin_fmaxf(ax, ay), az);
    const float s = (ox + oy) + oz;
    return mn >= 0x1p-125f && mx <= 0x1p125f && !__builtin_isunordered(dx, dy) && !__builtin_isunordered(dz, tMax) &&
           __builtin_fabsf(s) < __builtin_inff() && tMin > 0.0f;
}

// Fast form: lo = max(tMin, per-axis minima), hi = min(tMax, per-axis maxima).  Exactness under
// cube_fast_ok, against cube_hit_exact step by step:
//  * No NaN arises.  Every 1/d is finite and nonzero (|d| in [2^-125, 2^125]), and -1 - o, 1 - o are
//    finite for a finite o (|o| <= FLT_MAX rounds back to FLT_MAX), so each product is a finite
//    number times a finite nonzero one: finite or +-inf, never 0 * inf.  A zero or denormal direction
//    component, the case where the reference forms 0 * inf = NaN on a ray in a face plane and its
//    selects skip the NaN, is outside the guard and takes the exact form.
//  * The swap is min/max.  -1 - o <= 1 - o (rounding is monotone), so for 1/d > 0 the pair is already
//    (min, max) and for 1/d < 0 the exact form's swap makes it so.  Two products that compare equal
//    are the same bits unless both are zeros, and both cannot be: one of |-1 - o|, |1 - o| is at
//    least 1 and |1/d| >= 2^-125, so its product is at least 2^-125.  min/max therefore never has to
//    choose between +0 and -0.
//  * The running select `t0 > lo ? t0 : lo` from lo = tMin is the maximum of tMin and the three
//    minima: without NaNs the maximum does not depend on the order (v_max3), and a tie is between
//    equal bits, because lo >= tMin > 0 and positive numbers that compare equal are identical.  So
//    tOut = lo has the reference's bits; the ray that starts inside the cube keeps lo = tMin itself.
//    -0 as an origin component is an ordinary finite value (-1 - -0 = -1); -0 as a product can only
//    lose against lo > 0.
//  * hi is only compared (`hi <= lo`), so only its value counts, not the sign of a zero.  With a NaN
//    t_max the exact form keeps hi = NaN (`t1 < NaN` is false), reports a hit and returns lo, where
//    v_min3 would drop the NaN and could report a miss (DESIGN.md 3.1 has what that did to the node
//    test).  The guard excludes a NaN t_max, so hi = min(tMax, maxima) holds number for number.
PT_LF bool cube_hit_fast(float ox, float oy, float oz, float dx, float dy, float dz, float tMin, float tMax,
                         float& tOut)
{
    const float ix = PT_LF_RCP_FAST(dx), iy = PT_LF_RCP_FAST(dy), iz = PT_LF_RCP_FAST(dz);
    // (Scalar subtracts and multiplies: one packed subtract and multiply per axis is six instructions
    // fewer but measured slower, DESIGN.md Appendix A.)
    const float x0 = (-1.0f - ox) * ix, x1 = (1.0f - ox) * ix;
    const float y0 = (-1.0f - oy) * iy, y1 = (1.0f - oy) * iy;
    const float z0 = (-1.0f - oz) * iz, z1 = (1.0f - oz) * iz;
    // (a chain, so that the first two steps of each fold into one v_max3 / v_min3)
    const float lo = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(tMin, __builtin_fminf(x0, x1)), __builtin_fminf(y0, y1)),
                                     __builtin_fminf(z0, z1));
    const float hi = __builtin_fminf(__builtin_fminf(__builtin_fminf(tMax, __builtin_fmaxf(x0, x1)), __builtin_fmaxf(y0, y1)),
                                     __builtin_fmaxf(z0, z1));
    if (hi <= lo) return false;
    tOut = lo;
    return true;
}

} // namespace pt
