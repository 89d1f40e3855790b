// Host check of the cube leaf test's two forms (pathtracercuda_amd/csrc/pt_leaf_forms.h): wherever
// the guard admits the fast (min/max) form, it must give the exact form's verdict and bit-equal tOut.
//   g++ -O2 -ffp-contract=off -fsanitize=address,undefined -o leaf_forms_check tools/leaf_forms_check.cpp
//   ./leaf_forms_check [random cases, default 100000000]
// Directed grid: every local origin and direction component over +-0, +-1, +-1 +- 1 ulp, +-2^-126,
// +-2^-125, +-2^125, +-2^127, +-inf and NaN; t_max over FLT_MAX, 1, 0.001, 0 and NaN; t_min = 0.001
// (the kernel's constant).  Random: raw bit patterns, scene-like rays, and rays on the 1/8 grid
// (ties between axes).  Prints the counts per path; both must be non-zero.  Exit status 0 = clean.
#include <cfloat>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../pathtracercuda_amd/csrc/pt_leaf_forms.h"

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float flt(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static uint64_t g_fast = 0, g_exact = 0, g_hits = 0, g_bad = 0;

static void one(const float v[6], float tMin, float tMax)
{
    float te = 0.0f, tf = 0.0f;
    const bool he = pt::cube_hit_exact(v[0], v[1], v[2], v[3], v[4], v[5], tMin, tMax, te);
    if (!pt::cube_fast_ok(v[0], v[1], v[2], v[3], v[4], v[5], tMin, tMax)) {
        ++g_exact;                      // the wave would take the exact form: nothing to compare
        return;
    }
    ++g_fast;
    const bool hf = pt::cube_hit_fast(v[0], v[1], v[2], v[3], v[4], v[5], tMin, tMax, tf);
    g_hits += he;
    if (he != hf || (he && bits(te) != bits(tf))) {
        if (g_bad++ < 10)
            fprintf(stderr, "MISMATCH o=(%a %a %a) d=(%a %a %a) tMax=%a: exact %d %a (%08x), fast %d %a (%08x)\n", v[0],
                    v[1], v[2], v[3], v[4], v[5], tMax, (int)he, te, bits(te), (int)hf, tf, bits(tf));
    }
}

static uint64_t g_s = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()
{
    g_s ^= g_s >> 12;
    g_s ^= g_s << 25;
    g_s ^= g_s >> 27;
    return g_s * 0x2545f4914f6cdd1dull;
}
static float uni(float a, float b) { return a + (b - a) * (float)((rnd() >> 40) * (1.0 / 16777216.0)); }

int main(int argc, char** argv)
{
    const uint64_t nRandom = argc > 1 ? strtoull(argv[1], nullptr, 10) : 100000000ull;
    const float tMin = 0.001f;
    const float one_up = flt(0x3f800001u), one_dn = flt(0x3f7fffffu);
    const float mags[] = {0.0f, 1.0f, one_up, one_dn, 0x1p-126f, 0x1p-125f, 0x1p125f, 0x1p127f, __builtin_inff()};
    float grid[19];
    int ng = 0;
    for (float m : mags) { grid[ng++] = m; grid[ng++] = -m; }
    grid[ng++] = __builtin_nanf("");
    const float tMaxes[] = {FLT_MAX, 1.0f, 0.001f, 0.0f, __builtin_nanf("")};
    uint64_t nGrid = 0;
    int idx[6] = {0, 0, 0, 0, 0, 0};
    for (;;) {
        float v[6];
        for (int k = 0; k < 6; ++k) v[k] = grid[idx[k]];
        for (float tMax : tMaxes) { one(v, tMin, tMax); ++nGrid; }
        int k = 0;
        while (k < 6 && ++idx[k] == ng) idx[k++] = 0;
        if (k == 6) break;
    }
    const uint64_t gridFast = g_fast, gridExact = g_exact;
    for (uint64_t i = 0; i < nRandom; ++i) {
        float v[6], tMax;
        switch (i % 3) {
        case 0:                                                   // raw bit patterns
            for (int k = 0; k < 6; ++k) v[k] = flt((uint32_t)rnd());
            tMax = (rnd() & 7) ? flt((uint32_t)rnd() & 0x7fffffffu) : FLT_MAX;
            break;
        case 1:                                                   // scene-like rays
            for (int k = 0; k < 3; ++k) v[k] = uni(-3.0f, 3.0f);
            for (int k = 3; k < 6; ++k) v[k] = uni(-1.0f, 1.0f);
            tMax = (rnd() & 1) ? uni(0.0f, 8.0f) : FLT_MAX;
            break;
        default:                                                  // the 1/8 grid: edges, corners, ties
            for (int k = 0; k < 3; ++k) v[k] = (float)((int)(rnd() % 49) - 24) * 0.125f;
            for (int k = 3; k < 6; ++k) v[k] = (float)((int)(rnd() % 17) - 8) * 0.125f;
            tMax = (rnd() & 1) ? (float)(rnd() % 65) * 0.125f : FLT_MAX;
            break;
        }
        one(v, tMin, tMax);
    }
    printf("{\"grid_cases\": %llu, \"grid_fast\": %llu, \"grid_exact\": %llu, \"random_cases\": %llu, "
           "\"random_fast\": %llu, \"random_exact\": %llu, \"fast_hits\": %llu, \"mismatches\": %llu}\n",
           (unsigned long long)nGrid, (unsigned long long)gridFast, (unsigned long long)gridExact,
           (unsigned long long)nRandom, (unsigned long long)(g_fast - gridFast), (unsigned long long)(g_exact - gridExact),
           (unsigned long long)g_hits, (unsigned long long)g_bad);
    if (g_bad != 0 || g_fast == 0 || g_exact == 0 || g_hits == 0) return 1;
    return 0;
}
