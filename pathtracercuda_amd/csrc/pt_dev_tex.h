// The texture descriptor and the bilinear fetch of the trace kernel.
// Stands alone on pt_math.h, so that a second translation unit (tools/dev_functions.hip) evaluates the
// very text the kernel compiles.  Included by pt_dev_scene.h inside pt_kernels.hip's anonymous namespace;
// any other includer includes pt_math.h first, says `using namespace pt;` and opens a namespace of its own.
#pragma once
#include "pt_math.h"

struct DevTex {
    const float4* texels;
    uint32_t width, height;
    float fwidth, fheight;      // (float)width, (float)height, converted once on the host: a uniform
                                // conversion in the kernel would be a VALU result held in a VGPR
};

// ---------------------------------------------------------------------------------------------
// texture sampling: CUDA 2-D linear fetch, normalised coordinates, wrap (u) / clamp (v),
// weights quantised to 1/256 (sampler of Pathtracer.cpp:276-283)
// ---------------------------------------------------------------------------------------------
PT_DEV f3 tex2d(const DevTex& t, float u, float v)
{
    const float W = t.fwidth, H = t.fheight;
    const float uw = u - floorf(u);
    const float x = uw * W - 0.5f;
    const float y = v * H - 0.5f;
    const float fx = floorf(x), fy = floorf(y);
    float a = x - fx, b = y - fy;
    a = floorf(a * 256.0f + 0.5f) * (1.0f / 256.0f);
    b = floorf(b * 256.0f + 0.5f) * (1.0f / 256.0f);
    const int32_t w = (int32_t)t.width, h = (int32_t)t.height;
    int32_t i0 = (fx > -1.0e9f && fx < 1.0e9f) ? (int32_t)fx : 0;
    int32_t j0 = (fy > -1.0e9f && fy < 1.0e9f) ? (int32_t)fy : (fy > 0.0f ? h : -1);
    int32_t i1 = i0 + 1, j1 = j0 + 1;
    // wrap: u - floor(u) lies in [0, 1] (or is NaN, giving i0 = 0), so fx lies in [-1, w - 1] and
    // i0 in [-1, w - 1], i1 in [0, w]: one conditional add/subtract equals ((i % w) + w) % w here
    i0 = i0 < 0 ? i0 + w : i0;
    i1 = i1 >= w ? i1 - w : i1;
    j0 = j0 < 0 ? 0 : (j0 > h - 1 ? h - 1 : j0);
    j1 = j1 < 0 ? 0 : (j1 > h - 1 ? h - 1 : j1);
    const float4 T00 = t.texels[(size_t)j0 * t.width + (size_t)i0];
    const float4 T10 = t.texels[(size_t)j0 * t.width + (size_t)i1];
    const float4 T01 = t.texels[(size_t)j1 * t.width + (size_t)i0];
    const float4 T11 = t.texels[(size_t)j1 * t.width + (size_t)i1];
    const float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
    return mk(w00 * T00.x + w10 * T10.x + w01 * T01.x + w11 * T11.x,
              w00 * T00.y + w10 * T10.y + w01 * T01.y + w11 * T11.y,
              w00 * T00.z + w10 * T10.z + w01 * T01.z + w11 * T11.z);
}
