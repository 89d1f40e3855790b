// Tonemapping of one accumulation value.
// Stands alone on pt_math.h, so that a second translation unit (tools/dev_functions.hip) evaluates the
// very text the kernel compiles.  Included by pt_kernels.hip inside its anonymous namespace; any other
// includer includes pt_math.h first, says `using namespace pt;` and opens a namespace of its own.
#pragma once
#include "pt_math.h"

// tonemap (tonemap.cu:4-27) of one accumulation value over `frames` render() calls
PT_DEV uchar4 tonemap_pixel(const float4 a, uint32_t frames)
{
    f3 c = divs(mk(a.x, a.y, a.z), (float)frames);
    c = mul(mk(1.0f / (c.x + 1.0f), 1.0f / (c.y + 1.0f), 1.0f / (c.z + 1.0f)), c);
    const float g = 1.0f / 2.2f;
    const float ch[3] = {pow_(c.x, g), pow_(c.y, g), pow_(c.z, g)};
    unsigned char q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float f = ch[k] * 255.0f;
        const int32_t v = (f != f) ? 0 : f2i_x86(f);
        q[k] = (unsigned char)(v & 0xff);
    }
    return make_uchar4(q[0], q[1], q[2], 255);
}
