// Entry points of despike, the same-surface firefly clamp (pt_despike, pt_read_despiked, pt_tonemap_despiked,
// pt_holds_despiked, pt_read_despike_count, pt_read_despike_timing, pt_denoise_despiked, pt_despike_image); the kernels are in
// pt_dev_despike.h, the filter behind pt_denoise_despiked is pt_denoise.h's denoise_context unchanged.  Part of the
// trace kernel's single translation unit: included by pt_kernels.hip after pt_adaptive_variance.h; not a
// standalone header.
#pragma once

// The field a parameter set is refused for, or null.  Written so that a NaN fails every range.
static const char* despike_refusal(const pt_despike_params* p)
{
    if (!p) return "params is null";
    if (!(p->radius >= 1u && p->radius <= 3u)) return "radius must be 1..3";
    if (!(p->rank >= 1u && p->rank <= 4u)) return "rank must be 1..4";
    if (!(p->factor >= 1.0f) || !(p->factor - p->factor == 0.0f)) return "factor must be >= 1 and finite";
    if (!(p->floor >= 0.0f) || !(p->floor - p->floor == 0.0f)) return "floor must be >= 0 and finite";
    const uint32_t side = 2u * p->radius + 1u;
    if (!(p->min_neighbors >= p->rank && p->min_neighbors <= side * side - 1u))
        return "min_neighbors must be rank..(2 radius + 1)^2 - 1";
    if (!(p->sigma_plane >= 1e-6f) || !(p->sigma_plane - p->sigma_plane == 0.0f)) return "sigma_plane must be >= 1e-6 and finite";
    if (!(p->normal_cos_min >= -1.0f && p->normal_cos_min <= 1.0f)) return "normal_cos_min must be -1..1";
    if (p->flags & ~(PT_DENOISE_DEMODULATE | PT_DENOISE_SAME_PRIMITIVE)) return "flags has unknown bits";
    if (p->staging > 2u) return "staging must be 0, 1 or 2";
    return nullptr;
}

// The form the automatic choice (staging = 0) takes per radius: whichever measured faster in the same-session A/B at
// 1920 x 1080 (profiles/despike_probe.json).  The staged form won at every radius on both scenes: by 4
// to 6 % at radius 1, 17 to 29 % at radius 2 and 50 to 54 % at radius 3.
static bool despike_stage_auto(uint32_t radius)
{
    switch (radius) {
    case 1: return true;
    case 2: return true;
    default: return true;
    }
}

// Rule 6 on device buffers of width x height: planes = 3 planes (pt_render_features' layout), t0 and t1 = scratch
// of one float4 plane each, out = the result, count = one word.  ev (optional): 3 events, before the flat pass,
// between the two kernels and after despike_kernel.
static hipError_t despike_run(hipStream_t stream, const pt_despike_params& p, uint32_t width, uint32_t height,
                              const float4* color, const float4* planes, float4* t0, float4* t1, float4* out,
                              uint32_t* count, hipEvent_t* ev)
{
    const size_t npix = (size_t)width * height;
    DespikeArgs A = {};
    A.color = color;
    A.plane0 = planes;
    A.plane1 = planes + npix;
    A.plane2 = planes + 2 * npix;
    A.t0 = t0;
    A.t1 = t1;
    A.out = out;
    A.count = count;
    A.width = width;
    A.height = height;
    A.radius = p.radius;
    A.rank = p.rank;
    A.factor = p.factor;
    A.floor = p.floor;
    A.minNeighbors = p.min_neighbors;
    A.sigmaPlane = p.sigma_plane;
    A.normalCosMin = p.normal_cos_min;
    A.flags = p.flags;
    hipError_t e;
    if ((e = hipMemsetAsync(count, 0, sizeof(uint32_t), stream)) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[0], stream)) != hipSuccess) return e;
    despike_prepare_kernel<<<(unsigned)((npix + 255) / 256), 256, 0, stream>>>(A);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[1], stream)) != hipSuccess) return e;
    const dim3 grid((width + kDnTileW - 1) / kDnTileW, (height + kDnTileH - 1) / kDnTileH);
    if (p.staging == 1u || (p.staging == 0u && despike_stage_auto(p.radius)))
        despike_kernel<true><<<grid, 256, (2 * kDsMaxRN + 1) * sizeof(float4), stream>>>(A);
    else
        despike_kernel<false><<<grid, 256, 0, stream>>>(A);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[2], stream)) != hipSuccess) return e;
    return hipSuccess;
}

// The context's despike buffers in one allocation: the colour, the two tap planes, the despiked image, the count
static float4* despike_image(pt_context* ctx) { return ctx->dsBuf + 3 * (size_t)ctx->rows * ctx->width; }
static uint32_t* despike_count(pt_context* ctx) { return reinterpret_cast<uint32_t*>(ctx->dsBuf + 4 * (size_t)ctx->rows * ctx->width); }

static const char* const kNoDespiked = "no despiked image is held (no pt_despike since the accumulation was written, "
                                       "pt_render_features ran or the scene, a texture or the sky changed)";

extern "C" {

PT_API int pt_despike(pt_context* ctx, uint32_t frames, const pt_despike_params* params)
{
    if (!ctx) return PT_ERR_ARG;
    if (const char* why = despike_refusal(params)) return fail(ctx, PT_ERR_ARG, (std::string("pt_despike: ") + why).c_str());
    if (ctx->rows != ctx->height)
        return fail(ctx, PT_ERR_ARG, "pt_despike: the context holds a band partition, not the whole frame "
                                     "(gather the frame and use pt_despike_image)");
    if (!planes_current(ctx->st))
        return fail(ctx, PT_ERR_STATE, "pt_despike: no feature planes (no pt_render_features since the scene or a texture was set)");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    despike_begins(ctx->st);
    if (!ctx->dsBuf) PT_HIP_CHECK(ctx, hipMalloc(&ctx->dsBuf, (4 * npix + 1) * sizeof(float4)));
    for (auto& e : ctx->dsEv)                 // each on its own: a creation that failed is tried again by the next call
        if (!e) PT_HIP_CHECK(ctx, hipEventCreate(&e));
    const float inv = 1.0f / fmaxf((float)frames, 1.0f);
    dn_color_kernel<<<(unsigned)((npix + 255) / 256), 256, 0, ctx->stream>>>(
        ctx->dsBuf, ctx->accum, counts_describe_buffer(ctx->st) ? ctx->adMom + 2 * npix : nullptr, npix, inv);
    PT_HIP_CHECK(ctx, hipGetLastError());
    PT_HIP_CHECK(ctx, despike_run(ctx->stream, *params, ctx->width, ctx->height, ctx->dsBuf, ctx->feat, ctx->dsBuf + npix,
                                  ctx->dsBuf + 2 * npix, despike_image(ctx), despike_count(ctx), ctx->dsEv));
    PT_HIP_CHECK(ctx, hipMemcpyAsync(&ctx->dsCount, despike_count(ctx), sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    PT_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->dsMs[0], ctx->dsEv[0], ctx->dsEv[1]));
    PT_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->dsMs[1], ctx->dsEv[1], ctx->dsEv[2]));
    despike_done(ctx->st);
    return PT_OK;
}

PT_API int pt_holds_despiked(const pt_context* ctx) { return ctx && holds_despiked(ctx->st) ? 1 : 0; }

PT_API int pt_read_despiked(pt_context* ctx, float* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!holds_despiked(ctx->st)) return fail(ctx, PT_ERR_STATE, (std::string("pt_read_despiked: ") + kNoDespiked).c_str());
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    PT_HIP_CHECK(ctx, hipMemcpy(dst, despike_image(ctx), npix * sizeof(float4), hipMemcpyDeviceToHost));
    return PT_OK;
}

PT_API int pt_tonemap_despiked(pt_context* ctx, uint8_t* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!holds_despiked(ctx->st)) return fail(ctx, PT_ERR_STATE, (std::string("pt_tonemap_despiked: ") + kNoDespiked).c_str());
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    if (!ctx->ldr) PT_HIP_CHECK(ctx, hipMalloc(&ctx->ldr, npix * sizeof(uchar4)));
    tonemap_denoised_kernel<<<(unsigned)((npix + 255) / 256), 256, 0, ctx->stream>>>(ctx->ldr, despike_image(ctx), npix);
    PT_HIP_CHECK(ctx, hipGetLastError());
    PT_HIP_CHECK(ctx, hipMemcpyAsync(dst, ctx->ldr, npix * sizeof(uchar4), hipMemcpyDeviceToHost, ctx->stream));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return PT_OK;
}

PT_API int pt_read_despike_count(pt_context* ctx, uint32_t* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!holds_despiked(ctx->st)) return fail(ctx, PT_ERR_STATE, (std::string("pt_read_despike_count: ") + kNoDespiked).c_str());
    *dst = ctx->dsCount;
    return PT_OK;
}

PT_API int pt_read_despike_timing(pt_context* ctx, float* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!holds_despiked(ctx->st)) return fail(ctx, PT_ERR_STATE, (std::string("pt_read_despike_timing: ") + kNoDespiked).c_str());
    dst[0] = ctx->dsMs[0];
    dst[1] = ctx->dsMs[1];
    return PT_OK;
}

PT_API int pt_denoise_despiked(pt_context* ctx, const pt_denoise_params* params)
{
    if (!ctx) return PT_ERR_ARG;
    if (const char* why = denoise_refusal(params))
        return fail(ctx, PT_ERR_ARG, (std::string("pt_denoise_despiked: ") + why).c_str());
    if (!holds_despiked(ctx->st)) return fail(ctx, PT_ERR_STATE, (std::string("pt_denoise_despiked: ") + kNoDespiked).c_str());
    // (the whole frame and current planes: pt_despike refuses anything else, and a features call ends the image)
    return denoise_context(ctx, *params, despike_image(ctx), 0);
}

PT_API int pt_despike_image(int device, uint32_t width, uint32_t height, const float* color, const float* plane0,
                            const float* plane1, const float* plane2, const pt_despike_params* params, float* out,
                            uint32_t* out_count)
{
    auto refuse = [](int code, const std::string& msg) {
        g_freeError = "pt_despike_image: " + msg;
        return code;
    };
    if (const char* why = despike_refusal(params)) return refuse(PT_ERR_ARG, why);
    if (!color || !plane0 || !plane1 || !plane2 || !out) return refuse(PT_ERR_ARG, "an array is null");
    if (width == 0 || height == 0 || (uint64_t)width * height >= (1ull << 30) || height > 8u * 0xffffu)
        return refuse(PT_ERR_ARG, "width x height must be 1 .. 2^30 - 1 pixels, height at most 524280");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return refuse(PT_ERR_NO_DEVICE, "no GPU visible");
    if (device < 0 || device >= n) return refuse(PT_ERR_ARG, "device out of range");
    const size_t npix = (size_t)width * height, bytes = npix * sizeof(float4);
    float4* buf = nullptr;                  // colour, 3 planes, t0, t1, out, then the count
    const float* in[4] = {color, plane0, plane1, plane2};
    uint32_t spikes = 0;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc(&buf, 7 * bytes + sizeof(float4));
    for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipMemcpy(buf + k * npix, in[k], bytes, hipMemcpyHostToDevice);
    uint32_t* count = reinterpret_cast<uint32_t*>(buf + 7 * npix);
    if (e == hipSuccess)
        e = despike_run(nullptr, *params, width, height, buf, buf + npix, buf + 4 * npix, buf + 5 * npix, buf + 6 * npix, count,
                        nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, buf + 6 * npix, bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&spikes, count, sizeof(uint32_t), hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    if (e != hipSuccess) return refuse(PT_ERR_HIP, std::string("HIP error: ") + hipGetErrorString(e));
    if (out_count) *out_count = spikes;
    return PT_OK;
}

} // extern "C"
