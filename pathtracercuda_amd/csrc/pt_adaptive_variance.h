// Entry points of the variance of an adaptive render's image and the filter guided by it
// (pt_denoise_adaptive, pt_read_adaptive_variance, pt_read_adaptive_variance_timing,
// pt_adaptive_variance_image); the kernels are in pt_dev_adaptive_variance.h, the filter is pt_svgf.h's
// vdenoise_run unchanged.  Part of the trace kernel's single translation unit: included by pt_kernels.hip
// after pt_svgf.h; not a standalone header.
#pragma once

// The field a parameter set is refused for, or null.  Written so that a NaN fails every range.
static const char* avariance_refusal(const pt_adaptive_variance_params* p)
{
    if (!p) return "adaptive variance params is null";
    if (!(p->min_batches >= 2u && p->min_batches <= 255u)) return "min_batches must be 2..255";
    if (!(p->sigma_plane >= 1e-6f) || !(p->sigma_plane - p->sigma_plane == 0.0f)) return "sigma_plane must be >= 1e-6 and finite";
    if (!(p->normal_cos_min >= -1.0f && p->normal_cos_min <= 1.0f)) return "normal_cos_min must be -1..1";
    if (p->flags & ~(PT_DENOISE_DEMODULATE | PT_DENOISE_SAME_PRIMITIVE)) return "flags has unknown bits";
    return nullptr;
}

// The form the automatic choice (staging = 0) takes: the staged one, by the same-session A/B at 1920 x 1080
// (profiles/adaptive_variance_probe.json).  Where every pixel with a variance walks the window
// (min_batches 255) it takes 0.31 to 0.33 of the unstaged form's time; where no pixel does (the default min_batches on
// those renders) it votes, stages nothing and loses 0.2 to 0.5 us of 7 us.
static bool avariance_stage_auto() { return true; }

// The estimate on device buffers of width x height: planes = 3 planes (pt_render_features' layout), mom =
// [3][pixels] m1, m2, n (adMom's layout), t0 and t1 = scratch of one float4 plane each, var = the result.
// ev (optional): 2 events recorded around adaptive_variance_kernel.
static hipError_t avariance_run(hipStream_t stream, const pt_adaptive_variance_params& p, uint32_t staging, uint32_t width,
                                uint32_t height, const float4* color, const float4* planes, const uint32_t* mom, float4* t0,
                                float4* t1, float* var, hipEvent_t* ev)
{
    const size_t npix = (size_t)width * height;
    AVarianceArgs A = {};
    A.color = color;
    A.plane0 = planes;
    A.plane1 = planes + npix;
    A.plane2 = planes + 2 * npix;
    A.mom = mom;
    A.t0 = t0;
    A.t1 = t1;
    A.var = var;
    A.width = width;
    A.height = height;
    A.minBatches = p.min_batches;
    A.sigmaPlane = p.sigma_plane;
    A.normalCosMin = p.normal_cos_min;
    A.flags = p.flags;
    hipError_t e;
    avar_prepare_kernel<<<(unsigned)((npix + 255) / 256), 256, 0, stream>>>(A);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const dim3 grid((width + kDnTileW - 1) / kDnTileW, (height + kDnTileH - 1) / kDnTileH);
    if (ev && (e = hipEventRecord(ev[0], stream)) != hipSuccess) return e;
    if (staging == 1u || (staging == 0u && avariance_stage_auto()))
        adaptive_variance_kernel<true><<<grid, 256, (2 * kAvRN + 1) * sizeof(float4), stream>>>(A);
    else
        adaptive_variance_kernel<false><<<grid, 256, 0, stream>>>(A);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[1], stream)) != hipSuccess) return e;
    return hipSuccess;
}

// The context's two tap planes and its variance of the counts, in one allocation
static float* avariance_variance(pt_context* ctx) { return reinterpret_cast<float*>(ctx->avBuf + 2 * (size_t)ctx->rows * ctx->width); }

extern "C" {

PT_API int pt_denoise_adaptive(pt_context* ctx, const pt_adaptive_variance_params* variance, const pt_vdenoise_params* params)
{
    if (!ctx) return PT_ERR_ARG;
    const std::string who("pt_denoise_adaptive: ");
    if (const char* why = avariance_refusal(variance)) return fail(ctx, PT_ERR_ARG, (who + why).c_str());
    if (const char* why = vdenoise_refusal(params)) return fail(ctx, PT_ERR_ARG, (who + why).c_str());
    if ((params->flags ^ variance->flags) & PT_DENOISE_DEMODULATE)
        return fail(ctx, PT_ERR_ARG, (who + "flags: the DEMODULATE bit differs from the one the variance is made with").c_str());
    if (ctx->rows != ctx->height)
        return fail(ctx, PT_ERR_ARG, "pt_denoise_adaptive: the context holds a band partition, not the whole frame "
                                     "(gather the frame and use pt_adaptive_variance_image and pt_denoise_variance_image)");
    if (!counts_describe_buffer(ctx->st))
        return fail(ctx, PT_ERR_STATE, "pt_denoise_adaptive: no adaptive render describes the buffer (its moments are the variance's source)");
    if (!planes_current(ctx->st))
        return fail(ctx, PT_ERR_STATE, "pt_denoise_adaptive: no feature planes (no pt_render_features since the scene or a texture was set)");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    denoise_begins(ctx->st);
    adaptive_variance_begins(ctx->st);
    if (!ctx->dnBuf) {
        PT_HIP_CHECK(ctx, hipMalloc(&ctx->dnBuf, 6 * npix * sizeof(float4)));   // colour, g0, g1, ping, pong, out
        for (auto& e : ctx->dnEv) PT_HIP_CHECK(ctx, hipEventCreate(&e));
    }
    if (!ctx->avBuf) {
        PT_HIP_CHECK(ctx, hipMalloc(&ctx->avBuf, (2 * npix + (npix + 3) / 4 + 1) * sizeof(float4)));
        for (auto& e : ctx->avEv) PT_HIP_CHECK(ctx, hipEventCreate(&e));
    }
    dn_color_kernel<<<(unsigned)((npix + 255) / 256), 256, 0, ctx->stream>>>(ctx->dnBuf, ctx->accum, ctx->adMom + 2 * npix, npix, 1.0f);
    PT_HIP_CHECK(ctx, hipGetLastError());
    PT_HIP_CHECK(ctx, avariance_run(ctx->stream, *variance, params->staging, ctx->width, ctx->height, ctx->dnBuf, ctx->feat,
                                    ctx->adMom, ctx->avBuf, ctx->avBuf + npix, avariance_variance(ctx), ctx->avEv));
    PT_HIP_CHECK(ctx, vdenoise_run(ctx->stream, *params, ctx->width, ctx->height, ctx->dnBuf, ctx->feat, avariance_variance(ctx),
                                   ctx->dnBuf + npix, ctx->dnBuf + 2 * npix, ctx->dnBuf + 3 * npix, ctx->dnBuf + 4 * npix,
                                   ctx->dnBuf + 5 * npix, ctx->dnEv));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    PT_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->avMs, ctx->avEv[0], ctx->avEv[1]));
    for (float& m : ctx->dnMs) m = 0.0f;
    PT_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->dnMs[0], ctx->dnEv[0], ctx->dnEv[1]));
    for (uint32_t i = 0; i < params->iterations; ++i)
        PT_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->dnMs[1 + i], ctx->dnEv[1 + i], ctx->dnEv[2 + i]));
    PT_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->dnMs[9], ctx->dnEv[1 + params->iterations], ctx->dnEv[11]));
    denoise_done(ctx->st);
    adaptive_variance_done(ctx->st);
    return PT_OK;
}

PT_API int pt_read_adaptive_variance(pt_context* ctx, float* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!variance_of_counts(ctx->st))
        return fail(ctx, PT_ERR_STATE, "pt_read_adaptive_variance: no variance of the counts is held (no pt_denoise_adaptive since "
                                       "the accumulation was written or pt_render_features ran)");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    PT_HIP_CHECK(ctx, hipMemcpy(dst, avariance_variance(ctx), npix * sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
}

PT_API int pt_read_adaptive_variance_timing(pt_context* ctx, float* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!variance_of_counts(ctx->st))
        return fail(ctx, PT_ERR_STATE, "pt_read_adaptive_variance_timing: no variance of the counts is held (no pt_denoise_adaptive "
                                       "since the accumulation was written or pt_render_features ran)");
    *dst = ctx->avMs;
    return PT_OK;
}

PT_API int pt_adaptive_variance_image(int device, uint32_t width, uint32_t height, const float* color, const float* plane0,
                                      const float* plane1, const float* plane2, const float* moments,
                                      const pt_adaptive_variance_params* params, uint32_t staging, float* out_variance)
{
    auto refuse = [](int code, const std::string& msg) {
        g_freeError = "pt_adaptive_variance_image: " + msg;
        return code;
    };
    if (const char* why = avariance_refusal(params)) return refuse(PT_ERR_ARG, why);
    if (staging > 2u) return refuse(PT_ERR_ARG, "staging must be 0, 1 or 2");
    if (!color || !plane0 || !plane1 || !plane2 || !moments || !out_variance) return refuse(PT_ERR_ARG, "an array is null");
    if (width == 0 || height == 0 || (uint64_t)width * height >= (1ull << 30) || height > 8u * 0xffffu)
        return refuse(PT_ERR_ARG, "width x height must be 1 .. 2^30 - 1 pixels, height at most 524280");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return refuse(PT_ERR_NO_DEVICE, "no GPU visible");
    if (device < 0 || device >= n) return refuse(PT_ERR_ARG, "device out of range");
    const size_t npix = (size_t)width * height, bytes = npix * sizeof(float4);
    std::vector<uint32_t> soa(3 * npix);    // pt_read_moments' pixel-major triples into the kernel's planes
    for (size_t i = 0; i < npix; ++i)
        for (int k = 0; k < 3; ++k) memcpy(&soa[k * npix + i], &moments[3 * i + k], sizeof(uint32_t));
    float4* buf = nullptr;                  // colour, 3 planes, t0, t1, then the variance and the moments
    const float* in[4] = {color, plane0, plane1, plane2};
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc(&buf, 6 * bytes + 4 * npix * sizeof(uint32_t));
    for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipMemcpy(buf + k * npix, in[k], bytes, hipMemcpyHostToDevice);
    float* var = reinterpret_cast<float*>(buf + 6 * npix);
    uint32_t* mom = reinterpret_cast<uint32_t*>(var + npix);
    if (e == hipSuccess) e = hipMemcpy(mom, soa.data(), 3 * npix * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = avariance_run(nullptr, *params, staging, width, height, buf, buf + npix, mom, buf + 4 * npix, buf + 5 * npix, var,
                          nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out_variance, var, npix * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    if (e != hipSuccess) return refuse(PT_ERR_HIP, std::string("HIP error: ") + hipGetErrorString(e));
    return PT_OK;
}

} // extern "C"
