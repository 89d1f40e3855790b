// Entry points of the guided upsampling (pt_upsample, pt_holds_upsampled, pt_read_upsampled, pt_tonemap_upsampled,
// pt_read_upsample_counts, pt_read_upsample_timing, pt_upsample_image); the kernels are in pt_dev_upsample.h.  Part of
// the trace kernel's single translation unit: included by pt_kernels.hip after pt_despike.h; not a standalone header.
#pragma once

// The field a parameter set is refused for, or null (pt_denoise's ranges).  Written so that a NaN fails every range.
static const char* upsample_refusal(const pt_upsample_params* p)
{
    if (!p) return "params is null";
    if (!(p->sigma_plane >= 1e-6f) || !(p->sigma_plane - p->sigma_plane == 0.0f)) return "sigma_plane must be >= 1e-6 and finite";
    if (p->normal_power_log2 > 7u) return "normal_power_log2 must be 0..7";
    if (p->flags & ~(PT_DENOISE_DEMODULATE | PT_DENOISE_SAME_PRIMITIVE)) return "flags has unknown bits";
    if (p->staging > 2u) return "staging must be 0, 1 or 2";
    return nullptr;
}

// The form the automatic choice (staging = 0) takes: whichever measured faster in the same-session A/B at
// 1920 x 1080 (profiles/upsample_probe.json).  The staged form won in all four cases: 39.0 against
// 44.2 us and 36.9 against 42.6 us on cornell_box from 960 x 540 and 640 x 360, 39.1 against 41.5 us and 42.2 against
// 44.0 us on generated_scene.
static bool upsample_stage_auto() { return true; }

// Rule 8 on device buffers: color and loPlanes (3 planes, pt_render_features' layout) of w x h, hiPlanes of W x H,
// t = scratch of three planes of w x h, out of W x H, counts = two words.  ev (optional): 3 events, before the flat
// pass, between the two kernels and after upsample_kernel.
static hipError_t upsample_run(hipStream_t stream, const pt_upsample_params& p, uint32_t w, uint32_t h, const float4* color,
                               const float4* loPlanes, uint32_t W, uint32_t H, const float4* hiPlanes, float4* t,
                               float4* out, uint32_t* counts, hipEvent_t* ev)
{
    const size_t nlo = (size_t)w * h, nhi = (size_t)W * H;
    UpsampleArgs A = {};
    A.color = color;
    A.lo0 = loPlanes;
    A.lo1 = loPlanes + nlo;
    A.lo2 = loPlanes + 2 * nlo;
    A.t0 = t;
    A.t1 = t + nlo;
    A.t2 = t + 2 * nlo;
    A.hi0 = hiPlanes;
    A.hi1 = hiPlanes + nhi;
    A.hi2 = hiPlanes + 2 * nhi;
    A.out = out;
    A.counts = counts;
    A.w = w;
    A.h = h;
    A.W = W;
    A.H = H;
    A.sigmaPlane = p.sigma_plane;
    A.normalPower = p.normal_power_log2;
    A.flags = p.flags;
    hipError_t e;
    if ((e = hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t), stream)) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[0], stream)) != hipSuccess) return e;
    upsample_prepare_kernel<<<(unsigned)((nlo + 255) / 256), 256, 0, stream>>>(A);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[1], stream)) != hipSuccess) return e;
    const dim3 grid((W + kDnTileW - 1) / kDnTileW, (H + kDnTileH - 1) / kDnTileH);
    if (p.staging == 1u || (p.staging == 0u && upsample_stage_auto()))
        upsample_kernel<true><<<grid, 256, (kUsCountF4 + 3 * kUsMaxRN) * sizeof(float4), stream>>>(A);
    else
        upsample_kernel<false><<<grid, 256, kUsCountF4 * sizeof(float4), stream>>>(A);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[2], stream)) != hipSuccess) return e;
    return hipSuccess;
}

// The sizes both forms accept (pt_denoise_image's limits, for either image)
static bool upsample_size_ok(uint32_t width, uint32_t height)
{
    return width != 0 && height != 0 && (uint64_t)width * height < (1ull << 30) && height <= 8u * 0xffffu;
}

// hi's upsample buffers in one allocation: [3][usLoCap] the packed low texels, [usLoCap] the low colour
// (PT_UPSAMPLE_ACCUM), [pixels] the upsampled image, the counts
static float4* upsample_image(pt_context* ctx) { return ctx->usBuf + 4 * ctx->usLoCap; }
static uint32_t* upsample_counts(pt_context* ctx) { return reinterpret_cast<uint32_t*>(upsample_image(ctx) + (size_t)ctx->rows * ctx->width); }

static const char* const kNoUpsampled = "no upsampled image is held (no pt_upsample on this context yet)";

extern "C" {

PT_API int pt_upsample(pt_context* hi, pt_context* lo, uint32_t source, uint32_t frames, const pt_upsample_params* params)
{
    if (!hi) return PT_ERR_ARG;
    if (!lo) return fail(hi, PT_ERR_ARG, "pt_upsample: lo is null");
    if (const char* why = upsample_refusal(params)) return fail(hi, PT_ERR_ARG, (std::string("pt_upsample: ") + why).c_str());
    if (source > PT_UPSAMPLE_DESPIKED)
        return fail(hi, PT_ERR_ARG, "pt_upsample: source must be PT_UPSAMPLE_ACCUM, _DENOISED, _TEMPORAL or _DESPIKED");
    if (hi->device != lo->device) return fail(hi, PT_ERR_ARG, "pt_upsample: the two contexts are on different devices");
    if (hi->rows != hi->height)
        return fail(hi, PT_ERR_ARG, "pt_upsample: hi holds a band partition, not the whole frame (use pt_upsample_image)");
    if (lo->rows != lo->height)
        return fail(hi, PT_ERR_ARG, "pt_upsample: lo holds a band partition, not the whole frame (use pt_upsample_image)");
    if (lo->width > hi->width || lo->height > hi->height)
        return fail(hi, PT_ERR_ARG, "pt_upsample: lo is larger than hi (lo's width and height must not exceed hi's)");
    if (!upsample_size_ok(lo->width, lo->height) || !upsample_size_ok(hi->width, hi->height))
        return fail(hi, PT_ERR_ARG, "pt_upsample: width x height must be 1 .. 2^30 - 1 pixels, height at most 524280");
    if (!planes_current(hi->st))
        return fail(hi, PT_ERR_STATE, "pt_upsample: hi has no feature planes (no pt_render_features since the scene or a texture was set)");
    if (!planes_current(lo->st))
        return fail(hi, PT_ERR_STATE, "pt_upsample: lo has no feature planes (no pt_render_features since the scene or a texture was set)");
    if (source == PT_UPSAMPLE_DENOISED && !holds_denoised(lo->st))
        return fail(hi, PT_ERR_STATE, "pt_upsample: lo holds no denoised image (PT_UPSAMPLE_DENOISED)");
    if (source == PT_UPSAMPLE_TEMPORAL && !temporal_of_planes(lo->st))
        return fail(hi, PT_ERR_STATE, "pt_upsample: lo holds no temporal image of the planes it holds (PT_UPSAMPLE_TEMPORAL)");
    if (source == PT_UPSAMPLE_DESPIKED && !holds_despiked(lo->st))
        return fail(hi, PT_ERR_STATE, "pt_upsample: lo holds no despiked image (PT_UPSAMPLE_DESPIKED)");
    PT_HIP_CHECK(hi, hipSetDevice(hi->device));
    const size_t nlo = (size_t)lo->rows * lo->width, nhi = (size_t)hi->rows * hi->width;
    upsample_begins(hi->st);
    if (hi->usBuf && hi->usLoCap < nlo) {                 // a larger `lo` than the buffers were made for
        PT_HIP_CHECK(hi, hipStreamSynchronize(hi->stream));
        PT_HIP_CHECK(hi, hipFree(hi->usBuf));
        hi->usBuf = nullptr;
    }
    if (!hi->usBuf) {
        PT_HIP_CHECK(hi, hipMalloc(&hi->usBuf, (4 * nlo + nhi + 1) * sizeof(float4)));
        hi->usLoCap = nlo;
    }
    for (auto& e : hi->usEv)
        if (!e) PT_HIP_CHECK(hi, hipEventCreate(&e));
    PT_HIP_CHECK(hi, hipStreamSynchronize(lo->stream));   // lo's image and planes are complete; the rest runs on hi's stream
    const float4* color;
    if (source == PT_UPSAMPLE_ACCUM) {
        float4* c = hi->usBuf + 3 * hi->usLoCap;
        const float inv = 1.0f / fmaxf((float)frames, 1.0f);
        dn_color_kernel<<<(unsigned)((nlo + 255) / 256), 256, 0, hi->stream>>>(
            c, lo->accum, counts_describe_buffer(lo->st) ? lo->adMom + 2 * nlo : nullptr, nlo, inv);
        PT_HIP_CHECK(hi, hipGetLastError());
        color = c;
    } else if (source == PT_UPSAMPLE_DENOISED) {
        color = lo->dnBuf + 5 * nlo;
    } else if (source == PT_UPSAMPLE_TEMPORAL) {
        color = lo->tpBuf + nlo;
    } else {
        color = despike_image(lo);
    }
    PT_HIP_CHECK(hi, upsample_run(hi->stream, *params, lo->width, lo->height, color, lo->feat, hi->width, hi->height, hi->feat,
                                  hi->usBuf, upsample_image(hi), upsample_counts(hi), hi->usEv));
    PT_HIP_CHECK(hi, hipMemcpyAsync(hi->usCounts, upsample_counts(hi), 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, hi->stream));
    PT_HIP_CHECK(hi, hipStreamSynchronize(hi->stream));
    PT_HIP_CHECK(hi, hipEventElapsedTime(&hi->usMs[0], hi->usEv[0], hi->usEv[1]));
    PT_HIP_CHECK(hi, hipEventElapsedTime(&hi->usMs[1], hi->usEv[1], hi->usEv[2]));
    upsample_done(hi->st);
    return PT_OK;
}

PT_API int pt_holds_upsampled(const pt_context* ctx) { return ctx && holds_upsampled(ctx->st) ? 1 : 0; }

PT_API int pt_read_upsampled(pt_context* ctx, float* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!holds_upsampled(ctx->st)) return fail(ctx, PT_ERR_STATE, (std::string("pt_read_upsampled: ") + kNoUpsampled).c_str());
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    PT_HIP_CHECK(ctx, hipMemcpy(dst, upsample_image(ctx), npix * sizeof(float4), hipMemcpyDeviceToHost));
    return PT_OK;
}

PT_API int pt_tonemap_upsampled(pt_context* ctx, uint8_t* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!holds_upsampled(ctx->st)) return fail(ctx, PT_ERR_STATE, (std::string("pt_tonemap_upsampled: ") + kNoUpsampled).c_str());
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    if (!ctx->ldr) PT_HIP_CHECK(ctx, hipMalloc(&ctx->ldr, npix * sizeof(uchar4)));
    tonemap_denoised_kernel<<<(unsigned)((npix + 255) / 256), 256, 0, ctx->stream>>>(ctx->ldr, upsample_image(ctx), npix);
    PT_HIP_CHECK(ctx, hipGetLastError());
    PT_HIP_CHECK(ctx, hipMemcpyAsync(dst, ctx->ldr, npix * sizeof(uchar4), hipMemcpyDeviceToHost, ctx->stream));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return PT_OK;
}

PT_API int pt_read_upsample_counts(pt_context* ctx, uint32_t* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!holds_upsampled(ctx->st)) return fail(ctx, PT_ERR_STATE, (std::string("pt_read_upsample_counts: ") + kNoUpsampled).c_str());
    dst[0] = ctx->usCounts[0];
    dst[1] = ctx->usCounts[1];
    return PT_OK;
}

PT_API int pt_read_upsample_timing(pt_context* ctx, float* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!holds_upsampled(ctx->st)) return fail(ctx, PT_ERR_STATE, (std::string("pt_read_upsample_timing: ") + kNoUpsampled).c_str());
    dst[0] = ctx->usMs[0];
    dst[1] = ctx->usMs[1];
    return PT_OK;
}

PT_API int pt_upsample_image(int device, uint32_t lo_w, uint32_t lo_h, const float* color, const float* lo_plane0,
                             const float* lo_plane1, const float* lo_plane2, uint32_t hi_w, uint32_t hi_h,
                             const float* hi_plane0, const float* hi_plane1, const float* hi_plane2,
                             const pt_upsample_params* params, float* out, uint32_t* out_counts)
{
    auto refuse = [](int code, const std::string& msg) {
        g_freeError = "pt_upsample_image: " + msg;
        return code;
    };
    if (const char* why = upsample_refusal(params)) return refuse(PT_ERR_ARG, why);
    if (!color || !lo_plane0 || !lo_plane1 || !lo_plane2 || !hi_plane0 || !hi_plane1 || !hi_plane2 || !out)
        return refuse(PT_ERR_ARG, "an array is null");
    if (!upsample_size_ok(lo_w, lo_h) || !upsample_size_ok(hi_w, hi_h))
        return refuse(PT_ERR_ARG, "width x height must be 1 .. 2^30 - 1 pixels, height at most 524280");
    if (lo_w > hi_w || lo_h > hi_h) return refuse(PT_ERR_ARG, "lo is larger than hi (lo_w <= hi_w and lo_h <= hi_h)");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return refuse(PT_ERR_NO_DEVICE, "no GPU visible");
    if (device < 0 || device >= n) return refuse(PT_ERR_ARG, "device out of range");
    const size_t nlo = (size_t)lo_w * lo_h, nhi = (size_t)hi_w * hi_h;
    float4* buf = nullptr;                  // low: colour, 3 planes, 3 packed; high: 3 planes, out; then the counts
    float4* hiBuf = nullptr;
    const float* lows[4] = {color, lo_plane0, lo_plane1, lo_plane2};
    const float* highs[3] = {hi_plane0, hi_plane1, hi_plane2};
    uint32_t got[2] = {0, 0};
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc(&buf, (7 * nlo + 4 * nhi + 1) * sizeof(float4));
    if (e == hipSuccess) hiBuf = buf + 7 * nlo;
    for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipMemcpy(buf + k * nlo, lows[k], nlo * sizeof(float4), hipMemcpyHostToDevice);
    for (int k = 0; k < 3 && e == hipSuccess; ++k) e = hipMemcpy(hiBuf + k * nhi, highs[k], nhi * sizeof(float4), hipMemcpyHostToDevice);
    uint32_t* counts = reinterpret_cast<uint32_t*>(hiBuf + 4 * nhi);
    if (e == hipSuccess)
        e = upsample_run(nullptr, *params, lo_w, lo_h, buf, buf + nlo, hi_w, hi_h, hiBuf, buf + 4 * nlo, hiBuf + 3 * nhi, counts,
                         nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, hiBuf + 3 * nhi, nhi * sizeof(float4), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(got, counts, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    if (e != hipSuccess) return refuse(PT_ERR_HIP, std::string("HIP error: ") + hipGetErrorString(e));
    if (out_counts) {
        out_counts[0] = got[0];
        out_counts[1] = got[1];
    }
    return PT_OK;
}

} // extern "C"
