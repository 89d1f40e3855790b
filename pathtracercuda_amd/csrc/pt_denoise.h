// Feature pass and denoiser entry points (pt_render_features, pt_read_features, pt_denoise,
// pt_read_denoised, pt_tonemap_denoised, pt_denoise_image); kernels in pt_dev_denoise.h.
// Part of the trace kernel's single translation unit: included by pt_kernels.hip after the C ABI
// definitions (pt_context); not a standalone header.
#pragma once

static thread_local std::string g_freeError;      // pt_last_error(NULL): context-free calls

// The field a parameter set is refused for, or null.  Written so that a NaN fails every range.
static const char* denoise_refusal(const pt_denoise_params* p)
{
    if (!p) return "params is null";
    if (!(p->iterations >= 1u && p->iterations <= 8u)) return "iterations must be 1..8";
    if (!(p->sigma_color > 0.0f) || !(p->sigma_color - p->sigma_color == 0.0f)) return "sigma_color must be > 0 and finite";
    if (!(p->sigma_plane >= 1e-6f) || !(p->sigma_plane - p->sigma_plane == 0.0f)) return "sigma_plane must be >= 1e-6 and finite";
    if (p->normal_power_log2 > 7u) return "normal_power_log2 must be 0..7";
    if (p->flags & ~(PT_DENOISE_DEMODULATE | PT_DENOISE_SAME_PRIMITIVE)) return "flags has unknown bits";
    if (p->staging > 2u) return "staging must be 0, 1 or 2";
    return nullptr;
}

// Steps staged in LDS by the automatic choice (staging = 0): those where staging won the same-session
// A/B at 1920 x 1080 (profiles/denoise_probe.json): s = 1 (-2 to -10 %) and s = 2 (-3 to -6 %);
// at s = 4 the halo is 4.5 x the tile and the staged form lost by 26 to 38 %.  Steps above 4 are never
// staged: the tile and halo would take 120 KB (pt_dev_denoise.h).
static bool denoise_stage_auto(uint32_t step) { return step <= 2u; }

// The filter on device buffers of npix = width x height float4: planes = 3 planes (pt_render_features'
// layout), g0, g1, ping, pong = scratch, out = the result.  ev (optional): 12 events recorded around the
// kernels (prepare, 8 iterations, finish; unused iterations record nothing).
static hipError_t denoise_run(hipStream_t stream, const pt_denoise_params& p, uint32_t width, uint32_t height,
                              const float4* color, const float4* planes, float4* g0, float4* g1, float4* ping,
                              float4* pong, float4* out, hipEvent_t* ev)
{
    const size_t npix = (size_t)width * height;
    const unsigned flat = (unsigned)((npix + 255) / 256);
    DenoiseArgs A = {};
    A.color = color;
    A.plane0 = planes;
    A.plane1 = planes + npix;
    A.plane2 = planes + 2 * npix;
    A.g0 = g0;
    A.g1 = g1;
    A.width = width;
    A.height = height;
    A.sigmaPlane = p.sigma_plane;
    A.normalPower = p.normal_power_log2;
    A.flags = p.flags;
    hipError_t e;
    if (ev && (e = hipEventRecord(ev[0], stream)) != hipSuccess) return e;
    A.dst = ping;
    dn_prepare_kernel<<<flat, 256, 0, stream>>>(A);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[1], stream)) != hipSuccess) return e;
    const dim3 grid((width + kDnTileW - 1) / kDnTileW, (height + kDnTileH - 1) / kDnTileH);
    float4* src = ping;
    float4* dst = pong;
    for (uint32_t i = 0; i < p.iterations; ++i) {
        const uint32_t s = 1u << i;
        const float sigma = p.sigma_color * (1.0f / (float)s);        // exact: a power of two
        A.step = s;
        A.ss = sigma * sigma;
        A.src = src;
        A.dst = dst;
        const bool staged = s <= 4u && (p.staging == 1u || (p.staging == 0u && denoise_stage_auto(s)));
        if (staged) {
            const size_t lds = (size_t)3 * (kDnTileW + 4 * s) * (kDnTileH + 4 * s) * sizeof(float4);
            dn_iter_kernel<true><<<grid, 256, lds, stream>>>(A);
        } else {
            dn_iter_kernel<false><<<grid, 256, 0, stream>>>(A);
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (ev && (e = hipEventRecord(ev[2 + i], stream)) != hipSuccess) return e;
        std::swap(src, dst);
    }
    A.src = src;
    A.dst = out;
    dn_finish_kernel<<<flat, 256, 0, stream>>>(A);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[11], stream)) != hipSuccess) return e;
    return hipSuccess;
}

// The filter on a whole-frame context whose arguments and state have been checked, guided by its feature
// planes: of `color` (device memory of the context, pt_denoise_temporal) or, when that is null, of the
// accumulation over `frames` or the per-pixel counts (pt_denoise).  The result goes to the context's
// denoised image, the kernel times to dnMs.
static int denoise_context(pt_context* ctx, const pt_denoise_params& p, const float4* color, uint32_t frames)
{
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    denoise_begins(ctx->st);
    if (!ctx->dnBuf) {
        PT_HIP_CHECK(ctx, hipMalloc(&ctx->dnBuf, 6 * npix * sizeof(float4)));   // colour, g0, g1, ping, pong, out
        for (auto& e : ctx->dnEv) PT_HIP_CHECK(ctx, hipEventCreate(&e));
    }
    if (!color) {
        const float inv = 1.0f / fmaxf((float)frames, 1.0f);
        dn_color_kernel<<<(unsigned)((npix + 255) / 256), 256, 0, ctx->stream>>>(
            ctx->dnBuf, ctx->accum, counts_describe_buffer(ctx->st) ? ctx->adMom + 2 * npix : nullptr, npix, inv);
        PT_HIP_CHECK(ctx, hipGetLastError());
        color = ctx->dnBuf;
    }
    PT_HIP_CHECK(ctx, denoise_run(ctx->stream, p, ctx->width, ctx->height, color, ctx->feat, ctx->dnBuf + npix,
                                  ctx->dnBuf + 2 * npix, ctx->dnBuf + 3 * npix, ctx->dnBuf + 4 * npix,
                                  ctx->dnBuf + 5 * npix, ctx->dnEv));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (float& m : ctx->dnMs) m = 0.0f;
    PT_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->dnMs[0], ctx->dnEv[0], ctx->dnEv[1]));
    for (uint32_t i = 0; i < p.iterations; ++i)
        PT_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->dnMs[1 + i], ctx->dnEv[1 + i], ctx->dnEv[2 + i]));
    PT_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->dnMs[9], ctx->dnEv[1 + p.iterations], ctx->dnEv[11]));
    denoise_done(ctx->st);
    return PT_OK;
}

extern "C" {

PT_API int pt_render_features(pt_context* ctx, const pt_camera* camera)
{
    if (!ctx || !camera) return PT_ERR_ARG;
    if (!ctx->nodes || ctx->primCount == 0) return fail(ctx, PT_ERR_STATE, "pt_render_features: no scene is set");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    features_begin(ctx->st);
    ctx->featCam = *camera;
    if (!ctx->feat) PT_HIP_CHECK(ctx, hipMalloc(&ctx->feat, 3 * std::max(npix, (size_t)1) * sizeof(float4)));
    ctx->featMs = 0.0f;
    if (npix) {
        FeatureParams P = {};
        P.planes = ctx->feat;
        P.nodes = ctx->nodes;
        P.prims = ctx->prims;
        P.mats = ctx->mats;
        P.textures = ctx->texTable;
        P.width = ctx->width;
        P.rows = ctx->rows;
        P.rowOffset = ctx->rowOffset;
        P.rowStride = ctx->rowStride;
        P.bandShift = ctx->bandShift;
        P.fwidth = (float)ctx->width;
        P.fheight = (float)ctx->height;
        P.tilesX = (ctx->width + 7) / 8;
        P.tiles = P.tilesX * ((ctx->rows + 7) / 8);
        P.stackDepth = ctx->stackDepth;
        P.slabFast = ctx->slabFast ? 1u : 0u;
        P.cam.origin = hf3(camera->origin);
        P.cam.llc = hf3(camera->lower_left_corner);
        P.cam.horizontal = hf3(camera->horizontal);
        P.cam.vertical = hf3(camera->vertical);
        const size_t lds = (size_t)4 * ctx->stackDepth * 64 * sizeof(uint32_t);
        PT_HIP_CHECK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        features_kernel<<<(P.tiles + 3) / 4, 256, lds, ctx->stream>>>(P);
        PT_HIP_CHECK(ctx, hipGetLastError());
        PT_HIP_CHECK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        PT_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->featMs, ctx->ev0, ctx->ev1));
    }
    features_done(ctx->st);
    return PT_OK;
}

PT_API int pt_read_features(pt_context* ctx, uint32_t plane, float* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (plane > 2u) return fail(ctx, PT_ERR_ARG, "pt_read_features: plane must be 0, 1 or 2");
    if (!planes_current(ctx->st))
        return fail(ctx, PT_ERR_STATE, "pt_read_features: no feature planes (no pt_render_features since the scene or a texture was set)");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    PT_HIP_CHECK(ctx, hipMemcpy(dst, ctx->feat + plane * npix, npix * sizeof(float4), hipMemcpyDeviceToHost));
    return PT_OK;
}

PT_API int pt_read_features_timing(pt_context* ctx, float* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!planes_current(ctx->st)) return fail(ctx, PT_ERR_STATE, "pt_read_features_timing: no feature planes");
    *dst = ctx->featMs;
    return PT_OK;
}

PT_API int pt_denoise(pt_context* ctx, uint32_t frames, const pt_denoise_params* params)
{
    if (!ctx) return PT_ERR_ARG;
    if (const char* why = denoise_refusal(params)) return fail(ctx, PT_ERR_ARG, (std::string("pt_denoise: ") + why).c_str());
    if (ctx->rows != ctx->height)
        return fail(ctx, PT_ERR_ARG, "pt_denoise: the context holds a band partition, not the whole frame "
                                     "(gather the frame and use pt_denoise_image)");
    if (!planes_current(ctx->st))
        return fail(ctx, PT_ERR_STATE, "pt_denoise: no feature planes (no pt_render_features since the scene or a texture was set)");
    return denoise_context(ctx, *params, nullptr, frames);
}

PT_API int pt_read_denoise_timing(pt_context* ctx, float* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!holds_denoised(ctx->st)) return fail(ctx, PT_ERR_STATE, "pt_read_denoise_timing: no denoised image");
    for (int k = 0; k < 10; ++k) dst[k] = ctx->dnMs[k];
    return PT_OK;
}

PT_API int pt_read_denoised(pt_context* ctx, float* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!holds_denoised(ctx->st)) return fail(ctx, PT_ERR_STATE, "pt_read_denoised: no denoised image (no pt_denoise yet)");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    PT_HIP_CHECK(ctx, hipMemcpy(dst, ctx->dnBuf + 5 * npix, npix * sizeof(float4), hipMemcpyDeviceToHost));
    return PT_OK;
}

PT_API int pt_tonemap_denoised(pt_context* ctx, uint8_t* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!holds_denoised(ctx->st)) return fail(ctx, PT_ERR_STATE, "pt_tonemap_denoised: no denoised image (no pt_denoise yet)");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    if (!ctx->ldr) PT_HIP_CHECK(ctx, hipMalloc(&ctx->ldr, npix * sizeof(uchar4)));
    tonemap_denoised_kernel<<<(unsigned)((npix + 255) / 256), 256, 0, ctx->stream>>>(ctx->ldr, ctx->dnBuf + 5 * npix, npix);
    PT_HIP_CHECK(ctx, hipGetLastError());
    PT_HIP_CHECK(ctx, hipMemcpyAsync(dst, ctx->ldr, npix * sizeof(uchar4), hipMemcpyDeviceToHost, ctx->stream));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return PT_OK;
}

PT_API int pt_denoise_image(int device, uint32_t width, uint32_t height, const float* color, const float* plane0,
                            const float* plane1, const float* plane2, const pt_denoise_params* params, float* out)
{
    auto refuse = [](int code, const std::string& msg) {
        g_freeError = "pt_denoise_image: " + msg;
        return code;
    };
    if (const char* why = denoise_refusal(params)) return refuse(PT_ERR_ARG, why);
    if (!color || !plane0 || !plane1 || !plane2 || !out) return refuse(PT_ERR_ARG, "an array is null");
    if (width == 0 || height == 0 || (uint64_t)width * height >= (1ull << 30) || height > 8u * 0xffffu)
        return refuse(PT_ERR_ARG, "width x height must be 1 .. 2^30 - 1 pixels, height at most 524280");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return refuse(PT_ERR_NO_DEVICE, "no GPU visible");
    if (device < 0 || device >= n) return refuse(PT_ERR_ARG, "device out of range");
    const size_t npix = (size_t)width * height;
    float4* buf = nullptr;                  // colour, 3 planes, g0, g1, ping, pong, out
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc(&buf, 9 * npix * sizeof(float4));
    if (e == hipSuccess) e = hipMemcpy(buf, color, npix * sizeof(float4), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(buf + npix, plane0, npix * sizeof(float4), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(buf + 2 * npix, plane1, npix * sizeof(float4), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(buf + 3 * npix, plane2, npix * sizeof(float4), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = denoise_run(nullptr, *params, width, height, buf, buf + npix, buf + 4 * npix, buf + 5 * npix, buf + 6 * npix,
                        buf + 7 * npix, buf + 8 * npix, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, buf + 8 * npix, npix * sizeof(float4), hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    if (e != hipSuccess) return refuse(PT_ERR_HIP, std::string("HIP error: ") + hipGetErrorString(e));
    return PT_OK;
}

} // extern "C"
