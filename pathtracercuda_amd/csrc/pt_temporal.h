// Temporal reprojection entry points (pt_temporal, pt_read_temporal, pt_tonemap_temporal,
// pt_read_temporal_timing, pt_denoise_temporal, pt_temporal_image, pt_temporal_motion_image); the kernels are
// in pt_dev_temporal.h.
// Part of the trace kernel's single translation unit: included by pt_kernels.hip after pt_denoise.h;
// not a standalone header.
#pragma once

// The field a parameter set is refused for, or null.  Written so that a NaN fails every range.
static const char* temporal_refusal(const pt_temporal_params* p)
{
    if (!p) return "params is null";
    if (!(p->alpha_min >= 0.0f && p->alpha_min <= 1.0f)) return "alpha_min must be 0..1";
    if (!(p->max_history >= 1u && p->max_history <= 65535u)) return "max_history must be 1..65535";
    if (!(p->sigma_plane >= 1e-6f) || !(p->sigma_plane - p->sigma_plane == 0.0f)) return "sigma_plane must be >= 1e-6 and finite";
    if (!(p->normal_cos_min >= -1.0f && p->normal_cos_min <= 1.0f)) return "normal_cos_min must be -1..1";
    if (p->flags & ~(PT_TEMPORAL_DEMODULATE | PT_TEMPORAL_SAME_PRIMITIVE)) return "flags has unknown bits";
    return nullptr;
}

// One step on device buffers of width x height float4.  planes = 3 planes (pt_render_features' layout);
// prev = the previous history's 3 planes or null; next = the new history's 3 planes.  motion (optional): the
// table of rule 7, and the step is temporal_motion_kernel's.
static hipError_t temporal_run(hipStream_t stream, const pt_temporal_params& p, uint32_t width, uint32_t height,
                               const float4* color, const float4* planes, const pt_camera& cur, const float4* prev,
                               const pt_camera& prevCam, float4* image, float4* next, const MotionTable* motion = nullptr)
{
    const size_t npix = (size_t)width * height;
    TemporalArgs A = {};
    A.color = color;
    A.plane0 = planes;
    A.plane1 = planes + npix;
    A.plane2 = planes + 2 * npix;
    A.ph0 = prev;
    A.ph1 = prev ? prev + npix : nullptr;
    A.ph2 = prev ? prev + 2 * npix : nullptr;
    A.image = image;
    A.h0 = next;
    A.h1 = next + npix;
    A.h2 = next + 2 * npix;
    A.width = width;
    A.height = height;
    A.alphaMin = p.alpha_min;
    A.maxHistory = (float)p.max_history;
    A.sigmaPlane = p.sigma_plane;
    A.normalCosMin = p.normal_cos_min;
    A.flags = p.flags;
    A.cur = cur;
    A.prev = prevCam;
    const dim3 grid((width + kDnTileW - 1) / kDnTileW, (height + kDnTileH - 1) / kDnTileH);
    if (motion) {
        const TemporalMotionArgs B = {A, *motion};
        temporal_motion_kernel<<<grid, 256, 0, stream>>>(B);
    } else {
        temporal_kernel<<<grid, 256, 0, stream>>>(A);
    }
    return hipGetLastError();
}

extern "C" {

PT_API int pt_temporal(pt_context* ctx, uint32_t frames, const pt_temporal_params* params, int reset, int* history_used)
{
    if (!ctx) return PT_ERR_ARG;
    if (const char* why = temporal_refusal(params)) return fail(ctx, PT_ERR_ARG, (std::string("pt_temporal: ") + why).c_str());
    if (ctx->rows != ctx->height)
        return fail(ctx, PT_ERR_ARG, "pt_temporal: the context holds a band partition, not the whole frame "
                                     "(gather the frame and use pt_temporal_image)");
    if (!planes_current(ctx->st))
        return fail(ctx, PT_ERR_STATE, "pt_temporal: no feature planes (no pt_render_features since the scene or a texture was set)");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    const bool use = history_held(ctx->st) && !reset;
    const bool moved = holds_motion(ctx->st);                 // asked before the pass begins, as `use`
    const MotionTable table = {ctx->motion, ctx->motionCount};
    temporal_begins(ctx->st);
    if (!ctx->tpBuf) PT_HIP_CHECK(ctx, hipMalloc(&ctx->tpBuf, 8 * std::max(npix, (size_t)1) * sizeof(float4)));
    ctx->tpMs = 0.0f;
    const uint32_t from = ctx->tpSet, to = ctx->tpSet ^ 1u;
    if (npix) {
        float4* color = ctx->tpBuf;
        const float inv = 1.0f / fmaxf((float)frames, 1.0f);
        dn_color_kernel<<<(unsigned)((npix + 255) / 256), 256, 0, ctx->stream>>>(
            color, ctx->accum, counts_describe_buffer(ctx->st) ? ctx->adMom + 2 * npix : nullptr, npix, inv);
        PT_HIP_CHECK(ctx, hipGetLastError());
        PT_HIP_CHECK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        PT_HIP_CHECK(ctx, temporal_run(ctx->stream, *params, ctx->width, ctx->height, color, ctx->feat, ctx->featCam,
                                       use ? ctx->tpBuf + (2 + 3 * from) * npix : nullptr, ctx->tpCam, ctx->tpBuf + npix,
                                       ctx->tpBuf + (2 + 3 * to) * npix, moved ? &table : nullptr));
        PT_HIP_CHECK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        PT_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->tpMs, ctx->ev0, ctx->ev1));
    }
    ctx->tpSet = to;
    ctx->tpCam = ctx->featCam;
    if (history_used) *history_used = use ? 1 : 0;
    temporal_done(ctx->st);
    return PT_OK;
}

PT_API int pt_read_temporal(pt_context* ctx, float* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!holds_temporal(ctx->st)) return fail(ctx, PT_ERR_STATE, "pt_read_temporal: no temporal image (no pt_temporal yet)");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    PT_HIP_CHECK(ctx, hipMemcpy(dst, ctx->tpBuf + npix, npix * sizeof(float4), hipMemcpyDeviceToHost));
    return PT_OK;
}

PT_API int pt_tonemap_temporal(pt_context* ctx, uint8_t* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!holds_temporal(ctx->st)) return fail(ctx, PT_ERR_STATE, "pt_tonemap_temporal: no temporal image (no pt_temporal yet)");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    if (!ctx->ldr) PT_HIP_CHECK(ctx, hipMalloc(&ctx->ldr, npix * sizeof(uchar4)));
    tonemap_denoised_kernel<<<(unsigned)((npix + 255) / 256), 256, 0, ctx->stream>>>(ctx->ldr, ctx->tpBuf + npix, npix);
    PT_HIP_CHECK(ctx, hipGetLastError());
    PT_HIP_CHECK(ctx, hipMemcpyAsync(dst, ctx->ldr, npix * sizeof(uchar4), hipMemcpyDeviceToHost, ctx->stream));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return PT_OK;
}

PT_API int pt_read_temporal_timing(pt_context* ctx, float* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!holds_temporal(ctx->st)) return fail(ctx, PT_ERR_STATE, "pt_read_temporal_timing: no temporal image");
    *dst = ctx->tpMs;
    return PT_OK;
}

PT_API int pt_denoise_temporal(pt_context* ctx, const pt_denoise_params* params)
{
    if (!ctx) return PT_ERR_ARG;
    if (const char* why = denoise_refusal(params))
        return fail(ctx, PT_ERR_ARG, (std::string("pt_denoise_temporal: ") + why).c_str());
    if (!holds_temporal(ctx->st)) return fail(ctx, PT_ERR_STATE, "pt_denoise_temporal: no temporal image (no pt_temporal yet)");
    if (!temporal_of_planes(ctx->st))
        return fail(ctx, PT_ERR_STATE, "pt_denoise_temporal: pt_render_features has run since the temporal image was made "
                                       "(its planes are no longer held)");
    // (the whole frame: pt_temporal refuses anything else)
    return denoise_context(ctx, *params, ctx->tpBuf + (size_t)ctx->rows * ctx->width, 0);
}

PT_API int pt_temporal_image(int device, uint32_t width, uint32_t height, const float* color, const float* plane0,
                             const float* plane1, const float* plane2, const pt_camera* cur_cam, const float* hist0,
                             const float* hist1, const float* hist2, const pt_camera* prev_cam,
                             const pt_temporal_params* params, float* out_image, float* out_hist0, float* out_hist1,
                             float* out_hist2)
{
    auto refuse = [](int code, const std::string& msg) {
        g_freeError = "pt_temporal_image: " + msg;
        return code;
    };
    if (const char* why = temporal_refusal(params)) return refuse(PT_ERR_ARG, why);
    if (!color || !plane0 || !plane1 || !plane2 || !cur_cam || !out_image || !out_hist0 || !out_hist1 || !out_hist2)
        return refuse(PT_ERR_ARG, "an array or cur_cam is null");
    if (hist0 && (!hist1 || !hist2 || !prev_cam)) return refuse(PT_ERR_ARG, "hist0 is given without hist1, hist2 and prev_cam");
    if (width == 0 || height == 0 || (uint64_t)width * height >= (1ull << 30) || height > 8u * 0xffffu)
        return refuse(PT_ERR_ARG, "width x height must be 1 .. 2^30 - 1 pixels, height at most 524280");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return refuse(PT_ERR_NO_DEVICE, "no GPU visible");
    if (device < 0 || device >= n) return refuse(PT_ERR_ARG, "device out of range");
    const size_t npix = (size_t)width * height, bytes = npix * sizeof(float4);
    float4* buf = nullptr;                  // colour, 3 planes, 3 previous, image, 3 next
    const float* in[7] = {color, plane0, plane1, plane2, hist0, hist1, hist2};
    float* out[4] = {out_image, out_hist0, out_hist1, out_hist2};
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc(&buf, 11 * bytes);
    for (int k = 0; k < (hist0 ? 7 : 4) && e == hipSuccess; ++k) e = hipMemcpy(buf + k * npix, in[k], bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = temporal_run(nullptr, *params, width, height, buf, buf + npix, *cur_cam, hist0 ? buf + 4 * npix : nullptr,
                         hist0 ? *prev_cam : *cur_cam, buf + 7 * npix, buf + 8 * npix);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipMemcpy(out[k], buf + (7 + k) * npix, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    if (e != hipSuccess) return refuse(PT_ERR_HIP, std::string("HIP error: ") + hipGetErrorString(e));
    return PT_OK;
}

PT_API int pt_temporal_motion_image(int device, uint32_t width, uint32_t height, const float* color, const float* plane0,
                             const float* plane1, const float* plane2, const pt_camera* cur_cam, const float* hist0,
                             const float* hist1, const float* hist2, const pt_camera* prev_cam,
                             const pt_temporal_params* params, float* out_image, float* out_hist0, float* out_hist1,
                             float* out_hist2, uint32_t prim_count, const float* motion_rows, const uint32_t* prev_index)
{
    auto refuse = [](int code, const std::string& msg) {
        g_freeError = "pt_temporal_motion_image: " + msg;
        return code;
    };
    if (const char* why = temporal_refusal(params)) return refuse(PT_ERR_ARG, why);
    if (!color || !plane0 || !plane1 || !plane2 || !cur_cam || !out_image || !out_hist0 || !out_hist1 || !out_hist2)
        return refuse(PT_ERR_ARG, "an array or cur_cam is null");
    if (hist0 && (!hist1 || !hist2 || !prev_cam)) return refuse(PT_ERR_ARG, "hist0 is given without hist1, hist2 and prev_cam");
    if (width == 0 || height == 0 || (uint64_t)width * height >= (1ull << 30) || height > 8u * 0xffffu)
        return refuse(PT_ERR_ARG, "width x height must be 1 .. 2^30 - 1 pixels, height at most 524280");
    if (const char* why = motion_table_refusal(prim_count, motion_rows, prev_index)) return refuse(PT_ERR_ARG, why);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return refuse(PT_ERR_NO_DEVICE, "no GPU visible");
    if (device < 0 || device >= n) return refuse(PT_ERR_ARG, "device out of range");
    const size_t npix = (size_t)width * height, bytes = npix * sizeof(float4);
    float4* buf = nullptr;                  // colour, 3 planes, 3 previous, image, 3 next
    const float* in[7] = {color, plane0, plane1, plane2, hist0, hist1, hist2};
    float* out[4] = {out_image, out_hist0, out_hist1, out_hist2};
    const std::vector<float4> entries = motion_table_pack(prim_count, motion_rows, prev_index);
    float4* table = nullptr;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc(&buf, 11 * bytes);
    if (e == hipSuccess) e = hipMalloc(&table, entries.size() * sizeof(float4));
    if (e == hipSuccess) e = hipMemcpy(table, entries.data(), entries.size() * sizeof(float4), hipMemcpyHostToDevice);
    const MotionTable motion = {table, prim_count};
    for (int k = 0; k < (hist0 ? 7 : 4) && e == hipSuccess; ++k) e = hipMemcpy(buf + k * npix, in[k], bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = temporal_run(nullptr, *params, width, height, buf, buf + npix, *cur_cam, hist0 ? buf + 4 * npix : nullptr,
                         hist0 ? *prev_cam : *cur_cam, buf + 7 * npix, buf + 8 * npix, &motion);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipMemcpy(out[k], buf + (7 + k) * npix, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    (void)hipFree(table);
    if (e != hipSuccess) return refuse(PT_ERR_HIP, std::string("HIP error: ") + hipGetErrorString(e));
    return PT_OK;
}

} // extern "C"
