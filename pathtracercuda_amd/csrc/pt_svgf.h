// Entry points of the per-pixel variance and the variance-guided filter (pt_temporal_moments,
// pt_read_temporal_variance, pt_read_temporal_moments_timing, pt_denoise_variance, pt_temporal_moments_image,
// pt_denoise_variance_image) and of the feedback of the filtered colour into the history
// (pt_denoise_variance_feedback, pt_read_feedback_timing, pt_read_temporal_history,
// pt_denoise_variance_feedback_image), and the moments step across moved objects
// (pt_temporal_moments_motion_image); the kernels are in pt_dev_svgf.h.  Part of the trace kernel's single
// translation unit: included by pt_kernels.hip after pt_temporal.h; not a standalone header.
#pragma once

static const char* variance_refusal(const pt_variance_params* p)
{
    if (!p) return "variance params is null";
    if (!(p->min_temporal >= 1u && p->min_temporal <= 255u)) return "min_temporal must be 1..255";
    return nullptr;
}

// The field a parameter set is refused for, or null.  Written so that a NaN fails every range.
static const char* vdenoise_refusal(const pt_vdenoise_params* p)
{
    if (!p) return "params is null";
    if (!(p->iterations >= 1u && p->iterations <= 8u)) return "iterations must be 1..8";
    if (!(p->sigma_l > 0.0f && p->sigma_l <= 1048576.0f)) return "sigma_l must be in (0, 2^20]";
    if (!(p->variance_floor > 0.0f) || !(p->variance_floor - p->variance_floor == 0.0f))
        return "variance_floor must be > 0 and finite";
    if (!(p->sigma_plane >= 1e-6f) || !(p->sigma_plane - p->sigma_plane == 0.0f)) return "sigma_plane must be >= 1e-6 and finite";
    if (p->normal_power_log2 > 7u) return "normal_power_log2 must be 0..7";
    if (p->flags & ~(PT_DENOISE_DEMODULATE | PT_DENOISE_SAME_PRIMITIVE)) return "flags has unknown bits";
    if (p->staging > 2u) return "staging must be 0, 1 or 2";
    return nullptr;
}

// Steps staged in LDS by the automatic choice (staging = 0): those where staging won the same-session A/B at
// 1920 x 1080 (profiles/svgf_probe.json): s = 1 (-16 to -21 %) and s = 2 (-15 to -18 %); at
// s = 4 the staged form lost by 16 to 24 %.  The same steps as denoise_stage_auto, by this kernel's own times.
static bool vdenoise_stage_auto(uint32_t step) { return step <= 2u; }

// The step and the estimate on device buffers of width x height: temporal_run's arguments, with the
// previous moments plane (read only with prev), the new one and the variance.  ev (optional): 3 events
// recorded around the two kernels.  motion (optional): the table of rule 7, and the step is
// temporal_moments_motion_kernel's.
static hipError_t moments_run(hipStream_t stream, const pt_temporal_params& p, const pt_variance_params& v, uint32_t width,
                              uint32_t height, const float4* color, const float4* planes, const pt_camera& cur,
                              const float4* prev, const float4* prev3, const pt_camera& prevCam, float4* image, float4* next,
                              float4* next3, float* var, hipEvent_t* ev, const MotionTable* motion = nullptr)
{
    const size_t npix = (size_t)width * height;
    MomentsArgs M = {};
    TemporalArgs& A = M.T;
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
    M.ph3 = prev ? prev3 : nullptr;
    M.h3 = next3;
    VarianceArgs V = {};
    V.h0 = next;
    V.h1 = next + npix;
    V.h2 = next + 2 * npix;
    V.h3 = next3;
    V.var = var;
    V.width = width;
    V.height = height;
    V.minTemporal = (float)v.min_temporal;
    V.sigmaPlane = p.sigma_plane;
    V.normalCosMin = p.normal_cos_min;
    V.flags = p.flags;
    const dim3 grid((width + kDnTileW - 1) / kDnTileW, (height + kDnTileH - 1) / kDnTileH);
    hipError_t e;
    if (ev && (e = hipEventRecord(ev[0], stream)) != hipSuccess) return e;
    if (motion) {
        const MomentsMotionArgs B = {M, *motion};
        temporal_moments_motion_kernel<<<grid, 256, 0, stream>>>(B);
    } else {
        temporal_moments_kernel<<<grid, 256, 0, stream>>>(M);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[1], stream)) != hipSuccess) return e;
    variance_kernel<<<grid, 256, 0, stream>>>(V);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[2], stream)) != hipSuccess) return e;
    return hipSuccess;
}

// denoise_run with the variance: the same buffers and events.  level >= 1 (the feedback, checked by the
// caller to be <= iterations): the texel iteration level - 1 wrote goes into the history colours fbH0 right
// after that iteration, between the optional events fbEv[0] and fbEv[1]; the filter reads nothing of fbH0.
static hipError_t vdenoise_run(hipStream_t stream, const pt_vdenoise_params& p, uint32_t width, uint32_t height,
                               const float4* color, const float4* planes, const float* var, float4* g0, float4* g1,
                               float4* ping, float4* pong, float4* out, hipEvent_t* ev, uint32_t level = 0,
                               float4* fbH0 = nullptr, hipEvent_t* fbEv = nullptr)
{
    const size_t npix = (size_t)width * height;
    const unsigned flat = (unsigned)((npix + 255) / 256);
    VDenoiseArgs V = {};
    DenoiseArgs& A = V.D;
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
    V.var = var;
    V.sl2 = p.sigma_l * p.sigma_l;
    V.floorV = p.variance_floor;
    hipError_t e;
    if (ev && (e = hipEventRecord(ev[0], stream)) != hipSuccess) return e;
    A.dst = ping;
    vdn_prepare_kernel<<<flat, 256, 0, stream>>>(V);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[1], stream)) != hipSuccess) return e;
    const dim3 grid((width + kDnTileW - 1) / kDnTileW, (height + kDnTileH - 1) / kDnTileH);
    float4* src = ping;
    float4* dst = pong;
    for (uint32_t i = 0; i < p.iterations; ++i) {
        const uint32_t s = 1u << i;
        A.step = s;
        A.src = src;
        A.dst = dst;
        const bool staged = s <= 4u && (p.staging == 1u || (p.staging == 0u && vdenoise_stage_auto(s)));
        if (staged) {
            const size_t lds = (size_t)3 * (kDnTileW + 4 * s) * (kDnTileH + 4 * s) * sizeof(float4);
            vdn_iter_kernel<true><<<grid, 256, lds, stream>>>(V);
        } else {
            vdn_iter_kernel<false><<<grid, 256, 0, stream>>>(V);
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (ev && (e = hipEventRecord(ev[2 + i], stream)) != hipSuccess) return e;
        if (level == i + 1u) {                           // dst is the buffer this iteration wrote, whatever the parity
            const FeedbackArgs B = {dst, fbH0, npix};
            if (fbEv && (e = hipEventRecord(fbEv[0], stream)) != hipSuccess) return e;
            vdn_feedback_kernel<<<flat, 256, 0, stream>>>(B);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            if (fbEv && (e = hipEventRecord(fbEv[1], stream)) != hipSuccess) return e;
        }
        std::swap(src, dst);
    }
    A.src = src;
    A.dst = out;
    vdn_finish_kernel<<<flat, 256, 0, stream>>>(V);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[11], stream)) != hipSuccess) return e;
    return hipSuccess;
}

// The context's moments planes (two sets, beside tpBuf's two history sets) and its variance, in one allocation
static float* moments_variance(pt_context* ctx) { return reinterpret_cast<float*>(ctx->tmBuf + 2 * (size_t)ctx->rows * ctx->width); }

// pt_denoise_variance (level = 0) and pt_denoise_variance_feedback (level >= 1, already checked against
// params->iterations) on the context; `name` starts every message.
static int vdenoise_ctx(pt_context* ctx, const pt_vdenoise_params* params, uint32_t level, const char* name)
{
    if (!ctx) return PT_ERR_ARG;
    const std::string who(name);
    if (const char* why = vdenoise_refusal(params)) return fail(ctx, PT_ERR_ARG, (who + why).c_str());
    if (!history_has_moments(ctx->st))
        return fail(ctx, PT_ERR_STATE, (who + "no variance is held (no pt_temporal_moments since the history ended)").c_str());
    if (!temporal_of_planes(ctx->st))
        return fail(ctx, PT_ERR_STATE, (who + "pt_render_features has run since the variance was made "
                                              "(its planes are no longer held)").c_str());
    if ((params->flags ^ ctx->tmFlags) & PT_DENOISE_DEMODULATE)
        return fail(ctx, PT_ERR_ARG, (who + "flags: the DEMODULATE bit differs from the one the moments were made with").c_str());
    // (the whole frame: pt_temporal_moments refuses anything else)
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    denoise_begins(ctx->st);
    if (!ctx->dnBuf) {
        PT_HIP_CHECK(ctx, hipMalloc(&ctx->dnBuf, 6 * npix * sizeof(float4)));   // colour, g0, g1, ping, pong, out
        for (auto& e : ctx->dnEv) PT_HIP_CHECK(ctx, hipEventCreate(&e));
    }
    if (level && !ctx->fbEv[0])
        for (auto& e : ctx->fbEv) PT_HIP_CHECK(ctx, hipEventCreate(&e));
    // the history set the last moments step wrote: the one the next step reads
    PT_HIP_CHECK(ctx, vdenoise_run(ctx->stream, *params, ctx->width, ctx->height, ctx->tpBuf + npix, ctx->feat,
                                   moments_variance(ctx), ctx->dnBuf + npix, ctx->dnBuf + 2 * npix, ctx->dnBuf + 3 * npix,
                                   ctx->dnBuf + 4 * npix, ctx->dnBuf + 5 * npix, ctx->dnEv, level,
                                   ctx->tpBuf + (2 + 3 * ctx->tpSet) * npix, level ? ctx->fbEv : nullptr));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (float& m : ctx->dnMs) m = 0.0f;
    PT_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->dnMs[0], ctx->dnEv[0], ctx->dnEv[1]));
    // what follows the feedback kernel (iteration `level`, or the finish) starts at the feedback's second event
    for (uint32_t i = 0; i < params->iterations; ++i)
        PT_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->dnMs[1 + i], (level && i == level) ? ctx->fbEv[1] : ctx->dnEv[1 + i],
                                              ctx->dnEv[2 + i]));
    PT_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->dnMs[9],
                                          (level == params->iterations) ? ctx->fbEv[1] : ctx->dnEv[1 + params->iterations],
                                          ctx->dnEv[11]));
    if (level) {
        PT_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->fbMs, ctx->fbEv[0], ctx->fbEv[1]));
        ctx->fbRan = true;
    }
    denoise_done(ctx->st);
    return PT_OK;
}

static const char* vfeedback_refusal(const pt_vfeedback_params* f, uint32_t iterations)
{
    if (!f) return "feedback params is null";
    if (!(f->level >= 1u && f->level <= iterations)) return "level must be 1..iterations";
    return nullptr;
}

extern "C" {

PT_API int pt_temporal_moments(pt_context* ctx, uint32_t frames, const pt_temporal_params* params,
                               const pt_variance_params* variance, int reset, int* history_used)
{
    if (!ctx) return PT_ERR_ARG;
    if (const char* why = temporal_refusal(params)) return fail(ctx, PT_ERR_ARG, (std::string("pt_temporal_moments: ") + why).c_str());
    if (const char* why = variance_refusal(variance)) return fail(ctx, PT_ERR_ARG, (std::string("pt_temporal_moments: ") + why).c_str());
    if (ctx->rows != ctx->height)
        return fail(ctx, PT_ERR_ARG, "pt_temporal_moments: the context holds a band partition, not the whole frame "
                                     "(gather the frame and use pt_temporal_moments_image)");
    if (!planes_current(ctx->st))
        return fail(ctx, PT_ERR_STATE, "pt_temporal_moments: no feature planes (no pt_render_features since the scene or a texture was set)");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    const bool use = history_held(ctx->st) && history_has_moments(ctx->st) && !reset;
    const bool moved = holds_motion(ctx->st);                 // asked before the pass begins, as `use`
    const MotionTable table = {ctx->motion, ctx->motionCount};
    temporal_begins(ctx->st);
    if (!ctx->tpBuf) PT_HIP_CHECK(ctx, hipMalloc(&ctx->tpBuf, 8 * std::max(npix, (size_t)1) * sizeof(float4)));
    if (!ctx->tmBuf) {
        PT_HIP_CHECK(ctx, hipMalloc(&ctx->tmBuf, (2 * npix + (npix + 3) / 4 + 1) * sizeof(float4)));
        for (auto& e : ctx->tmEv) PT_HIP_CHECK(ctx, hipEventCreate(&e));
    }
    ctx->tpMs = ctx->tmMs[0] = ctx->tmMs[1] = 0.0f;
    ctx->fbRan = false;                       // the feedback time is of a call on the held history
    const uint32_t from = ctx->tpSet, to = ctx->tpSet ^ 1u;
    if (npix) {
        float4* color = ctx->tpBuf;
        const float inv = 1.0f / fmaxf((float)frames, 1.0f);
        dn_color_kernel<<<(unsigned)((npix + 255) / 256), 256, 0, ctx->stream>>>(
            color, ctx->accum, counts_describe_buffer(ctx->st) ? ctx->adMom + 2 * npix : nullptr, npix, inv);
        PT_HIP_CHECK(ctx, hipGetLastError());
        PT_HIP_CHECK(ctx, moments_run(ctx->stream, *params, *variance, ctx->width, ctx->height, color, ctx->feat, ctx->featCam,
                                      use ? ctx->tpBuf + (2 + 3 * from) * npix : nullptr, ctx->tmBuf + from * npix, ctx->tpCam,
                                      ctx->tpBuf + npix, ctx->tpBuf + (2 + 3 * to) * npix, ctx->tmBuf + to * npix,
                                      moments_variance(ctx), ctx->tmEv, moved ? &table : nullptr));
        PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        PT_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->tmMs[0], ctx->tmEv[0], ctx->tmEv[1]));
        PT_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->tmMs[1], ctx->tmEv[1], ctx->tmEv[2]));
        ctx->tpMs = ctx->tmMs[0];
    }
    ctx->tpSet = to;
    ctx->tpCam = ctx->featCam;
    ctx->tmFlags = params->flags;
    if (history_used) *history_used = use ? 1 : 0;
    temporal_done(ctx->st);
    moments_done(ctx->st);
    return PT_OK;
}

PT_API int pt_read_temporal_variance(pt_context* ctx, float* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!history_has_moments(ctx->st))
        return fail(ctx, PT_ERR_STATE, "pt_read_temporal_variance: no variance is held (no pt_temporal_moments since the history ended)");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    PT_HIP_CHECK(ctx, hipMemcpy(dst, moments_variance(ctx), npix * sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
}

PT_API int pt_read_temporal_moments_timing(pt_context* ctx, float* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!history_has_moments(ctx->st))
        return fail(ctx, PT_ERR_STATE, "pt_read_temporal_moments_timing: no variance is held (no pt_temporal_moments since the history ended)");
    dst[0] = ctx->tmMs[0];
    dst[1] = ctx->tmMs[1];
    return PT_OK;
}

PT_API int pt_denoise_variance(pt_context* ctx, const pt_vdenoise_params* params)
{
    return vdenoise_ctx(ctx, params, 0, "pt_denoise_variance: ");
}

PT_API int pt_denoise_variance_feedback(pt_context* ctx, const pt_vdenoise_params* params, const pt_vfeedback_params* feedback)
{
    if (!ctx) return PT_ERR_ARG;
    const char* name = "pt_denoise_variance_feedback: ";
    if (const char* why = vdenoise_refusal(params)) return fail(ctx, PT_ERR_ARG, (std::string(name) + why).c_str());
    if (const char* why = vfeedback_refusal(feedback, params->iterations))
        return fail(ctx, PT_ERR_ARG, (std::string(name) + why).c_str());
    return vdenoise_ctx(ctx, params, feedback->level, name);
}

PT_API int pt_read_feedback_timing(pt_context* ctx, float* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!history_has_moments(ctx->st) || !ctx->fbRan)
        return fail(ctx, PT_ERR_STATE, "pt_read_feedback_timing: no pt_denoise_variance_feedback has run on the held history");
    *dst = ctx->fbMs;
    return PT_OK;
}

PT_API int pt_read_temporal_history(pt_context* ctx, uint32_t plane, float* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!history_held(ctx->st))
        return fail(ctx, PT_ERR_STATE, "pt_read_temporal_history: no history is held (no pt_temporal since it ended)");
    if (plane > 3u) return fail(ctx, PT_ERR_ARG, "pt_read_temporal_history: plane must be 0..3");
    if (plane == 3u && !history_has_moments(ctx->st))
        return fail(ctx, PT_ERR_ARG, "pt_read_temporal_history: plane 3: the held history has no moments "
                                     "(no pt_temporal_moments step)");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    const float4* src = plane == 3u ? ctx->tmBuf + ctx->tpSet * npix : ctx->tpBuf + (2 + 3 * ctx->tpSet + plane) * npix;
    PT_HIP_CHECK(ctx, hipMemcpy(dst, src, npix * sizeof(float4), hipMemcpyDeviceToHost));
    return PT_OK;
}

PT_API int pt_temporal_moments_image(int device, uint32_t width, uint32_t height, const float* color, const float* plane0,
                                     const float* plane1, const float* plane2, const pt_camera* cur_cam, const float* hist0,
                                     const float* hist1, const float* hist2, const float* hist3, const pt_camera* prev_cam,
                                     const pt_temporal_params* params, const pt_variance_params* variance, float* out_image,
                                     float* out_hist0, float* out_hist1, float* out_hist2, float* out_hist3, float* out_variance)
{
    auto refuse = [](int code, const std::string& msg) {
        g_freeError = "pt_temporal_moments_image: " + msg;
        return code;
    };
    if (const char* why = temporal_refusal(params)) return refuse(PT_ERR_ARG, why);
    if (const char* why = variance_refusal(variance)) return refuse(PT_ERR_ARG, why);
    if (!color || !plane0 || !plane1 || !plane2 || !cur_cam || !out_image || !out_hist0 || !out_hist1 || !out_hist2 ||
        !out_hist3 || !out_variance)
        return refuse(PT_ERR_ARG, "an array or cur_cam is null");
    if (hist0 && (!hist1 || !hist2 || !hist3 || !prev_cam))
        return refuse(PT_ERR_ARG, "hist0 is given without hist1, hist2, hist3 and prev_cam");
    if (width == 0 || height == 0 || (uint64_t)width * height >= (1ull << 30) || height > 8u * 0xffffu)
        return refuse(PT_ERR_ARG, "width x height must be 1 .. 2^30 - 1 pixels, height at most 524280");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return refuse(PT_ERR_NO_DEVICE, "no GPU visible");
    if (device < 0 || device >= n) return refuse(PT_ERR_ARG, "device out of range");
    const size_t npix = (size_t)width * height, bytes = npix * sizeof(float4);
    float4* buf = nullptr;                  // colour, 3 planes, 4 previous, image, 4 next, the variance
    const float* in[8] = {color, plane0, plane1, plane2, hist0, hist1, hist2, hist3};
    float* out[5] = {out_image, out_hist0, out_hist1, out_hist2, out_hist3};
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc(&buf, 13 * bytes + npix * sizeof(float));
    for (int k = 0; k < (hist0 ? 8 : 4) && e == hipSuccess; ++k) e = hipMemcpy(buf + k * npix, in[k], bytes, hipMemcpyHostToDevice);
    float* var = reinterpret_cast<float*>(buf + 13 * npix);
    if (e == hipSuccess)
        e = moments_run(nullptr, *params, *variance, width, height, buf, buf + npix, *cur_cam, hist0 ? buf + 4 * npix : nullptr,
                        buf + 7 * npix, hist0 ? *prev_cam : *cur_cam, buf + 8 * npix, buf + 9 * npix, buf + 12 * npix, var,
                        nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    for (int k = 0; k < 5 && e == hipSuccess; ++k) e = hipMemcpy(out[k], buf + (8 + k) * npix, bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_variance, var, npix * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    if (e != hipSuccess) return refuse(PT_ERR_HIP, std::string("HIP error: ") + hipGetErrorString(e));
    return PT_OK;
}

PT_API int pt_temporal_moments_motion_image(int device, uint32_t width, uint32_t height, const float* color, const float* plane0,
                                     const float* plane1, const float* plane2, const pt_camera* cur_cam, const float* hist0,
                                     const float* hist1, const float* hist2, const float* hist3, const pt_camera* prev_cam,
                                     const pt_temporal_params* params, const pt_variance_params* variance, float* out_image,
                                     float* out_hist0, float* out_hist1, float* out_hist2, float* out_hist3, float* out_variance,
                                            uint32_t prim_count, const float* motion_rows, const uint32_t* prev_index)
{
    auto refuse = [](int code, const std::string& msg) {
        g_freeError = "pt_temporal_moments_motion_image: " + msg;
        return code;
    };
    if (const char* why = temporal_refusal(params)) return refuse(PT_ERR_ARG, why);
    if (const char* why = variance_refusal(variance)) return refuse(PT_ERR_ARG, why);
    if (!color || !plane0 || !plane1 || !plane2 || !cur_cam || !out_image || !out_hist0 || !out_hist1 || !out_hist2 ||
        !out_hist3 || !out_variance)
        return refuse(PT_ERR_ARG, "an array or cur_cam is null");
    if (hist0 && (!hist1 || !hist2 || !hist3 || !prev_cam))
        return refuse(PT_ERR_ARG, "hist0 is given without hist1, hist2, hist3 and prev_cam");
    if (width == 0 || height == 0 || (uint64_t)width * height >= (1ull << 30) || height > 8u * 0xffffu)
        return refuse(PT_ERR_ARG, "width x height must be 1 .. 2^30 - 1 pixels, height at most 524280");
    if (const char* why = motion_table_refusal(prim_count, motion_rows, prev_index)) return refuse(PT_ERR_ARG, why);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return refuse(PT_ERR_NO_DEVICE, "no GPU visible");
    if (device < 0 || device >= n) return refuse(PT_ERR_ARG, "device out of range");
    const size_t npix = (size_t)width * height, bytes = npix * sizeof(float4);
    float4* buf = nullptr;                  // colour, 3 planes, 4 previous, image, 4 next, the variance
    const float* in[8] = {color, plane0, plane1, plane2, hist0, hist1, hist2, hist3};
    float* out[5] = {out_image, out_hist0, out_hist1, out_hist2, out_hist3};
    const std::vector<float4> entries = motion_table_pack(prim_count, motion_rows, prev_index);
    float4* table = nullptr;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc(&buf, 13 * bytes + npix * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&table, entries.size() * sizeof(float4));
    if (e == hipSuccess) e = hipMemcpy(table, entries.data(), entries.size() * sizeof(float4), hipMemcpyHostToDevice);
    const MotionTable motion = {table, prim_count};
    for (int k = 0; k < (hist0 ? 8 : 4) && e == hipSuccess; ++k) e = hipMemcpy(buf + k * npix, in[k], bytes, hipMemcpyHostToDevice);
    float* var = reinterpret_cast<float*>(buf + 13 * npix);
    if (e == hipSuccess)
        e = moments_run(nullptr, *params, *variance, width, height, buf, buf + npix, *cur_cam, hist0 ? buf + 4 * npix : nullptr,
                        buf + 7 * npix, hist0 ? *prev_cam : *cur_cam, buf + 8 * npix, buf + 9 * npix, buf + 12 * npix, var,
                        nullptr, &motion);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    for (int k = 0; k < 5 && e == hipSuccess; ++k) e = hipMemcpy(out[k], buf + (8 + k) * npix, bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_variance, var, npix * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    (void)hipFree(table);
    if (e != hipSuccess) return refuse(PT_ERR_HIP, std::string("HIP error: ") + hipGetErrorString(e));
    return PT_OK;
}

PT_API int pt_denoise_variance_image(int device, uint32_t width, uint32_t height, const float* color, const float* plane0,
                                     const float* plane1, const float* plane2, const float* variance,
                                     const pt_vdenoise_params* params, float* out)
{
    auto refuse = [](int code, const std::string& msg) {
        g_freeError = "pt_denoise_variance_image: " + msg;
        return code;
    };
    if (const char* why = vdenoise_refusal(params)) return refuse(PT_ERR_ARG, why);
    if (!color || !plane0 || !plane1 || !plane2 || !variance || !out) return refuse(PT_ERR_ARG, "an array is null");
    if (width == 0 || height == 0 || (uint64_t)width * height >= (1ull << 30) || height > 8u * 0xffffu)
        return refuse(PT_ERR_ARG, "width x height must be 1 .. 2^30 - 1 pixels, height at most 524280");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return refuse(PT_ERR_NO_DEVICE, "no GPU visible");
    if (device < 0 || device >= n) return refuse(PT_ERR_ARG, "device out of range");
    const size_t npix = (size_t)width * height, bytes = npix * sizeof(float4);
    float4* buf = nullptr;                  // colour, 3 planes, g0, g1, ping, pong, out, the variance
    const float* in[4] = {color, plane0, plane1, plane2};
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc(&buf, 9 * bytes + npix * sizeof(float));
    for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipMemcpy(buf + k * npix, in[k], bytes, hipMemcpyHostToDevice);
    float* var = reinterpret_cast<float*>(buf + 9 * npix);
    if (e == hipSuccess) e = hipMemcpy(var, variance, npix * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = vdenoise_run(nullptr, *params, width, height, buf, buf + npix, var, buf + 4 * npix, buf + 5 * npix, buf + 6 * npix,
                         buf + 7 * npix, buf + 8 * npix, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, buf + 8 * npix, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    if (e != hipSuccess) return refuse(PT_ERR_HIP, std::string("HIP error: ") + hipGetErrorString(e));
    return PT_OK;
}

PT_API int pt_denoise_variance_feedback_image(int device, uint32_t width, uint32_t height, const float* color,
                                              const float* plane0, const float* plane1, const float* plane2,
                                              const float* variance, const float* hist0, const pt_vdenoise_params* params,
                                              const pt_vfeedback_params* feedback, float* out, float* out_hist0)
{
    auto refuse = [](int code, const std::string& msg) {
        g_freeError = "pt_denoise_variance_feedback_image: " + msg;
        return code;
    };
    if (const char* why = vdenoise_refusal(params)) return refuse(PT_ERR_ARG, why);
    if (const char* why = vfeedback_refusal(feedback, params->iterations)) return refuse(PT_ERR_ARG, why);
    if (!color || !plane0 || !plane1 || !plane2 || !variance || !out) return refuse(PT_ERR_ARG, "an array is null");
    if (!hist0 || !out_hist0) return refuse(PT_ERR_ARG, "hist0 or out_hist0 is null");
    if (width == 0 || height == 0 || (uint64_t)width * height >= (1ull << 30) || height > 8u * 0xffffu)
        return refuse(PT_ERR_ARG, "width x height must be 1 .. 2^30 - 1 pixels, height at most 524280");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return refuse(PT_ERR_NO_DEVICE, "no GPU visible");
    if (device < 0 || device >= n) return refuse(PT_ERR_ARG, "device out of range");
    const size_t npix = (size_t)width * height, bytes = npix * sizeof(float4);
    float4* buf = nullptr;                  // colour, 3 planes, g0, g1, ping, pong, out, hist0, the variance
    const float* in[4] = {color, plane0, plane1, plane2};
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc(&buf, 10 * bytes + npix * sizeof(float));
    for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipMemcpy(buf + k * npix, in[k], bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(buf + 9 * npix, hist0, bytes, hipMemcpyHostToDevice);
    float* var = reinterpret_cast<float*>(buf + 10 * npix);
    if (e == hipSuccess) e = hipMemcpy(var, variance, npix * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = vdenoise_run(nullptr, *params, width, height, buf, buf + npix, var, buf + 4 * npix, buf + 5 * npix, buf + 6 * npix,
                         buf + 7 * npix, buf + 8 * npix, nullptr, feedback->level, buf + 9 * npix, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, buf + 8 * npix, bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_hist0, buf + 9 * npix, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    if (e != hipSuccess) return refuse(PT_ERR_HIP, std::string("HIP error: ") + hipGetErrorString(e));
    return PT_OK;
}

} // extern "C"
