// Entry points of the guided upsampling onto supersampled planes (pt_upsample_resolve, pt_upsample_resolve_image); the
// kernel is in pt_dev_upsample_resolve.h.  Part of the trace kernel's single translation unit: included by
// pt_kernels.hip after pt_upsample.h; not a standalone header.
#pragma once

// The automatic choice (staging = 0) is rule 8's, the staged form: it measured faster in all four cases at 1920 x 1080
// from 960 x 540 (profiles/upsample_resolve_probe.json): 125.9 against 158.0 us (S = 2) and 298.4 against
// 426.5 us (S = 3) on cornell_box, 123.4 against 150.9 us and 281.3 against 391.6 us on generated_scene.
static bool upsample_resolve_stage_auto() { return upsample_stage_auto(); }

// Rule 9 on device buffers: color and loPlanes (3 planes) of w x h, ssPlanes of S W x S H, t = scratch of three planes
// of w x h, out of W x H, counts = two words.  ev (optional): 3 events, as upsample_run.
static hipError_t upsample_resolve_run(hipStream_t stream, const pt_upsample_params& p, uint32_t w, uint32_t h,
                                       const float4* color, const float4* loPlanes, uint32_t W, uint32_t H, uint32_t S,
                                       const float4* ssPlanes, float4* t, float4* out, uint32_t* counts, hipEvent_t* ev)
{
    const size_t nlo = (size_t)w * h, nss = (size_t)W * H * S * S;
    UpsampleResolveArgs R = {};
    UpsampleArgs& A = R.U;
    A.color = color;
    A.lo0 = loPlanes;
    A.lo1 = loPlanes + nlo;
    A.lo2 = loPlanes + 2 * nlo;
    A.t0 = t;
    A.t1 = t + nlo;
    A.t2 = t + 2 * nlo;
    A.hi0 = ssPlanes;
    A.hi1 = ssPlanes + nss;
    A.hi2 = ssPlanes + 2 * nss;
    A.out = nullptr;
    A.counts = counts;
    A.w = w;
    A.h = h;
    A.W = S * W;
    A.H = S * H;
    A.sigmaPlane = p.sigma_plane;
    A.normalPower = p.normal_power_log2;
    A.flags = p.flags;
    R.out = out;
    R.OW = W;
    R.OH = H;
    R.S = S;
    hipError_t e;
    if ((e = hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t), stream)) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[0], stream)) != hipSuccess) return e;
    upsample_prepare_kernel<<<(unsigned)((nlo + 255) / 256), 256, 0, stream>>>(A);     // rule 8's flat pass at the S-times size
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[1], stream)) != hipSuccess) return e;
    const dim3 grid((W + kDnTileW - 1) / kDnTileW, (H + kDnTileH - 1) / kDnTileH);
    if (p.staging == 1u || (p.staging == 0u && upsample_resolve_stage_auto()))
        upsample_resolve_kernel<true><<<grid, 256, (kUsCountF4 + 3 * kUsMaxRN) * sizeof(float4), stream>>>(R);
    else
        upsample_resolve_kernel<false><<<grid, 256, kUsCountF4 * sizeof(float4), stream>>>(R);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[2], stream)) != hipSuccess) return e;
    return hipSuccess;
}

// The S-times frame is within rule 8's sizes
static bool upsample_resolve_size_ok(uint32_t W, uint32_t H, uint32_t S)
{
    const uint64_t sw = (uint64_t)W * S, sh = (uint64_t)H * S;
    return sw <= 0xffffffffull && sh <= 0xffffffffull && upsample_size_ok((uint32_t)sw, (uint32_t)sh) && sw * sh < (1ull << 30);
}

extern "C" {

PT_API int pt_upsample_resolve(pt_context* hi, pt_context* planes, pt_context* lo, uint32_t source, uint32_t frames,
                               uint32_t factor, const pt_upsample_params* params)
{
    if (!hi) return PT_ERR_ARG;
    if (!planes) return fail(hi, PT_ERR_ARG, "pt_upsample_resolve: planes is null");
    if (!lo) return fail(hi, PT_ERR_ARG, "pt_upsample_resolve: lo is null");
    if (const char* why = upsample_refusal(params)) return fail(hi, PT_ERR_ARG, (std::string("pt_upsample_resolve: ") + why).c_str());
    if (source > PT_UPSAMPLE_DESPIKED)
        return fail(hi, PT_ERR_ARG, "pt_upsample_resolve: source must be PT_UPSAMPLE_ACCUM, _DENOISED, _TEMPORAL or _DESPIKED");
    if (hi->device != lo->device || hi->device != planes->device)
        return fail(hi, PT_ERR_ARG, "pt_upsample_resolve: the three contexts are on different devices");
    if (hi->rows != hi->height)
        return fail(hi, PT_ERR_ARG, "pt_upsample_resolve: hi holds a band partition, not the whole frame (use pt_upsample_resolve_image)");
    if (planes->rows != planes->height)
        return fail(hi, PT_ERR_ARG, "pt_upsample_resolve: planes holds a band partition, not the whole frame (use pt_upsample_resolve_image)");
    if (lo->rows != lo->height)
        return fail(hi, PT_ERR_ARG, "pt_upsample_resolve: lo holds a band partition, not the whole frame (use pt_upsample_resolve_image)");
    if (factor < 2u || factor > 4u) return fail(hi, PT_ERR_ARG, "pt_upsample_resolve: factor must be 2, 3 or 4");
    if ((uint64_t)hi->width * factor != planes->width || (uint64_t)hi->height * factor != planes->height)
        return fail(hi, PT_ERR_ARG, "pt_upsample_resolve: planes is not factor x hi (its width and height must be factor times hi's)");
    if (lo->width > hi->width || lo->height > hi->height)
        return fail(hi, PT_ERR_ARG, "pt_upsample_resolve: lo is larger than hi (lo's width and height must not exceed hi's)");
    if (!upsample_size_ok(lo->width, lo->height) || !upsample_resolve_size_ok(hi->width, hi->height, factor))
        return fail(hi, PT_ERR_ARG, "pt_upsample_resolve: width x height must be 1 .. 2^30 - 1 pixels, height at most 524280, for lo and for planes");
    if (!planes_current(planes->st))
        return fail(hi, PT_ERR_STATE, "pt_upsample_resolve: planes has no feature planes (no pt_render_features since the scene or a texture was set)");
    if (!planes_current(lo->st))
        return fail(hi, PT_ERR_STATE, "pt_upsample_resolve: lo has no feature planes (no pt_render_features since the scene or a texture was set)");
    if (source == PT_UPSAMPLE_DENOISED && !holds_denoised(lo->st))
        return fail(hi, PT_ERR_STATE, "pt_upsample_resolve: lo holds no denoised image (PT_UPSAMPLE_DENOISED)");
    if (source == PT_UPSAMPLE_TEMPORAL && !temporal_of_planes(lo->st))
        return fail(hi, PT_ERR_STATE, "pt_upsample_resolve: lo holds no temporal image of the planes it holds (PT_UPSAMPLE_TEMPORAL)");
    if (source == PT_UPSAMPLE_DESPIKED && !holds_despiked(lo->st))
        return fail(hi, PT_ERR_STATE, "pt_upsample_resolve: lo holds no despiked image (PT_UPSAMPLE_DESPIKED)");
    PT_HIP_CHECK(hi, hipSetDevice(hi->device));
    const size_t nlo = (size_t)lo->rows * lo->width, nhi = (size_t)hi->rows * hi->width;
    upsample_begins(hi->st);
    if (hi->usBuf && hi->usLoCap < nlo) {                 // a larger `lo` than the buffers were made for
        PT_HIP_CHECK(hi, hipStreamSynchronize(hi->stream));
        PT_HIP_CHECK(hi, hipFree(hi->usBuf));
        hi->usBuf = nullptr;
    }
    if (!hi->usBuf) {                                     // pt_upsample's layout, so either call serves the other's reads
        PT_HIP_CHECK(hi, hipMalloc(&hi->usBuf, (4 * nlo + nhi + 1) * sizeof(float4)));
        hi->usLoCap = nlo;
    }
    for (auto& e : hi->usEv)
        if (!e) PT_HIP_CHECK(hi, hipEventCreate(&e));
    PT_HIP_CHECK(hi, hipStreamSynchronize(lo->stream));       // lo's image and planes and the S-times planes are complete;
    PT_HIP_CHECK(hi, hipStreamSynchronize(planes->stream));   // the rest runs on hi's stream
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
    PT_HIP_CHECK(hi, upsample_resolve_run(hi->stream, *params, lo->width, lo->height, color, lo->feat, hi->width, hi->height,
                                          factor, planes->feat, hi->usBuf, upsample_image(hi), upsample_counts(hi), hi->usEv));
    PT_HIP_CHECK(hi, hipMemcpyAsync(hi->usCounts, upsample_counts(hi), 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, hi->stream));
    PT_HIP_CHECK(hi, hipStreamSynchronize(hi->stream));
    PT_HIP_CHECK(hi, hipEventElapsedTime(&hi->usMs[0], hi->usEv[0], hi->usEv[1]));
    PT_HIP_CHECK(hi, hipEventElapsedTime(&hi->usMs[1], hi->usEv[1], hi->usEv[2]));
    upsample_done(hi->st);
    return PT_OK;
}

PT_API int pt_upsample_resolve_image(int device, uint32_t lo_w, uint32_t lo_h, const float* color, const float* lo_plane0,
                                     const float* lo_plane1, const float* lo_plane2, uint32_t ss_w, uint32_t ss_h,
                                     const float* ss_plane0, const float* ss_plane1, const float* ss_plane2, uint32_t factor,
                                     const pt_upsample_params* params, float* out, uint32_t* out_counts)
{
    auto refuse = [](int code, const std::string& msg) {
        g_freeError = "pt_upsample_resolve_image: " + msg;
        return code;
    };
    if (const char* why = upsample_refusal(params)) return refuse(PT_ERR_ARG, why);
    if (!color || !lo_plane0 || !lo_plane1 || !lo_plane2 || !ss_plane0 || !ss_plane1 || !ss_plane2 || !out)
        return refuse(PT_ERR_ARG, "an array is null");
    if (factor < 2u || factor > 4u) return refuse(PT_ERR_ARG, "factor must be 2, 3 or 4");
    if (ss_w % factor != 0u || ss_h % factor != 0u) return refuse(PT_ERR_ARG, "factor does not divide ss_w and ss_h");
    if (!upsample_size_ok(lo_w, lo_h) || !upsample_size_ok(ss_w, ss_h))
        return refuse(PT_ERR_ARG, "width x height must be 1 .. 2^30 - 1 pixels, height at most 524280");
    const uint32_t W = ss_w / factor, H = ss_h / factor;
    if (lo_w > W || lo_h > H) return refuse(PT_ERR_ARG, "lo is larger than the output (lo_w <= ss_w / factor and lo_h <= ss_h / factor)");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return refuse(PT_ERR_NO_DEVICE, "no GPU visible");
    if (device < 0 || device >= n) return refuse(PT_ERR_ARG, "device out of range");
    const size_t nlo = (size_t)lo_w * lo_h, nss = (size_t)ss_w * ss_h, nout = (size_t)W * H;
    float4* buf = nullptr;                  // low: colour, 3 planes, 3 packed; S-times: 3 planes; out; then the counts
    float4* ssBuf = nullptr;
    const float* lows[4] = {color, lo_plane0, lo_plane1, lo_plane2};
    const float* highs[3] = {ss_plane0, ss_plane1, ss_plane2};
    uint32_t got[2] = {0, 0};
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc(&buf, (7 * nlo + 3 * nss + nout + 1) * sizeof(float4));
    if (e == hipSuccess) ssBuf = buf + 7 * nlo;
    for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipMemcpy(buf + k * nlo, lows[k], nlo * sizeof(float4), hipMemcpyHostToDevice);
    for (int k = 0; k < 3 && e == hipSuccess; ++k) e = hipMemcpy(ssBuf + k * nss, highs[k], nss * sizeof(float4), hipMemcpyHostToDevice);
    float4* const dOut = ssBuf + 3 * nss;
    uint32_t* counts = reinterpret_cast<uint32_t*>(dOut + nout);
    if (e == hipSuccess)
        e = upsample_resolve_run(nullptr, *params, lo_w, lo_h, buf, buf + nlo, W, H, factor, ssBuf, buf + 4 * nlo, dOut, counts, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dOut, nout * sizeof(float4), hipMemcpyDeviceToHost);
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
