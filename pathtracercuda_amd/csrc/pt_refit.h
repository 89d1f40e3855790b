// Entry points of moving primitives without a rebuild (pt_set_primitive_boxes, pt_holds_primitive_boxes,
// pt_move_primitives, pt_read_bvh, pt_read_primitive, pt_read_refit_timing); the kernels are in pt_dev_refit.h.  Part
// of the trace kernel's single translation unit: included by pt_kernels.hip after pt_upsample_resolve.h; not a
// standalone header.
#pragma once

// The component a box is refused for, or -1: 0..2 min, 3..5 max not finite, 6..8 min[k] > max[k].
static int box_refusal(const float* b)
{
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(b[k])) return k;
    for (int k = 0; k < 3; ++k)
        if (!(b[k] <= b[3 + k])) return 6 + k;
    return -1;
}

static std::string box_refusal_text(const char* call, uint32_t prim, int why)
{
    char buf[200];
    if (why < 6)
        snprintf(buf, sizeof(buf), "%s: primitive %u: box %s[%d] is not finite", call, prim, why < 3 ? "min" : "max", why % 3);
    else
        snprintf(buf, sizeof(buf), "%s: primitive %u: box min[%d] is above max[%d]", call, prim, why - 6, why - 6);
    return buf;
}

static const char* const kGrouped = "the context is part of a device group";

extern "C" {

PT_API int pt_set_primitive_boxes(pt_context* ctx, const float* boxes)
{
    if (!ctx) return PT_ERR_ARG;
    if (!boxes) return fail(ctx, PT_ERR_ARG, "pt_set_primitive_boxes: boxes is null");
    if (ctx->grouped) return fail(ctx, PT_ERR_STATE, (std::string("pt_set_primitive_boxes: ") + kGrouped).c_str());
    if (!ctx->nodes || ctx->primCount == 0) return fail(ctx, PT_ERR_STATE, "pt_set_primitive_boxes: no scene is set");
    const uint32_t np = ctx->primCount, nn = ctx->nodeCount;
    for (uint32_t i = 0; i < np; ++i) {
        const int why = box_refusal(boxes + 6 * (size_t)i);
        if (why >= 0) return fail(ctx, PT_ERR_ARG, box_refusal_text("pt_set_primitive_boxes", i, why).c_str());
    }
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    // the topology as pt_set_scene accepted it, from the device: only the words it validated are followed
    std::vector<float4> hn(2 * (size_t)nn);
    PT_HIP_CHECK(ctx, hipMemcpy(hn.data(), ctx->nodes, hn.size() * sizeof(float4), hipMemcpyDeviceToHost));
    auto offsetOf = [&](uint32_t i) { uint32_t u; memcpy(&u, &hn[2 * (size_t)i + 1].z, 4); return u; };
    auto countOf = [&](uint32_t i) { uint32_t u; memcpy(&u, &hn[2 * (size_t)i + 1].w, 4); return u >> 16; };
    // record numbers as set_scene_impl gives them: interior nodes in array order, reachable or not
    std::vector<uint32_t> rec(nn, 0xffffffffu);
    uint32_t interior = 0;
    for (uint32_t i = 0; i < nn; ++i)
        if (countOf(i) == 0) rec[i] = interior++;
    // the depth of every reachable node (the root's is 0; the largest, should two paths reach one node)
    std::vector<uint32_t> depth(nn, 0xffffffffu);
    std::vector<std::pair<uint32_t, uint32_t>> st(1, {0u, 0u});
    size_t visits = 0;
    uint32_t deepest = 0;
    bool any = false;
    while (!st.empty()) {
        const auto [i, d] = st.back();
        st.pop_back();
        if (i >= nn || ++visits > (size_t)nn || d > 32u)
            return fail(ctx, PT_ERR_STATE, "pt_set_primitive_boxes: the nodes on the device are not the tree pt_set_scene accepted");
        depth[i] = depth[i] == 0xffffffffu ? d : std::max(depth[i], d);
        if (countOf(i) != 0) {
            if ((uint64_t)offsetOf(i) + countOf(i) > np)
                return fail(ctx, PT_ERR_STATE, "pt_set_primitive_boxes: the nodes on the device are not the tree pt_set_scene accepted");
            continue;
        }
        if (i + 1 >= nn || offsetOf(i) >= nn)
            return fail(ctx, PT_ERR_STATE, "pt_set_primitive_boxes: the nodes on the device are not the tree pt_set_scene accepted");
        deepest = any ? std::max(deepest, d) : d;
        any = true;
        st.push_back({i + 1, d + 1});
        st.push_back({offsetOf(i), d + 1});
    }
    std::vector<uint32_t> lists;
    for (uint32_t i = 0; i < nn; ++i)
        if (depth[i] != 0xffffffffu && countOf(i) != 0) lists.push_back(i);
    const uint32_t leafCount = (uint32_t)lists.size();
    std::vector<uint32_t> levelOff(1, 0u);
    for (uint32_t d = 0; any && d <= deepest; ++d) {
        for (uint32_t i = 0; i < nn; ++i)
            if (depth[i] == d && countOf(i) == 0) {
                lists.push_back(i);
                lists.push_back(rec[i]);
            }
        levelOff.push_back((uint32_t)((lists.size() - leafCount) / 2));
    }
    std::vector<float4> hb(2 * (size_t)np);
    for (uint32_t i = 0; i < np; ++i) {
        const float* b = boxes + 6 * (size_t)i;
        hb[2 * (size_t)i] = make_float4(b[0], b[1], b[2], 0.0f);
        hb[2 * (size_t)i + 1] = make_float4(b[3], b[4], b[5], 0.0f);
    }
    (void)hipFree(ctx->rfBoxes);
    (void)hipFree(ctx->rfLists);
    ctx->rfBoxes = nullptr;
    ctx->rfLists = nullptr;
    // (the leaf list is padded to an even number of words, so the pairs after it are 8-byte aligned)
    const uint32_t pad = leafCount & 1u;
    if (pad) lists.insert(lists.begin() + leafCount, 0u);
    PT_HIP_CHECK(ctx, hipMalloc(&ctx->rfBoxes, hb.size() * sizeof(float4)));
    PT_HIP_CHECK(ctx, hipMalloc(&ctx->rfLists, lists.size() * sizeof(uint32_t)));
    PT_HIP_CHECK(ctx, hipMemcpy(ctx->rfBoxes, hb.data(), hb.size() * sizeof(float4), hipMemcpyHostToDevice));
    PT_HIP_CHECK(ctx, hipMemcpy(ctx->rfLists, lists.data(), lists.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    ctx->rfLeafCount = leafCount;
    ctx->rfLevelOff.swap(levelOff);
    boxes_set(ctx->st);
    return PT_OK;
}

PT_API int pt_holds_primitive_boxes(const pt_context* ctx) { return ctx && holds_boxes(ctx->st) ? 1 : 0; }

PT_API int pt_move_primitives(pt_context* ctx, uint32_t count, const uint32_t* index, const pt_hittable* prims,
                              const float* boxes, const float* motion_rows, const uint32_t* prev_index)
{
    if (!ctx) return PT_ERR_ARG;
    if (!index || !prims || !boxes) return fail(ctx, PT_ERR_ARG, "pt_move_primitives: index, prims or boxes is null");
    if ((motion_rows == nullptr) != (prev_index == nullptr))
        return fail(ctx, PT_ERR_ARG, "pt_move_primitives: motion_rows and prev_index are given together or not at all");
    if (count == 0) return fail(ctx, PT_ERR_ARG, "pt_move_primitives: count is 0");
    if (ctx->grouped) return fail(ctx, PT_ERR_STATE, (std::string("pt_move_primitives: ") + kGrouped).c_str());
    if (!holds_boxes(ctx->st))
        return fail(ctx, PT_ERR_STATE, "pt_move_primitives: no primitive boxes are held (no pt_set_primitive_boxes since the "
                                       "scene or a texture was set)");
    const uint32_t np = ctx->primCount;
    char buf[240];
    std::vector<uint32_t> sorted(index, index + count);
    std::sort(sorted.begin(), sorted.end());
    if (sorted.back() >= np) {
        snprintf(buf, sizeof(buf), "pt_move_primitives: index %u is not below the scene's %u primitives", sorted.back(), np);
        return fail(ctx, PT_ERR_ARG, buf);
    }
    for (uint32_t j = 1; j < count; ++j)
        if (sorted[j] == sorted[j - 1]) {
            snprintf(buf, sizeof(buf), "pt_move_primitives: index %u is given twice", sorted[j]);
            return fail(ctx, PT_ERR_ARG, buf);
        }
    for (uint32_t j = 0; j < count; ++j) {
        if (prims[j].type > 6u) {
            snprintf(buf, sizeof(buf), "pt_move_primitives: primitive %u: invalid hittable type", index[j]);
            return fail(ctx, PT_ERR_ARG, buf);
        }
        if (prims[j].texture_index > PT_MAX_TEXTURES) {
            snprintf(buf, sizeof(buf), "pt_move_primitives: primitive %u: invalid texture index", index[j]);
            return fail(ctx, PT_ERR_ARG, buf);
        }
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c)
                if (!std::isfinite(prims[j].inv_transform_rows[r][c])) {
                    snprintf(buf, sizeof(buf), "pt_move_primitives: primitive %u: inv_transform_rows[%d][%d] is not finite "
                             "(every value must be a finite float)", index[j], r, c);
                    return fail(ctx, PT_ERR_ARG, buf);
                }
        const int why = box_refusal(boxes + 6 * (size_t)j);
        if (why >= 0) return fail(ctx, PT_ERR_ARG, box_refusal_text("pt_move_primitives", index[j], why).c_str());
        if (prev_index && prev_index[j] != index[j] && prev_index[j] != 0xffffffffu) {
            snprintf(buf, sizeof(buf), "pt_move_primitives: primitive %u: prev_index %u is neither its own index nor 0xffffffff "
                     "(a move keeps every primitive's place)", index[j], prev_index[j]);
            return fail(ctx, PT_ERR_ARG, buf);
        }
    }
    // ---- accepted: pack, one copy, the kernels ----
    const auto packBegan = std::chrono::steady_clock::now();
    std::vector<float4>& hp = ctx->rfHost;
    hp.assign((size_t)kMoveQuads * count, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (uint32_t j = 0; j < count; ++j) {
        float4* q = &hp[(size_t)kMoveQuads * j];
        pack_primitive(ctx, prims[j], q, q + 4);
        const float* b = boxes + 6 * (size_t)j;
        q[7] = make_float4(b[0], b[1], b[2], u2f(index[j]));
        q[8] = make_float4(b[3], b[4], b[5], 0.0f);
        if (motion_rows) {
            const float* r = motion_rows + 12 * (size_t)j;
            for (int k = 0; k < 3; ++k) q[9 + k] = make_float4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
            q[12] = make_float4(u2f(prev_index[j]), 0.0f, 0.0f, 0.0f);
        }
    }
    ctx->rfPackMs = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - packBegan).count();
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (ctx->rfPackCap < count) {
        PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        (void)hipFree(ctx->rfPack);
        ctx->rfPack = nullptr;
        ctx->rfPackCap = 0;
        PT_HIP_CHECK(ctx, hipMalloc(&ctx->rfPack, (size_t)kMoveQuads * count * sizeof(float4)));
        ctx->rfPackCap = count;
    }
    if (motion_rows && ctx->motionCount != np) {
        PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        (void)hipFree(ctx->motion);
        ctx->motion = nullptr;
        ctx->motionCount = 0;
        PT_HIP_CHECK(ctx, hipMalloc(&ctx->motion, 4 * (size_t)np * sizeof(float4)));
        ctx->motionCount = np;
    }
    for (auto& e : ctx->rfEv)
        if (!e) PT_HIP_CHECK(ctx, hipEventCreate(&e));
    // from here on the scene's words change: whatever fails below, the history must not outlive it
    primitives_moved(ctx->st, motion_rows != nullptr);
    hipStream_t s = ctx->stream;
    hipError_t e = hipEventRecord(ctx->rfEv[2], s);
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->rfPack, hp.data(), hp.size() * sizeof(float4), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipEventRecord(ctx->rfEv[0], s);
    if (e == hipSuccess && motion_rows) {
        motion_fill_kernel<<<(np + 255) / 256, 256, 0, s>>>(ctx->motion, np);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        move_scatter_kernel<<<(count + 255) / 256, 256, 0, s>>>(ctx->rfPack, count, ctx->prims, ctx->mats, ctx->rfBoxes,
                                                                motion_rows ? ctx->motion : nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        refit_leaves_kernel<<<(ctx->rfLeafCount + 255) / 256, 256, 0, s>>>(ctx->rfLists, ctx->rfLeafCount, ctx->rfBoxes, ctx->nodes);
        e = hipGetLastError();
    }
    const uint2* levels = reinterpret_cast<const uint2*>(ctx->rfLists + ((ctx->rfLeafCount + 1u) & ~1u));
    for (size_t d = ctx->rfLevelOff.size() - 1; e == hipSuccess && d-- > 0;) {      // the deepest depth first, the root last
        const uint32_t n = ctx->rfLevelOff[d + 1] - ctx->rfLevelOff[d];
        if (n == 0) continue;
        refit_level_kernel<<<(n + 255) / 256, 256, 0, s>>>(levels + ctx->rfLevelOff[d], n, ctx->nodes, ctx->cnodes);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(ctx->rfEv[1], s);
    float4 root[2];
    if (e == hipSuccess) e = hipMemcpyAsync(root, ctx->nodes, sizeof(root), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipEventElapsedTime(&ctx->rfMs, ctx->rfEv[0], ctx->rfEv[1]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ctx->rfCopyMs, ctx->rfEv[2], ctx->rfEv[0]);
    if (e != hipSuccess) {
        if (motion_rows) scene_or_texture_changed(ctx->st);        // (as a failed table upload in pt_set_scene_moved)
        PT_HIP_CHECK(ctx, e);
    }
    // the trace kernel takes the root's box by value.  slabFast stays what pt_set_scene found: a caller tree that had an
    // unordered reachable box keeps the exact slab test although the refit has ordered every reachable box (the two
    // tests give the same words on ordered boxes; a fresh pt_set_scene of the same words would take the fast one)
    ctx->rootBox[0] = root[0].x;
    ctx->rootBox[1] = root[0].y;
    ctx->rootBox[2] = root[0].z;
    ctx->rootBox[3] = root[0].w;
    ctx->rootBox[4] = root[1].x;
    ctx->rootBox[5] = root[1].y;
    ctx->rfRan = true;
    return PT_OK;
}

PT_API int pt_read_bvh(pt_context* ctx, pt_bvh_node* nodes, float* records)
{
    if (!ctx || !nodes) return PT_ERR_ARG;
    if (!ctx->nodes) return fail(ctx, PT_ERR_STATE, "pt_read_bvh: no scene is set");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<float4> hn(2 * (size_t)ctx->nodeCount);
    PT_HIP_CHECK(ctx, hipMemcpy(hn.data(), ctx->nodes, hn.size() * sizeof(float4), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < ctx->nodeCount; ++i) {
        const float4 a = hn[2 * (size_t)i], b = hn[2 * (size_t)i + 1];
        pt_bvh_node& n = nodes[i];
        n.aabb_min[0] = a.x;
        n.aabb_max[0] = a.y;
        n.aabb_min[1] = a.z;
        n.aabb_max[1] = a.w;
        n.aabb_min[2] = b.x;
        n.aabb_max[2] = b.y;
        memcpy(&n.offset, &b.z, 4);
        memcpy(&n.primitive_count_axis, &b.w, 4);
    }
    if (records && ctx->cnodes)
        PT_HIP_CHECK(ctx, hipMemcpy(records, ctx->cnodes, 4 * (size_t)std::max(ctx->cnodeCount, 1u) * sizeof(float4),
                                    hipMemcpyDeviceToHost));
    return PT_OK;
}

PT_API int pt_read_primitive(pt_context* ctx, uint32_t index, float* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!ctx->prims) return fail(ctx, PT_ERR_STATE, "pt_read_primitive: no scene is set");
    if (index >= ctx->primCount) return fail(ctx, PT_ERR_ARG, "pt_read_primitive: index is not below the scene's primitive count");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    PT_HIP_CHECK(ctx, hipMemcpy(dst, ctx->prims + 4 * (size_t)index, 4 * sizeof(float4), hipMemcpyDeviceToHost));
    PT_HIP_CHECK(ctx, hipMemcpy(dst + 16, ctx->mats + 3 * (size_t)index, 3 * sizeof(float4), hipMemcpyDeviceToHost));
    return PT_OK;
}

PT_API int pt_read_refit_timing(pt_context* ctx, float* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!ctx->rfRan) return fail(ctx, PT_ERR_STATE, "pt_read_refit_timing: no pt_move_primitives has run on this context");
    dst[0] = ctx->rfMs;
    dst[1] = ctx->rfPackMs;
    dst[2] = ctx->rfCopyMs;
    return PT_OK;
}

} // extern "C"
