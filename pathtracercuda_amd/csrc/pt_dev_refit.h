// Moving primitives and refitting the BVH on the device (pt_move_primitives; rule 10 of include/pt_hip.h, restated
// in tests/refit_model.py).
// Part of the trace kernel's single translation unit: included by pt_kernels.hip inside its anonymous
// namespace after pt_dev_upsample_resolve.h; not a standalone header.
// Nothing here is used by an existing kernel, and no existing kernel or parameter struct changes.
// The kernels hand nothing to one another inside a launch: the leaves are one launch, every depth of interior nodes
// is one launch, deepest first, and the boundary between two launches is what makes a child's box visible to its
// parent (a parent may run on another XCD than its children, and the per-XCD L2s are not coherent).  No flags, no
// counters, no waiting.  Every store is a whole float4.
#pragma once

// What the host packs per moved primitive, in float4: the four primitive quads, the three material quads, the box
// (min xyz with the primitive's index as bits in w, then max xyz), the four quads of rule 7's table entry.
constexpr uint32_t kMoveQuads = 13;

// ---------------------------------------------------------------------------------------------
// Rule 7's table for primitives that did not move: the identity and their own index.  Flat, one primitive per lane.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) motion_fill_kernel(float4* __restrict__ motion, uint32_t primCount)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= primCount) return;
    float4* e = motion + 4 * (size_t)i;
    e[0] = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
    e[1] = make_float4(0.0f, 1.0f, 0.0f, 0.0f);
    e[2] = make_float4(0.0f, 0.0f, 1.0f, 0.0f);
    e[3] = make_float4(__uint_as_float(i), 0.0f, 0.0f, 0.0f);
}

// ---------------------------------------------------------------------------------------------
// The packed records into their places.  One moved primitive per lane; the host has checked that every index is
// below the primitive count and that no two are equal.  motion is null when the move makes no table.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) move_scatter_kernel(const float4* __restrict__ pack, uint32_t count,
                                                           float4* __restrict__ prims, float4* __restrict__ mats,
                                                           float4* __restrict__ boxes, float4* __restrict__ motion)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const float4* q = pack + (size_t)kMoveQuads * j;
    const float4 lo = q[7], hi = q[8];
    const size_t i = __float_as_uint(lo.w);
    for (int k = 0; k < 4; ++k) prims[4 * i + k] = q[k];
    for (int k = 0; k < 3; ++k) mats[3 * i + k] = q[4 + k];
    boxes[2 * i] = make_float4(lo.x, lo.y, lo.z, 0.0f);
    boxes[2 * i + 1] = make_float4(hi.x, hi.y, hi.z, 0.0f);
    if (motion)
        for (int k = 0; k < 4; ++k) motion[4 * i + k] = q[9 + k];
}

// ---------------------------------------------------------------------------------------------
// Rule 10, leaves: the fold of the leaf's primitive boxes in index order.  Flat over the list of reachable leaves
// (node indices; the host made it from the topology pt_set_scene validated, so every index and every primitive range
// is inside its array).  The node's second quad keeps offset and primitive_count_axis.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) refit_leaves_kernel(const uint32_t* __restrict__ leaves, uint32_t count,
                                                           const float4* __restrict__ boxes, float4* __restrict__ nodes)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const size_t i = leaves[j];
    const float4 n1 = nodes[2 * i + 1];
    const size_t f = __float_as_uint(n1.z);
    const uint32_t c = __float_as_uint(n1.w) >> 16;
    float4 lo = boxes[2 * f], hi = boxes[2 * f + 1];
    for (uint32_t k = 1; k < c; ++k) {
        const float4 l = boxes[2 * (f + k)], h = boxes[2 * (f + k) + 1];
        lo.x = l.x < lo.x ? l.x : lo.x;
        lo.y = l.y < lo.y ? l.y : lo.y;
        lo.z = l.z < lo.z ? l.z : lo.z;
        hi.x = h.x > hi.x ? h.x : hi.x;
        hi.y = h.y > hi.y ? h.y : hi.y;
        hi.z = h.z > hi.z ? h.z : hi.z;
    }
    nodes[2 * i] = make_float4(lo.x, hi.x, lo.y, hi.y);
    nodes[2 * i + 1] = make_float4(lo.z, hi.z, n1.z, n1.w);
}

// ---------------------------------------------------------------------------------------------
// Rule 10, one depth of interior nodes, whose children an earlier launch has finished.  Flat over that depth's list
// of (node index, record index).  A node quad is (min.x, max.x, min.y, max.y), (min.z, max.z, offset, count_axis);
// the record's quads 0-2 are set_scene_impl's: the first child's x and y, both children's z, the second child's x
// and y.  Quad 3 is not written.  cnodes is null when the scene has no child-box records.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) refit_level_kernel(const uint2* __restrict__ level, uint32_t count,
                                                          float4* __restrict__ nodes, float4* __restrict__ cnodes)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const uint2 e = level[j];
    const size_t i = e.x;
    const float4 n1 = nodes[2 * i + 1];
    const size_t a = i + 1, b = __float_as_uint(n1.z);
    const float4 a0 = nodes[2 * a], a1 = nodes[2 * a + 1], b0 = nodes[2 * b], b1 = nodes[2 * b + 1];
    float4 o0, o1;
    o0.x = b0.x < a0.x ? b0.x : a0.x;
    o0.y = b0.y > a0.y ? b0.y : a0.y;
    o0.z = b0.z < a0.z ? b0.z : a0.z;
    o0.w = b0.w > a0.w ? b0.w : a0.w;
    o1.x = b1.x < a1.x ? b1.x : a1.x;
    o1.y = b1.y > a1.y ? b1.y : a1.y;
    o1.z = n1.z;
    o1.w = n1.w;
    nodes[2 * i] = o0;
    nodes[2 * i + 1] = o1;
    if (cnodes) {
        float4* q = cnodes + 4 * (size_t)e.y;
        q[0] = a0;
        q[1] = make_float4(a1.x, a1.y, b1.x, b1.y);
        q[2] = b0;
    }
}
