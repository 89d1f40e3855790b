// pt_builds.h -- the builds of trace_kernel as one table, and the LDS a workgroup of one needs.
// Plain C++17, no HIP: pt_kernels.hip instantiates its kernels from the table (launch_build), the
// launch policy (pt_launch_plan.h) and tools/launch_plan_check.cpp read it on the host.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace pt {

// A launch mode is a (STATS, MODE) pair of trace_kernel's template parameters (MODE: trace_kernel's
// comment); the instrumented kernel exists for MODE 0 only and has a bit of its own.
constexpr int kModePlain = 0, kModeGrouped = 1, kModeAux = 2, kModeStrip = 3, kModeAhead = 4, kModeAdaptive = 5;
constexpr uint32_t kInstrumented = 1u << 6;
constexpr uint32_t mode_bit(bool stats, int mode) { return stats ? (mode == kModePlain ? kInstrumented : 0u) : 1u << mode; }

// The WW parameter of the resumable walk encodes 100000 * NOREPAIR + 10000 * SKYQ + 1000 * DEFERQ + 200 + EXITQ
// (deferred shading and the traversal's exit threshold, see trace_kernel); 0 and 1 are the
// node-at-a-time walks, 3 the one-loop child-box walk.
constexpr int kWalk40 = 14212;      // SKYQ 1, DEFERQ 4, exit <= 12/64 (retuned in round 3, profiles/r03_walk_params_ab.json)
constexpr int kWalk39 = 224;        // no deferred shading, exit <= 24/64
constexpr int kWalk48 = 13216;      // SKYQ 1, DEFERQ 3, exit <= 16/64
constexpr int kWalkNoRepair = 100000;

struct Build {
    int id;             // pt_set_kernel_variant / pt_last_variant
    int SL;             // staged in LDS: 0 nothing, 1 child-box records (or nodes), 2 primitives too
    int WPB;            // waves per workgroup
    int WW;             // walk word
    int MINW;           // waves per SIMD the build is compiled for
    bool PERSIST;       // waves take their tiles from a cursor
    uint32_t modes;     // launch modes the build is instantiated for (mode_bit)
    bool settable;      // pt_set_kernel_variant accepts it
};

constexpr uint32_t kOnlyPlain = mode_bit(false, kModePlain);
constexpr uint32_t kPlain = kOnlyPlain | kInstrumented;
constexpr uint32_t kResumable = kPlain | mode_bit(false, kModeGrouped) | mode_bit(false, kModeAux) |
                                mode_bit(false, kModeStrip) | mode_bit(false, kModeAhead) | mode_bit(false, kModeAdaptive);

// Every build gives the same bits.  Measured-and-rejected builds of earlier rounds (single loop with
// LDS nodes, other exit thresholds, 2/8/16-wave groups, 6-8 waves/SIMD, speculative traversal,
// select-form primitive tests, a ballot-driven phase scheduler) are recorded in DESIGN.md and git
// history, not shipped; so are 50/51 (leaf tests compacted across a round's lanes by shape family,
// -14.6 % on C3: measured in round 3, removed in round 4; commit 1b0d322 has them).
constexpr Build kBuilds[] = {
    // reference control flow (one loop, node at a time), scene read through the caches
    {1, 0, 4, 0, 1, false, kPlain, true},
    // node-at-a-time while-while, caches, 5 waves/SIMD (scenes outside the child-box encoding); adaptive
    // launches too, as the automatic choice can be this build
    {4, 0, 4, 1, 5, false, kPlain | mode_bit(false, kModeAdaptive), true},
    // the same with the nodes in LDS (small BVH)
    {6, 1, 4, 1, 5, false, kPlain | mode_bit(false, kModeAdaptive), true},
    // child-box traversal, one tile per wave (counts the reference's node/prim tests)
    {20, 0, 4, 3, 5, false, kPlain, true},
    // 40 without deferred shading, exit <= 24/64 (the round-1 default; A/B reference); grouped launches
    // and their resume / pre-pass launches too
    {39, 1, 4, kWalk39, 5, true, kPlain | mode_bit(false, kModeGrouped) | mode_bit(false, kModeAux), true},
    // default: resumable lean child-box walk, records in LDS, persistent waves, deferred shading
    // (hits >= 4/8, misses >= 1/8 with a sky texture), exit <= 12/64
    {40, 1, 4, kWalk40, 5, true, kResumable, true},
    // default for cache-read scenes: same, records through the caches
    {41, 0, 4, kWalk40, 5, true, kResumable, true},
    // default for deep cache-read BVHs: 41 compiled for 4 waves/SIMD (128 VGPRs)
    {46, 0, 4, kWalk40, 4, true, kResumable, true},
    // small grids (<= 4 tiles per SIMD): 39 compiled for 4 waves/SIMD (128 VGPRs); no deferral, which
    // costs a single pass of latency-bound waves 2.8 %
    {47, 1, 4, kWalk39, 4, true, kPlain, true},
    // small grids whose primitives fit in LDS too: records and primitives in LDS, 4 waves/SIMD, deferred hits
    {48, 2, 4, kWalk48, 4, true, kPlain, true},
    // 40 and 41 compiled for six waves per SIMD (80 VGPRs): 60 as 8-wave workgroups, the records staged
    // once per eight waves.  Their instrumented builds are the six-wave kernels themselves,
    // so the counters of an instrumented launch (lane utilisation, repairs) come from the kernel that is timed
    {60, 1, 8, kWalk40, 6, true, kResumable, true},
    {61, 0, 4, kWalk40, 6, true, kResumable, true},
    // test only (pt_set_rise_repair): 40 without the rising-t_max rebuild
    {90, 1, 4, kWalkNoRepair + kWalk40, 5, true, kOnlyPlain, false},
    // A/B of the rebuild's cost only, not the reference's bits: 48 without it
    {91, 2, 4, kWalkNoRepair + kWalk48, 4, true, kOnlyPlain, true},
};
constexpr size_t kBuildCount = sizeof(kBuilds) / sizeof(kBuilds[0]);

constexpr const Build* find_build(int id)
{
    for (size_t i = 0; i < kBuildCount; ++i)
        if (kBuilds[i].id == id) return &kBuilds[i];
    return nullptr;
}

constexpr bool build_has(int id, uint32_t modeBit)
{
    const Build* b = find_build(id);
    return b && (b->modes & modeBit) != 0;
}

constexpr bool build_settable(int id)
{
    const Build* b = find_build(id);
    return b && b->settable;
}

constexpr bool walks_child_boxes(const Build& b) { return b.WW >= 3; }

// Waves per SIMD a build is compiled for (its wave slots: CUs x 4 SIMDs x this).
constexpr uint32_t build_waves(int id)
{
    const Build* b = find_build(id);
    return b ? (uint32_t)b->MINW : 0u;
}

// The five-wave build of the same walk (60 -> 40, 61 -> 41; any other build is its own).
constexpr int five_wave_build(int id) { return id == 60 ? 40 : id == 61 ? 41 : id; }

constexpr size_t kLdsLimit = 160 * 1024;    // dynamic LDS a workgroup may ask for (a CU's whole LDS)
constexpr size_t kStageLimit = 48 * 1024;   // records (or nodes) are staged by default up to this size

// What the LDS layout of trace_kernel depends on.
struct SceneSize {
    uint32_t nodes, records, prims;     // BVH nodes, child-box records (interior nodes), primitives
    uint32_t stackRows;
};

// Bytes of the scene staged at level SL: child-box records are 64 B, nodes 32 B, primitives 64 B.
constexpr size_t staged_bytes(int SL, bool childBox, const SceneSize& s)
{
    const size_t nodeF4 = childBox ? 4 * (size_t)s.records : 2 * (size_t)s.nodes;
    return ((SL >= 1 ? nodeF4 : 0) + (SL >= 2 ? 4 * (size_t)s.prims : 0)) * 16;
}

// Dynamic LDS of a workgroup (layout: wave_lds): the staged scene, then per wave stackRows x 64 stack
// entries (8 B in the child-box walks, which keep the entry distance, 4 B otherwise) and a 768 B
// accumulation slice.
constexpr size_t lds_bytes(int SL, int WPB, bool childBox, const SceneSize& s)
{
    return staged_bytes(SL, childBox, s) + (size_t)WPB * ((size_t)s.stackRows * 64 * (childBox ? 8 : 4) + 64 * 12);
}

} // namespace pt
