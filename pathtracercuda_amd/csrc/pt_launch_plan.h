// pt_launch_plan.h -- what a render launch runs, decided from plain values: no HIP call, no context,
// no side effect.  render_impl (pt_kernels.hip) fills LaunchInputs, calls plan_launch and executes the
// plan; tools/launch_plan_check.cpp and tests/test_launch_plan.py run the same function on the CPU.
#pragma once
#include <algorithm>

#include "pt_builds.h"

namespace pt {

struct SceneFacts {
    SceneSize size;
    bool hasRecords;        // the scene has the child-box layout (leaf counts < 256)
    bool dfsOrder;          // leaves hold their primitives in DFS order (repair_pending)
};

// The knobs of pt_set_*, as a context holds them (0 is the default of each mode).
struct LaunchKnobs {
    int variant = 0;                    // 0 = automatic
    int schedule = 0;                   // 0 = cost-sorted tiles, 1 = row-major, 2 = scattered
    int stripMode = 0;                  // strip units: 0 automatic, 1 off, K >= 2 always K tiles per unit
    int ssgMode = 0;                    // sample groups: 0 automatic, 1 off, G >= 2 always G groups (tests)
    int aheadMode = 0;                  // run-ahead: 0 automatic, 1 off, 2 always make a stash, 3 make but never use
    int prioMode = 0;                   // issue priority: 0 automatic, 1 off, 2 explicit bounds prioBounds
    uint32_t prioBounds[3] = {0, 0, 0};
    uint32_t prepassSpp = 0;            // pt_set_cold_start: 0 = first call split off (pre-pass of kPrepassSpp for
                                        // one-call launches), > 0 = a discarded pre-pass of that many spp
    bool coldPriority = true;           // pt_set_cold_start: issue priority on the cold start's order
    bool riseRepair = true;             // pt_set_rise_repair (tests' negative control only)
};

// The cost order of a context.
struct OrderState {
    bool valid = false;                 // `order` holds a cost-sorted permutation
    bool stale = true;                  // rebuild it after the next launch (scene, texture or camera changed)
    uint64_t samples = 0;               // samples per pixel of the launch whose tile costs built it
    uint32_t strip = 1;                 // tiles per unit of that launch
};

struct LaunchInputs {
    uint32_t cus;                       // compute units of the device
    uint32_t tilesX, tilesY;
    uint32_t spp, chunks;
    bool instrumented;
    SceneFacts scene;
    LaunchKnobs knobs;
    OrderState order;                   // when the launch is decided
    bool stashMatches;                  // the previous launch made a run-ahead stash under this camera and state
    uint32_t aheadMisses;               // consecutive launches whose camera or state had changed
};

enum class LaunchMode { Plain, Instrumented, Strip, Ahead, Grouped };
enum class ColdStart { None, SplitCall, Prepass };

// Issue priority of a pass: order-position bounds of levels 3, 2, 1 (the rest run at 0), and whether
// every position dealt at the start runs in the first band (launch_one).
struct PassPriority {
    uint32_t prio[3];
    bool dealt;
};

struct LaunchPlan {
    const char* refusal;                // the launch is refused with this message (nothing else is valid then
                                        // but K, units and dropOrder)
    int build;                          // the build every pass of the launch runs
    LaunchMode mode;                    // of the main pass
    uint32_t K, units;                  // tiles per dispatch unit, units
    uint32_t G, ssgCap;                 // sample groups (0 = none) and an item's log capacity in samples
    bool aheadUse, aheadMake;
    bool dropOrder;                     // K differs from the order's: the order is void and stale
    bool costOrder;                     // the main pass runs in cost order (else row-major over units)
    ColdStart cold;
    uint32_t coldSpp;                   // samples per pixel of the cold-start pass
    bool coldPairs;                     // the pre-pass also measures draw pairs per sample
    PassPriority coldPrio, mainPrio;
    bool rebuildOrder;                  // sort the order from the main pass's tile costs
    bool biasedOrder;                   // those costs were measured under priority: rebuild once more
};

// Tiles per dispatch unit.  A launch of few samples per pixel idles the lanes whose pixels finish
// first for the rest of their tile; strips of K tiles let those lanes go on with the next tile.
// Measured at 1080p (tools/call_loop.py, profiles/r04_call_loop.json): 1-spp progressive frames
// 0.673 -> 0.646 ms (K = 2) -> 0.592 ms (K = 4); the reference's 8-spp calls 316 -> 320 ms (K = 2)
// -> 466 ms (K = 4) per 128 calls -- units of several tiles are too few to balance the launch's tail
// there.  Automatic: K = 4 for launches of at most 2 samples per pixel with at least ~6 tiles per
// wave slot; the build must be a strip-capable one.
constexpr uint64_t kStripMaxSamples = 2;
// Run-ahead (MODE 4): launches of kAheadMinSamples..kAheadMaxSamples samples per pixel make a stash
// of the next call's first samples (the reference's render(cam, 8, ...) calls, main.cpp:272-279);
// 1-2 spp progressive frames use strip units instead.
constexpr uint64_t kAheadMinSamples = 3, kAheadMaxSamples = 64;
// Cost pre-pass of a cold-start launch: samples per pixel, and the smallest launch (spp x chunks)
// that gets one.
constexpr uint32_t kPrepassSpp = 2;
constexpr uint64_t kPrepassMinSpp = 16;

// The build a launch starts from: the forced one, or the automatic choice for the scene.
inline int picked_build(int variant, const SceneFacts& sc)
{
    // (a BVH whose leaves are not in DFS primitive order cannot be descended by repair_pending, and a
    // child-box walk needs the child-box layout: without them the node-at-a-time walks run, which push
    // every far child as the reference does -- so grouped and strip launches, which exist only for the
    // child-box walks, are never chosen for such scenes)
    const int nodeWalk = staged_bytes(1, false, sc.size) <= kStageLimit ? 6 : 4;
    if (variant > 0) {
        const Build* b = find_build(variant);
        return (b && walks_child_boxes(*b) && (!sc.dfsOrder || !sc.hasRecords)) ? nodeWalk : variant;
    }
    // measured on MI355X (tools/ab_variants.py, profiles/): child-box traversal (one dependent
    // fetch per interior visit, leaves inline) with while-while leaf batching and 5 waves/SIMD
    // wins on every scene; the child-box records are staged in LDS when they fit in 48 KB
    // (cornell, the 484-object scene) and read through the caches otherwise (100k objects).
    // Scenes outside the child-box encoding fall back to the node-at-a-time walk (launch_one).
    // The resumable form wins everywhere (the wave shades its finished lanes once at most 12/64
    // still walk), and so do persistent waves pulling tiles from a cursor (variants 30/34: +6% on
    // the 484-object scene, +11% on 100k objects over the one-tile-per-wave grid, variants 28/26).
    // A cache-read scene whose four LDS stacks per workgroup leave room for fewer than five
    // workgroups per CU (BVH depth > 16) runs at 4 waves/SIMD anyway: variant 46 is variant 41
    // compiled for that occupancy (128 VGPRs, no spill), +1% on the 100k-object scene (depth 19).
    // Six waves per SIMD (variants 60 / 61: the same walks compiled for 80 VGPRs) when the LDS holds
    // them: with the records in LDS as three 8-wave workgroups per CU (the records staged once per
    // eight waves), with cache-read records as six 4-wave workgroups.  Measured on C3
    // (profiles/r05_six_waves.json): 60 224.2 ms against 40 231.2; 61 237.5 against 41 245.7.
    if (!sc.hasRecords || !sc.dfsOrder) return nodeWalk;
    const bool stages = staged_bytes(1, true, sc.size) <= kStageLimit;
    if (stages && 3 * lds_bytes(1, 8, true, sc.size) <= kLdsLimit) return 60;
    if (stages && 5 * lds_bytes(1, 4, true, sc.size) <= kLdsLimit) return 40;
    if (6 * lds_bytes(0, 4, true, sc.size) <= kLdsLimit) return 61;
    return stages ? 40 : (5 * lds_bytes(0, 4, true, sc.size) > kLdsLimit ? 46 : 41);
}

// `build` is the picked one (which already replaces a forced child-box build by a node-at-a-time one
// on scenes without the child-box layout or DFS leaf order).
inline uint32_t strip_tiles(const LaunchInputs& in, int build, uint32_t tiles, uint64_t samples)
{
    if (in.knobs.stripMode == 1 || !build_has(build, mode_bit(false, kModeStrip)) || !in.scene.hasRecords) return 1;
    if (in.knobs.stripMode >= 2) return (uint32_t)in.knobs.stripMode;
    if (samples > kStripMaxSamples) return 1;
    const uint64_t slots = (uint64_t)in.cus * 4 * 5;    // (the threshold was measured at five waves)
    return (uint64_t)tiles >= 6 * slots ? 4u : 1u;
}

// Speculative sample groups: how many groups a launch uses (0 = a plain launch).  A launch of
// `tiles` 8x8 tiles on a chip with `resident` wave slots is grouped when six work items per slot
// would take at least 4 groups (under ~1.5 tiles per slot; with more, the cost-sorted list schedule
// balances well enough), and then gets 3.5 items per slot, at least 4 groups, at most 8, each at
// least 64 samples long.  Measured at six waves per SIMD (profiles/r05_six_waves.json, C3 rank-0
// shares): N = 4 G = 4 / 5 / 6 / 8 78.4 / 79.5 / 80.6 / 83.7 ms; N = 8 G = 4 / 5 / 6 / 8 46.8 / 44.5 /
// 44.5 / 46.0 ms (the six-items rule gave 5 and 8).
inline uint32_t ssg_groups(const LaunchInputs& in, int build, uint32_t tiles, uint32_t total)
{
    if (in.knobs.ssgMode == 1 || !build_has(build, mode_bit(false, kModeGrouped))) return 0;
    if (in.knobs.ssgMode >= 2) return std::min<uint32_t>((uint32_t)in.knobs.ssgMode, std::max(total, 1u));
    const uint64_t resident = (uint64_t)in.cus * 4 * build_waves(build);
    // measured (tools/ssg_probe.py): with 2 or 3 groups the logging, the fold and the
    // extra samples cost more than the shorter tail returns; from 4 groups on the tail wins
    if ((6 * resident + tiles - 1) / tiles < 4) return 0;
    uint64_t g = std::max<uint64_t>(4, (7 * resident + 2 * (uint64_t)tiles - 1) / (2 * (uint64_t)tiles));
    g = std::min<uint64_t>({g, 8, total / 64});
    return g >= 4 ? (uint32_t)g : 0;
}

// A plain launch with at most four tiles per SIMD runs every tile in one pass at four waves per
// SIMD, so the fifth wave slot the default kernels are compiled for (96 VGPRs, with spills) buys
// nothing: the same walk compiled for four waves (128 VGPRs, no spill) shortens every wave's chain,
// and when the primitives fit in LDS next to the child-box records, four workgroups per CU still
// fit and leaf tests read LDS instead of L1/L2.  Measured (tools/ab_variants.py, MI355X): cornell
// 512x512x64 +5.5 % (48), one rank's share of 1080p x 1024 at N = 8 +4 % (47).
inline int small_grid_build(const LaunchInputs& in, int build, uint32_t tiles)
{
    if ((uint64_t)tiles > (uint64_t)in.cus * 4 * 4) return build;
    if (five_wave_build(build) == 41) return 46;
    if (five_wave_build(build) != 40) return build;
    return 4 * lds_bytes(2, 4, true, in.scene.size) <= kLdsLimit ? 48 : 47;
}

// Issue priority of a pass over `units` order positions (pt_set_issue_priority).
inline PassPriority issue_priority(const LaunchInputs& in, uint32_t units)
{
    if (in.knobs.prioMode == 2) return {{in.knobs.prioBounds[0], in.knobs.prioBounds[1], in.knobs.prioBounds[2]}, false};
    if (in.knobs.prioMode == 1) return {};
    // automatic: graded by quarter of the order -- the most expensive quarter of the tiles at
    // priority 3, the next at 2, then 1, the cheapest quarter at 0.  Measured on the refined cost
    // order (tools/sched_probe.py, profiles/r03_priority_policies.json): C3 N = 1 239.7 -> 235.8 ms,
    // its N = 2 share 141.6 -> 128.6 ms, the C4 N = 8 share 552.6 -> 496.2 ms; no setting was slower.
    return {{units / 4, units / 2, units - units / 4}, false};
}

// The passes of a launch whose build, K, G and run-ahead use are decided: the main pass's mode, the
// cold start, priorities, and what happens to the order afterwards.  Also the second half of
// plan_launch, and run again by render_impl after it has set G = 0 because the groups' buffers could
// not be reserved (the launch then runs plain on the planned build).
inline void plan_passes(const LaunchInputs& in, LaunchPlan& p)
{
    const bool sorted = in.knobs.schedule == 0, stats = in.instrumented, ahead = p.aheadUse || p.aheadMake;
    const bool valid = in.order.valid && !p.dropOrder, stale = in.order.stale || p.dropOrder;
    const uint64_t samples = (uint64_t)in.spp * in.chunks;
    const uint32_t total = in.spp * in.chunks;
    p.mode = p.G     ? LaunchMode::Grouped
             : stats ? LaunchMode::Instrumented
             : ahead ? LaunchMode::Ahead
                     : (p.K > 1 ? LaunchMode::Strip : LaunchMode::Plain);
    // Issue priority follows the order position, so it is meaningful only on a current cost order.
    // A launch whose tile costs will rebuild the order (stale order, or this launch measures >= 4x
    // the samples the order came from; see rebuildOrder below) runs without it: graded priority
    // shortens the head quarter's tiles, and costs measured under it would rank those tiles lower
    // on every rebuild (a feedback the order would carry over camera moves).
    const bool rebuilds = sorted && (stale || !valid || samples >= 4 * in.order.samples);
    p.mainPrio = (!rebuilds || in.knobs.prioMode == 2) ? issue_priority(in, p.units) : PassPriority{};   // explicit bounds: always
    p.mainPrio.dealt = in.knobs.prioMode == 0 && p.mainPrio.prio[0] != 0;
    // Cold start (first launch, or the scene, a texture or the camera changed): no tile costs yet.
    // Progressive 1-spp frames reuse the previous order for one launch.  A launch of several render()
    // calls runs its FIRST call as a launch of its own in row-major order, sorts the tiles by that
    // call's costs on the device and runs the other calls in that order -- nothing is computed twice,
    // and two launches of 1 and chunks - 1 calls are the reference's calls exactly as one launch is
    // (each call folds into the accumulation, ignoreHistory applies to the first).  Other launches
    // (one call, or sample groups, which take their draw-pair guesses from it) run a short discarded
    // pre-pass instead: kPrepassSpp samples per pixel (8 when it measures draw pairs) from the pixels'
    // current RNG state, nothing written back.  Either way the cold pass runs in row-major positions
    // without priority grading, and the launch then runs with issue priority on that order
    // (pt_set_cold_start; measured: one-shot C3 251-255 -> 238-240 ms, tools/cold_start.py); as its
    // tile costs are measured under priority, the order rebuilt from them is biased toward the head's
    // tiles, so the next launch rebuilds it again without priority.
    const bool cold = sorted && (stale || !valid) && samples >= kPrepassMinSpp && !stats;
    const bool split = cold && in.chunks >= 2 && !p.G && p.K == 1 && !ahead && in.knobs.prepassSpp == 0;
    p.cold = split ? ColdStart::SplitCall : cold ? ColdStart::Prepass : ColdStart::None;
    p.coldPairs = cold && !split && p.G != 0;      // speculative groups also take their offset guesses from it
    p.coldSpp = split ? in.spp : !cold ? 0u : p.coldPairs ? 8u : (in.knobs.prepassSpp ? in.knobs.prepassSpp : kPrepassSpp);
    p.coldPrio = {};
    p.costOrder = (sorted && valid) || cold;
    p.biasedOrder = cold && in.knobs.coldPriority && in.knobs.prioMode == 0;
    if (p.biasedOrder) {
        p.mainPrio = issue_priority(in, p.units);
        p.mainPrio.dealt = true;
    }
    if (p.G) p.mainPrio.dealt = false;     // (grouped positions are (tile, group) items: measured slower with it)
    // The order is rebuilt from this launch's tile costs when it is stale, or when this launch
    // measured every tile over at least 4x as many samples as the costs the order came from (a cold
    // start's 2-spp pre-pass, an 8-spp first launch): short launches rank tiles noisily, and a heavy
    // tile ranked light is dispatched late and becomes the launch's tail.
    p.rebuildOrder = sorted && (cold ? total >= 4 * (uint64_t)p.coldSpp : (stale || !valid || total >= 4 * in.order.samples));
}

inline LaunchPlan plan_launch(const LaunchInputs& in)
{
    LaunchPlan p = {};
    const bool sorted = in.knobs.schedule == 0, stats = in.instrumented;
    const bool noRepair = !in.knobs.riseRepair;             // test knob: plain launches of build 90 only
    const uint32_t tiles = in.tilesX * in.tilesY;
    const uint64_t samples = (uint64_t)in.spp * in.chunks;
    const uint32_t total = in.spp * in.chunks;
    const int picked = picked_build(in.knobs.variant, in.scene);
    // Run-ahead across render() calls (MODE 4).  A context whose camera or state changed on the last
    // two launches (a moving progressive camera) stops making stashes until it holds still again.
    // (strip units or sample groups forced by their knobs take precedence over automatic run-ahead)
    const bool aheadCapable = !stats && !noRepair && in.scene.hasRecords && build_has(picked, mode_bit(false, kModeAhead)) &&
                              in.knobs.aheadMode != 1 && (in.knobs.aheadMode == 2 || (in.knobs.stripMode < 2 && in.knobs.ssgMode < 2));
    p.aheadUse = aheadCapable && in.stashMatches && in.knobs.aheadMode != 3;     // 3: diagnostic, never consume
    // Automatic run-ahead only where tiles wait for a wave slot: a grid that holds every tile in one
    // pass (cornell 512x512: 4,096 tiles, 5,120-6,144 slots) has no next tile for a finished lane's
    // wave to delay, and run-ahead measured neutral there (4.37-4.42 vs 4.35-4.36 ms)
    // while it keeps the small-grid build from running.
    const bool aheadFits = in.knobs.aheadMode != 0 || (uint64_t)tiles > (uint64_t)in.cus * 4 * build_waves(picked);
    p.aheadMake = aheadCapable && (in.knobs.aheadMode == 2 || (samples >= kAheadMinSamples && samples <= kAheadMaxSamples &&
                                                         in.aheadMisses < 2 && aheadFits));
    const bool ahead = p.aheadUse || p.aheadMake;
    // Strip units (MODE 3): launches of few samples per pixel dispatch row strips of K tiles.  The cost
    // order is over units, so it is void when K changes.
    p.K = (sorted && !stats && !noRepair && !ahead) ? strip_tiles(in, picked, tiles, samples) : 1u;
    p.units = (in.tilesX + p.K - 1) / p.K * in.tilesY;
    p.dropOrder = p.K != in.order.strip;
    // speculative sample groups; the fold state packs (sample in call, call) into one
    // word as sIdx | c << 16 (ssg_fold_kernel)
    const bool groupable = !stats && sorted && samples < (1ull << 31) && in.spp <= 0xffffu && in.chunks <= 0xffffu;
    const bool plainOnly = p.K == 1 && !noRepair && !ahead;
    p.build = picked;
    p.G = groupable && plainOnly ? ssg_groups(in, picked, tiles, total) : 0;
    if (!p.G && in.knobs.variant == 0 && plainOnly) p.build = small_grid_build(in, picked, tiles);
    // The sixth wave slot (builds 60 / 61) raises throughput but gives each wave a smaller share of
    // the SIMD's issue: a plain launch of few tiles per slot, whose end is its heaviest tiles' sample
    // chains, runs longer with it (the C4 N = 8 share, 2.6 tiles per six-wave slot: 532 against 498 ms;
    // C3, 5.3 tiles per slot: 224.2 against 231.2; profiles/r05_six_waves.json).  Plain launches of
    // fewer than 4 dispatch units per six-wave slot (also 1-spp strip-unit frames) run the five-wave build.
    // (Round 3 sent grouped launches of at most one tile per wave slot to the undeferred walk, 39;
    // measured again on the C3 N = 8 share it costs 8-10 %: 52.9 ms against 47.1 (40) and 47.8-48.9
    // (60) with deferred shading, profiles/r05_six_waves.json.  Grouped launches keep the picked walk.)
    if (!p.G && in.knobs.variant == 0 && (uint64_t)p.units < 4ull * in.cus * 4 * 6) p.build = five_wave_build(p.build);
    if (noRepair) {
        // (the no-repair build exists at five waves only)
        if (five_wave_build(p.build) != 40 || stats) {
            p.refusal = "pt_set_rise_repair(0): only plain launches of variant 40 have a no-repair build";
            return p;
        }
        p.build = 90;
    }
    if (p.G) {
        // an item runs its group and, where the next group's guess missed, into the group after it;
        // further dead ends go to patch rounds
        const uint32_t ssgN = total / p.G;
        p.ssgCap = std::min<uint32_t>({total, 2 * ssgN + 64, 10000u});   // end offsets: 16-bit draw pairs (<= 6 per sample)
    }
    plan_passes(in, p);
    return p;
}

} // namespace pt
