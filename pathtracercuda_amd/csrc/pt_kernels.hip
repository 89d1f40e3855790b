// pt_kernels.hip -- gfx950 path-tracing megakernel, RNG seeding and tonemap kernels, and the C ABI
// of include/pt_hip.h.
//
// Reference behaviour (PathtracerCUDA/src/pathtracer/):
//   traceKernel  kernels/trace.cu:158-199 (+ getColor :101-156, hitBVH :28-98)
//   intersection Hittable.inl:88-358, AABB.inl:22-69
//   shading      Material.inl:20-144, MonteCarlo.h:5-114, brdf.h:4-62
//   seeding      kernels/initRandState.cu:4-17
//   tonemap      kernels/tonemap.cu:4-27
//
// MI355X design (DESIGN.md has the full rationale):
//   * one wave64 = one 8x8 pixel tile, one lane = one pixel: the per-pixel XORWOW stream is serial
//     (SURVEY.md fact 3), so pixels are the only parallel unit;
//   * the lane runs a flat state machine (segment = traverse + shade) and starts its pixel's next
//     sample as soon as a path ends, so a wave stays busy until its lanes have finished all
//     samples of all chunks of the launch, instead of idling at every path end;
//   * all `chunks` render() calls of the headless loop run in one launch; the per-chunk summation
//     (color = sum of spp paths, then color + accum) is reproduced exactly (the colour sum in LDS,
//     the accumulation value in registers);
//   * RNG state (24 B/pixel) and accum (16 B/pixel) are read once and written once per launch, SoA;
//   * the BVH node test hoists the per-ray reciprocals (bit-identical to recomputing them) and the
//     hit record is reconstructed once for the closest hit instead of for every candidate hit.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rccl/rccl.h>
#include <stdint.h>
#include <cmath>
#include <string.h>
#include <stdio.h>
#include <string>
#include <vector>
#include <algorithm>
#include <atomic>
#include <thread>
#include <chrono>
#include <utility>

#include "pt_math.h"
#include "pt_leaf_forms.h"
#include "pt_launch_plan.h"
#include "pt_ctx_state.h"
#include "../../include/pt_hip.h"

using namespace pt;

namespace {

// The kernel's dynamic LDS (layout: trace_kernel).  Declared here so device functions address it
// directly (ds_* instructions; a generic pointer kept in a struct would compile to flat_*).
extern __shared__ float4 lds4[];

__device__ __forceinline__ float* lds_f() { return reinterpret_cast<float*>(lds4); }
#include "pt_dev_scene.h"

#include "pt_dev_walk.h"

#include "pt_dev_path.h"

#include "pt_dev_groups.h"

// ---------------------------------------------------------------------------------------------
// Kernel A: lane-synchronous segments (traverse, then shade), per-lane path regeneration.
// LDS layout per workgroup: [scene nodes (2 float4 each) | scene prims (4 float4 each)] when
// SCENE_LDS, then WPB wave stacks of stackDepth x 64 u32.
// ---------------------------------------------------------------------------------------------
// The scene copied into the workgroup's LDS (SL >= 1), once per workgroup.
template <int SL, int WPB, int WW>
PT_DEV void stage_scene_impl(const TraceParams& P)
{
    if (SL < 1) return;
    const float4* gnodes = WW >= 3 ? P.cnodes : P.nodes;
    const uint32_t nodeF4 = WW >= 3 ? 4u * P.cnodeCount : 2u * P.nodeCount;
    for (uint32_t i = threadIdx.x; i < nodeF4; i += WPB * 64) lds4[i] = gnodes[i];
    if (SL >= 2)
        for (uint32_t i = threadIdx.x; i < 4u * P.primCount; i += WPB * 64) lds4[nodeF4 + i] = P.prims[i];
    __syncthreads();
}

// The LDS of a wave (trace_kernel's layout): the scene (SL >= 1: child-box records or nodes, SL >= 2:
// primitives too), WPB wave stacks of stackDepth x 64 entries (u32 node index, or uint2 (word, lo) for
// WW >= 3), then one accumulation slice per wave (3 planes of 64 floats).  Recomputed by every user
// from threadIdx, so the pointers stay LDS pointers even in a non-inlined item function.
template <int SL, int WPB, int WW>
struct WaveLds {
    const float4* nodes;
    const float4* prims;
    uint32_t* stack;
    uint32_t accL;            // float index of this lane's accumulation value in the dynamic LDS
};

template <int SL, int WPB, int WW>
PT_DEV WaveLds<SL, WPB, WW> wave_lds(const TraceParams& P)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const float4* gnodes = WW >= 3 ? P.cnodes : P.nodes;
    const uint32_t nodeF4 = WW >= 3 ? 4u * P.cnodeCount : 2u * P.nodeCount;
    const uint32_t sceneF4 = (SL >= 1 ? nodeF4 : 0u) + (SL >= 2 ? 4u * P.primCount : 0u);
    WaveLds<SL, WPB, WW> L;
    L.nodes = SL >= 1 ? lds4 : gnodes;
    L.prims = SL >= 2 ? lds4 + nodeF4 : P.prims;
    const uint32_t stackWords = (WW >= 3 ? 2u : 1u) * P.stackDepth * 64u;
    L.stack = reinterpret_cast<uint32_t*>(lds4 + sceneF4) + wave * stackWords + (WW >= 3 ? 2u : 1u) * lane;
    L.accL = 4u * sceneF4 + WPB * stackWords + wave * 192u + lane;
    return L;
}

// One work item of trace_kernel: the tile at dispatch slot `slot` (MODE 1: the (tile, group) item).
template <bool STATS, int SL, int WPB, int WW, int MINW, bool PERSIST, int MODE>
PT_DEV void run_item(const TraceParams& P, uint32_t slot, Counters& cnt)
{
    // MODE 4 (AHEAD): run-ahead across render() calls.  A launch of one or a few render() calls ends a
    // tile when its slowest pixel has finished; the lanes whose pixels finished first would idle until
    // then (28 % of lane time at 8 spp per call).  Here a lane whose pixel has finished
    // its last call stores the pixel (the call's final RNG state and accumulation value) and goes on
    // with the pixel's NEXT call -- the same XORWOW stream -- stashing after every sample the colour
    // sum so far, the sample count and the state (ahead_store), until the tile ends or a whole next
    // call is done.  A wave leaves the tile as soon as no lane has samples of this launch left.  The
    // next launch continues from the stash when its camera and scene are the ones it was made with
    // (host key, render_impl); otherwise the stored state is the exact one to continue from.
    // MODE 5 (ADAPT): adaptive sampling.  The wave's 64 pixels are entries of a compacted list of the
    // active pixels (pixel_of_list); each runs `chunks` render() calls from its own stream and folds
    // every call's luminance into its moments (end_call); no tile costs, no run-ahead stash.
    constexpr bool SSG = MODE == 1, AUX = MODE == 2, STRIP = MODE == 3, AHEAD = MODE == 4, ADAPT = MODE == 5;
    // the call's colour sum in LDS (get_color): the plain six-wave launch only (measured there; the
    // run-ahead build was 0.9 % slower with it on the reference's call loop)
    constexpr bool CL = MINW >= 6 && MODE == 0;
    const uint32_t lane = threadIdx.x & 63u;
    const WaveLds<SL, WPB, WW> Lw = wave_lds<SL, WPB, WW>(P);
    const float4* __restrict__ nodes = Lw.nodes;
    const float4* __restrict__ prims = Lw.prims;
    uint32_t* stack = Lw.stack;
    const uint32_t accL = Lw.accL;
    uint32_t tile, grp = 0, pos = slot;              // pos: the tile's position in the order
    if (SSG && !P.ssgPatch) {
        const uint32_t J = 2 * P.ssgG - 1;
        pos = slot / J;
        grp = slot - pos * J;                        // item within the tile (ssg_load)
    }
    tile = P.order ? P.order[pos] : pos;          // packed coordinates (scatter mode: wave index)
    // Issue priority: the cost order puts the most expensive tiles first, and at full occupancy
    // such a tile's chain runs ~3x slower than alone (tools/occupancy_probe.py) -- long enough to
    // end the launch.  Waves on the head of the order take issue slots first (s_setprio), the rest
    // fill the gaps.  pos is wave-uniform (an SGPR), so only one s_setprio executes.  Scheduling
    // only: results are identical.
    if (pos < P.prio[0]) __builtin_amdgcn_s_setprio(3);
    else if (pos < P.prio[1]) __builtin_amdgcn_s_setprio(2);
    else if (pos < P.prio[2]) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
    PixelCtx pc;
    if constexpr (ADAPT) pc = pixel_of_list(P, slot, lane);
    else pc = pixel_of(P, tile, lane);
    const uint64_t tWave = __builtin_amdgcn_s_memtime();
    const bool run = pc.valid && (!AUX || !P.fold || (P.fold[F_FLAG * pc.npix + pc.li] & 1u));
    if (run) {
        Xorwow rng;
        PathState ps;
        SsgLane sl;
        if (SSG) ssg_load(P, pos, grp, lane, pc.li, pc.npix, rng, ps, sl);
        else load_pixel<AUX, CL>(P, pc, rng, ps, accL);
        if (AHEAD && P.aheadUse) {
            ahead_load<CL>(P, pc, rng, ps);
            if (ps.s == P.spp) end_call<true, CL>(P, pc, ps, rng);     // a whole call was stashed
        }
        float fx = (float)(int32_t)pc.px, fy = (float)(int32_t)pc.py;
        camera_ray(P, fx, fy, rng, ps.o, ps.d);
        uint32_t stripK = 0;                     // STRIP: this lane's tile within the unit
        uint64_t tAll = STATS ? __builtin_amdgcn_s_memtime() : 0;
        uint64_t tDone = 0;
        if (WW >= 100) {
            // DEFERQ (WW / 1000, eighths; 0 = off): a wave shades its pending hits only once they are at
            // least DEFERQ/8 of its live lanes.  A lane whose hit is held back skips the traversal
            // rounds until then (its closest hit stays in ts), so hit shading -- the longest branch
            // -- runs for more lanes at once and in fewer rounds.  Every lane still performs its own
            // sequence of operations in order; only the round in which it shades changes.
            // SKYQ (WW / 10000): the same for misses (sky lookup, end of path, next camera ray).
            // DEFERQ + SKYQ <= 8, so when every live lane is ready one class always runs.
            constexpr int DEFERQ = (WW / 1000) % 10, SKYQ = (WW / 10000) % 10;
            constexpr bool NOREPAIR = (WW / 100000) % 10 != 0;     // test-only (pt_set_rise_repair)
            static_assert(DEFERQ + SKYQ <= 8, "a wave whose lanes are all ready must shade one class");
            bool fresh = true, held = false;
            TravState ts = {0u, 0u, 0xffffffffu, kFltMax};
            while (ps.alive) {
                if (AHEAD && __ballot(ps.c < P.chunks) == 0ull) break;   // only run-ahead lanes left
                if (STATS && fresh && !held) { cnt.segments++; wave_tick(cnt.w_segments); }
                bool tdone = true;
                if (!held) {
                    tdone = traverse_cb_phase<STATS, WW % 100, NOREPAIR>(nodes, prims, reinterpret_cast<uint2*>(stack), P,
                                                                                 ps.o, ps.d, fresh, ts, cnt);
                    fresh = tdone;
                }
                if (DEFERQ > 0 || SKYQ > 0) {
                    const bool hitReady = tdone && ts.elem != 0xffffffffu;
                    const bool missReady = tdone && ts.elem == 0xffffffffu;
                    const uint32_t na = (uint32_t)__popcll(__ballot(1));
                    bool hold = false;
                    if (DEFERQ > 0) hold = hitReady && (uint32_t)__popcll(__ballot(hitReady)) * 8u < na * (uint32_t)DEFERQ;
                    if (SKYQ > 0 && P.skybox != 0)     // without a sky texture a miss costs next to nothing
                        hold = hold || (missReady && (uint32_t)__popcll(__ballot(missReady)) * 8u < na * (uint32_t)SKYQ);
                    held = hold;
                    if (held) continue;
                }
                if (!tdone) continue;                              // suspended: resumes next round
                uint64_t tS = STATS ? __builtin_amdgcn_s_memtime() : 0;
                if (shade<STATS>(P, prims, ts.elem, ts.tMax, ps, rng, cnt)) {
                    if (SSG) ssg_finish<STATS>(P, ps, rng, fx, fy, sl, lane, pc.li, cnt);
                    else finish_path<STATS, AHEAD, CL, ADAPT>(P, ps, rng, fx, fy, cnt, pc);
                    if (STRIP && !ps.alive && stripK + 1 < P.strip) {
                        // Strip units (launches of few samples per pixel): a lane whose pixel is done
                        // stores it and takes the same position in the unit's next tile -- the tile to
                        // the right, so the wave's rays stay spatially coherent -- instead of idling
                        // until the slowest pixel of its tile is done.  Pixels are independent
                        // (their own RNG stream and accumulation value): results are unchanged.
                        const PixelCtx nx = pixel_of(P, tile + stripK + 1, lane);
                        if (nx.valid) {
                            if (!P.discard) store_pixel<CL>(P, pc, rng, ps);   // a cost pre-pass writes nothing
                            pc = nx;
                            ++stripK;
                            load_pixel<false, CL>(P, pc, rng, ps, accL);
                            fx = (float)(int32_t)pc.px;
                            fy = (float)(int32_t)pc.py;
                            camera_ray(P, fx, fy, rng, ps.o, ps.d);
                        }
                    }
                }
                if (STATS) wave_time(cnt.cyc_shade, tS);
                if (STATS && !ps.alive) tDone = __builtin_amdgcn_s_memtime();
            }
        }
        while (WW < 100 && ps.alive) {
            if (STATS) { cnt.segments++; wave_tick(cnt.w_segments); }
            float t;
            const uint32_t e = WW >= 3 ? traverse_cb<STATS>(nodes, prims, reinterpret_cast<uint2*>(stack), P, ps.o, ps.d, t, cnt)
                                       : traverse<STATS, WW>(nodes, prims, stack, ps.o, ps.d, P.slabFast != 0, t, cnt);
            uint64_t tS = STATS ? __builtin_amdgcn_s_memtime() : 0;
            if (shade<STATS>(P, prims, e, t, ps, rng, cnt)) {
                if (SSG) ssg_finish<STATS>(P, ps, rng, fx, fy, sl, lane, pc.li, cnt);
                else finish_path<STATS, false, CL, ADAPT>(P, ps, rng, fx, fy, cnt, pc);
            }
            if (STATS) wave_time(cnt.cyc_shade, tS);
        }
        if (STATS && WW >= 100 && tDone) {
            const uint64_t idle = __builtin_amdgcn_s_memtime() - tDone;
            cnt.cyc_lane_idle += idle;
            if (P.tileIdle && (tile >> 16) < P.tilesY)
                atomicAdd(&P.tileIdle[(tile >> 16) * P.tilesX + (tile & 0xffffu)], (uint32_t)min(idle >> 6, (uint64_t)0x3ffffffu));
        }
        if (STATS) wave_time(cnt.cyc_total, tAll);
        if (SSG) P.ssgCount[(size_t)sl.logItem * 64 + lane] = sl.k;
        else if (AHEAD) {}                    // stored when its last call ended (end_call)
        else if (!P.discard) store_pixel<CL>(P, pc, rng, ps);
        else if (AUX && P.pairsOut)           // cost pre-pass: draw pairs per sample of this pixel
        {
            P.pairsOut[pc.li] = (float)(((rng.d - P.rng[pc.li]) * kInvWeyl) >> 1) / (float)(P.spp * P.chunks);
            P.pairsOut[pc.npix + pc.li] = -1.0f;      // odd-length fraction unknown
        }
    }
    if (!ADAPT && P.tileCost && lane == 0 && (tile >> 16) < P.tilesY) {
        const uint32_t cyc = (uint32_t)min(__builtin_amdgcn_s_memtime() - tWave, (uint64_t)0xffffffffu);
        const uint32_t lin = (tile >> 16) * P.tilesX + (tile & 0xffffu);
        // SSG: zeroed before the launch (idle items add ~0)
        if (SSG) atomicAdd(&P.tileCost[lin], cyc / P.ssgG);
        else P.tileCost[lin] = cyc;
        if (STATS && P.tileTrace) {              // schedule trace (pt_set_tile_trace): start, hardware ids
            P.tileTrace[2 * lin] = (uint32_t)tWave;
            P.tileTrace[2 * lin + 1] = (__builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 20) << 16) |
                                       (__builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4) & 0xffffu);
        }
        // STRIP: the unit's cost sits at its first tile, the other tiles' entries are 0, so a sort of
        // the tile costs lists the units first (pt_render: the order of a strip launch)
        if (STRIP)
            for (uint32_t k = 1; k < P.strip && (tile & 0xffffu) + k < P.tilesX; ++k) P.tileCost[lin + k] = 0u;
    }
}

// SL = 0: scene read through the caches; 1: BVH nodes staged in LDS; 2: nodes and primitives in LDS.
// One wave = one 8x8 tile.  PERSIST: the grid holds only the resident waves, and each wave takes
// the next dispatch slot from a global counter when its tile is done, so a wave never waits for
// the other waves of its workgroup (which would keep the group's LDS and slots idle).
// MODE 0: plain; 1 (SSG): speculative sample groups (ssg_load / ssg_finish), one work item per
// (tile, group); 2: auxiliary launches -- the resume pass after a grouped launch, and the cost
// pre-pass that also measures draw pairs per sample; 3: strip units; 4: run-ahead across render()
// calls (run_item); 5: adaptive sampling -- a wave's pixels are 64 entries of the compacted list of
// active pixels, a slot is a wave of the list (pt_render_adaptive).  Separate instantiations keep the plain kernel's register allocation free of
// their code.
// First dispatch slot of wave `w` of workgroup `b` in a persistent grid of nCU x k workgroups.  The
// hardware places workgroups 0..nCU-1 on distinct CUs (round robin over the XCDs) and a workgroup's
// waves on distinct SIMDs, four apart (tools/hwid_probe.hip), so the slots -- positions in the cost
// order -- are dealt one per SIMD per round, every other round in reverse: a SIMD holds one of the
// heaviest tiles next to lighter ones of the later rounds.  A shared cursor instead hands the head to
// whichever waves start first, which cluster on a few CUs (208 distinct SIMDs among the first 1,024
// waves to start).  A bijection onto [0, grid x WPB); later slots come from the cursor after that range.
template <int WPB>
PT_DEV uint32_t spread_slot(uint32_t b, uint32_t w, uint32_t nCU)
{
    const uint32_t per = 4u * nCU;
    const uint32_t r = (b / nCU) * (uint32_t)(WPB / 4) + (w >> 2);
    const uint32_t idx = (w & 3u) * nCU + b % nCU;
    return r * per + ((r & 1u) ? per - 1u - idx : idx);
}

template <bool STATS, int SL, int WPB, int WW, int MINW, bool PERSIST = false, int MODE = 0>
__global__ void __launch_bounds__(WPB * 64, MINW) trace_kernel(TraceParams P)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    stage_scene_impl<SL, WPB, WW>(P);
    Counters cnt = {};
    const bool spread = PERSIST && P.spreadCU != 0;
    const uint32_t base = spread ? gridDim.x * (uint32_t)WPB : 0u;
    uint32_t slot = !PERSIST ? __builtin_amdgcn_readfirstlane(blockIdx.x * (uint32_t)WPB + wave)
                  : spread   ? spread_slot<WPB>(blockIdx.x, __builtin_amdgcn_readfirstlane(wave), P.spreadCU)
                             : wave_fetch(P.tileCursor, 1u);
    for (;;) {
    if (slot >= P.numSlots) break;               // also the grid's spare slots past the last item
    run_item<STATS, SL, WPB, WW, MINW, PERSIST, MODE>(P, slot, cnt);
    if (!PERSIST) break;
    slot = base + wave_fetch(P.tileCursor, 1u);
    }
    if (PERSIST) {
        // the last wave to leave rewinds the cursor for the next launch (every wave has made its
        // final fetch before it counts itself out), so no memset precedes the launch
        if (wave_fetch(P.tileCursor + 1, 1u) == gridDim.x * (uint32_t)WPB - 1 && lane == 0) {
            P.tileCursor[0] = 0;
            P.tileCursor[1] = 0;
        }
    }
    flush_counters<STATS>(P, cnt);
}

// initRandState (initRandState.cu:4-17): curand_init(1984 + x + y * width, 0, 0)
__global__ void __launch_bounds__(256) init_rng_kernel(uint32_t* rng, uint32_t width, uint32_t rows, uint32_t rowOffset,
                                                       uint32_t rowStride, uint32_t bandShift)
{
    const size_t npix = (size_t)rows * width;
    const size_t li = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (li >= npix) return;
    const uint32_t x = (uint32_t)(li % width);
    const uint32_t ly = (uint32_t)(li / width);
    const uint32_t y = global_row(ly, rowOffset, rowStride, bandShift);
    const uint32_t idx = x + y * width;
    const Xorwow s = xorwow_init((uint64_t)(uint32_t)(1984u + idx));
    rng[li] = s.d;
    rng[npix + li] = s.v0;
    rng[2 * npix + li] = s.v1;
    rng[3 * npix + li] = s.v2;
    rng[4 * npix + li] = s.v3;
    rng[5 * npix + li] = s.v4;
}

#include "pt_dev_tonemap.h"

__global__ void __launch_bounds__(256) tonemap_kernel(uchar4* out, const float4* accum, size_t npix, uint32_t frames)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    out[i] = tonemap_pixel(accum[i], frames);
}

// The same over an adaptive render's buffer: every pixel divided by its own number of calls.
__global__ void __launch_bounds__(256) tonemap_adaptive_kernel(uchar4* out, const float4* accum, const uint32_t* calls,
                                                               size_t npix)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    out[i] = tonemap_pixel(accum[i], calls[i]);
}

// ---------------------------------------------------------------------------------------------
// Adaptive sampling (pt_render_adaptive): after every round each pixel is re-evaluated from its
// moments and the active pixels are compacted into the list the next MODE 5 launch runs.
// ---------------------------------------------------------------------------------------------
// Pass 1: flag = the pixel has its minimum of calls and is not converged.  Batch-means standard
// error of the per-call luminance against tolerance x (|mean| + floor); the float operations and
// their order are the contract (tests/test_adaptive_rule.py restates them in numpy).  tolerance 0
// never converges; a non-finite pixel (the reference's 0/0 pdf NaNs) counts as converged.
__global__ void __launch_bounds__(256) adapt_flag_kernel(const uint32_t* __restrict__ mom, uint8_t* __restrict__ flag,
                                                         size_t npix, float tolerance, float floorv, uint32_t minCalls)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const float m1 = __uint_as_float(mom[i]), m2 = __uint_as_float(mom[npix + i]);
    const uint32_t n = mom[2 * npix + i];
    const float k = (float)n;
    const float mean = m1 / k;
    float ss = m2 - m1 * mean;
    if (ss < 0.0f) ss = 0.0f;
    const float se2 = ss / (k * (k - 1.0f));
    const float t = tolerance * (fabsf(mean) + floorv);
    const bool conv = tolerance > 0.0f && ((se2 <= t * t) || !__builtin_isfinite(m2));
    flag[i] = (n >= minCalls && !conv) ? 1u : 0u;
}

// Pass 2, one wave per 8x8 tile: a pixel is active below its minimum of calls, or below its maximum
// when any pixel of its 3x3 neighbourhood (clipped to the context's rows and width) is flagged -- a
// zero-variance dark pixel next to a noisy one keeps sampling.  `all`: every pixel (the first launch
// of a reset render).  The tile's ballot and its popcount feed the scan and the scatter.
__global__ void __launch_bounds__(256) adapt_mark_kernel(const uint8_t* __restrict__ flag, const uint32_t* __restrict__ calls,
                                                         uint32_t width, uint32_t rows, uint32_t tilesX, uint32_t tiles,
                                                         uint32_t minCalls, uint32_t maxCalls, uint32_t all,
                                                         unsigned long long* __restrict__ masks, uint32_t* __restrict__ counts)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (tile >= tiles) return;
    const uint32_t ty = tile / tilesX, tx = tile - ty * tilesX;
    const uint32_t x = tx * 8u + (lane & 7u), ly = ty * 8u + (lane >> 3);
    bool active = false;
    if (x < width && ly < rows) {
        const size_t li = (size_t)ly * width + x;
        const uint32_t n = all ? 0u : calls[li];
        if (all || n < minCalls) active = true;
        else if (n < maxCalls) {
            const uint32_t y0 = ly > 0u ? ly - 1u : 0u, y1 = ly + 1u < rows ? ly + 1u : rows - 1u;
            const uint32_t x0 = x > 0u ? x - 1u : 0u, x1 = x + 1u < width ? x + 1u : width - 1u;
            for (uint32_t yy = y0; yy <= y1; ++yy)
                for (uint32_t xx = x0; xx <= x1; ++xx) active = active || flag[(size_t)yy * width + xx] != 0u;
        }
    }
    const unsigned long long m = __ballot(active);
    if (lane == 0) {
        masks[tile] = m;
        counts[tile] = (uint32_t)__popcll(m);
    }
}

// Scatter, one wave per tile: the tile's active pixels go to list[offset of the tile + the lane's rank
// inside the ballot], so the list is tile-major and a wave of the next launch holds neighbouring pixels.
__global__ void __launch_bounds__(256) adapt_scatter_kernel(const unsigned long long* __restrict__ masks,
                                                            const uint32_t* __restrict__ offsets, uint32_t* __restrict__ list,
                                                            uint32_t width, uint32_t tilesX, uint32_t tiles)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (tile >= tiles) return;
    const unsigned long long m = masks[tile];
    if (!((m >> lane) & 1ull)) return;
    const uint32_t ty = tile / tilesX, tx = tile - ty * tilesX;
    const uint32_t x = tx * 8u + (lane & 7u), ly = ty * 8u + (lane >> 3);
    const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    list[offsets[tile] + rank] = ly * width + x;
}

#include "pt_dev_fold.h"

#include "pt_dev_denoise.h"

#include "pt_dev_temporal.h"

#include "pt_dev_svgf.h"

#include "pt_dev_adaptive_variance.h"

#include "pt_dev_despike.h"

#include "pt_dev_upsample.h"

#include "pt_dev_upsample_resolve.h"

#include "pt_dev_refit.h"

// Multi-device gather, second half: scatter one device's received rows (its bands, in local row
// order) into the full image.  A band is band-rows consecutive image rows in both buffers, so every
// lane copies one float4 of a coalesced row.
__global__ void __launch_bounds__(256) unpermute_rows_kernel(float4* __restrict__ full, const float4* __restrict__ part,
                                                             uint32_t width, uint32_t rows, uint32_t offset,
                                                             uint32_t stride, uint32_t shift)
{
    const size_t li = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (li >= (size_t)rows * width) return;
    const uint32_t ly = (uint32_t)(li / width);
    const uint32_t x = (uint32_t)(li - (size_t)ly * width);
    full[(size_t)global_row(ly, offset, stride, shift) * width + x] = part[li];
}

} // namespace

// =============================================================================================
// C ABI
// =============================================================================================
struct pt_context {
    int device = 0;
    int cus = 0;                      // compute units of the device
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint32_t width = 0, height = 0, rowOffset = 0, rowStride = 1, rows = 0, bandShift = 0;
    float4* accum = nullptr;
    uint32_t* rng = nullptr;
    float4* nodes = nullptr;
    float4* prims = nullptr;
    float4* mats = nullptr;
    float4* cnodes = nullptr;   // child-box records (traverse_cb); null when the scene exceeds its encoding
    uint32_t cnodeCount = 0, rootWord = 0;
    bool dfsOrder = true;             // leaves hold their primitives in DFS order (repair_pending)
    int zeroConstsType = -1;          // pt_set_zero_quadric_consts (tests' negative control only)
    CtxState st;                      // what one call leaves for the next: every validity flag (pt_ctx_state.h)
    uint32_t* ahead = nullptr;        // run-ahead across render() calls (MODE 4): the stash, [kAheadWords][pixels]
    float rootBox[6] = {};
    uint32_t nodeCount = 0, primCount = 0, stackDepth = 1;
    bool slabFast = true;
    LaunchKnobs knobs;                // pt_set_* (pt_launch_plan.h)
    uint32_t lastLaunch[4] = {};      // pt_last_launch: LDS bytes, staging level, waves per workgroup, workgroups
    DevTex* texTable = nullptr;
    DevTex hostTex[PT_MAX_TEXTURES] = {};
    uint32_t skybox = 0;
    unsigned long long* stats = nullptr;
    // tile scheduling: per-tile cost of the last launch and the cost-sorted dispatch order
    uint32_t* tileCost = nullptr;
    uint32_t* tileIdle = nullptr;     // instrumented launches: per-tile mean lane idle cycles (pt_read_tile_idle)
    uint32_t* tileTrace = nullptr;    // pt_set_tile_trace: per tile {start cycles, hardware ids} of the last launch
    bool traceTiles = false;
    uint32_t traceCap = 0;
    uint32_t* order = nullptr;
    uint32_t* rowMajor = nullptr;     // the row-major order (packed coordinates), before costs are known
    uint32_t* tileCursor = nullptr;   // persistent variants
    uint32_t* sortKeys = nullptr; // radix-sort scratch: sorted costs, tile ids, temp storage
    uint32_t* tileIds = nullptr;
    void* sortTemp = nullptr;
    size_t sortTempBytes = 0;
    uchar4* ldr = nullptr;        // tonemap staging buffer (pt_tonemap)
    uint32_t orderTiles = 0;      // tiles the device buffers hold
    uint32_t* unitMajor = nullptr;    // row-major order of strip units (packed first tiles), for unitK
    uint32_t unitK = 0, unitTiles = 0;
    uint32_t occupancy = 0;       // tuning knob: workgroups per CU of persistent grids (0 = all that fit)
    // speculative sample groups
    uint32_t patchRounds = 6;     // patch rounds before the remaining dead ends run plain
    uint32_t ssgLook[2] = {64, 16}; // second-phase lag tolerances in samples (TraceParams::ssgLook)
    float* pairs = nullptr;       // per-pixel draw pairs per sample (start-offset guesses)
    uint32_t* ssgStart = nullptr;
    unsigned long long* ssgBits = nullptr;
    uint32_t* ssgCount = nullptr;
    float* ssgLog = nullptr;
    uint16_t* ssgEnd = nullptr;
    uint32_t* fold = nullptr;     // [kFoldWords][pixels] fold state between rounds
    uint32_t* deadCount = nullptr;
    float* patchLog = nullptr;    // patch-round carriers: [tile][patchCap][3][64]
    uint16_t* patchEnd = nullptr;
    uint32_t* patchCount = nullptr;
    size_t ssgItems = 0, ssgSamples = 0, patchSamples = 0;   // allocated capacities (records)
    size_t ssgBitsWords = 0;
    uint32_t lastGroups = 0;      // groups of the last launch (0 = plain launch)
    int lastVariant = 0;          // trace-kernel variant of the last launch's main pass
    uint32_t groupStats[10] = {}; // G, patch rounds, dead-end pixels after fold rounds 0..7
    // adaptive sampling (pt_render_adaptive): per-pixel moments and the compaction buffers
    uint32_t* adMom = nullptr;        // [3][pixels]: m1, m2 (float bits), n
    uint32_t adSteps = 0;             // steps (calls of the active pixels) made since the last reset
    uint8_t* adFlag = nullptr;        // [pixels] has its minimum of calls and is not converged
    unsigned long long* adMasks = nullptr;   // [tiles] ballot of the tile's active pixels
    uint32_t* adCounts = nullptr;     // [tiles + 1] their popcounts (the last entry stays 0)
    uint32_t* adOffsets = nullptr;    // [tiles + 1] exclusive scan; the last entry is the active count
    uint32_t* adList = nullptr;       // [pixels] active local pixel indices, tile-major
    void* adTemp = nullptr;
    size_t adTempBytes = 0;
    // first-hit feature planes and the denoiser (pt_denoise.h); no render state
    float4* feat = nullptr;           // [3][pixels], allocated by the first pt_render_features
    float featMs = 0.0f;
    float4* dnBuf = nullptr;          // [6][pixels]: colour, two guide planes, two iteration buffers, the result
    hipEvent_t dnEv[12] = {};
    float dnMs[10] = {};
    // temporal reprojection (pt_temporal.h); no render state
    pt_camera featCam = {};           // the camera of the last pt_render_features
    float4* tpBuf = nullptr;          // [8][pixels]: colour, image, two history sets of three planes
    uint32_t tpSet = 0;               // the set the last pt_temporal wrote
    pt_camera tpCam = {};             // its camera
    float tpMs = 0.0f;
    // the history's moments and the variance (pt_svgf.h); no render state
    float4* motion = nullptr;         // [motionCount][4]: rule 7's table, of the scene set by the last pt_set_scene_moved
    uint32_t motionCount = 0;
    float4* tmBuf = nullptr;          // [2][pixels] moments planes of tpBuf's two history sets, then [pixels] float: the variance
    hipEvent_t tmEv[3] = {};
    float tmMs[2] = {};               // the step, the estimate
    uint32_t tmFlags = 0;             // the flags the held moments were made with
    hipEvent_t fbEv[2] = {};          // around the feedback kernel (pt_denoise_variance_feedback)
    float fbMs = 0.0f;
    bool fbRan = false;               // a feedback call has run since the last moments step
    // the variance of an adaptive render's image (pt_adaptive_variance.h); no render state
    float4* avBuf = nullptr;          // [2][pixels] the tap planes (N, l), (P, id), then [pixels] float: the variance
    hipEvent_t avEv[2] = {};          // around adaptive_variance_kernel
    float avMs = 0.0f;
    // despike (pt_despike.h); no render state
    float4* dsBuf = nullptr;          // [pixels] the colour, [2][pixels] the tap planes (N, l), (P, id), [pixels] the despiked image, the count
    hipEvent_t dsEv[3] = {};          // before the flat pass, between the kernels, after despike_kernel
    float dsMs[2] = {};
    uint32_t dsCount = 0;
    // guided upsampling (pt_upsample.h), held by the context of the larger frame; no render state
    float4* usBuf = nullptr;          // [3][usLoCap] the packed low texels, [usLoCap] the low colour, [pixels] the upsampled image, the counts
    size_t usLoCap = 0;               // low pixels the buffers were made for
    hipEvent_t usEv[3] = {};          // before the flat pass, between the kernels, after upsample_kernel
    float usMs[2] = {};
    uint32_t usCounts[2] = {};        // guided pixels that needed ring 2, that took the nearest low pixel
    // moving primitives and the refit (pt_refit.h); the boxes and lists are of the scene while holds_boxes
    bool grouped = false;             // a member of a device group (pt_group_create): the refit is refused there
    float4* rfBoxes = nullptr;        // [primCount][2]: min xyz, max xyz (w = 0)
    uint32_t* rfLists = nullptr;      // the reachable leaves' node indices, then (node, record) per interior node by depth
    uint32_t rfLeafCount = 0;
    std::vector<uint32_t> rfLevelOff; // interior depth d (the root's is 0) holds pairs rfLevelOff[d] .. rfLevelOff[d + 1]
    float4* rfPack = nullptr;         // the packed records of a move, kMoveQuads each
    size_t rfPackCap = 0;             // moved primitives it was made for
    std::vector<float4> rfHost;       // the same on the host, kept until the copy is done
    hipEvent_t rfEv[3] = {};          // before and after the kernels of a move; [2] before the copy
    float rfMs = 0.0f, rfPackMs = 0.0f, rfCopyMs = 0.0f;   // the kernels, the host packing, the copy
    bool rfRan = false;               // a move has run on this context
    std::string err;
};

#define PT_HIP_CHECK(ctx, ...)                                                               \
    do {                                                                                     \
        hipError_t e_ = (__VA_ARGS__);                                                         \
        if (e_ != hipSuccess) {                                                              \
            if (ctx) {                                                                       \
                char b_[512];                                                                \
                snprintf(b_, sizeof(b_), "HIP error = %u (%s) at %s:%d '%s'", (unsigned)e_,  \
                         hipGetErrorString(e_), __FILE__, __LINE__, #__VA_ARGS__);           \
                (ctx)->err = b_;                                                             \
            }                                                                                \
            return PT_ERR_HIP;                                                               \
        }                                                                                    \
    } while (0)

static inline float u2f(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}

static inline f3 hf3(const float* v) { f3 r; r.x = v[0]; r.y = v[1]; r.z = v[2]; return r; }

static int fail(pt_context* ctx, int code, const char* msg)
{
    if (ctx) ctx->err = msg;
    return code;
}

// What launch_one launched last on this host thread (a device group renders one context per thread):
// dynamic LDS bytes of a workgroup, staging level, waves per workgroup, workgroups.  launch_one has
// no context; render_impl copies it after its main pass (pt_last_launch; diagnostics and tests).
static thread_local uint32_t g_lastLaunch[4] = {};

static inline void note_launch(size_t lds, int sl, int wpb, unsigned groups)
{
    g_lastLaunch[0] = (uint32_t)lds;
    g_lastLaunch[1] = (uint32_t)sl;
    g_lastLaunch[2] = (uint32_t)wpb;
    g_lastLaunch[3] = groups;
}

// One instantiation of trace_kernel on a device of `cus` compute units, and its fallbacks: no
// child-box layout -> the node-at-a-time walk, too large to stage -> the scene through the caches, a
// grid that fits in one pass -> the plain (non-persistent) kernel.
template <bool STATS, int SL, int WPB, int WW, int MINW, bool PERSIST = false, int MODE = 0>
static hipError_t launch_one(const TraceParams& P, int cus, hipStream_t stream)
{
    const size_t lds = lds_bytes(SL, WPB, WW >= 3, SceneSize{P.nodeCount, P.cnodeCount, P.primCount, P.stackDepth});
    // no child-box layout: the node-at-a-time walk -- except for grouped and strip launches, whose
    // item and strip hand-off logic lives only in the resumable walk (picked_build never sends them here)
    if (WW >= 3 && P.cnodes == nullptr) {
        if constexpr (MODE == 1 || MODE >= 3) return hipErrorInvalidValue;
        else return launch_one<STATS, SL, WPB, 1, MINW, PERSIST, MODE>(P, cus, stream);
    }
    if (lds > kLdsLimit) {
        // scene too large to stage in LDS: the same variant reading the scene through the caches
        if (SL > 0) return launch_one<STATS, 0, WPB, WW, MINW, PERSIST, MODE>(P, cus, stream);
        return hipErrorInvalidValue;                   // the stacks alone exceed the LDS
    }
    // the dynamic-LDS limit is raised once per device (contexts on several devices may run on
    // several host threads, as the CLI's -gpus mode does)
    static std::atomic<uint64_t> attrSet{0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const uint64_t bit = 1ull << (dev & 63);
    if (!(attrSet.load() & bit)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&trace_kernel<STATS, SL, WPB, WW, MINW, PERSIST, MODE>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit);
        if (e != hipSuccess) return e;
        attrSet.fetch_or(bit);
    }
    unsigned blocks = (P.numSlots + WPB - 1) / WPB;    // numSlots = tiles, or tiles x groups (SSG)
    if (PERSIST) {
        // resident workgroups per device, cached per instantiation; a grid that fits in one
        // pass gains nothing from the cursor and runs the plain kernel
        static std::atomic<int> resident[64];
        int cap = resident[dev & 63].load();
        if (cap == 0) {
            int perCu = 0;
            hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
                &perCu, reinterpret_cast<const void*>(&trace_kernel<STATS, SL, WPB, WW, MINW, PERSIST, MODE>), WPB * 64, lds);
            if (e != hipSuccess) return e;
            cap = cus * std::max(perCu, 1);
            resident[dev & 63].store(cap);
        }
        if (P.occCap)                                  // tuning knob (pt_set_occupancy): fewer waves per SIMD
            cap = cus * std::min(cap / cus, (int)P.occCap);
        if constexpr (MODE == 5) {
            // adaptive rounds shrink from launch to launch: a list that fits in one pass runs the same
            // kernel on a grid of its own size, every wave taking its slot from the cursor (one build
            // per variant instead of two)
            if (!P.occCap && blocks <= (unsigned)cap) {
                note_launch(lds, SL, WPB, blocks);
                trace_kernel<STATS, SL, WPB, WW, MINW, PERSIST, MODE><<<blocks, WPB * 64, lds, stream>>>(P);
                return hipGetLastError();
            }
        } else {
            if (!P.occCap && blocks <= (unsigned)cap) return launch_one<STATS, SL, WPB, WW, MINW, false, MODE>(P, cus, stream);
        }
        if (cap <= 0) return hipErrorInvalidValue;
        TraceParams Q = P;                             // first slots dealt per SIMD (spread_slot)
        Q.spreadCU = (WPB % 4 == 0 && cap % cus == 0) ? (uint32_t)cus : 0u;
        if (P.prioDealt) {
            // Every position dealt at the start runs in the first priority band.  Waves of equal
            // priority issue oldest first (the resident grid's dispatch order: tools/tile_trace.py shows
            // the dealing rounds' tiles at 164 / 175 / 235 / 273 ms median and the last round's, at level
            // 2 below the others, at 373 ms -- the launch's end on the C4 N = 8 share); in one band the
            // order of the rounds follows the cost order.  C4 N = 8 share 464-481 -> 446-456 ms
            // (tools/prio_probe.py, profiles/r06_schedule_trace.json).
            const uint32_t dealt = std::min<uint32_t>(P.numSlots, (uint32_t)cap * WPB);
            Q.prio[0] = std::max(Q.prio[0], dealt);
            Q.prio[1] = std::max(Q.prio[1], Q.prio[0]);
            Q.prio[2] = std::max(Q.prio[2], Q.prio[1]);
        }
        note_launch(lds, SL, WPB, (unsigned)cap);
        trace_kernel<STATS, SL, WPB, WW, MINW, PERSIST, MODE><<<(unsigned)cap, WPB * 64, lds, stream>>>(Q);
        return hipGetLastError();
    }
    note_launch(lds, SL, WPB, blocks);
    trace_kernel<STATS, SL, WPB, WW, MINW, PERSIST, MODE><<<blocks, WPB * 64, lds, stream>>>(P);
    return hipGetLastError();
}

// Launch build `v` (pt_builds.h) in launch mode (STATS, MODE): the table's row with that id, if it has
// the mode.  Rows without it are not instantiated; the others are, in table order (a left fold), all
// from this one body -- the order their kernels take in the code object.
template <bool STATS, int MODE, size_t... ROW>
static hipError_t launch_rows(int v, const TraceParams& P, int cus, hipStream_t stream, std::index_sequence<ROW...>)
{
    hipError_t e = hipErrorInvalidValue;
    (..., [&] {
        constexpr Build B = kBuilds[ROW];
        if constexpr ((B.modes & mode_bit(STATS, MODE)) != 0)
            if (v == B.id) e = launch_one<STATS, B.SL, B.WPB, B.WW, B.MINW, B.PERSIST, MODE>(P, cus, stream);
    }());
    return e;
}

template <bool STATS, int MODE>
static hipError_t launch_build(int v, const TraceParams& P, int cus, hipStream_t stream)
{
    return launch_rows<STATS, MODE>(v, P, cus, stream, std::make_index_sequence<kBuildCount>{});
}

// Strip-unit, run-ahead and adaptive launches (kModeStrip, kModeAhead, kModeAdaptive as a value): the
// modes in which a lane that is done goes on with other work, built for the resumable walks (adaptive
// launches also for the node-at-a-time fallbacks).
static hipError_t launch_resumable(int v, int mode, const TraceParams& P, int cus, hipStream_t stream)
{
    switch (mode) {
    case kModeStrip: return launch_build<false, kModeStrip>(v, P, cus, stream);
    case kModeAhead: return launch_build<false, kModeAhead>(v, P, cus, stream);
    case kModeAdaptive: return launch_build<false, kModeAdaptive>(v, P, cus, stream);
    default: return hipErrorInvalidValue;
    }
}

extern "C" {

PT_API int pt_device_count(int* count)
{
    if (!count) return PT_ERR_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return PT_OK;
}

PT_API uint32_t pt_band_rows(uint32_t height, uint32_t band_rows, uint32_t band_offset, uint32_t band_stride)
{
    if (band_rows == 0 || band_stride == 0 || (band_rows & (band_rows - 1)) != 0) return 0;
    const uint32_t nb = (height + band_rows - 1) / band_rows;
    if (band_offset >= nb) return 0;
    const uint32_t own = (nb - band_offset + band_stride - 1) / band_stride;
    const uint32_t last = band_offset + (own - 1) * band_stride;
    return (own - 1) * band_rows + std::min(band_rows, height - last * band_rows);
}

PT_API int pt_unpermute_bands(int device, void* full, const void* part, uint32_t width, uint32_t height, uint32_t band_rows,
                              uint32_t band_offset, uint32_t band_stride)
{
    if (!full || !part || width == 0 || band_stride == 0 || band_rows == 0 || band_rows > 256 ||
        (band_rows & (band_rows - 1)) != 0)
        return PT_ERR_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return PT_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return PT_ERR_ARG;
    const uint32_t rows = pt_band_rows(height, band_rows, band_offset, band_stride);
    const size_t npix = (size_t)rows * width;
    if (npix == 0) return PT_OK;
    if (hipSetDevice(device) != hipSuccess) return PT_ERR_HIP;
    // the caller's buffers may be in use on any stream of the device: synchronise around the copy
    if (hipDeviceSynchronize() != hipSuccess) return PT_ERR_HIP;
    unpermute_rows_kernel<<<(unsigned)((npix + 255) / 256), 256, 0, 0>>>(
        static_cast<float4*>(full), static_cast<const float4*>(part), width, rows, band_offset, band_stride,
        (uint32_t)__builtin_ctz(band_rows));
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return PT_ERR_HIP;
    return PT_OK;
}

PT_API int pt_create(int device, uint32_t width, uint32_t height, uint32_t row_offset, uint32_t row_stride,
                     pt_context** out)
{
    return pt_create_banded(device, width, height, 1, row_offset, row_stride, out);
}

PT_API int pt_create_banded(int device, uint32_t width, uint32_t height, uint32_t band_rows, uint32_t band_offset,
                            uint32_t band_stride, pt_context** out)
{
    if (!out || width == 0 || height == 0 || band_stride == 0) return PT_ERR_ARG;
    *out = nullptr;
    if (band_rows == 0 || band_rows > 256 || (band_rows & (band_rows - 1)) != 0) return PT_ERR_ARG;
    // tiles are addressed by packed 16-bit coordinates (tileY << 16 | tileX), pixels by 32-bit indices
    {
        const uint64_t r = pt_band_rows(height, band_rows, band_offset, band_stride);
        if (width > 8u * 0xffffu || r > 8u * 0xfffeu || r * width >= (1ull << 30)) return PT_ERR_ARG;
    }
    const uint32_t row_offset = band_offset, row_stride = band_stride;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return PT_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return PT_ERR_ARG;
    pt_context* ctx = new pt_context();
    ctx->device = device;
    ctx->width = width;
    ctx->height = height;
    ctx->rowOffset = row_offset;
    ctx->rowStride = row_stride;
    ctx->bandShift = (uint32_t)__builtin_ctz(band_rows);
    ctx->rows = pt_band_rows(height, band_rows, band_offset, band_stride);
    auto bail = [&](int code) { pt_destroy(ctx); return code; };
    if (hipSetDevice(device) != hipSuccess) return bail(PT_ERR_HIP);
    if (hipDeviceGetAttribute(&ctx->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ctx->cus < 1)
        return bail(PT_ERR_HIP);
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) return bail(PT_ERR_HIP);
    if (hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess) return bail(PT_ERR_HIP);
    const size_t npix = (size_t)ctx->rows * width;
    const size_t nalloc = npix ? npix : 1;
    if (hipMalloc(&ctx->accum, nalloc * sizeof(float4)) != hipSuccess) return bail(PT_ERR_HIP);
    if (hipMalloc(&ctx->rng, nalloc * 6 * sizeof(uint32_t)) != hipSuccess) return bail(PT_ERR_HIP);
    if (hipMalloc(&ctx->texTable, PT_MAX_TEXTURES * sizeof(DevTex)) != hipSuccess) return bail(PT_ERR_HIP);
    if (hipMalloc(&ctx->stats, kStatWords * sizeof(unsigned long long)) != hipSuccess) return bail(PT_ERR_HIP);
    if (hipMemsetAsync(ctx->accum, 0, nalloc * sizeof(float4), ctx->stream) != hipSuccess) return bail(PT_ERR_HIP);
    if (hipMemcpyAsync(ctx->texTable, ctx->hostTex, sizeof(ctx->hostTex), hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        return bail(PT_ERR_HIP);
    if (npix) {
        const unsigned blocks = (unsigned)((npix + 255) / 256);
        init_rng_kernel<<<blocks, 256, 0, ctx->stream>>>(ctx->rng, width, ctx->rows, row_offset, row_stride,
                                                                ctx->bandShift);
        if (hipGetLastError() != hipSuccess) return bail(PT_ERR_HIP);
    }
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return bail(PT_ERR_HIP);
    *out = ctx;
    return PT_OK;
}

PT_API void pt_destroy(pt_context* ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(ctx->accum);
    (void)hipFree(ctx->rng);
    (void)hipFree(ctx->nodes);
    (void)hipFree(ctx->prims);
    (void)hipFree(ctx->mats);
    (void)hipFree(ctx->cnodes);
    (void)hipFree(ctx->tileCost);
    (void)hipFree(ctx->tileIdle);
    (void)hipFree(ctx->tileTrace);
    (void)hipFree(ctx->order);
    (void)hipFree(ctx->rowMajor);
    (void)hipFree(ctx->unitMajor);
    (void)hipFree(ctx->tileCursor);
    (void)hipFree(ctx->ldr);
    (void)hipFree(ctx->sortKeys);
    (void)hipFree(ctx->tileIds);
    (void)hipFree(ctx->sortTemp);
    (void)hipFree(ctx->texTable);
    (void)hipFree(ctx->stats);
    (void)hipFree(ctx->pairs);
    (void)hipFree(ctx->ssgStart);
    (void)hipFree(ctx->ssgBits);
    (void)hipFree(ctx->ssgCount);
    (void)hipFree(ctx->ssgLog);
    (void)hipFree(ctx->ssgEnd);
    (void)hipFree(ctx->fold);
    (void)hipFree(ctx->deadCount);
    (void)hipFree(ctx->patchLog);
    (void)hipFree(ctx->patchEnd);
    (void)hipFree(ctx->patchCount);
    (void)hipFree(ctx->ahead);
    (void)hipFree(ctx->adMom);
    (void)hipFree(ctx->adFlag);
    (void)hipFree(ctx->adMasks);
    (void)hipFree(ctx->adCounts);
    (void)hipFree(ctx->adOffsets);
    (void)hipFree(ctx->adList);
    (void)hipFree(ctx->adTemp);
    (void)hipFree(ctx->feat);
    (void)hipFree(ctx->dnBuf);
    (void)hipFree(ctx->tpBuf);
    (void)hipFree(ctx->tmBuf);
    (void)hipFree(ctx->motion);
    (void)hipFree(ctx->avBuf);
    (void)hipFree(ctx->dsBuf);
    (void)hipFree(ctx->usBuf);
    (void)hipFree(ctx->rfBoxes);
    (void)hipFree(ctx->rfLists);
    (void)hipFree(ctx->rfPack);
    for (auto& e : ctx->rfEv)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : ctx->dnEv)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : ctx->tmEv)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : ctx->fbEv)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : ctx->avEv)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : ctx->dsEv)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : ctx->usEv)
        if (e) (void)hipEventDestroy(e);
    for (auto& t : ctx->hostTex) (void)hipFree((void*)t.texels);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

// Rule 7's table as the host arrays give it: refused, or packed into the kernels' four float4 per primitive.
static const char* motion_table_refusal(uint32_t prim_count, const float* rows, const uint32_t* prev_index)
{
    if (!rows || !prev_index) return "motion_rows or prev_index is null";
    if (prim_count == 0 || prim_count >= (1u << 26)) return "prim_count must be 1 .. 2^26 - 1";
    return nullptr;
}

static std::vector<float4> motion_table_pack(uint32_t prim_count, const float* rows, const uint32_t* prev_index)
{
    std::vector<float4> e(4 * (size_t)prim_count);
    for (uint32_t i = 0; i < prim_count; ++i) {
        const float* r = rows + 12 * (size_t)i;
        for (int k = 0; k < 3; ++k) e[4 * (size_t)i + k] = make_float4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
        e[4 * (size_t)i + 3] = make_float4(u2f(prev_index[i]), 0.0f, 0.0f, 0.0f);
    }
    return e;
}

// A primitive's four quads and its material's three as the kernels read them (pt_set_scene and pt_move_primitives).
static void pack_primitive(const pt_context* ctx, const pt_hittable& h, float4* p, float4* m)
{
    const float(&R)[3][4] = h.inv_transform_rows;
    p[0] = make_float4(R[0][0], R[1][0], R[0][1], R[1][1]);
    p[1] = make_float4(R[0][2], R[1][2], R[0][3], R[1][3]);
    p[2] = make_float4(R[2][0], R[2][1], R[2][2], R[2][3]);
    // fourth quad: the type and the shape's quadric constants (quadric_roots reads them here)
    float qB, qH, qJ;
    quadric_consts(h.type, qB, qH, qJ);
    if ((int)h.type == ctx->zeroConstsType)                      // test knob, see pt_hip.h: zeros for a
        qB = qH = qJ = (h.type == 2u || h.type >= 5u) ? std::nanf("") : 0.0f;   // quadric, NaN for a plane or cube
    p[3] = make_float4(u2f(h.type), qB, qH, qJ);
    m[0] = make_float4(h.base_color[0], h.base_color[1], h.base_color[2], h.roughness);
    m[1] = make_float4(h.emissive[0], h.emissive[1], h.emissive[2], h.metalness);
    m[2] = make_float4(u2f(h.texture_index), u2f(h.material_type), 0.0f, 0.0f);
}

// Host-side validation of the BVH so a malformed scene can never make the kernel read out of
// bounds or overflow its 32-entry stack (the reference does not check, trace.cu:39).
static int validate_scene(pt_context* ctx, const pt_bvh_node* nodes, uint32_t nn, const pt_hittable* prims, uint32_t np,
                          uint32_t& maxDepthOut, std::vector<uint8_t>& reach)
{
    for (uint32_t i = 0; i < np; ++i) {
        if (prims[i].type > 6u) return fail(ctx, PT_ERR_ARG, "pt_set_scene: invalid hittable type");
        if (prims[i].texture_index > PT_MAX_TEXTURES) return fail(ctx, PT_ERR_ARG, "pt_set_scene: invalid texture index");
    }
    // iterative DFS computing the depth (number of nodes on the root-to-node path)
    std::vector<std::pair<uint32_t, uint32_t>> st;
    st.push_back({0u, 1u});
    uint32_t maxDepth = 0, visited = 0;
    while (!st.empty()) {
        auto [i, depth] = st.back();
        st.pop_back();
        if (i >= nn) return fail(ctx, PT_ERR_ARG, "pt_set_scene: node index out of range");
        if (++visited > nn) return fail(ctx, PT_ERR_ARG, "pt_set_scene: BVH is not a tree");
        reach[i] = 1;
        maxDepth = std::max(maxDepth, depth);
        const uint32_t pca = nodes[i].primitive_count_axis;
        const uint32_t count = pca >> 16;
        if (count > 0) {
            if ((uint64_t)nodes[i].offset + count > np) return fail(ctx, PT_ERR_ARG, "pt_set_scene: leaf range out of bounds");
        } else {
            if (((pca >> 8) & 0xffu) > 2u) return fail(ctx, PT_ERR_ARG, "pt_set_scene: invalid split axis");
            if (nodes[i].offset <= i + 1 || nodes[i].offset >= nn || i + 1 >= nn)
                return fail(ctx, PT_ERR_ARG, "pt_set_scene: invalid child index");
            st.push_back({i + 1, depth + 1});
            st.push_back({nodes[i].offset, depth + 1});
        }
    }
    if (maxDepth > 33) return fail(ctx, PT_ERR_DEPTH, "pt_set_scene: BVH depth exceeds the 32-entry traversal stack");
    maxDepthOut = maxDepth;
    return PT_OK;
}

// pt_set_scene (motion_rows null) and pt_set_scene_moved: the same validation, refusals and uploads; the moved
// form also checks and uploads rule 7's table and raises scene_moved in place of scene_or_texture_changed.
static int set_scene_impl(pt_context* ctx, const pt_bvh_node* nodes, uint32_t node_count, const pt_hittable* prims,
                          uint32_t prim_count, const float* motion_rows, const uint32_t* prev_index)
{
    if (node_count == 0 || prim_count == 0 || !nodes || !prims) return fail(ctx, PT_ERR_ARG, "pt_set_scene: empty scene");
    uint32_t maxDepth = 1;
    // nodes reachable from the root: only they are validated, so only they are read below (an
    // unreachable node may hold any offset; the reference never visits it either)
    std::vector<uint8_t> reach(node_count, 0);
    int rc = validate_scene(ctx, nodes, node_count, prims, prim_count, maxDepth, reach);
    if (rc != PT_OK) return rc;
    // Refused (include/pt_hip.h): a primitive whose inverse transform holds inf or NaN (a zero scale)
    for (uint32_t i = 0; i < prim_count; ++i)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c)
                if (!std::isfinite(prims[i].inv_transform_rows[r][c])) {
                    char buf[160];
                    snprintf(buf, sizeof(buf), "pt_set_scene: primitive %u: inv_transform_rows[%d][%d] is not finite "
                             "(every value must be a finite float)", i, r, c);
                    return fail(ctx, PT_ERR_ARG, buf);
                }
    std::vector<float4> table;
    if (motion_rows) {
        if (const char* why = motion_table_refusal(prim_count, motion_rows, prev_index))
            return fail(ctx, PT_ERR_ARG, (std::string("pt_set_scene_moved: ") + why).c_str());
        for (uint32_t i = 0; i < prim_count; ++i)
            if (prev_index[i] != 0xffffffffu && prev_index[i] >= ctx->primCount) {
                char buf[200];
                snprintf(buf, sizeof(buf), "pt_set_scene_moved: primitive %u: prev_index %u is neither 0xffffffff nor below "
                         "the %u primitives of the scene it replaces", i, prev_index[i], ctx->primCount);
                return fail(ctx, PT_ERR_ARG, buf);
            }
        table = motion_table_pack(prim_count, motion_rows, prev_index);
    }
    std::vector<float4> hn(2 * (size_t)node_count), hp(4 * (size_t)prim_count), hm(3 * (size_t)prim_count);
    bool slabFast = true;
    for (uint32_t i = 0; i < node_count; ++i) {
        const pt_bvh_node& n = nodes[i];
        hn[2 * i] = make_float4(n.aabb_min[0], n.aabb_max[0], n.aabb_min[1], n.aabb_max[1]);
        hn[2 * i + 1] = make_float4(n.aabb_min[2], n.aabb_max[2], u2f(n.offset), u2f(n.primitive_count_axis));
        for (int k = 0; k < 3; ++k)   // the fast slab test needs ordered, non-NaN bounds
            if (!(n.aabb_min[k] <= n.aabb_max[k])) slabFast = false;
    }
    // child-box records: interior nodes renumbered in order; a child word is (count << 24 | prim
    // offset) for a leaf, the record index otherwise (needs counts < 256 and offsets < 2^24)
    std::vector<uint32_t> rec(node_count, 0xffffffffu);
    uint32_t interior = 0;
    bool cbOk = node_count < (1u << 24) && prim_count < (1u << 24);
    for (uint32_t i = 0; i < node_count; ++i) {
        const uint32_t count = nodes[i].primitive_count_axis >> 16;
        if (count == 0) rec[i] = interior++;
        else if (count > 255 && reach[i]) cbOk = false;
    }
    auto word = [&](uint32_t i) {
        const uint32_t count = nodes[i].primitive_count_axis >> 16;
        return count ? (count << 24) | nodes[i].offset : rec[i];
    };
    // first and last primitive under each node (children follow their parent in the array); the
    // rising-t_max rebuild (repair_pending) finds a leaf's path by the first primitive of each
    // second child, which needs every left subtree's primitives below the right subtree's
    std::vector<uint32_t> firstPrim(node_count), lastPrim(node_count);
    bool dfsOrder = true;
    for (uint32_t i = node_count; i-- > 0;) {
        const uint32_t count = nodes[i].primitive_count_axis >> 16;
        if (!reach[i]) {
            firstPrim[i] = lastPrim[i] = 0;
        } else if (count) {
            firstPrim[i] = nodes[i].offset;
            lastPrim[i] = nodes[i].offset + count - 1;
        } else {
            const uint32_t a = i + 1, b = nodes[i].offset;
            firstPrim[i] = std::min(firstPrim[a], firstPrim[b]);
            lastPrim[i] = std::max(lastPrim[a], lastPrim[b]);
            if (!(lastPrim[a] < firstPrim[b])) dfsOrder = false;
        }
    }
    std::vector<float4> hc(4 * (size_t)std::max(interior, 1u), make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (uint32_t i = 0; cbOk && i < node_count; ++i) {
        if (rec[i] == 0xffffffffu || !reach[i]) continue;   // an unreachable record stays zero
        const pt_bvh_node& L = nodes[i + 1];
        const pt_bvh_node& R = nodes[nodes[i].offset];
        float4* q = &hc[4 * (size_t)rec[i]];
        q[0] = make_float4(L.aabb_min[0], L.aabb_max[0], L.aabb_min[1], L.aabb_max[1]);
        q[1] = make_float4(L.aabb_min[2], L.aabb_max[2], R.aabb_min[2], R.aabb_max[2]);
        q[2] = make_float4(R.aabb_min[0], R.aabb_max[0], R.aabb_min[1], R.aabb_max[1]);
        q[3] = make_float4(u2f(word(i + 1)), u2f(word(nodes[i].offset)), u2f(1u << ((nodes[i].primitive_count_axis >> 8) & 0xffu)),
                           u2f(firstPrim[nodes[i].offset]));
    }
    for (uint32_t i = 0; i < prim_count; ++i) pack_primitive(ctx, prims[i], &hp[4 * (size_t)i], &hm[3 * (size_t)i]);
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    (void)hipFree(ctx->nodes);
    (void)hipFree(ctx->prims);
    (void)hipFree(ctx->mats);
    (void)hipFree(ctx->cnodes);
    ctx->nodes = ctx->prims = ctx->mats = ctx->cnodes = nullptr;
    ctx->nodeCount = ctx->primCount = ctx->cnodeCount = 0;
    PT_HIP_CHECK(ctx, hipMalloc(&ctx->nodes, hn.size() * sizeof(float4)));
    PT_HIP_CHECK(ctx, hipMalloc(&ctx->prims, hp.size() * sizeof(float4)));
    PT_HIP_CHECK(ctx, hipMalloc(&ctx->mats, hm.size() * sizeof(float4)));
    PT_HIP_CHECK(ctx, hipMemcpy(ctx->nodes, hn.data(), hn.size() * sizeof(float4), hipMemcpyHostToDevice));
    PT_HIP_CHECK(ctx, hipMemcpy(ctx->prims, hp.data(), hp.size() * sizeof(float4), hipMemcpyHostToDevice));
    PT_HIP_CHECK(ctx, hipMemcpy(ctx->mats, hm.data(), hm.size() * sizeof(float4), hipMemcpyHostToDevice));
    if (cbOk) {
        PT_HIP_CHECK(ctx, hipMalloc(&ctx->cnodes, hc.size() * sizeof(float4)));
        PT_HIP_CHECK(ctx, hipMemcpy(ctx->cnodes, hc.data(), hc.size() * sizeof(float4), hipMemcpyHostToDevice));
        ctx->cnodeCount = interior;
    }
    ctx->dfsOrder = dfsOrder;
    if (motion_rows) {
        // (a failed upload leaves no table: the scene is changed by then, so the history must not survive it)
        (void)hipFree(ctx->motion);
        ctx->motion = nullptr;
        ctx->motionCount = 0;
        hipError_t e = hipMalloc(&ctx->motion, table.size() * sizeof(float4));
        if (e == hipSuccess) e = hipMemcpy(ctx->motion, table.data(), table.size() * sizeof(float4), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            scene_or_texture_changed(ctx->st);
            PT_HIP_CHECK(ctx, e);
        }
        ctx->motionCount = prim_count;
        scene_moved(ctx->st);
    } else {
        scene_or_texture_changed(ctx->st);
    }
    ctx->rootWord = word(0);
    for (int k = 0; k < 3; ++k) {
        ctx->rootBox[2 * k] = nodes[0].aabb_min[k];
        ctx->rootBox[2 * k + 1] = nodes[0].aabb_max[k];
    }
    ctx->nodeCount = node_count;
    ctx->primCount = prim_count;
    ctx->slabFast = slabFast;
    // LDS stack rows.  A lane visiting node v holds at most pend(v) pending entries: the ancestors
    // whose near child (trace.cu:69-76, by the sign of the ray direction along their split axis) is
    // on the path to v -- their far child is pushed (and repair_pending rebuilds exactly these).
    // The walks write one entry unconditionally above the top at an interior visit (walk_interior;
    // the node-at-a-time walks push there), so the rows needed are the maximum over the 8 direction
    // octants of pend(v) + 1 over interior v; pend(v) <= depth(v) - 1, the reference's bound.  pend is
    // carried down the same root DFS validate_scene runs (only reachable nodes; an orphan node that
    // names a reachable child cannot overwrite that child's value).
    {
        uint32_t need = 1;
        std::vector<std::pair<uint32_t, uint32_t>> st;
        for (uint32_t o = 0; o < 8; ++o) {
            st.assign(1, {0u, 0u});
            while (!st.empty()) {
                const auto [i, pend] = st.back();
                st.pop_back();
                const uint32_t pca = nodes[i].primitive_count_axis;
                if ((pca >> 16) != 0) continue;
                need = std::max(need, pend + 1u);
                const bool neg = (o >> ((pca >> 8) & 0xffu)) & 1u;
                const uint32_t a = i + 1, b = nodes[i].offset;
                st.push_back({neg ? b : a, pend + 1u});    // near child: its sibling is pending
                st.push_back({neg ? a : b, pend});
            }
        }
        ctx->stackDepth = std::min(need, maxDepth > 1 ? maxDepth - 1 : 1u);
    }
    return PT_OK;
}

PT_API int pt_set_scene(pt_context* ctx, const pt_bvh_node* nodes, uint32_t node_count, const pt_hittable* prims,
                        uint32_t prim_count)
{
    if (!ctx) return PT_ERR_ARG;
    return set_scene_impl(ctx, nodes, node_count, prims, prim_count, nullptr, nullptr);
}

PT_API int pt_set_scene_moved(pt_context* ctx, const pt_bvh_node* nodes, uint32_t node_count, const pt_hittable* prims,
                              uint32_t prim_count, const float* motion_rows, const uint32_t* prev_index)
{
    if (!ctx) return PT_ERR_ARG;
    if (!motion_rows || !prev_index) return fail(ctx, PT_ERR_ARG, "pt_set_scene_moved: motion_rows or prev_index is null");
    return set_scene_impl(ctx, nodes, node_count, prims, prim_count, motion_rows, prev_index);
}

PT_API int pt_holds_motion(const pt_context* ctx) { return ctx && holds_motion(ctx->st) ? 1 : 0; }

PT_API int pt_set_texture(pt_context* ctx, uint32_t handle, const float* rgba, uint32_t width, uint32_t height)
{
    if (!ctx) return PT_ERR_ARG;
    if (handle == 0 || handle > PT_MAX_TEXTURES || !rgba || width == 0 || height == 0)
        return fail(ctx, PT_ERR_ARG, "pt_set_texture: invalid argument");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    DevTex& t = ctx->hostTex[handle - 1];
    (void)hipFree((void*)t.texels);
    t = DevTex{};
    float4* mem = nullptr;
    const size_t bytes = (size_t)width * height * sizeof(float4);
    PT_HIP_CHECK(ctx, hipMalloc(&mem, bytes));
    PT_HIP_CHECK(ctx, hipMemcpy(mem, rgba, bytes, hipMemcpyHostToDevice));
    t.texels = mem;
    t.width = width;
    t.height = height;
    t.fwidth = (float)width;
    t.fheight = (float)height;
    scene_or_texture_changed(ctx->st);
    PT_HIP_CHECK(ctx, hipMemcpy(ctx->texTable, ctx->hostTex, sizeof(ctx->hostTex), hipMemcpyHostToDevice));
    return PT_OK;
}

PT_API int pt_set_skybox(pt_context* ctx, uint32_t handle)
{
    if (!ctx) return PT_ERR_ARG;
    if (handle > PT_MAX_TEXTURES) return fail(ctx, PT_ERR_ARG, "pt_set_skybox: invalid handle");
    sky_set(ctx->st, ctx->skybox, handle);
    ctx->skybox = handle;
    return PT_OK;
}

// Grow-only device buffers of the speculative groups; false if the device is out of memory (the
// launch then runs plain).
static bool ssg_reserve(pt_context* ctx, size_t tiles, size_t items, size_t samples, size_t patchSamples,
                        size_t bitsWords = 0)
{
    const size_t npix = (size_t)ctx->rows * ctx->width;
    auto fail_ = [] { (void)hipGetLastError(); return false; };
    if (!ctx->pairs) {
        if (hipMalloc(&ctx->pairs, 3 * npix * sizeof(float)) != hipSuccess ||
            hipMalloc(&ctx->fold, kFoldWords * npix * sizeof(uint32_t)) != hipSuccess ||
            hipMalloc(&ctx->deadCount, sizeof(uint32_t)) != hipSuccess ||
            hipMalloc(&ctx->patchCount, tiles * 64 * sizeof(uint32_t)) != hipSuccess)
            return fail_();
        // guess statistics until a pre-pass or fold measures them: 2 pairs per sample, odd-length
        // fraction unknown (< 0), variance 1
        if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ctx->pairs), 0x40000000, npix, ctx->stream) != hipSuccess ||
            hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ctx->pairs + npix), 0xbf800000, npix, ctx->stream) != hipSuccess ||
            hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ctx->pairs + 2 * npix), 0x3f800000, npix, ctx->stream) != hipSuccess)
            return fail_();
    }
    if (items > ctx->ssgItems) {
        (void)hipFree(ctx->ssgStart);
        (void)hipFree(ctx->ssgCount);
        ctx->ssgStart = nullptr;
        ctx->ssgCount = nullptr;
        ctx->ssgItems = 0;
        if (hipMalloc(&ctx->ssgStart, items * kStartWords * 64 * sizeof(uint32_t)) != hipSuccess ||
            hipMalloc(&ctx->ssgCount, items * 64 * sizeof(uint32_t)) != hipSuccess)
            return fail_();
        ctx->ssgItems = items;
    }
    if (bitsWords > ctx->ssgBitsWords) {           // [item][window words][64 lanes]
        (void)hipFree(ctx->ssgBits);
        ctx->ssgBits = nullptr;
        ctx->ssgBitsWords = 0;
        if (hipMalloc(&ctx->ssgBits, bitsWords * 64 * sizeof(unsigned long long)) != hipSuccess) return fail_();
        ctx->ssgBitsWords = bitsWords;
    }
    if (samples > ctx->ssgSamples) {
        (void)hipFree(ctx->ssgLog);
        (void)hipFree(ctx->ssgEnd);
        ctx->ssgLog = nullptr;
        ctx->ssgEnd = nullptr;
        ctx->ssgSamples = 0;
        if (hipMalloc(&ctx->ssgLog, samples * 64 * 3 * sizeof(float)) != hipSuccess ||
            hipMalloc(&ctx->ssgEnd, samples * 64 * sizeof(uint16_t)) != hipSuccess)
            return fail_();
        ctx->ssgSamples = samples;
    }
    if (patchSamples > ctx->patchSamples) {
        (void)hipFree(ctx->patchLog);
        (void)hipFree(ctx->patchEnd);
        ctx->patchLog = nullptr;
        ctx->patchEnd = nullptr;
        ctx->patchSamples = 0;
        if (hipMalloc(&ctx->patchLog, patchSamples * 64 * 3 * sizeof(float)) != hipSuccess ||
            hipMalloc(&ctx->patchEnd, patchSamples * 64 * sizeof(uint16_t)) != hipSuccess)
            return fail_();
        ctx->patchSamples = patchSamples;
    }
    return true;
}

// The sample-group logs of a context that launches plain again (up to ~15 GB at a 1080p rank share
// at N = 8) are released; the per-pixel statistics (pairs, fold state) stay for the next guesses.
static void ssg_release(pt_context* ctx)
{
    if (!ctx->ssgItems && !ctx->ssgSamples && !ctx->patchSamples && !ctx->ssgBitsWords) return;
    (void)hipStreamSynchronize(ctx->stream);
    for (void* q : {(void*)ctx->ssgStart, (void*)ctx->ssgCount, (void*)ctx->ssgBits, (void*)ctx->ssgLog,
                    (void*)ctx->ssgEnd, (void*)ctx->patchLog, (void*)ctx->patchEnd})
        (void)hipFree(q);
    ctx->ssgStart = nullptr;
    ctx->ssgCount = nullptr;
    ctx->ssgBits = nullptr;
    ctx->ssgLog = nullptr;
    ctx->ssgEnd = nullptr;
    ctx->patchLog = nullptr;
    ctx->patchEnd = nullptr;
    ctx->ssgItems = ctx->ssgSamples = ctx->patchSamples = ctx->ssgBitsWords = 0;
}

// Stable radix sort of (cost, tile) pairs, descending, into the dispatch order: deterministic, ties
// in tile order.
static int sort_order(pt_context* ctx, uint32_t tiles, uint64_t samples, uint32_t strip)
{
    size_t bytes = ctx->sortTempBytes;
    PT_HIP_CHECK(ctx, rocprim::radix_sort_pairs_desc(ctx->sortTemp, bytes, ctx->tileCost, ctx->sortKeys, ctx->tileIds,
                                                     ctx->order, tiles, 0, 32, ctx->stream));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    order_sorted(ctx->st, samples, strip);
    return PT_OK;
}

// Guess, grouped launch, fold, patch rounds and resume of speculative sample groups over the first
// `groupTiles` tiles of P.order (all tiles when P.order is null), on `s`.
static int run_groups(pt_context* ctx, int variant, const TraceParams& P0, uint32_t G, uint32_t groupTiles,
                      uint32_t ssgCap, hipStream_t s)
{
    TraceParams P = P0;
    const uint32_t total = P.spp * P.chunks;
    const uint32_t ssgN = total / G;
    const size_t items = (size_t)groupTiles * (2 * G - 1);
    const unsigned pixBlocks = (unsigned)(((size_t)groupTiles * 64 + 255) / 256);
    P.ssgG = G;
    P.ssgTiles = groupTiles;
    P.ssgCap = ssgCap;
    P.ssgLog = ctx->ssgLog;
    P.ssgEnd = ctx->ssgEnd;
    P.ssgStart = ctx->ssgStart;
    P.ssgBits = ctx->ssgBits;
    P.ssgCount = ctx->ssgCount;
    P.ssgWin = ssg_window_words(G, ssgN);
    P.fold = ctx->fold;
    P.numSlots = (uint32_t)items;
    ctx->groupStats[0] = G;
    PT_HIP_CHECK(ctx, hipMemsetAsync(ctx->ssgBits, 0, items * P.ssgWin * 64 * sizeof(unsigned long long), s));
    PT_HIP_CHECK(ctx, hipMemsetAsync(ctx->deadCount, 0, sizeof(uint32_t), s));
    ssg_guess_kernel<<<pixBlocks, 256, 0, s>>>(P, ctx->pairs, ssgN, ctx->ssgStart);
    PT_HIP_CHECK(ctx, hipGetLastError());
    P.ssgLook[0] = ctx->ssgLook[0];
    P.ssgLook[1] = ctx->ssgLook[1];
    PT_HIP_CHECK(ctx, launch_build<false, kModeGrouped>(variant, P, ctx->cus, s));
    ssg_fold_kernel<<<pixBlocks, 256, 0, s>>>(P, 0, ctx->patchLog, ctx->patchEnd, ctx->patchCount, ssgCap, ctx->pairs,
                                              ctx->deadCount);
    PT_HIP_CHECK(ctx, hipGetLastError());
    // Patch rounds: a carrier from each dead end (the exact state there) runs until it meets a
    // later group's parse, and the fold continues; what is left after them runs plain.
    TraceParams Q = P;
    Q.ssgPatch = 1;
    Q.ssgLog = ctx->patchLog;
    Q.ssgEnd = ctx->patchEnd;
    Q.ssgCount = ctx->patchCount;
    Q.numSlots = groupTiles;
    Q.tileCost = nullptr;
    uint32_t dead = 0;
    for (uint32_t r = 1;; ++r) {
        PT_HIP_CHECK(ctx, hipMemcpyAsync(&dead, ctx->deadCount, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        PT_HIP_CHECK(ctx, hipStreamSynchronize(s));
        if (r - 1 < 8) ctx->groupStats[2 + r - 1] = dead;
        if (dead == 0 || r > ctx->patchRounds) break;
        ctx->groupStats[1] = r;
        PT_HIP_CHECK(ctx, hipMemsetAsync(ctx->deadCount, 0, sizeof(uint32_t), s));
        PT_HIP_CHECK(ctx, launch_build<false, kModeGrouped>(variant, Q, ctx->cus, s));
        ssg_fold_kernel<<<pixBlocks, 256, 0, s>>>(P, r, ctx->patchLog, ctx->patchEnd, ctx->patchCount, ssgCap, ctx->pairs,
                                                  ctx->deadCount);
        PT_HIP_CHECK(ctx, hipGetLastError());
    }
    if (dead) {
        TraceParams R = P;
        R.ssgG = 0;
        R.numSlots = groupTiles;
        R.tileCost = nullptr;
        PT_HIP_CHECK(ctx, launch_build<false, kModeAux>(variant, R, ctx->cus, s));
    }
    return PT_OK;
}

// The launch parameters every trace launch of the context shares: buffers, scene, image, camera.
static void base_params(const pt_context* ctx, const pt_camera* cam, uint32_t spp, uint32_t chunks, int ignore,
                        TraceParams& P)
{
    memset(&P, 0, sizeof(P));
    P.accum = ctx->accum;
    P.rng = ctx->rng;
    P.nodes = ctx->nodes;
    P.prims = ctx->prims;
    P.mats = ctx->mats;
    P.textures = ctx->texTable;
    P.stats = ctx->stats;
    P.skybox = ctx->skybox;
    if (ctx->skybox != 0) P.skyTex = ctx->hostTex[ctx->skybox - 1];
    P.width = ctx->width;
    P.height = ctx->height;
    P.fwidth = (float)ctx->width;
    P.fheight = (float)ctx->height;
    P.rowOffset = ctx->rowOffset;
    P.rowStride = ctx->rowStride;
    P.rows = ctx->rows;
    P.bandShift = ctx->bandShift;
    P.spp = spp;
    P.chunks = chunks;
    P.ignoreFirst = ignore ? 1u : 0u;
    P.tilesX = (ctx->width + 7) / 8;
    P.tilesY = (ctx->rows + 7) / 8;
    P.cam.origin = hf3(cam->origin);
    P.cam.llc = hf3(cam->lower_left_corner);
    P.cam.horizontal = hf3(cam->horizontal);
    P.cam.vertical = hf3(cam->vertical);
    P.nodeCount = ctx->nodeCount;
    P.primCount = ctx->primCount;
    P.stackDepth = ctx->stackDepth;
    P.slabFast = ctx->slabFast ? 1u : 0u;
    P.cnodes = ctx->cnodes;
    P.cnodeCount = ctx->cnodeCount;
    P.rootWord = ctx->rootWord;
    for (int k = 0; k < 6; ++k) P.rootBox[k] = ctx->rootBox[k];
}

static SceneFacts scene_facts(const pt_context* ctx)
{
    return {{ctx->nodeCount, ctx->cnodeCount, ctx->primCount, ctx->stackDepth}, ctx->cnodes != nullptr, ctx->dfsOrder};
}

// The cursor of the persistent builds.
static int cursor_reserve(pt_context* ctx)
{
    if (ctx->tileCursor) return PT_OK;
    PT_HIP_CHECK(ctx, hipMalloc(&ctx->tileCursor, 2 * sizeof(uint32_t)));
    PT_HIP_CHECK(ctx, hipMemset(ctx->tileCursor, 0, 2 * sizeof(uint32_t)));
    return PT_OK;
}

// Tile scheduling: a pixel's samples are sequential (one XORWOW stream), so a tile is the
// smallest unit of work, and tiles differ several-fold in cost (sky vs geometry).  Every
// launch records each tile's cycle count; after a scene, texture or camera change the
// dispatch order is rebuilt on the device from the latest costs (most expensive first, a
// stable radix sort), so
// the launch tail consists of cheap tiles and the waves of a workgroup (which hold the
// group's LDS until the last one ends) have similar lengths.  A camera move keeps using the
// previous order for one launch.  The order changes which wave renders a tile, never how:
// results are identical.
// The buffers of that order for a frame of tilesX x tilesY tiles.
static int order_reserve(pt_context* ctx, uint32_t tilesX, uint32_t tilesY)
{
    const uint32_t tiles = tilesX * tilesY;
    if (ctx->orderTiles == tiles) return PT_OK;
    (void)hipFree(ctx->tileCost);
    (void)hipFree(ctx->order);
    (void)hipFree(ctx->tileIdle);
    ctx->tileCost = nullptr;
    ctx->order = nullptr;
    ctx->tileIdle = nullptr;
    ctx->orderTiles = 0;
    order_replaced(ctx->st);
    PT_HIP_CHECK(ctx, hipMalloc(&ctx->tileCost, (size_t)tiles * sizeof(uint32_t)));
    PT_HIP_CHECK(ctx, hipMalloc(&ctx->order, ((size_t)tiles + 64) * sizeof(uint32_t)));
    (void)hipFree(ctx->sortKeys);
    (void)hipFree(ctx->tileIds);
    (void)hipFree(ctx->sortTemp);
    ctx->sortKeys = ctx->tileIds = nullptr;
    ctx->sortTemp = nullptr;
    PT_HIP_CHECK(ctx, hipMalloc(&ctx->sortKeys, (size_t)tiles * sizeof(uint32_t)));
    PT_HIP_CHECK(ctx, hipMalloc(&ctx->tileIds, (size_t)tiles * sizeof(uint32_t)));
    ctx->sortTempBytes = 0;
    PT_HIP_CHECK(ctx, rocprim::radix_sort_pairs_desc(nullptr, ctx->sortTempBytes, ctx->tileCost, ctx->sortKeys,
                                                     ctx->tileIds, ctx->order, tiles, 0, 32, ctx->stream));
    PT_HIP_CHECK(ctx, hipMalloc(&ctx->sortTemp, ctx->sortTempBytes ? ctx->sortTempBytes : 4));
    PT_HIP_CHECK(ctx, hipMemsetAsync(ctx->tileCost, 0, (size_t)tiles * sizeof(uint32_t), ctx->stream));
    // tiles as packed coordinates (tileY << 16 | tileX: the kernel needs no division by tilesX);
    // slots past the last tile stay invalid (tileY = tilesY)
    std::vector<uint32_t> ident((size_t)tiles + 64);
    for (size_t i = 0; i < ident.size(); ++i)
        ident[i] = i < tiles ? ((uint32_t)(i / tilesX) << 16) | (uint32_t)(i % tilesX) : tilesY << 16;
    (void)hipFree(ctx->rowMajor);
    ctx->rowMajor = nullptr;
    PT_HIP_CHECK(ctx, hipMalloc(&ctx->rowMajor, ident.size() * sizeof(uint32_t)));
    PT_HIP_CHECK(ctx, hipMemcpy(ctx->rowMajor, ident.data(), ident.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    PT_HIP_CHECK(ctx, hipMemcpy(ctx->order, ident.data(), ident.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    PT_HIP_CHECK(ctx, hipMemcpy(ctx->tileIds, ident.data(), (size_t)tiles * sizeof(uint32_t), hipMemcpyHostToDevice));
    ctx->orderTiles = tiles;
    return PT_OK;
}

// The row-major order of strip units of K tiles (packed first tiles), kept for the last K.
static int units_reserve(pt_context* ctx, uint32_t K, uint32_t tilesX, uint32_t tilesY)
{
    const uint32_t tiles = tilesX * tilesY, unitsX = (tilesX + K - 1) / K, units = unitsX * tilesY;
    if (ctx->unitK == K && ctx->unitTiles == tiles) return PT_OK;
    (void)hipFree(ctx->unitMajor);
    ctx->unitMajor = nullptr;
    std::vector<uint32_t> um((size_t)units + 64);
    for (size_t i = 0; i < um.size(); ++i)
        um[i] = i < units ? ((uint32_t)(i / unitsX) << 16) | (uint32_t)(i % unitsX * K) : tilesY << 16;
    PT_HIP_CHECK(ctx, hipMalloc(&ctx->unitMajor, um.size() * sizeof(uint32_t)));
    PT_HIP_CHECK(ctx, hipMemcpy(ctx->unitMajor, um.data(), um.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    ctx->unitK = K;
    ctx->unitTiles = tiles;
    return PT_OK;
}

static void set_priority(TraceParams& P, const PassPriority& pp)
{
    for (int i = 0; i < 3; ++i) P.prio[i] = pp.prio[i];
    P.prioDealt = pp.dealt ? 1u : 0u;
}

// Execute a plan (pt_launch_plan.h): the buffers it needs, the cold-start pass, the main pass, the
// order's rebuild.  P holds base_params.
static int run_plan(pt_context* ctx, const LaunchInputs& in, LaunchPlan plan, TraceParams P, float* gpu_ms,
                    pt_render_stats* stats)
{
    if (plan.dropOrder) order_dropped(ctx->st);
    if (plan.refusal) return fail(ctx, PT_ERR_STATE, plan.refusal);
    const uint32_t tiles = P.tilesX * P.tilesY, K = plan.K, total = P.spp * P.chunks, chunks = P.chunks;
    const bool sorted = ctx->knobs.schedule == 0;
    if (K > 1) {
        const int rc = units_reserve(ctx, K, P.tilesX, P.tilesY);
        if (rc != PT_OK) return rc;
    }
    uint32_t* const firstOrder = K > 1 ? ctx->unitMajor : ctx->rowMajor;
    P.strip = K;
    P.tileCost = sorted ? ctx->tileCost : nullptr;
    P.scatterWaves = ctx->knobs.schedule == 2 ? (uint32_t)(((size_t)ctx->rows * ctx->width + 63) / 64) : 0u;
    P.tileCursor = ctx->tileCursor;
    P.numSlots = plan.units;
    P.occCap = ctx->occupancy;
    if (ctx->traceTiles && stats && P.tileCost) {
        if (ctx->tileTrace && ctx->traceCap < tiles) {
            (void)hipFree(ctx->tileTrace);
            ctx->tileTrace = nullptr;
        }
        if (!ctx->tileTrace) {
            PT_HIP_CHECK(ctx, hipMalloc(&ctx->tileTrace, 2 * (size_t)tiles * sizeof(uint32_t)));
            ctx->traceCap = tiles;
        }
        P.tileTrace = ctx->tileTrace;
    }
    if (stats) {
        PT_HIP_CHECK(ctx, hipMemsetAsync(ctx->stats, 0, kStatWords * sizeof(unsigned long long), ctx->stream));
        if (!ctx->tileIdle) PT_HIP_CHECK(ctx, hipMalloc(&ctx->tileIdle, (size_t)tiles * sizeof(uint32_t)));
        PT_HIP_CHECK(ctx, hipMemsetAsync(ctx->tileIdle, 0, (size_t)tiles * sizeof(uint32_t), ctx->stream));
        P.tileIdle = ctx->tileIdle;
    }
    if (plan.aheadUse || plan.aheadMake) {
        if (!ctx->ahead) {
            const size_t n = std::max<size_t>((size_t)ctx->rows * ctx->width, 1);
            PT_HIP_CHECK(ctx, hipMalloc(&ctx->ahead, kAheadWords * n * sizeof(uint32_t)));
        }
        P.ahead = ctx->ahead;
        P.aheadUse = plan.aheadUse ? 1u : 0u;
        P.aheadMake = plan.aheadMake ? 1u : 0u;
    }
    ctx->lastGroups = 0;
    ctx->lastVariant = plan.build;
    memset(ctx->groupStats, 0, sizeof(ctx->groupStats));
    accum_written(ctx->st);
    if (plan.G) {
        const size_t J = 2 * (size_t)plan.G - 1;
        if (!ssg_reserve(ctx, tiles, (size_t)tiles * J, (size_t)tiles * J * plan.ssgCap, (size_t)tiles * plan.ssgCap,
                         (size_t)tiles * J * ssg_window_words(plan.G, total / plan.G))) {
            plan.G = plan.ssgCap = 0;             // out of memory: a plain launch of the planned build
            plan_passes(in, plan);
        }
    }
    // a plain launch after grouped ones releases the group logs (a stream synchronisation and frees
    // of up to ~15 GB): before the timed region starts
    if (!plan.G) ssg_release(ctx);
    PT_HIP_CHECK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    if (plan.cold != ColdStart::None) {
        TraceParams Q = P;
        Q.chunks = 1;
        Q.order = firstOrder;                            // (a cold start is a sorted schedule's)
        set_priority(Q, plan.coldPrio);
        if (plan.cold == ColdStart::SplitCall) {
            P.chunks = chunks - 1;
            P.ignoreFirst = 0;                               // the first call is done
        } else {
            Q.spp = plan.coldSpp;
            Q.ignoreFirst = 1;
            Q.discard = 1;
            Q.pairsOut = plan.coldPairs && ssg_reserve(ctx, tiles, 0, 0, 0) ? ctx->pairs : nullptr;
        }
        PT_HIP_CHECK(ctx, Q.pairsOut ? launch_build<false, kModeAux>(plan.build, Q, ctx->cus, ctx->stream)
                          : K > 1    ? launch_resumable(plan.build, kModeStrip, Q, ctx->cus, ctx->stream)
                                     : launch_build<false, kModePlain>(plan.build, Q, ctx->cus, ctx->stream));
        const int rs = sort_order(ctx, tiles, plan.coldSpp, K);
        if (rs != PT_OK) return rs;
    }
    P.order = P.scatterWaves ? nullptr : (plan.costOrder ? ctx->order : firstOrder);   // scattered mapping: slot = wave index
    set_priority(P, plan.mainPrio);
    if (plan.G) {
        if (P.tileCost) PT_HIP_CHECK(ctx, hipMemsetAsync(P.tileCost, 0, (size_t)tiles * sizeof(uint32_t), ctx->stream));
        const int rc = run_groups(ctx, plan.build, P, plan.G, tiles, plan.ssgCap, ctx->stream);
        if (rc != PT_OK) return rc;
        ctx->lastGroups = plan.G;
    } else {
        // (90 and 91 have no instrumented build: their counters read zero)
        const bool counted = stats && build_has(plan.build, kInstrumented);
        PT_HIP_CHECK(ctx, plan.mode == LaunchMode::Ahead   ? launch_resumable(plan.build, kModeAhead, P, ctx->cus, ctx->stream)
                          : plan.mode == LaunchMode::Strip ? launch_resumable(plan.build, kModeStrip, P, ctx->cus, ctx->stream)
                          : counted                        ? launch_build<true, kModePlain>(plan.build, P, ctx->cus, ctx->stream)
                                                           : launch_build<false, kModePlain>(plan.build, P, ctx->cus, ctx->stream));
    }
    memcpy(ctx->lastLaunch, g_lastLaunch, sizeof(ctx->lastLaunch));
    if (plan.aheadMake) stash_made(ctx->st);
    PT_HIP_CHECK(ctx, hipGetLastError());
    PT_HIP_CHECK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    PT_HIP_CHECK(ctx, hipEventSynchronize(ctx->ev1));
    float ms = 0.0f;
    PT_HIP_CHECK(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    if (gpu_ms) *gpu_ms = ms;
    if (plan.rebuildOrder) {
        const int rs = sort_order(ctx, tiles, total, K);
        if (rs != PT_OK) return rs;
        if (plan.biasedOrder) order_biased(ctx->st);
    }
    if (stats) {
        static_assert(sizeof(pt_render_stats) == kStatWords * sizeof(uint64_t), "the counters in the order of pt_render_stats");
        PT_HIP_CHECK(ctx, hipMemcpy(stats, ctx->stats, sizeof(*stats), hipMemcpyDeviceToHost));
    }
    return PT_OK;
}

// A render: validate, make sure the buffers exist, describe the launch, plan it, execute the plan.
static int render_impl(pt_context* ctx, const pt_camera* cam, uint32_t spp, uint32_t chunks, int ignore, float* gpu_ms,
                       pt_render_stats* stats)
{
    if (!ctx || !cam) return PT_ERR_ARG;
    if (gpu_ms) *gpu_ms = 0.0f;
    if (stats) memset(stats, 0, sizeof(*stats));
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (ctx->nodeCount < 1 || ctx->primCount < 1 || spp == 0 || chunks == 0 || ctx->rows == 0) return PT_OK;
    // textures referenced by the launch must exist (the reference would read an invalid object)
    if (ctx->skybox != 0 && ctx->hostTex[ctx->skybox - 1].texels == nullptr)
        return fail(ctx, PT_ERR_STATE, "pt_render: skybox handle has no texture");
    TraceParams P;
    base_params(ctx, cam, spp, chunks, ignore, P);
    const RenderStart begun = render_begins(ctx->st, *cam);
    int rc = order_reserve(ctx, P.tilesX, P.tilesY);
    if (rc == PT_OK) rc = cursor_reserve(ctx);
    if (rc != PT_OK) return rc;
    LaunchInputs in = {};
    in.cus = (uint32_t)ctx->cus;
    in.tilesX = P.tilesX;
    in.tilesY = P.tilesY;
    in.spp = spp;
    in.chunks = chunks;
    in.instrumented = stats != nullptr;
    in.scene = scene_facts(ctx);
    in.knobs = ctx->knobs;
    in.order = ctx->st.order;
    in.stashMatches = begun.stashMatches;
    in.aheadMisses = begun.aheadMisses;
    return run_plan(ctx, in, plan_launch(in), P, gpu_ms, stats);
}

PT_API int pt_set_cold_start(pt_context* ctx, uint32_t prepass_spp, int priority)
{
    if (!ctx || prepass_spp > 64 || priority < 0 || priority > 1) return PT_ERR_ARG;
    ctx->knobs.prepassSpp = prepass_spp;
    ctx->knobs.coldPriority = priority != 0;
    return PT_OK;
}

PT_API int pt_set_run_ahead(pt_context* ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 3) return PT_ERR_ARG;
    ctx->knobs.aheadMode = mode;
    return PT_OK;
}

PT_API int pt_set_rise_repair(pt_context* ctx, int enabled)
{
    if (!ctx || enabled < 0 || enabled > 1) return PT_ERR_ARG;
    ctx->knobs.riseRepair = enabled != 0;
    return PT_OK;
}

PT_API int pt_set_zero_quadric_consts(pt_context* ctx, int type)
{
    if (!ctx || type < -1 || type > 6) return PT_ERR_ARG;
    ctx->zeroConstsType = type;
    return PT_OK;
}

PT_API int pt_set_strip_units(pt_context* ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 16) return PT_ERR_ARG;
    ctx->knobs.stripMode = mode;
    return PT_OK;
}

PT_API int pt_set_sample_groups(pt_context* ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 4096) return PT_ERR_ARG;
    ctx->knobs.ssgMode = mode;
    return PT_OK;
}

PT_API int pt_set_group_lookback(pt_context* ctx, uint32_t far, uint32_t near)
{
    if (!ctx || far > 256 || near > 256) return PT_ERR_ARG;
    ctx->ssgLook[0] = far;
    ctx->ssgLook[1] = near;
    return PT_OK;
}

PT_API int pt_set_patch_rounds(pt_context* ctx, uint32_t rounds)
{
    if (!ctx || rounds > 64) return PT_ERR_ARG;
    ctx->patchRounds = rounds;
    return PT_OK;
}

PT_API int pt_last_sample_groups(const pt_context* ctx)
{
    return ctx ? (int)ctx->lastGroups : 0;
}

PT_API int pt_last_variant(const pt_context* ctx) { return ctx ? ctx->lastVariant : 0; }

PT_API int pt_last_launch(const pt_context* ctx, uint32_t* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    memcpy(dst, ctx->lastLaunch, sizeof(ctx->lastLaunch));
    return PT_OK;
}


PT_API int pt_read_group_log_counts(pt_context* ctx, uint32_t* dst, size_t count)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!ctx->ssgCount || ctx->lastGroups == 0) return PT_ERR_STATE;
    const size_t tiles = (size_t)((ctx->width + 7) / 8) * ((ctx->rows + 7) / 8);
    const size_t n = tiles * (2 * ctx->lastGroups - 1) * 64;
    if (count < n) return PT_ERR_ARG;
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PT_HIP_CHECK(ctx, hipMemcpy(dst, ctx->ssgCount, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return PT_OK;
}

PT_API int pt_read_group_fold(pt_context* ctx, uint32_t word, uint32_t* dst)
{
    if (!ctx || !dst || word >= kFoldWords + 3) return PT_ERR_ARG;
    if (!ctx->fold) return PT_ERR_STATE;
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    const void* src = word >= kFoldWords ? (const void*)(ctx->pairs + (word - kFoldWords) * npix)
                                         : (const void*)(ctx->fold + (size_t)word * npix);
    PT_HIP_CHECK(ctx, hipMemcpy(dst, src, npix * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return PT_OK;
}

PT_API int pt_read_group_stats(const pt_context* ctx, uint32_t* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    memcpy(dst, ctx->groupStats, sizeof(ctx->groupStats));
    return PT_OK;
}

PT_API int pt_set_issue_priority(pt_context* ctx, int mode, uint32_t level3, uint32_t level2, uint32_t level1)
{
    if (!ctx || mode < 0 || mode > 2 || (mode == 2 && !(level3 <= level2 && level2 <= level1))) return PT_ERR_ARG;
    ctx->knobs.prioMode = mode;
    ctx->knobs.prioBounds[0] = level3;
    ctx->knobs.prioBounds[1] = level2;
    ctx->knobs.prioBounds[2] = level1;
    return PT_OK;
}

PT_API int pt_set_occupancy(pt_context* ctx, uint32_t workgroups_per_cu)
{
    if (!ctx || workgroups_per_cu > 16) return PT_ERR_ARG;
    ctx->occupancy = workgroups_per_cu;
    return PT_OK;
}

PT_API int pt_set_schedule(pt_context* ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 2) return PT_ERR_ARG;
    ctx->knobs.schedule = mode;
    schedule_changed(ctx->st);
    return PT_OK;
}

PT_API int pt_render(pt_context* ctx, const pt_camera* camera, uint32_t spp, uint32_t chunks, int ignore_history,
                     float* gpu_ms)
{
    return render_impl(ctx, camera, spp, chunks, ignore_history, gpu_ms, nullptr);
}

PT_API int pt_render_instrumented(pt_context* ctx, const pt_camera* camera, uint32_t spp, uint32_t chunks, int ignore_history,
                           float* gpu_ms, pt_render_stats* stats)
{
    if (!stats) return PT_ERR_ARG;
    return render_impl(ctx, camera, spp, chunks, ignore_history, gpu_ms, stats);
}

// Buffers of the adaptive path, allocated by the first adaptive render of the context.
static int adaptive_reserve(pt_context* ctx, uint32_t tiles)
{
    if (ctx->adMom) return PT_OK;
    const size_t npix = (size_t)ctx->rows * ctx->width;
    PT_HIP_CHECK(ctx, hipMalloc(&ctx->adMom, 3 * npix * sizeof(uint32_t)));
    PT_HIP_CHECK(ctx, hipMalloc(&ctx->adFlag, npix));
    PT_HIP_CHECK(ctx, hipMalloc(&ctx->adList, npix * sizeof(uint32_t)));
    PT_HIP_CHECK(ctx, hipMalloc(&ctx->adMasks, (size_t)tiles * sizeof(unsigned long long)));
    PT_HIP_CHECK(ctx, hipMalloc(&ctx->adCounts, ((size_t)tiles + 1) * sizeof(uint32_t)));
    PT_HIP_CHECK(ctx, hipMalloc(&ctx->adOffsets, ((size_t)tiles + 1) * sizeof(uint32_t)));
    PT_HIP_CHECK(ctx, hipMemsetAsync(ctx->adCounts, 0, ((size_t)tiles + 1) * sizeof(uint32_t), ctx->stream));
    ctx->adTempBytes = 0;
    PT_HIP_CHECK(ctx, rocprim::exclusive_scan(nullptr, ctx->adTempBytes, ctx->adCounts, ctx->adOffsets, 0u, (size_t)tiles + 1,
                                              rocprim::plus<uint32_t>(), ctx->stream));
    PT_HIP_CHECK(ctx, hipMalloc(&ctx->adTemp, ctx->adTempBytes ? ctx->adTempBytes : 4));
    return PT_OK;
}

// Evaluate every pixel and compact the active ones into ctx->adList; the count is the one readback.
static int adaptive_compact(pt_context* ctx, const pt_adaptive_params& ap, bool all, uint32_t tilesX, uint32_t tiles,
                            uint32_t* count)
{
    const size_t npix = (size_t)ctx->rows * ctx->width;
    hipStream_t s = ctx->stream;
    if (!all) {
        adapt_flag_kernel<<<(unsigned)((npix + 255) / 256), 256, 0, s>>>(ctx->adMom, ctx->adFlag, npix, ap.tolerance, ap.floor,
                                                                         ap.min_calls);
        PT_HIP_CHECK(ctx, hipGetLastError());
    }
    const unsigned tileBlocks = (tiles + 3) / 4;
    adapt_mark_kernel<<<tileBlocks, 256, 0, s>>>(ctx->adFlag, ctx->adMom + 2 * npix, ctx->width, ctx->rows, tilesX, tiles,
                                                 ap.min_calls, ap.max_calls, all ? 1u : 0u, ctx->adMasks, ctx->adCounts);
    PT_HIP_CHECK(ctx, hipGetLastError());
    size_t bytes = ctx->adTempBytes;
    PT_HIP_CHECK(ctx, rocprim::exclusive_scan(ctx->adTemp, bytes, ctx->adCounts, ctx->adOffsets, 0u, (size_t)tiles + 1,
                                              rocprim::plus<uint32_t>(), s));
    adapt_scatter_kernel<<<tileBlocks, 256, 0, s>>>(ctx->adMasks, ctx->adOffsets, ctx->adList, ctx->width, tilesX, tiles);
    PT_HIP_CHECK(ctx, hipGetLastError());
    PT_HIP_CHECK(ctx, hipMemcpyAsync(count, ctx->adOffsets + tiles, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(s));
    return PT_OK;
}

PT_API int pt_render_adaptive(pt_context* ctx, const pt_camera* camera, const pt_adaptive_params* params,
                              pt_adaptive_result* result)
{
    if (!ctx) return PT_ERR_ARG;
    if (result) memset(result, 0, sizeof(*result));
    if (!camera || !params) return fail(ctx, PT_ERR_ARG, "pt_render_adaptive: null argument");
    const pt_adaptive_params ap = *params;
    if (ap.spp == 0 || ap.min_calls < 2 || ap.max_calls < ap.min_calls || !(ap.tolerance >= 0.0f) || !(ap.floor >= 0.0f))
        return fail(ctx, PT_ERR_ARG, "pt_render_adaptive: needs spp >= 1, 2 <= min_calls <= max_calls, tolerance >= 0, floor >= 0");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (ctx->nodeCount < 1 || ctx->primCount < 1) return fail(ctx, PT_ERR_STATE, "pt_render_adaptive: no scene set");
    if (ctx->skybox != 0 && ctx->hostTex[ctx->skybox - 1].texels == nullptr)
        return fail(ctx, PT_ERR_STATE, "pt_render_adaptive: skybox handle has no texture");
    if (!ap.reset && !moments_continue(ctx->st))
        return fail(ctx, PT_ERR_STATE, "pt_render_adaptive: reset = 0 needs the moments of an adaptive render; there has been "
                                       "none since the last plain render, RNG write or scene, texture or sky change");
    const int variant = picked_build(ctx->knobs.variant, scene_facts(ctx));
    if (!build_has(variant, mode_bit(false, kModeAdaptive)))
        return fail(ctx, PT_ERR_ARG, "pt_render_adaptive: the kernel variant set has no adaptive build (0, 4, 6, 40, 41, 46, 60, 61 have)");
    if (ctx->rows == 0) return PT_OK;
    const uint32_t tilesX = (ctx->width + 7) / 8, tiles = tilesX * ((ctx->rows + 7) / 8);
    const int rr = adaptive_reserve(ctx, tiles);
    if (rr != PT_OK) return rr;
    const int cr = cursor_reserve(ctx);
    if (cr != PT_OK) return cr;
    TraceParams P;
    base_params(ctx, camera, ap.spp, 1, 0, P);
    P.tileCursor = ctx->tileCursor;
    P.occCap = ctx->occupancy;
    P.adList = ctx->adList;
    P.adMom = ctx->adMom;
    adaptive_begins(ctx->st);
    ctx->lastGroups = 0;
    ctx->lastVariant = variant;
    PT_HIP_CHECK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    uint32_t rounds = 0, count = 0;
    uint64_t samples = 0;
    if (ap.reset) {
        // every pixel is active for its first min_calls calls: one fused launch, the first call
        // overwriting the accumulation value (ignoreHistory) and starting from zero moments
        const int rc = adaptive_compact(ctx, ap, true, tilesX, tiles, &count);
        if (rc != PT_OK) return rc;
        P.adCount = count;
        P.numSlots = (count + 63) / 64;
        P.chunks = ap.min_calls;
        P.ignoreFirst = 1;
        PT_HIP_CHECK(ctx, launch_resumable(variant, kModeAdaptive, P, ctx->cus, ctx->stream));
        rounds = 1;
        ctx->adSteps = ap.min_calls;
        samples = (uint64_t)count * ap.min_calls * ap.spp;
        P.chunks = 1;
        P.ignoreFirst = 0;
    }
    // one step per launch, at most max_calls steps since the reset: a pixel that stopped and started
    // again ends below max_calls, and the render's length is bounded by its budget
    while (ctx->adSteps < ap.max_calls) {
        const int rc = adaptive_compact(ctx, ap, false, tilesX, tiles, &count);
        if (rc != PT_OK) return rc;
        if (count == 0) break;            // nothing active: no launch
        P.adCount = count;
        P.numSlots = (count + 63) / 64;
        PT_HIP_CHECK(ctx, launch_resumable(variant, kModeAdaptive, P, ctx->cus, ctx->stream));
        ++rounds;
        ++ctx->adSteps;
        samples += (uint64_t)count * ap.spp;
    }
    memcpy(ctx->lastLaunch, g_lastLaunch, sizeof(ctx->lastLaunch));
    PT_HIP_CHECK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    PT_HIP_CHECK(ctx, hipEventSynchronize(ctx->ev1));
    float ms = 0.0f;
    PT_HIP_CHECK(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    adaptive_done(ctx->st);
    if (result) {
        result->rounds = rounds;
        result->samples = samples;
        result->gpu_ms = ms;
    }
    return PT_OK;
}

PT_API int pt_holds_adaptive(const pt_context* ctx) { return ctx && counts_describe_buffer(ctx->st) ? 1 : 0; }

PT_API int pt_read_moments(pt_context* ctx, float* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!counts_describe_buffer(ctx->st)) return fail(ctx, PT_ERR_STATE, "pt_read_moments: no adaptive render describes the buffer");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    std::vector<uint32_t> soa(3 * npix);
    PT_HIP_CHECK(ctx, hipMemcpy(soa.data(), ctx->adMom, soa.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < npix; ++i)
        for (int k = 0; k < 3; ++k) dst[3 * i + k] = u2f(soa[k * npix + i]);
    return PT_OK;
}

PT_API int pt_read_adaptive_hdr(pt_context* ctx, float* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!counts_describe_buffer(ctx->st)) return fail(ctx, PT_ERR_STATE, "pt_read_adaptive_hdr: no adaptive render describes the buffer");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    std::vector<uint32_t> calls(npix);
    PT_HIP_CHECK(ctx, hipMemcpy(dst, ctx->accum, npix * sizeof(float4), hipMemcpyDeviceToHost));
    PT_HIP_CHECK(ctx, hipMemcpy(calls.data(), ctx->adMom + 2 * npix, npix * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < npix; ++i) {
        const float n = (float)std::max(calls[i], 1u);
        for (int k = 0; k < 4; ++k) dst[4 * i + k] = dst[4 * i + k] / n;
    }
    return PT_OK;
}

PT_API int pt_tonemap_adaptive(pt_context* ctx, uint8_t* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!counts_describe_buffer(ctx->st)) return fail(ctx, PT_ERR_STATE, "pt_tonemap_adaptive: no adaptive render describes the buffer");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    if (npix == 0) return PT_OK;
    if (!ctx->ldr) PT_HIP_CHECK(ctx, hipMalloc(&ctx->ldr, npix * sizeof(uchar4)));
    tonemap_adaptive_kernel<<<(unsigned)((npix + 255) / 256), 256, 0, ctx->stream>>>(ctx->ldr, ctx->accum,
                                                                                      ctx->adMom + 2 * npix, npix);
    PT_HIP_CHECK(ctx, hipGetLastError());
    PT_HIP_CHECK(ctx, hipMemcpyAsync(dst, ctx->ldr, npix * sizeof(uchar4), hipMemcpyDeviceToHost, ctx->stream));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return PT_OK;
}

PT_API int pt_read_accum(pt_context* ctx, float* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    PT_HIP_CHECK(ctx, hipMemcpy(dst, ctx->accum, (size_t)ctx->rows * ctx->width * sizeof(float4), hipMemcpyDeviceToHost));
    return PT_OK;
}

PT_API int pt_copy_accum_device(pt_context* ctx, void* dst_device, size_t bytes)
{
    if (!ctx || !dst_device) return PT_ERR_ARG;
    const size_t need = (size_t)ctx->rows * ctx->width * sizeof(float4);
    if (bytes < need) return fail(ctx, PT_ERR_ARG, "pt_copy_accum_device: destination too small");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PT_HIP_CHECK(ctx, hipMemcpyAsync(dst_device, ctx->accum, need, hipMemcpyDeviceToDevice, ctx->stream));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return PT_OK;
}

PT_API int pt_tonemap_device(pt_context* ctx, uint32_t frames, void* dst, size_t dst_bytes)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    const size_t npix = (size_t)ctx->rows * ctx->width;
    if (dst_bytes < npix * sizeof(uchar4)) return fail(ctx, PT_ERR_ARG, "pt_tonemap_device: destination too small");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (npix == 0) return PT_OK;
    tonemap_kernel<<<(unsigned)((npix + 255) / 256), 256, 0, ctx->stream>>>(static_cast<uchar4*>(dst), ctx->accum, npix,
                                                                             frames);
    PT_HIP_CHECK(ctx, hipGetLastError());
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return PT_OK;
}

PT_API int pt_tonemap(pt_context* ctx, uint32_t frames, uint8_t* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    if (npix == 0) return PT_OK;
    if (!ctx->ldr) PT_HIP_CHECK(ctx, hipMalloc(&ctx->ldr, npix * sizeof(uchar4)));   // kept for per-frame use
    tonemap_kernel<<<(unsigned)((npix + 255) / 256), 256, 0, ctx->stream>>>(ctx->ldr, ctx->accum, npix, frames);
    PT_HIP_CHECK(ctx, hipGetLastError());
    PT_HIP_CHECK(ctx, hipMemcpyAsync(dst, ctx->ldr, npix * sizeof(uchar4), hipMemcpyDeviceToHost, ctx->stream));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return PT_OK;
}

PT_API int pt_read_rng(pt_context* ctx, uint32_t* dst)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    std::vector<uint32_t> soa(6 * npix);
    PT_HIP_CHECK(ctx, hipMemcpy(soa.data(), ctx->rng, soa.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < npix; ++i)
        for (int k = 0; k < 6; ++k) dst[6 * i + k] = soa[k * npix + i];
    return PT_OK;
}

PT_API int pt_write_rng(pt_context* ctx, const uint32_t* src)
{
    if (!ctx || !src) return PT_ERR_ARG;
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const size_t npix = (size_t)ctx->rows * ctx->width;
    std::vector<uint32_t> soa(6 * npix);
    for (size_t i = 0; i < npix; ++i)
        for (int k = 0; k < 6; ++k) soa[k * npix + i] = src[6 * i + k];
    PT_HIP_CHECK(ctx, hipMemcpy(ctx->rng, soa.data(), soa.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    rng_written(ctx->st);
    return PT_OK;
}

PT_API uint32_t pt_local_rows(const pt_context* ctx) { return ctx ? ctx->rows : 0; }

PT_API int pt_read_tile_costs(pt_context* ctx, uint32_t* dst, uint32_t count)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!ctx->tileCost || count != ctx->orderTiles) return fail(ctx, PT_ERR_STATE, "pt_read_tile_costs: no costs of that size");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    PT_HIP_CHECK(ctx, hipMemcpy(dst, ctx->tileCost, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return PT_OK;
}

PT_API int pt_read_tile_idle(pt_context* ctx, uint32_t* dst, uint32_t count)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!ctx->tileIdle || count != ctx->orderTiles) return fail(ctx, PT_ERR_STATE, "pt_read_tile_idle: no instrumented launch of that size");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    PT_HIP_CHECK(ctx, hipMemcpy(dst, ctx->tileIdle, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return PT_OK;
}

PT_API int pt_set_tile_trace(pt_context* ctx, int enabled)
{
    if (!ctx) return PT_ERR_ARG;
    ctx->traceTiles = enabled != 0;
    return PT_OK;
}

PT_API int pt_read_tile_trace(pt_context* ctx, uint32_t* dst, uint32_t count)
{
    if (!ctx || !dst) return PT_ERR_ARG;
    if (!ctx->tileTrace || count != 2 * ctx->orderTiles || ctx->traceCap < ctx->orderTiles)
        return fail(ctx, PT_ERR_STATE, "pt_read_tile_trace: no traced launch of that size");
    PT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    PT_HIP_CHECK(ctx, hipMemcpy(dst, ctx->tileTrace, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return PT_OK;
}

PT_API int pt_set_kernel_variant(pt_context* ctx, int variant)
{
    if (!ctx) return PT_ERR_ARG;
    if (variant != 0 && !build_settable(variant)) return fail(ctx, PT_ERR_ARG, "pt_set_kernel_variant: not a shipped variant");
    ctx->knobs.variant = variant;
    return PT_OK;
}

} // extern "C"

#include "pt_denoise.h"

#include "pt_temporal.h"

#include "pt_svgf.h"

#include "pt_adaptive_variance.h"

#include "pt_despike.h"

#include "pt_upsample.h"

#include "pt_upsample_resolve.h"

#include "pt_refit.h"

extern "C" PT_API const char* pt_last_error(const pt_context* ctx)
{
    if (ctx) return ctx->err.c_str();
    return g_freeError.empty() ? "null context" : g_freeError.c_str();
}

#include "pt_group.h"
