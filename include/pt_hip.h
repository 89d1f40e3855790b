/*
 * pt_hip.h -- C ABI of the MI355X (gfx950) path-tracing device layer, libpt_hip.so.
 *
 * This is the drop-in boundary below the reference's `Pathtracer` class: it replaces the CUDA
 * resource management and kernel launches of PathtracerCUDA/src/pathtracer/Pathtracer.cpp and the
 * three kernels of src/pathtracer/kernels/ (trace.cu, initRandState.cu, tonemap.cu).  Plain C:
 * POD structs, pointers and sizes only; no C++ or torch types.  The host C++ layer
 * (include/pt_host.h, libpt_host.so) owns scene loading, the SAH BVH build and the frame counter,
 * exactly as the reference's host code does, and calls down into these entry points.
 *
 * Every call returns PT_OK (0) or a PT_ERR_* code; pt_last_error() gives the message.  All calls
 * on one context must come from one host thread (reference: single thread, Pathtracer.cpp:40).
 */
#ifndef PT_HIP_H
#define PT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_API __attribute__((visibility("default")))

enum {
    PT_OK = 0,
    PT_ERR_HIP = 1,        /* a HIP runtime call failed (reference: checkCudaErrors -> exit) */
    PT_ERR_ARG = 2,        /* invalid argument */
    PT_ERR_STATE = 3,      /* call not valid in the current state */
    PT_ERR_DEPTH = 4,      /* BVH deeper than the 32-entry traversal stack (trace.cu:39) allows */
    PT_ERR_NO_DEVICE = 5   /* no GPU visible */
};

#define PT_MAX_TEXTURES 64 /* Pathtracer.cpp:15 MAX_TEXTURE_COUNT */

/* Camera (reference Camera.h:14-22, 92 B, passed by value to traceKernel, trace.h:20) */
typedef struct pt_camera {
    float tan_half_fovy;
    float aspect_ratio;
    float origin[3];
    float lower_left_corner[3];
    float horizontal[3];
    float vertical[3];
    float right[3];
    float up[3];
    float backward[3];
} pt_camera;

/* BVH node (reference BVH.h:6-11, 32 B): interior nodes have primitive count 0 in bits 16-31 and
 * the split axis in bits 8-15; left child = index + 1, right child = offset; leaves hold the first
 * primitive index in offset. */
typedef struct pt_bvh_node {
    float aabb_min[3];
    float aabb_max[3];
    uint32_t offset;
    uint32_t primitive_count_axis;
} pt_bvh_node;

/* Device hittable (reference Hittable.h:23-27 + Material.h:22-27, 96 B): world->object 3x4 rows,
 * material, shape type (0 SPHERE .. 6 CUBE, Hittable.h:9-12); material_type 0 LAMBERT, 1 GGX,
 * 2 LAMBERT_GGX (Material.h:9-12); texture_index is a 1-based handle, 0 = none. */
typedef struct pt_hittable {
    float inv_transform_rows[3][4];
    float base_color[3];
    float roughness;
    float emissive[3];
    float metalness;
    uint32_t texture_index;
    uint32_t material_type;
    uint32_t type;
    uint32_t pad;
} pt_hittable;

/* Traversal statistics of an instrumented render (for the algorithmic-byte count of DESIGN.md). */
typedef struct pt_render_stats {
    uint64_t node_tests;   /* AABB::hit calls                         */
    uint64_t prim_tests;   /* Hittable::hit calls                     */
    uint64_t hits;         /* segments that hit a primitive           */
    uint64_t sky_lookups;  /* misses that sampled the skybox texture  */
    uint64_t segments;     /* hitBVH calls                            */
    uint64_t samples;      /* camera paths                            */
    /* wave-level executions of the same events: SIMD efficiency of a phase = lane count / (64 x
     * wave count) */
    uint64_t wave_node_iters;
    uint64_t wave_prim_iters;
    uint64_t wave_hits;
    uint64_t wave_sky;
    uint64_t wave_segments;
    /* shader-clock cycles summed over waves (s_memtime stamps; while-while variants): interior
     * walk, leaf tests, shading, whole lane loop */
    uint64_t cycles_node_walk;
    uint64_t cycles_leaf_tests;
    uint64_t cycles_shading;
    uint64_t cycles_total;
    uint64_t cycles_lane_idle;  /* resumable variants: lane cycles spent done while the tile still ran */
    /* leaf tests by shape family (plane = disk/quad, cube, quadric: the three code paths of the
     * primitive test), resumable variants: leaf rounds (the wave's pending leaves after an interior
     * walk), family-path executions as run (per leaf position, one per family present), and as a
     * perfect cross-lane compaction would run them (per leaf round, ceil(pairs of the family / 64)) */
    uint64_t leaf_rounds;
    uint64_t family_execs;
    uint64_t family_execs_compacted;
    /* per leaf round: the lanes taking part and their (lane, primitive) pairs, summed; and the
     * family-path executions a compaction over only those lanes would need (the pairs in
     * family-major order, batches of as many pairs as lanes, one execution per batch and family) */
    uint64_t leaf_round_lanes;
    uint64_t leaf_pairs;
    uint64_t family_execs_compacted_in_round;
    /* child-box walks: leaf rounds that ended with t_max above its value at the leaf's start (the
     * sphere's far-root quirk, Hittable.inl:152-158) and rebuilt the reference's pending far
     * children (trace.cu:48-98; repair_pending in pt_kernels.hip) */
    uint64_t repairs;
} pt_render_stats;

typedef struct pt_context pt_context;

/* Number of visible GPUs. */
PT_API int pt_device_count(int *count);

/* Pathtracer ctor (Pathtracer.cpp:30-68): allocates the accumulation buffer and the per-pixel
 * XORWOW state and seeds it with curand_init(1984 + x + y * width, 0, 0) (initRandState.cu:16).
 * The context covers rows y = row_offset + k * row_stride (k = 0 .. local rows - 1) of a
 * width x height image, so an image can be tiled across GPUs (row_offset = rank, row_stride = N);
 * seeds and camera coordinates always use global pixel coordinates. */
PT_API int pt_create(int device, uint32_t width, uint32_t height, uint32_t row_offset, uint32_t row_stride,
                     pt_context **out);

/* Same, tiling the image in bands of band_rows rows (a power of two, 1..256): the context covers
 * the bands b = band_offset + k * band_stride, i.e. global row
 *     y(ly) = (band_offset + (ly / band_rows) * band_stride) * band_rows + ly % band_rows
 * for local row ly.  band_rows = 1 is pt_create's row interleave; band_rows = 8 (the multi-GPU
 * default) keeps each 8x8 tile of a context a spatially coherent 8x8 tile of the image. */
PT_API int pt_create_banded(int device, uint32_t width, uint32_t height, uint32_t band_rows, uint32_t band_offset,
                            uint32_t band_stride, pt_context **out);

/* Number of local rows of such a context (0 if it owns no band or the arguments are invalid). */
PT_API uint32_t pt_band_rows(uint32_t height, uint32_t band_rows, uint32_t band_offset, uint32_t band_stride);
/* Scatter one tile's rows (pt_band_rows(height, ...) x width float4, local row order, device memory
 * `part`) into the full image (height x width float4, device memory `full`) on `device`: the
 * unpermute step of pt_group_gather, for callers that gathered the tiles themselves (the
 * one-process-per-GPU path over torch.distributed / RCCL, pathtracercuda_amd/distributed.py).
 * Synchronises the device before and after. */
PT_API int pt_unpermute_bands(int device, void *full, const void *part, uint32_t width, uint32_t height,
                              uint32_t band_rows, uint32_t band_offset, uint32_t band_stride);
PT_API void pt_destroy(pt_context *ctx);

/* Pathtracer::setScene upload half (Pathtracer.cpp:137-159): nodes and primitives as produced by
 * the host BVH build (elements already reordered).  Replaces the previous scene.  Returns
 * PT_ERR_DEPTH if a traversal could overflow the reference's 32-entry stack.
 * Checked: node and primitive indices, leaf ranges, split axes, the tree's shape and depth, the
 * shape and material types and texture handles.
 * Floats: every entry of a primitive's inv_transform_rows must be finite; PT_ERR_ARG otherwise, and
 * the message names the primitive and the entry.  (A scale of 0, or below 2^-128 where 1 / scale
 * overflows, produces such rows; the scene loader refuses it for the same reason, naming
 * objects[i].scale.)  All other floats are taken as they are, and every finite float32 renders as
 * the reference's source does (words equal, or both NaN: DESIGN.md 3.1): roughness of any value
 * (the loader raises it to 0.04, a caller's smaller value is used as given), metalness outside
 * [0, 1], negative and huge base colours and emission, mirrored scales, scales of 1e-6 to 1e6.
 * NaN or infinite values elsewhere (a NaN roughness, a NaN box) are not refused and not tested. */
PT_API int pt_set_scene(pt_context *ctx, const pt_bvh_node *nodes, uint32_t node_count, const pt_hittable *prims,
                        uint32_t prim_count);

/* Pathtracer::loadTexture upload half (Pathtracer.cpp:258-288): RGBA float texels (LDR textures
 * already normalised to [0,1]), row 0 = first image row; handle is 1-based (1..64).  Sampled with
 * bilinear filtering, wrap in u, clamp in v, normalised coordinates. */
PT_API int pt_set_texture(pt_context *ctx, uint32_t handle, const float *rgba, uint32_t width, uint32_t height);

/* Pathtracer::setSkyboxTextureHandle (Pathtracer.cpp:294-297); 0 = no skybox (black). */
PT_API int pt_set_skybox(pt_context *ctx, uint32_t handle);

/* traceKernel launch (Pathtracer.cpp:162-199, trace.cu:158-199).  Equivalent to `chunks`
 * successive reference render(camera, spp, ignore) calls where the first call uses
 * ignore = ignore_history and the others ignore = false (the headless loop, main.cpp:275-279).
 * Synchronous.  gpu_ms (optional) receives the kernel time measured with hipEvents on the
 * context's stream (it includes the cost pre-pass below).  No launch (and no error) when no scene
 * is set or spp == 0, as in the reference (Pathtracer.cpp:174).
 * Tiles are dispatched most expensive first.  When no cost order is known yet for the scene and
 * camera and spp * chunks >= 16, a 2-spp pre-pass that writes nothing back measures the tile
 * costs first; results never depend on the order. */
PT_API int pt_render(pt_context *ctx, const pt_camera *camera, uint32_t spp, uint32_t chunks, int ignore_history,
                     float *gpu_ms);

/* Same as pt_render with the instrumented kernel variant: identical results plus counters. */
PT_API int pt_render_instrumented(pt_context *ctx, const pt_camera *camera, uint32_t spp, uint32_t chunks,
                           int ignore_history, float *gpu_ms, pt_render_stats *stats);

/* ---- Adaptive sampling ------------------------------------------------------------------------
 * "Render until the noise is below a tolerance, at most max_calls x spp samples per pixel."  A pixel
 * advances in render() calls of spp samples from its own XORWOW stream, so a pixel that stops after n
 * calls holds exactly the accumulation value and RNG state n reference render(camera, spp, ...) calls
 * leave.  Next to them the context keeps per pixel m1, m2 (float) and n (calls folded); at the end of
 * every call, with S the call's colour sum, in exactly these float operations (no contraction):
 *     y = (0.2126f*S.x + 0.7152f*S.y) + 0.0722f*S.z;   m1 = m1 + y;   m2 = m2 + y*y;   n = n + 1
 * After every round each pixel is re-evaluated (the batch-means standard error of the per-call
 * luminance against tolerance x (|mean| + floor)):
 *     k = (float)n;  mean = m1 / k;  ss = m2 - m1*mean;  if (ss < 0) ss = 0
 *     se2 = ss / (k*(k - 1));  t = tolerance * (fabsf(mean) + floor)
 *     conv = tolerance > 0 && ((se2 <= t*t) || !isfinite(m2))
 *     active = n < min_calls || (n < max_calls && any pixel q of the 3x3 neighbourhood, clipped to the
 *              context's rows and width, has n_q >= min_calls && !conv_q)
 * and every active pixel runs one more call (a step).  The render ends when no pixel is active or
 * when max_calls steps have been made since the reset (steps made by earlier renders count, so a
 * render to max_calls = 4 continued with reset = 0 to 8 is the render to 8).  The rule has no memory:
 * a stopped pixel can start again, and n ends anywhere in [min_calls, max_calls].  Non-finite
 * pixels count as converged (more samples cannot repair them); tolerance = 0 never converges: the
 * result is pt_render(spp, max_calls, 1)'s plus the moments.
 * reset != 0: a pixel's first call overwrites its accumulation value (as ignore_history does) and
 * starts from zero moments.  reset = 0 continues from the stored moments; PT_ERR_STATE when there are
 * none (no adaptive render since the last pt_render, pt_write_rng or scene, texture or sky change).
 * The kernel variant set by pt_set_kernel_variant is honoured when it has an adaptive build (0, 4, 6,
 * 40, 41, 46, 60, 61); otherwise PT_ERR_ARG.  All builds produce identical results. */
typedef struct pt_adaptive_params {
    uint32_t spp;          /* samples per call, >= 1 */
    uint32_t min_calls;    /* >= 2 */
    uint32_t max_calls;    /* >= min_calls */
    float tolerance;       /* >= 0 */
    float floor;           /* >= 0 */
    int reset;
} pt_adaptive_params;

typedef struct pt_adaptive_result {
    uint32_t rounds;       /* trace launches (the first min_calls calls of a reset render are one) */
    uint64_t samples;      /* camera paths traced */
    float gpu_ms;          /* hipEvent time of the whole render, evaluation passes included */
} pt_adaptive_result;

PT_API int pt_render_adaptive(pt_context *ctx, const pt_camera *camera, const pt_adaptive_params *params,
                              pt_adaptive_result *result);
/* The context keeps two facts about an adaptive render apart:
 *   "the counts describe the buffer": every pixel's accumulation value is the sum of its own n calls.  True
 *   from the end of a pt_render_adaptive until the next launch that writes the accumulation (a pt_render that
 *   launches, or the next pt_render_adaptive).  A scene, texture, sky or RNG-state change writes neither the
 *   accumulation nor the counts, so the three reads below and pt_denoise go on returning the same image.
 *   "the moments can be continued": the former, and no scene, texture, sky or RNG-state change since -- what
 *   reset = 0 needs (samples of another scene or stream must not be folded into the same moments).
 * pt_holds_adaptive: 1 while the counts describe the buffer, else 0. */
PT_API int pt_holds_adaptive(const pt_context *ctx);
/* Moments of the last adaptive render: rows x width x 3 (m1, m2, n -- n as uint32 bits).  This and the two
 * reads below: PT_ERR_STATE unless the counts describe the buffer. */
PT_API int pt_read_moments(pt_context *ctx, float *dst);
/* accum / (float)n per pixel (rows x width float4): getHDRImageData's units with frames = calls. */
PT_API int pt_read_adaptive_hdr(pt_context *ctx, float *dst);
/* pt_tonemap with every pixel divided by its own n (RGBA8, rows x width). */
PT_API int pt_tonemap_adaptive(pt_context *ctx, uint8_t *dst);

/* Raw accumulation sums (float4 per local pixel, rows x width, y-up), the data behind
 * getHDRImageData (Pathtracer.cpp:299-315) before the division by the frame count. */
PT_API int pt_read_accum(pt_context *ctx, float *dst);

/* Device-to-device copy of the raw accumulation buffer (rows * width * 16 bytes) into memory of
 * the same device, e.g. a send buffer for the multi-GPU framebuffer gather. */
PT_API int pt_copy_accum_device(pt_context *ctx, void *dst_device, size_t bytes);

/* tonemap kernel (tonemap.cu:4-27) over the local rows: accum / frames, Reinhard, gamma 2.2,
 * truncation to 8 bits, alpha 255 (RGBA8, rows x width). */
PT_API int pt_tonemap(pt_context *ctx, uint32_t frames, uint8_t *dst);
/* Same, into a device buffer of >= rows*width*4 bytes (RGBA8): the replacement of render()'s
 * OpenGL pixel-buffer tonemap (Pathtracer.cpp:207-221) for a progressive viewer. */
PT_API int pt_tonemap_device(pt_context *ctx, uint32_t frames, void *dst, size_t dst_bytes);

/* Per-pixel XORWOW state (d, v0..v4 as uint32, rows x width x 6) -- for tests/checkpoints. */
PT_API int pt_read_rng(pt_context *ctx, uint32_t *dst);
PT_API int pt_write_rng(pt_context *ctx, const uint32_t *src);

PT_API uint32_t pt_local_rows(const pt_context *ctx);

/* Shader-clock cycles each 8x8 tile took in the last launch (row-major over the context's tiles,
 * count = ceil(width / 8) * ceil(rows / 8)); the input of the cost order. */
PT_API int pt_read_tile_costs(pt_context *ctx, uint32_t *dst, uint32_t count);
/* Diagnostics: per tile (row-major, same count), the mean over its lanes of the shader-clock cycles
 * between a lane finishing its pixel and the tile's end, from the last pt_render_instrumented launch
 * (resumable variants).  Divided by the tile's cycles (pt_read_tile_costs) it is the tile's
 * idle-lane fraction. */
PT_API int pt_read_tile_idle(pt_context *ctx, uint32_t *dst, uint32_t count);
/* Diagnostics: schedule trace.  With enabled != 0 every instrumented launch (pt_render_instrumented;
 * the plain kernel carries no trace code) also records per tile (row-major) two words: the
 * shader-clock cycle (low 32 bits; the counter is per CU) at which its wave started it, and the
 * wave's hardware ids (XCC_ID << 16 | HW_ID bits 0-15: wave, SIMD, pipe, CU, SH, SE).
 * pt_read_tile_trace reads the last such launch's 2 x tiles words.  Results are unchanged. */
PT_API int pt_set_tile_trace(pt_context *ctx, int enabled);
PT_API int pt_read_tile_trace(pt_context *ctx, uint32_t *dst, uint32_t count);

/* Tuning knob for A/B measurements: 0 = automatic (default); otherwise one of the shipped
 * trace-kernel variants (traversal loop shape, deferred shading, BVH staged in LDS or read through
 * the caches, occupancy target; see pt_kernels.hip).  All variants produce bit-identical results.
 *   picked automatically (0):   60 and 40 (records in LDS, six / five waves per SIMD), 61 and 41
 *                               (records through the caches), 46 (deep BVHs, four waves), 47 / 48
 *                               (small grids);
 *   fallbacks the automatic choice also uses: 4 and 6 (node-at-a-time walks for scenes outside the
 *                               child-box encoding or whose leaves are not in DFS order);
 *   reference / counting:       1 (the reference's control flow), 20 (counts the reference's node and
 *                               primitive tests; the bench's algorithmic bytes);
 *   test / A-B only:            39 (no deferred shading), 91 (48 without the rising-t_max rebuild;
 *                               not the reference's results -- its cost A/B only).
 * Other numbers return PT_ERR_ARG. */
PT_API int pt_set_kernel_variant(pt_context *ctx, int variant);

/* Tile dispatch order: 0 = by the measured cost of each 8x8 tile, most expensive first (default:
 * every launch records the tile costs, and after a scene, texture or camera change the order is
 * rebuilt on the device from the latest launch), 1 = always row-major.  Results are identical;
 * only the launch tail changes. */
PT_API int pt_set_schedule(pt_context *ctx, int mode);

/* Tuning knob for measurements: persistent trace-kernel grids hold at most workgroups_per_cu
 * workgroups (of four waves, one per SIMD) per CU, i.e. that many waves per SIMD (0 = as many as
 * fit, the default).  Results are identical. */
PT_API int pt_set_occupancy(pt_context *ctx, uint32_t workgroups_per_cu);

/* Issue priority by position in the cost order (s_setprio): mode 0 = automatic (default: graded by
 * quarter of the order, the first band raised to every position a persistent plain launch deals at
 * its start), 1 = off, 2 = explicit -- positions < level3 run at wave priority 3, < level2 at 2,
 * < level1 at 1, the rest at 0 (level3 <= level2 <= level1).  Results are identical. */
PT_API int pt_set_issue_priority(pt_context *ctx, int mode, uint32_t level3, uint32_t level2, uint32_t level1);

/* Speculative sample groups.  A pixel's samples are one serial XORWOW stream
 * (trace.cu:183-193), so a launch with fewer 8x8 tiles than about four per wave slot of the chip
 * (multi-GPU strong scaling, small images) lasts as long as its slowest tile's whole chain.  With
 * groups, each pixel's chain is cut into G pieces started at guessed draw offsets and stitched where
 * the guessed parse meets the true one; results stay bit-identical.  mode: 0 = automatic (default),
 * 1 = never, G >= 2 = always G groups (tests).  pt_last_sample_groups: groups of the last launch
 * (0 = plain).  pt_read_group_stats fills 10 words: G, patch rounds run, and the pixels at a dead end
 * after fold rounds 0..7.  pt_read_group_log_counts: samples each (tile, item) logged per lane
 * ([tile][2G - 1][64], tiles in dispatch (cost) order; item 0 = group 0, items 2g - 1 and 2g =
 * group g at its guessed offset and one draw pair later).  pt_set_patch_rounds: patch rounds before
 * the remaining dead ends run as a plain resume launch (default 6; 0 exercises the resume path).
 * pt_set_group_lookback: a second phase (the item one pair later) also stops where its first
 * phase's parse holds the second phase's sample start `far` or `near` samples back -- the first
 * phase may run behind on the parse the two share (defaults 64 and 16; 0 = off: only the current
 * start).  Scheduling only: results are identical for every setting. */
/* Tuning knob: tiles per dispatch unit of launches with few samples per pixel (a row strip of K
 * tiles; a lane whose pixel is done takes the same position in the next tile of its strip).
 * 0 = automatic (K = 4 at <= 2 samples per pixel on large images), 1 = off, K = 2..16 = always K
 * (resumable variants).  Results are identical for every setting. */
PT_API int pt_set_strip_units(pt_context *ctx, int mode);
/* Test knob (negative control): enabled = 0 skips the child-box walks' rebuild of the pending far
 * children after a leaf raised t_max (the sphere's far-root quirk, Hittable.inl:152-158), so those
 * walks drop boxes the reference would test (trace.cu:48-98) and results are NOT the reference's on
 * rays that meet the quirk.  Default 1.  Exists so a test can show that a scene exercises the rebuild. */
PT_API int pt_set_rise_repair(pt_context *ctx, int enabled);
/* Test knob (negative control): the next pt_set_scene uploads other values than the quadric constants
 * B, H, J (kept in the device record of every primitive) for every primitive of shape `type` (0..6;
 * -1 = none, the default): zeros for a quadric shape, so its tests read a wrong quadric and results are
 * NOT the reference's; NaN for a disk, quad or cube, whose tests must never read the words, so results
 * stay the reference's.  Exists so a test can show which paths read the constants from the record. */
PT_API int pt_set_zero_quadric_consts(pt_context *ctx, int type);
/* Run-ahead across render() calls: a launch of 3..64 samples per pixel (the reference's
 * render(camera, 8, ...) calls, main.cpp:272-279) lets the lanes whose pixels are done go on with the
 * pixel's next call (same XORWOW stream) until their tile ends, and keeps per pixel the colour sum,
 * count and state after the last finished sample; the next pt_render with the same camera, scene,
 * textures, sky and RNG state starts every pixel from there.  Any other next launch ignores the
 * stash: the stored RNG state and accumulation are always those of the calls made, so results are
 * the reference's either way.
 * 0 = automatic (the default; stops while the camera or scene changes at every launch),
 * 1 = off, 2 = make a stash at every launch (tests), 3 = make stashes but never use them
 * (diagnostic: the cost of the run-ahead work alone). */
PT_API int pt_set_run_ahead(pt_context *ctx, int mode);
/* Tuning knob of the cold start (the first launch after a scene, texture or camera change, which has
 * no tile costs yet).  prepass_spp = 0 (default): a launch of several render() calls runs its first
 * call alone in row-major order and the rest in the cost order of that call (a one-call launch runs a
 * discarded 2-spp cost pre-pass); prepass_spp > 0 (at most 64): always a discarded pre-pass of that
 * many spp.  priority: issue priority on that order (1, the default) or not (0).  Scheduling only:
 * results are identical for every setting. */
PT_API int pt_set_cold_start(pt_context *ctx, uint32_t prepass_spp, int priority);
PT_API int pt_set_sample_groups(pt_context *ctx, int mode);
PT_API int pt_set_patch_rounds(pt_context *ctx, uint32_t rounds);
PT_API int pt_set_group_lookback(pt_context *ctx, uint32_t far, uint32_t near);
PT_API int pt_last_sample_groups(const pt_context *ctx);
/* The trace-kernel variant the last launch ran (its main pass; diagnostics and tests). */
PT_API int pt_last_variant(const pt_context *ctx);
/* The last trace launch of the context (the main pass of pt_render, the last round of
 * pt_render_adaptive; diagnostics and tests), 4 words: dynamic LDS bytes of a workgroup; what it staged
 * in LDS (0 nothing -- the scene is read through the caches --, 1 the child-box records or the nodes,
 * 2 the primitives too); waves per workgroup; workgroups launched. */
PT_API int pt_last_launch(const pt_context *ctx, uint32_t *dst);
PT_API int pt_read_group_stats(const pt_context *ctx, uint32_t *dst);
PT_API int pt_read_group_log_counts(pt_context *ctx, uint32_t *dst, size_t count);
/* Diagnostics: one word plane of the per-pixel fold state (rows x width; word 16 = dead-end flag,
 * 7 = samples done, 8 = draw-pair offset), or with words 19 / 20 / 21 the statistics the next
 * launch's guesses use (float): draw pairs per sample, odd-length fraction, variance. */
PT_API int pt_read_group_fold(pt_context *ctx, uint32_t word, uint32_t *dst);
/* The message of the context's last failed call.  With ctx = NULL: the message of the calling thread's
 * last failed context-free call (pt_denoise_image, pt_temporal_image). */
PT_API const char *pt_last_error(const pt_context *ctx);

/* ---- First-hit feature buffers ------------------------------------------------------------------
 * pt_render_features traces one ray per pixel -- the pixel's FIRST sample of a reset render: the XORWOW
 * state is curand_init(1984 + x + y * width, 0, 0) of the global pixel, computed in the kernel (the
 * context's RNG buffer is not read), and two uniforms are drawn, x then y, as for every camera ray --
 * with the reference's loop over the BVH (valid for every scene pt_set_scene accepts), and stores the
 * closest hit in three planes of rows x width float4 (local row order), allocated on first use:
 *   plane 0: x, y, z = the material's base colour as shading forms it (after the texture lookup and
 *            pow 2.2 for a textured material); w = the primitive index as uint32 bits, 0xffffffff on a miss
 *   plane 1: x, y, z = the world normal, turned against the ray as shading uses it; w = the hit distance t
 *   plane 2: x, y, z = the world position of the hit; w = flags as uint32 bits: PT_FEATURE_HIT,
 *            PT_FEATURE_EMISSIVE (any component of the material's emission != 0)
 * On a miss every float is +0 and the flags word is 0.  The pass reads and writes nothing of the render
 * state (accumulation, RNG, moments, tile costs and order, run-ahead stash, frame counter), so it
 * is reproducible, the same for every band partition, and a render continues after it as if it had
 * not run.  PT_ERR_STATE without a scene.  A scene or texture change voids the planes. */
#define PT_FEATURE_HIT 1u
#define PT_FEATURE_EMISSIVE 2u
PT_API int pt_render_features(pt_context *ctx, const pt_camera *camera);
/* One plane (0..2) of the last pt_render_features: rows x width float4.  PT_ERR_STATE if there is none. */
PT_API int pt_read_features(pt_context *ctx, uint32_t plane, float *dst);

/* ---- Edge-avoiding a-trous denoiser -------------------------------------------------------------
 * Dammertz et al.'s a-trous filter (B3 spline taps, 5 x 5, step doubling and colour sigma halving per
 * level) guided by the feature planes, with rational edge-stopping weights (+ - x /, compares and selects
 * only: no exp) and a scale-free plane-distance term, so the result is reproducible word for word.
 * All float32, no contraction, in exactly these operations (tests/denoise_model.py restates them):
 *
 * Per pixel p: colour C (3 floats); A = plane 0 xyz, id = plane 0 w; N = plane 1 xyz, t = plane 1 w;
 * P = plane 2 xyz, flags = plane 2 w.
 * Prepare:
 *     keep_p = HIT && !EMISSIVE && every component x of C, N, P has x - x == 0
 *     D_p    = DEMODULATE ? (A > 1/64 ? A : 1/64) per channel : 1
 *     I_p    = C_p / D_p                                       (IEEE division, per channel)
 * Iteration i = 0 .. iterations - 1, step s = 1 << i, sigma_i = sigma_color * 2^-i (exact):
 *     for a kept p:  sumW = 0, sumI = (0, 0, 0);  m = sigma_plane * t_p;  mm = m * m;  ss = sigma_i * sigma_i
 *       for dy = -2 .. 2 (outer), dx = -2 .. 2 (inner), q = p + s * (dx, dy);
 *       q is skipped (by a select, never by a zero weight) when it is outside the image, when !keep_q,
 *       or when SAME_PRIMITIVE is set and id_q != id_p; otherwise
 *         h  = k[|dx|] * k[|dy|],  k = {3/8, 1/4, 1/16}
 *         c  = (N_p.x * N_q.x + N_p.y * N_q.y) + N_p.z * N_q.z;  c = c > 0 ? c : 0;
 *              normal_power_log2 times: c = c * c;               w_n = c
 *         e  = P_q - P_p;  g = (N_p.x * e.x + N_p.y * e.y) + N_p.z * e.z;  w_p = 1 / (1 + (g * g) / mm)
 *         d  = I_q - I_p;  d2 = (d.r * d.r + d.g * d.g) + d.b * d.b;       w_c = 1 / (1 + d2 / ss)
 *         w  = ((h * w_n) * w_p) * w_c;   sumW = sumW + w;   sumI = sumI + w * I_q  (per channel)
 *       I'_p = sumI / sumW
 *     for a p that is not kept: I'_p = I_p
 * Final:  out_p = keep_p ? I_p * D_p : C_p;  out.w = 1
 * A NaN or infinite pixel is not kept: it passes through unchanged and never reaches a neighbour.
 *
 * Every iteration is one kernel launch between two buffers.  `staging`: 0 = automatic (a workgroup's
 * tile and its halo of 2 s pixels are staged in LDS for the steps where that wins -- s = 1 and 2, measured --
 * and the taps are read through the caches otherwise), 1 = staged for every step that fits (s <= 4), 2 = never staged; tests
 * and A/B only: the words are the same.
 * Accepted: iterations 1..8, sigma_color > 0, sigma_plane >= 1e-6, normal_power_log2 0..7, flags within
 * the two bits, staging 0..2; anything else (a NaN included) is PT_ERR_ARG and the message names the field. */
#define PT_DENOISE_DEMODULATE 1u
#define PT_DENOISE_SAME_PRIMITIVE 2u
#define PT_DENOISE_TILE_W 32 /* the filter's workgroup tile (pixels) */
#define PT_DENOISE_TILE_H 8
/* Defaults of the layers above (C++ Pathtracer::denoise, Python, the CLI's -denoise), chosen by the sweep of
 * tools/denoise_probe.py (profiles/denoise_probe.json).  The automatic sigma_color is
 * SIGMA_FACTOR x the median luminance (0.2126, 0.7152, 0.0722) of the kept pixels' I_p, computed on the
 * host: the device rule stays free of a reduction whose order would have to be specified. */
#define PT_DENOISE_DEFAULT_ITERATIONS 5
#define PT_DENOISE_DEFAULT_SIGMA_FACTOR 4.0f
#define PT_DENOISE_DEFAULT_SIGMA_PLANE 0.005f
#define PT_DENOISE_DEFAULT_NORMAL_POWER_LOG2 3
#define PT_DENOISE_DEFAULT_FLAGS 1u
typedef struct pt_denoise_params {
    uint32_t iterations;
    float sigma_color;       /* in units of the (demodulated) colour */
    float sigma_plane;       /* relative to the hit distance */
    uint32_t normal_power_log2;
    uint32_t flags;
    uint32_t staging;
} pt_denoise_params;

/* Filters the context's image: C = accumulation * (1 / max(frames, 1)), the HDR read-out's arithmetic, or,
 * while the counts of an adaptive render describe the buffer (pt_holds_adaptive), accumulation / n per pixel
 * (pt_read_adaptive_hdr's; `frames` is not used then); features = the planes of the last
 * pt_render_features.  The accumulation is not changed.  PT_ERR_STATE, naming the reason, when there are
 * no feature planes or the scene or a texture changed since; PT_ERR_ARG, naming the reason, on a context that does not hold the whole frame (the
 * filter needs every pixel's neighbours: gather the frame and use pt_denoise_image). */
PT_API int pt_denoise(pt_context *ctx, uint32_t frames, const pt_denoise_params *params);
/* hipEvent times in ms of the last pt_denoise's kernels, 10 floats: prepare, iterations 0..7 (0 for
 * those not run), finish; and of the last pt_render_features (one float).  Measurements only. */
PT_API int pt_read_denoise_timing(pt_context *ctx, float *dst);
PT_API int pt_read_features_timing(pt_context *ctx, float *dst);
/* The last pt_denoise's result (rows x width float4, w = 1), and its tonemap (pt_tonemap's arithmetic with
 * divisor 1; RGBA8).  PT_ERR_STATE when there is none. */
PT_API int pt_read_denoised(pt_context *ctx, float *dst);
PT_API int pt_tonemap_denoised(pt_context *ctx, uint8_t *dst);
/* The same filter on host arrays, without a context: color, plane0..2 and out are height x width float4
 * (color's w is ignored).  For a frame gathered from several devices, and for tests.  Errors:
 * pt_last_error(NULL). */
PT_API int pt_denoise_image(int device, uint32_t width, uint32_t height, const float *color, const float *plane0,
                            const float *plane1, const float *plane2, const pt_denoise_params *params, float *out);

/* ---- Temporal reprojection ------------------------------------------------------------------------
 * One step per frame: last frame's result is reprojected into this frame's camera through the feature
 * planes, what is no longer the same surface is rejected, and the new frame is blended in.  All float32,
 * no contraction, + - x /, floor, compares and selects only, in exactly these operations
 * (tests/temporal_model.py restates them).  Every dot product a . b is (a.x*b.x + a.y*b.y) + a.z*b.z;
 * "finite" means x - x == 0.
 *
 * History, three float4 per pixel:  h0 = (I.rgb, n): the accumulated (demodulated) colour and the history
 * length n, a float holding an integer, 0 = no history here;  h1 = (N, id bits);  h2 = (P, t).
 * Inputs of a step: the colour C; the planes 0..2 (A, id | N, t | P, flags) and their camera `cur`; the
 * previous history with its camera `prev`, or none.  W, H = the image's width and height as floats.
 *
 * Per pixel p = (x, y), y the global row:
 *     ok_p  = HIT && every component x of C, N, P is finite        (emissive surfaces are included)
 *     D     = DEMODULATE ? (A > 1/64 ? A : 1/64) per channel : 1;    I_cur = C / D
 *     h1 = (N_p, id_p), h2 = (P_p, t_p) in every case
 *     !ok_p:  image = (C.rgb, 0), h0 = (C.rgb, 0), and nothing else is done for the pixel
 *     project(cam, P):  e = P - cam.origin;  z = -(e . cam.backward);  hh = cam.tan_half_fovy;
 *                       hw = cam.aspect_ratio * hh;
 *                       su = ((e . cam.right / z) / hw) * 0.5 + 0.5;  sv = ((e . cam.up / z) / hh) * 0.5 + 0.5
 *     (su0, sv0, z0) = project(cur, P_p);  (su1, sv1, z1) = project(prev, P_p)
 *     fx = (float)x + (su1 - su0) * W;  fy = (float)y + (sv1 - sv0) * H
 *       (the planes hold the hit of a jittered ray: subtracting the current projection removes the jitter;
 *       with prev == cur both projections are the same operations on the same words: fx = x, fy = y)
 *     reproj = z0 > 0 && z1 > 0 && fx > -1 && fx < W && fy > -1 && fy < H        (a NaN fails it; floats
 *       are converted to integers only behind it)
 *     x0 = floor(fx), ax = fx - x0;  y0 = floor(fy), ay = fy - y0
 *     sumW = 0, sumI = (0, 0, 0), nh = (float)max_history
 *     taps (i, j) = (0,0), (1,0), (0,1), (1,1) at q = (x0 + i, y0 + j):  w = (i ? ax : 1 - ax) * (j ? ay : 1 - ay)
 *       a tap is skipped (by a select, never by a zero weight; its index is clamped into the image before
 *       the load) when  !(w > 0),  or q is outside the image,  or n_q < 1,  or a component of I_q is not
 *       finite,  or SAME_PRIMITIVE is set and id_q != id_p,  or N_p . N_q < normal_cos_min,  or, with
 *       g = N_p . (P_q - P_p) and m = sigma_plane * t_p,  !(g*g <= m*m);  otherwise
 *         sumW = sumW + w;  sumI = sumI + w * I_q (per channel);  nh = n_q < nh ? n_q : nh
 *     have = there is a previous history && reproj && sumW >= 1/64
 *     have:   Hc = sumI / sumW;  n = nh + 1;  n = n < (float)max_history ? n : (float)max_history;
 *             a = 1 / n;  a = a > alpha_min ? a : alpha_min;  I = Hc + a * (I_cur - Hc)
 *     else:   I = I_cur, n = 1
 *     image = (I * D, n);  h0 = (I, n)
 * With prev == cur, flags 0 and alpha_min 0 every hit pixel takes exactly one tap of weight 1 (itself), so
 * after K steps h0 is the running mean  m = m + (1/k) * (C_k - m)  word for word, and n = K.
 * Accepted: alpha_min 0..1, max_history 1..65535, sigma_plane >= 1e-6 and finite, normal_cos_min -1..1,
 * flags within the two bits; anything else (a NaN included) is PT_ERR_ARG and the message names the field. */
#define PT_TEMPORAL_DEMODULATE 1u
#define PT_TEMPORAL_SAME_PRIMITIVE 2u
/* Defaults of the layers above (C++ Pathtracer::temporal, Python), chosen by the sweep of
 * tools/temporal_probe.py (profiles/temporal_probe.json). */
#define PT_TEMPORAL_DEFAULT_ALPHA_MIN 0.02f
#define PT_TEMPORAL_DEFAULT_MAX_HISTORY 64
#define PT_TEMPORAL_DEFAULT_SIGMA_PLANE 0.3f
#define PT_TEMPORAL_DEFAULT_NORMAL_COS_MIN 0.0f
#define PT_TEMPORAL_DEFAULT_FLAGS 1u
typedef struct pt_temporal_params {
    float alpha_min;         /* the least weight of the new frame */
    uint32_t max_history;    /* n is capped here */
    float sigma_plane;       /* relative to the hit distance */
    float normal_cos_min;
    uint32_t flags;
} pt_temporal_params;

/* One step on the context.  C is formed as pt_denoise forms it (accumulation * (1 / max(frames, 1)), or
 * accumulation / n per pixel while pt_holds_adaptive); the planes and `cur` are those of the last
 * pt_render_features; the previous history is the one the last pt_temporal left, used when one is held and
 * reset == 0 (history_used, optional, receives 1 then, else 0).  The context keeps two history sets: a step
 * reads one and writes the other.  A history is held from the end of a pt_temporal until the next one
 * begins, a scene or texture change, or a sky change to another handle; a camera change, a render and an
 * RNG write end nothing.  The pass reads and writes nothing of the render state, as the denoiser.
 * PT_ERR_STATE, naming the reason, without current feature planes; PT_ERR_ARG, naming the reason, on a
 * context that does not hold the whole frame (gather the frame and use pt_temporal_image). */
PT_API int pt_temporal(pt_context *ctx, uint32_t frames, const pt_temporal_params *params, int reset,
                       int *history_used);
/* The last pt_temporal's image (rows x width float4, w = n), its tonemap (pt_tonemap_denoised's
 * arithmetic; RGBA8) and its kernel's hipEvent time in ms (one float).  PT_ERR_STATE when there is none. */
PT_API int pt_read_temporal(pt_context *ctx, float *dst);
PT_API int pt_tonemap_temporal(pt_context *ctx, uint8_t *dst);
PT_API int pt_read_temporal_timing(pt_context *ctx, float *dst);
/* pt_denoise's filter with the temporal image as its colour and the planes that image was made from as its
 * guide; the result goes where pt_denoise's goes (pt_read_denoised, pt_tonemap_denoised).  PT_ERR_STATE
 * when there is no temporal image or pt_render_features has run since it was made. */
PT_API int pt_denoise_temporal(pt_context *ctx, const pt_denoise_params *params);
/* The same step on host arrays, without a context: color, plane0..2, hist0..2, out_image and out_hist0..2
 * are height x width float4 (color's w is ignored); hist0 = NULL means no previous history (hist1, hist2
 * and prev_cam are not read then).  For a frame gathered from several devices, and for tests.  Errors:
 * pt_last_error(NULL). */
PT_API int pt_temporal_image(int device, uint32_t width, uint32_t height, const float *color, const float *plane0,
                             const float *plane1, const float *plane2, const pt_camera *cur_cam, const float *hist0,
                             const float *hist1, const float *hist2, const pt_camera *prev_cam,
                             const pt_temporal_params *params, float *out_image, float *out_hist0, float *out_hist1,
                             float *out_hist2);

/* ---- Per-pixel variance from the temporal history, and the variance-guided filter ------------------
 * The estimation and filtering of SVGF (Schied et al. 2017) without its feedback: luminance moments are
 * carried in a fourth history plane, a variance is estimated per pixel, and an a-trous filter takes its
 * colour weight from that variance instead of one sigma_color for the image.  All float32, no contraction,
 * + - x /, compares and selects only, in exactly these operations (tests/svgf_model.py restates them).
 *   lum(c) = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z;   "finite" means x - x == 0;
 *   clamp0(v) = (v > 0 && v finite) ? v : 0
 *
 * 1. The temporal step with moments.  pt_temporal's rule unchanged (same pt_temporal_params, same taps, same
 *    image and h0..h2 word for word) with a fourth history plane  h3 = (m1, m2, v, 0):
 *     l = lum(I_cur);  q = l * l
 *     !ok_p:  h3 = (0, 0, -1, 0)
 *     sumM1 = 0, sumM2 = 0;  in every tap the colour accepts, after its sums:
 *         sumM1 = sumM1 + w * m1_q;  sumM2 = sumM2 + w * m2_q        (m1_q, m2_q = the previous h3's x, y)
 *     have:   Hm1 = sumM1 / sumW;  Hm2 = sumM2 / sumW;  m1 = Hm1 + a * (l - Hm1);  m2 = Hm2 + a * (q - Hm2)
 *     else:   m1 = l, m2 = q
 *     if m1 or m2 is not finite:  m1 = l, m2 = q                    (the moments restart)
 *     v = clamp0(m2 - m1 * m1);   h3 = (m1, m2, v, 0)
 *
 * 2. The variance estimate, one float per pixel, from the NEW history of the same step (n_p = h0.w,
 *    I = h0.rgb, N, id = h1, P, t = h2) and its h3:
 *     n_p < 1 (a pixel that is not ok):  var = -1
 *     n_p >= (float)min_temporal:        var = h3.z
 *     otherwise (a young history):  k = 0, s1 = 0, s2 = 0;  m = sigma_plane * t_p;  mm = m * m
 *       for dy = -3 .. 3 (outer), dx = -3 .. 3 (inner), q = p + (dx, dy):
 *       the centre tap (dx = dy = 0) always counts; any other tap is skipped (by a select; its index is
 *       clamped into the image before the load) when q is outside the image, or n_q < 1, or
 *       N_p . N_q < normal_cos_min, or with g = N_p . (P_q - P_p)  !(g*g <= mm), or SAME_PRIMITIVE is set
 *       and id_q != id_p;  otherwise
 *         lq = lum(I_q);  k = k + 1;  s1 = s1 + lq;  s2 = s2 + lq * lq
 *       mean = s1 / k;  vs = clamp0(s2 / k - mean * mean);  var = vs * ((float)min_temporal / n_p)
 *    min_temporal 1..255 (pt_variance_params); anything else is PT_ERR_ARG naming the field.
 *
 * 3. The variance-guided filter.  pt_denoise's structure (prepare, one launch per iteration between two
 *    buffers, finish; 32 x 8 tile; staged and unstaged forms with the same words), with these changes:
 *    Prepare:  keep_p = pt_denoise's keep_p && var_p >= 0 && var_p finite && lum(I_p) finite
 *              v_p = var_p < 2^60 ? var_p : 2^60;   the texel is (I_p, keep_p ? v_p : -1)
 *              "kept" below means: the texel's w is not < 0
 *    Iteration i, step s = 1 << i (sigma_l is the same at every level), for a kept p:
 *       sumG = 0, sumV = 0;  for dy = -1 .. 1 (outer), dx = -1 .. 1 (inner), q = p + (dx, dy) (unit spacing):
 *         q is skipped (by a select) when it is outside the image or not kept;  otherwise
 *         g = k3[|dx|] * k3[|dy|],  k3 = {1/2, 1/4};  sumG = sumG + g;  sumV = sumV + g * v_q
 *       vg = sumV / sumG;  den = (sigma_l * sigma_l) * vg + variance_floor;  lp = lum(I_p)
 *       sumW = 0, sumI = (0, 0, 0), sumV2 = 0;  the 25 taps q = p + s * (dx, dy) in pt_denoise's order, with
 *       its skips (outside, not kept, SAME_PRIMITIVE) and its h, w_n, w_p and mm:
 *         d = lum(I_q) - lp;  w_c = 1 / (1 + (d * d) / den);  w = ((h * w_n) * w_p) * w_c
 *         sumW = sumW + w;  sumI = sumI + w * I_q (per channel);  sumV2 = sumV2 + (w * w) * v_q
 *       I'_p = sumI / sumW;  v'_p = sumV2 / (sumW * sumW)
 *    A pixel that is not kept is handed on unchanged.
 *    Final:  out_p = kept ? I_p * D_p : C_p;  out.w = 1
 *    Accepted: iterations 1..8, sigma_l in (0, 2^20], variance_floor > 0 and finite, sigma_plane >= 1e-6 and
 *    finite, normal_power_log2 0..7, flags within the two denoise bits, staging 0..2 (as pt_denoise's);
 *    anything else (a NaN included) is PT_ERR_ARG and the message names the field.  With v <= 2^60 and
 *    sigma_l <= 2^20 the product (sigma_l * sigma_l) * vg is at most 2^100: den never overflows. */
/* Defaults of the layers above (C++ Pathtracer::temporalMoments / denoiseVariance, Python), chosen by the
 * sweep of tools/svgf_probe.py (profiles/svgf_probe.json); sigma_plane, normal_power_log2
 * and flags are pt_denoise's. */
#define PT_VARIANCE_DEFAULT_MIN_TEMPORAL 4
#define PT_VDENOISE_DEFAULT_ITERATIONS 5
#define PT_VDENOISE_DEFAULT_SIGMA_L 16.0f
#define PT_VDENOISE_DEFAULT_VARIANCE_FLOOR 1e-4f
#define PT_VDENOISE_DEFAULT_SIGMA_PLANE 0.005f
#define PT_VDENOISE_DEFAULT_NORMAL_POWER_LOG2 3
#define PT_VDENOISE_DEFAULT_FLAGS 1u
typedef struct pt_variance_params {
    uint32_t min_temporal;   /* history length from which the temporal variance is trusted */
} pt_variance_params;
typedef struct pt_vdenoise_params {
    uint32_t iterations;
    float sigma_l;           /* in standard deviations of the luminance */
    float variance_floor;
    float sigma_plane;       /* relative to the hit distance */
    uint32_t normal_power_log2;
    uint32_t flags;          /* PT_DENOISE_DEMODULATE, PT_DENOISE_SAME_PRIMITIVE */
    uint32_t staging;
} pt_vdenoise_params;

/* pt_temporal with moments and the variance estimate, on the context: arguments, refusals and results as
 * pt_temporal's, and the image and history planes 0..2 are word for word those pt_temporal gives.  The
 * moments planes and the variance are a separate allocation, made on first use.  "The held history has
 * moments" from the end of this call until whatever ends the history, or a pt_temporal step (which may still
 * reproject the colour history of this one: planes 0..2 have one layout); a call that meets a history
 * without moments acts as reset (history_used = 0). */
PT_API int pt_temporal_moments(pt_context *ctx, uint32_t frames, const pt_temporal_params *params,
                               const pt_variance_params *variance, int reset, int *history_used);
/* The variance of the last pt_temporal_moments (rows x width float) and the hipEvent times in ms of its two
 * kernels (step, estimate).  PT_ERR_STATE unless a moments step has finished and its history is still held. */
PT_API int pt_read_temporal_variance(pt_context *ctx, float *dst);
PT_API int pt_read_temporal_moments_timing(pt_context *ctx, float *dst);
/* The variance-guided filter of the temporal image with the variance of the same step; the result goes where
 * pt_denoise's goes (pt_read_denoised, pt_tonemap_denoised, pt_read_denoise_timing).  PT_ERR_STATE, naming
 * the reason, without a held variance or when pt_render_features has run since; PT_ERR_ARG when the
 * DEMODULATE bit differs from the one the moments were made with. */
PT_API int pt_denoise_variance(pt_context *ctx, const pt_vdenoise_params *params);
/* The same on host arrays, without a context (as pt_temporal_image, pt_denoise_image): hist3 and out_hist3
 * are height x width float4, out_variance and variance height x width float.  hist0 = NULL means no
 * previous history.  pt_denoise_variance_image takes a variance from any source.  Errors: pt_last_error(NULL). */
PT_API int pt_temporal_moments_image(int device, uint32_t width, uint32_t height, const float *color,
                                     const float *plane0, const float *plane1, const float *plane2,
                                     const pt_camera *cur_cam, const float *hist0, const float *hist1,
                                     const float *hist2, const float *hist3, const pt_camera *prev_cam,
                                     const pt_temporal_params *params, const pt_variance_params *variance,
                                     float *out_image, float *out_hist0, float *out_hist1, float *out_hist2,
                                     float *out_hist3, float *out_variance);
PT_API int pt_denoise_variance_image(int device, uint32_t width, uint32_t height, const float *color,
                                     const float *plane0, const float *plane1, const float *plane2,
                                     const float *variance, const pt_vdenoise_params *params, float *out);

/* ---- The feedback: the filtered colour becomes the history the next frame reprojects ---------------
 * SVGF's feedback (Schied et al. 2017, section 4.3): the output of an early wavelet level replaces the colour
 * of the temporal history, so that the filter's noise reduction compounds over frames.  The variance-guided
 * filter above is unchanged (prepare, iterations between two buffers, finish): the feedback reads an
 * iteration's output and steers nothing, so the filter's result is word for word pt_denoise_variance's for
 * the same parameters.  tests/feedback_model.py restates the rule.
 *
 * 4. One more parameter, level L with 1 <= L <= iterations.  After iteration index L - 1 (L iterations), for
 *    every pixel p of the history the last pt_temporal_moments step wrote (h0 = (I, n)):
 *       T_p = the texel iteration L - 1 wrote for p:  (I'.rgb, v') for a kept pixel, w < 0 otherwise
 *       fed_p = !(T_p.w < 0) && I'.x finite && I'.y finite && I'.z finite          ("finite": x - x == 0)
 *       h0_p = fed_p ? (I'.x, I'.y, I'.z, n_p) : h0_p       (a select, then one unconditional 16-byte store)
 *    n_p is the word that was there; it is never recomputed.  h1, h2, h3 and the variance are not written:
 *    the moments stay those of the unfiltered signal, so the variance goes on describing the noise of the
 *    input, not of the filter's output.  The filter's input is the temporal image, not h0: a second call in
 *    the same frame with the same arguments writes the same words.  I' and h0 are in the same units because
 *    the DEMODULATE bit must equal the one the moments were made with (pt_denoise_variance's check).  An I'
 *    that overflowed is not fed back: the pixel keeps its unfiltered history and the next step does not skip
 *    it.  A pixel that is not kept (a miss, an emissive hit, a variance that is negative or not finite) keeps
 *    its history too. */
#define PT_VFEEDBACK_DEFAULT_LEVEL 3
typedef struct pt_vfeedback_params {
    uint32_t level;          /* 1..iterations: the iteration whose output is fed back */
} pt_vfeedback_params;
/* pt_denoise_variance with the feedback into the held history (the set the last moments step wrote, which
 * the next step reads).  Allowed exactly where pt_denoise_variance is, with its refusals, and it ends nothing;
 * in addition PT_ERR_ARG naming `level` unless 1 <= level <= params->iterations, and a null struct is refused.
 * The result goes where pt_denoise_variance's goes, the same words. */
PT_API int pt_denoise_variance_feedback(pt_context *ctx, const pt_vdenoise_params *params,
                                        const pt_vfeedback_params *feedback);
/* The hipEvent time in ms of the feedback kernel (one float).  PT_ERR_STATE until a feedback call has run on
 * the held history. */
PT_API int pt_read_feedback_timing(pt_context *ctx, float *dst);
/* Plane 0..3 of the held history (rows x width float4): (I, n), (N, id), (P, t), (m1, m2, v, 0).  PT_ERR_STATE
 * without a held history; PT_ERR_ARG naming `plane` for a plane above 3, or plane 3 of a history without
 * moments.  What the _image forms take as hist0..3 when a frame is gathered. */
PT_API int pt_read_temporal_history(pt_context *ctx, uint32_t plane, float *dst);
/* The same on host arrays, as pt_denoise_variance_image: hist0 (the h0 a pt_temporal_moments_image step
 * returned) and out_hist0 (the fed h0) are height x width float4.  Errors: pt_last_error(NULL). */
PT_API int pt_denoise_variance_feedback_image(int device, uint32_t width, uint32_t height, const float *color,
                                              const float *plane0, const float *plane1, const float *plane2,
                                              const float *variance, const float *hist0,
                                              const pt_vdenoise_params *params, const pt_vfeedback_params *feedback,
                                              float *out, float *out_hist0);

/* ---- The variance of an adaptive render's image, and the filter guided by it ------------------------
 * pt_render_adaptive keeps, per pixel, m1 = sum y, m2 = sum y^2 and n, y being the luminance of each call's
 * colour sum: what an error estimate is made of.  Rule 5 turns them into the per-pixel variance that rule 3
 * (the variance-guided filter above) takes, so that one adaptively rendered still image can be filtered with a
 * per-pixel colour weight and without a temporal history.  All float32, no contraction, + - x /, compares and
 * selects only; lum, clamp0 and "finite" as above.  tests/adaptive_variance_model.py restates the rule.
 *
 * 5. The variance of an adaptive render's image.  Per pixel p: the colour C_p = accum_p / (float)max(n_p, 1)
 *    (the image pt_denoise filters after an adaptive render), the feature planes of the last
 *    pt_render_features (A, id; N, t; P, flags), and m1_p, m2_p, n_p.  Parameters: pt_adaptive_variance_params.
 *     D_p = pt_denoise's: per channel  A > 1/64 ? A : 1/64  when DEMODULATE, else 1;   I_p = C_p / D_p
 *     l_p = lum(I_p);   g_p = DEMODULATE ? lum(D_p) : 1
 *     ok_p = HIT && !EMISSIVE && l_p finite && every component of N_p, P_p finite
 *     !ok_p, or n_p < 2, or m1_p or m2_p not finite:  var_p = -1
 *     otherwise the batch-means variance of the mean, in adapt_flag_kernel's operations up to se2 (the
 *     convergence rule of pt_render_adaptive forms the same words):
 *         k = (float)n;  mean = m1 / k;  ss = m2 - m1 * mean;  if (ss < 0) ss = 0;  se2 = ss / (k * (k - 1))
 *         own = clamp0(se2 / (g_p * g_p))
 *       The units match with no spp in the rule: y is the luminance of a call's sum and C the accumulation
 *       over n, so se2 is the variance of lum(C_p).  Dividing by lum(D)^2 takes it to the variance of l_p
 *       exactly for a grey albedo (D.x = D.y = D.z) and approximately otherwise: lum(C / D) is not
 *       lum(C) / lum(D) when the channels of D differ.
 *     n_p >= min_batches:  var_p = own
 *     otherwise (a young pixel) the 7 x 7 same-surface window of rule 2 at unit spacing:
 *       k = 0, s1 = 0, s2 = 0;  m = sigma_plane * t_p;  mm = m * m
 *       for dy = -3 .. 3 (outer), dx = -3 .. 3 (inner), q = p + (dx, dy):
 *       the centre tap always counts; any other tap is skipped (by a select; its index is clamped into the
 *       image before the load) when q is outside the image, or !ok_q, or N_p . N_q < normal_cos_min, or with
 *       g = N_p . (P_q - P_p)  !(g*g <= mm), or SAME_PRIMITIVE is set and id_q != id_p;  otherwise
 *         k = k + 1;  s1 = s1 + l_q;  s2 = s2 + l_q * l_q
 *       mean = s1 / k;  vs = clamp0(s2 / k - mean * mean);  var_p = vs > own ? vs : own
 *     The maximum is what the window is for.  A pixel whose few calls all returned the same value (the
 *     zero-variance dark pixel of a noisy neighbourhood) has own = 0 exactly; with den = variance_floor alone
 *     rule 3's colour weight would shut out every neighbour and leave it as a speck.  The spread of its
 *     same-surface neighbourhood is the evidence that it is not converged.
 *    Accepted: min_batches 2..255, sigma_plane >= 1e-6 and finite, normal_cos_min -1..1, flags within
 *    PT_DENOISE_DEMODULATE | PT_DENOISE_SAME_PRIMITIVE; anything else (a NaN included) is PT_ERR_ARG and the
 *    message names the field.
 *    The filter is rule 3 unchanged, with color = C and var = this rule's output; its DEMODULATE bit must be
 *    this rule's. */
/* Defaults of the layers above (C++ Pathtracer::denoiseAdaptive, Python); sigma_plane, normal_cos_min and flags
 * are the shipped values of rule 2 (PT_TEMPORAL_DEFAULT_*).  min_batches and the filter's sigma_l for this source
 * are the minimiser of the sweep of tools/adaptive_variance_probe.py (profiles/adaptive_variance_probe.json,
 * DESIGN.md 5.12); the filter's other defaults are PT_VDENOISE_DEFAULT_*. */
#define PT_AVARIANCE_DEFAULT_MIN_BATCHES 32
#define PT_ADENOISE_DEFAULT_SIGMA_L 2.0f
#define PT_AVARIANCE_DEFAULT_SIGMA_PLANE 0.3f
#define PT_AVARIANCE_DEFAULT_NORMAL_COS_MIN 0.0f
#define PT_AVARIANCE_DEFAULT_FLAGS 1u
typedef struct pt_adaptive_variance_params {
    uint32_t min_batches;    /* calls from which a pixel's own batch-means estimate is trusted */
    float sigma_plane;       /* relative to the hit distance */
    float normal_cos_min;
    uint32_t flags;          /* PT_DENOISE_DEMODULATE, PT_DENOISE_SAME_PRIMITIVE */
} pt_adaptive_variance_params;

/* Rule 5 on the context's adaptive render and planes, then rule 3 with that variance: the colour (per-pixel
 * division, as pt_denoise after an adaptive render), the estimate, the filter.  The result goes where
 * pt_denoise's goes (pt_read_denoised, pt_tonemap_denoised, pt_read_denoise_timing).  params->staging selects
 * the form of the estimate kernel as it does the filter's (0 automatic, 1 staged in LDS, 2 unstaged).  The
 * accumulation, RNG, moments, counts, tile costs and run-ahead stash are not written.  PT_ERR_STATE, naming the
 * reason, unless an adaptive render describes the buffer and the feature planes are current; PT_ERR_ARG on a
 * band partition and when the DEMODULATE bits of the two parameter sets differ.  A refused call changes nothing.
 * "The held variance is of the counts" from the end of this call until a launch writes the accumulation (a
 * render, the next adaptive render) or pt_render_features begins. */
PT_API int pt_denoise_adaptive(pt_context *ctx, const pt_adaptive_variance_params *variance,
                               const pt_vdenoise_params *params);
/* The variance of the last pt_denoise_adaptive (rows x width float; -1 where rule 5 gives none) and the
 * hipEvent time in ms of its adaptive_variance_kernel (one float; the per-pixel pass before it is not in it).
 * PT_ERR_STATE unless the held variance is of the counts. */
PT_API int pt_read_adaptive_variance(pt_context *ctx, float *dst);
PT_API int pt_read_adaptive_variance_timing(pt_context *ctx, float *dst);
/* Rule 5 on host arrays, without a context (as pt_denoise_variance_image), for a gathered frame: color and the
 * planes are height x width float4, moments is height x width x 3 as pt_read_moments returns it (m1, m2, n as
 * uint32 bits), out_variance height x width float.  staging 0..2 as above.  The filter on host arrays is
 * pt_denoise_variance_image.  Errors: pt_last_error(NULL). */
PT_API int pt_adaptive_variance_image(int device, uint32_t width, uint32_t height, const float *color,
                                      const float *plane0, const float *plane1, const float *plane2,
                                      const float *moments, const pt_adaptive_variance_params *params,
                                      uint32_t staging, float *out_variance);

/* ---- Despike: a same-surface firefly clamp ahead of the filters ------------------------------------
 * An edge-stopping colour weight leaves a firefly where it is, and only the variance-guided filters pull an
 * outlier in.  Rule 6 clamps a pixel whose luminance stands far above its same-surface neighbourhood's, before any
 * filter sees it: one Jacobi pass (every neighbour is read unclamped, so no order of pixels matters).  All float32,
 * no contraction, + - x /, compares and selects only; lum, "finite" and every dot product as above.
 * tests/despike_model.py restates the rule.
 *
 * 6. Per pixel p: the colour C_p and the feature planes (A, id; N, t; P, flags).  Parameters: pt_despike_params.
 *     D_p = pt_denoise's: per channel  A > 1/64 ? A : 1/64  when DEMODULATE, else 1;   I_p = C_p / D_p
 *     l_p = lum(I_p)
 *     ok_p = HIT && !EMISSIVE && l_p finite && every component of N_p, P_p finite        (rule 5's ok)
 *     !ok_p:  out_p.xyz = C_p.xyz, and p is never anyone's neighbour
 *     otherwise  top[0..3] = -inf, k = 0;  m = sigma_plane * t_p;  mm = m * m
 *       for dy = -radius .. radius (outer), dx = -radius .. radius (inner), q = p + (dx, dy), the centre left out:
 *       a tap is skipped (by a select; its index is clamped into the image before the load) when q is outside
 *       the image, or !ok_q, or N_p . N_q < normal_cos_min, or with g = N_p . (P_q - P_p)  !(g*g <= mm), or
 *       SAME_PRIMITIVE is set and id_q != id_p;  otherwise
 *         k = k + 1;  v = l_q;  for j = 0 .. 3 in order:  if (v > top[j]) swap(v, top[j])
 *       (top holds the four largest accepted luminances, largest first; the compare is strict and the taps come
 *       in this order, which fixes which of +0 and -0 is kept)
 *     k < min_neighbors:  out_p.xyz = C_p.xyz
 *     otherwise  M = top[rank - 1];  limit = factor * M + floor;  spike = (limit >= 0) && (l_p > limit)
 *       spike:   s = limit / l_p;  out_p.xyz = (I_p * s) * D_p          (per channel; s lies in [0, 1))
 *       else:    out_p.xyz = C_p.xyz                                    (the input words, not I_p * D_p)
 *     out_p.w = 1.   count = the number of spikes.
 *    `rank` is how many equally bright neighbours a pixel may have and still be a spike: 1 catches single pixels,
 *    2..4 catch clusters.  `floor` keeps a lone lit pixel among black neighbours from being scaled to zero.
 *    Accepted: radius 1..3, rank 1..4, factor >= 1 and finite, floor >= 0 and finite, min_neighbors from rank to
 *    (2 radius + 1)^2 - 1, sigma_plane >= 1e-6 and finite, normal_cos_min -1..1, flags within PT_DENOISE_DEMODULATE |
 *    PT_DENOISE_SAME_PRIMITIVE, staging 0..2; anything else (a NaN included) is PT_ERR_ARG and the message names
 *    the field.
 *    Two kernels: a flat pass packs what a tap needs, (N, l) and (P, id), l not finite where the pixel is not ok
 *    (rule 5's layout); despike_kernel runs on the filter's 32 x 8 tile, its taps either staged in LDS with a halo
 *    of `radius` (staging 1) or read through the caches (2); 0 = automatic.  The words are the same. */
/* Defaults of the layers above (C++ Pathtracer::despike, Python, the CLI's -despike), chosen by the sweep of
 * tools/despike_probe.py (profiles/despike_probe.json, DESIGN.md 5.13, which also says what they cost in energy);
 * sigma_plane and normal_cos_min are the shipped values of rule 2 (PT_TEMPORAL_DEFAULT_*). */
#define PT_DESPIKE_DEFAULT_RADIUS 1
#define PT_DESPIKE_DEFAULT_RANK 2
#define PT_DESPIKE_DEFAULT_FACTOR 4.0f
#define PT_DESPIKE_DEFAULT_FLOOR 0.2f
#define PT_DESPIKE_DEFAULT_MIN_NEIGHBORS 3
#define PT_DESPIKE_DEFAULT_SIGMA_PLANE 0.3f
#define PT_DESPIKE_DEFAULT_NORMAL_COS_MIN 0.0f
#define PT_DESPIKE_DEFAULT_FLAGS 2u
typedef struct pt_despike_params {
    uint32_t radius;         /* the window is (2 radius + 1)^2 - 1 taps */
    uint32_t rank;           /* the limit follows the rank-th largest accepted neighbour */
    float factor;
    float floor;             /* in units of the (demodulated) luminance */
    uint32_t min_neighbors;  /* accepted taps below which the pixel is left alone */
    float sigma_plane;       /* relative to the hit distance */
    float normal_cos_min;
    uint32_t flags;          /* PT_DENOISE_DEMODULATE, PT_DENOISE_SAME_PRIMITIVE */
    uint32_t staging;
} pt_despike_params;

/* Rule 6 on the context's image -- pt_denoise's: accumulation * (1 / max(frames, 1)), or accumulation / n per pixel
 * while pt_holds_adaptive -- with the planes of the last pt_render_features; the result is the context's despiked
 * image.  It refuses exactly what pt_denoise refuses, with the same codes (PT_ERR_ARG for the parameters and on a
 * band partition, PT_ERR_STATE without current planes).  The accumulation, RNG, moments, counts, tile costs and
 * run-ahead stash are not written, and a refused call changes nothing.
 * "A despiked image is held, of the accumulation and the planes the context holds" from the end of this call until
 * the next one begins, a launch writes the accumulation (a render, an adaptive render), pt_render_features begins,
 * a scene or texture change, or a sky change to another handle. */
PT_API int pt_despike(pt_context *ctx, uint32_t frames, const pt_despike_params *params);
/* 1 while a despiked image is held, else 0 (as pt_holds_adaptive: a question, never an error). */
PT_API int pt_holds_despiked(const pt_context *ctx);
/* The held despiked image (rows x width float4, w = 1), its tonemap (pt_tonemap_denoised's arithmetic; RGBA8),
 * the number of spikes (one uint32) and the hipEvent times in ms of the two kernels (2 floats: the flat pass,
 * despike_kernel).  PT_ERR_STATE unless a despiked image is held. */
PT_API int pt_read_despiked(pt_context *ctx, float *dst);
PT_API int pt_tonemap_despiked(pt_context *ctx, uint8_t *dst);
PT_API int pt_read_despike_count(pt_context *ctx, uint32_t *dst);
PT_API int pt_read_despike_timing(pt_context *ctx, float *dst);
/* pt_denoise's filter with the held despiked image as its colour (as pt_denoise_temporal takes the temporal
 * image); the result goes where pt_denoise's goes.  PT_ERR_STATE unless a despiked image is held. */
PT_API int pt_denoise_despiked(pt_context *ctx, const pt_denoise_params *params);
/* Rule 6 on host arrays, without a context (as pt_denoise_image): color, plane0..2 and out are height x width
 * float4 (color's w is ignored), out_count (optional) one uint32.  Errors: pt_last_error(NULL). */
PT_API int pt_despike_image(int device, uint32_t width, uint32_t height, const float *color, const float *plane0,
                            const float *plane1, const float *plane2, const pt_despike_params *params, float *out,
                            uint32_t *out_count);

/* ---- Guided upsampling of a low-resolution image to the full frame -----------------------------------
 * Tracing costs per pixel; the first-hit planes are one ray per pixel.  Rule 8 takes a colour image and its planes
 * at w x h (what was traced, and filtered if wanted) and the planes at W x H (what is shown), and gives every high
 * pixel the demodulated colour of the low pixels around it that lie on its surface, times its own albedo: texture
 * and silhouettes come from the high planes, lighting from the low image.  All float32, no contraction, + - x /,
 * floor, compares and selects only; "finite" and every dot product as above.  tests/upsample_model.py restates it.
 *
 * 8. Low pixel q: colour C_q and planes (A, id; N, t; P, flags)_q.  High pixel p = (x, y): planes (A, id; N, t;
 *    P, flags)_p.  1 <= w <= W, 1 <= h <= H.  Parameters: pt_upsample_params.
 *    Per low pixel q (a flat pass):
 *     keep_q is pt_denoise's (its Prepare);  raw_q = every component of C_q is finite
 *     F_q = the high pixels p with (xn_p, yn_p) = q (below) and id_p == id_q: q's footprint on its own primitive
 *     D_q = 1 without DEMODULATE;  else, with d(A) = pt_denoise's divisor (A > 1/64 ? A : 1/64 per channel),
 *           F_q empty:  d(A_q);   otherwise  (sum of d(A_p) over F_q, y outer, x inner, begun at 0) / (float)|F_q|
 *     I_q = C_q / D_q
 *    (pt_denoise divides a pixel's colour by its own albedo.  Here that is wrong wherever the albedo is textured: C_q is
 *    the mean of albedo x light over the low pixel, A_q one sample of the albedo, and across a texture edge of contrast
 *    50 : 1 the quotient is off by up to that factor, which every high pixel around q then inherits -- the guided
 *    result measured worse than bilinear on a checker.  The high plane holds several samples of the albedo inside q, and
 *    their mean is what C_q was multiplied by, to within their own sampling error.  With w = W, F_q = {q} and D_q = d(A_p).)
 *    Per high pixel p:
 *     sx = (float)w / (float)W;  u = ((float)x + 0.5f) * sx - 0.5f;  x0 = floor(u);  fx = u - x0
 *     sy = (float)h / (float)H;  v = ((float)y + 0.5f) * sy - 0.5f;  y0 = floor(v);  fy = v - y0
 *     xn = min((int)(((float)x + 0.5f) * sx), w - 1);  yn = min((int)(((float)y + 0.5f) * sy), h - 1)
 *     guide_p = HIT && !EMISSIVE && every component of N_p, P_p finite
 *     guide_p:
 *       m = sigma_plane * t_p;  mm = m * m;  D_p = pt_denoise's divisor of A_p
 *       ring 1:  sumW = 0, sumI = (0, 0, 0);  for j = 0, 1 (outer), i = 0, 1 (inner), q = (x0 + i, y0 + j):
 *         b = (i ? fx : 1 - fx) * (j ? fy : 1 - fy)
 *         the tap is skipped (by a select; its index is clamped into the low image before the load) when q is
 *         outside the low image, when !keep_q, or when SAME_PRIMITIVE is set and id_q != id_p;  otherwise
 *           w_n, w_p = rule 1's, of N_p, P_p, mm and N_q, P_q:
 *             c = N_p . N_q;  c = c > 0 ? c : 0;  normal_power_log2 times: c = c * c;  w_n = c
 *             g = N_p . (P_q - P_p);  w_p = 1 / (1 + (g * g) / mm)
 *           wgt = (b * w_n) * w_p;   sumW = sumW + wgt;   sumI = sumI + wgt * I_q          (per channel)
 *       sumW finite and > 0:  out_p.xyz = (sumI / sumW) * D_p
 *       otherwise ring 2, with both sums begun again at 0:  for dy = -1 .. 2 (outer), dx = -1 .. 2 (inner), the four
 *         taps of ring 1 left out, q = (x0 + dx, y0 + dy):
 *         ex = (float)q.x - u;  ey = (float)q.y - v;  b = 1 / (1 + (ex * ex + ey * ey));  skips and weights as in ring 1
 *         sumW finite and > 0:  out_p.xyz = (sumI / sumW) * D_p,  count_wide = count_wide + 1
 *         otherwise            out_p.xyz = the words of C at (xn, yn),  count_nearest = count_nearest + 1
 *     !guide_p (a miss, an emitter, a guide that is not finite): ring 1 on the raw colour, with b alone:
 *         sumB = 0, sumC = (0, 0, 0);  the tap is skipped when q is outside the low image, when !raw_q, when keep_q,
 *         when flags_q != flags_p (as bits), or, for an EMISSIVE p, when id_q != id_p;  otherwise
 *           sumB = sumB + b;   sumC = sumC + b * C_q
 *         sumB finite and > 0:  out_p.xyz = sumC / sumB;  otherwise the words of C at (xn, yn).  No demodulation
 *         (the sky and the emitters have no albedo to divide by) and no count.
 *     out_p.w = 1
 *    A kept pixel never reaches an unguided one and the other way round, and a pixel that is not finite reaches none.
 *    With w = W and h = H: sx = 1, u = x exactly, fx = 0, so ring 1 has one tap of b = 1 (q = p) and three of b = 0.
 *    A kept p then gives (((1 * w_n) * w_p) * I_p / ((1 * w_n) * w_p)) * D_p with w_n = (N_p . N_p)^(2^power) and
 *    w_p = 1: C_p to within four roundings (I_p's division, the product, the quotient and the demodulation), not the identity; where
 *    w_n underflows to 0 (a normal far from unit length) the pixel goes to ring 2.
 *    Accepted: sigma_plane >= 1e-6 and finite, normal_power_log2 0..7, flags within PT_DENOISE_DEMODULATE |
 *    PT_DENOISE_SAME_PRIMITIVE, staging 0..2 (pt_denoise's ranges); anything else (a NaN included) is PT_ERR_ARG and
 *    the message names the field.
 *    Two kernels: a flat pass over the low image forms D_q from the high plane 0 and packs what a tap needs into three float4, (I or C, class), (N, id),
 *    (P, flags), class = 1 kept, 2 raw and not kept, 0 neither; upsample_kernel takes one high pixel per lane on the
 *    filter's 32 x 8 tile, whose ring-1 footprint of at most 35 x 11 low texels is staged in LDS (staging 1) or read
 *    through the caches (2); 0 = automatic.  Ring 2 and the nearest pixel are always read through the caches.  The
 *    words are the same. */
/* Defaults of the layers above (C++ Pathtracer::upsample, Python, the CLI's -upsample): sigma_plane and the normal
 * power are pt_denoise's shipped values; both flags are set (the low pixel beside a silhouette is of one surface or
 * the other, and the id keeps it from the wrong one). */
#define PT_UPSAMPLE_DEFAULT_SIGMA_PLANE 0.005f
#define PT_UPSAMPLE_DEFAULT_NORMAL_POWER_LOG2 3
#define PT_UPSAMPLE_DEFAULT_FLAGS 3u
typedef struct pt_upsample_params {
    float sigma_plane;       /* relative to the hit distance of the high pixel */
    uint32_t normal_power_log2;
    uint32_t flags;          /* PT_DENOISE_DEMODULATE, PT_DENOISE_SAME_PRIMITIVE */
    uint32_t staging;
} pt_upsample_params;
/* The image of `lo` that pt_upsample takes: the accumulation (pt_denoise's colour: * 1 / max(frames, 1), or / n per
 * pixel while pt_holds_adaptive), or the held denoised, temporal or despiked image. */
#define PT_UPSAMPLE_ACCUM 0u
#define PT_UPSAMPLE_DENOISED 1u
#define PT_UPSAMPLE_TEMPORAL 2u
#define PT_UPSAMPLE_DESPIKED 3u

/* Rule 8 from `lo`'s image and planes to `hi`'s planes; the result is held by `hi` (hi's width x height float4).
 * `frames` is used by PT_UPSAMPLE_ACCUM only.  Refused, naming the reason: PT_ERR_ARG for the parameters, an unknown
 * source, two contexts on different devices, a band partition on either context, and a `lo` larger than `hi` in either
 * dimension; PT_ERR_STATE when the planes of either context are not current, or `lo` does not hold the source (a
 * denoised image; a temporal image made from the planes it holds; a despiked image).  Errors are `hi`'s
 * (pt_last_error(hi)).  Nothing of either context's render state is written, nothing at all of `lo` changes, and a
 * refused call changes nothing.
 * "An upsampled image is held" by `hi` from the end of this call until the next one begins (as the denoised image). */
PT_API int pt_upsample(pt_context *hi, pt_context *lo, uint32_t source, uint32_t frames,
                       const pt_upsample_params *params);
/* 1 while an upsampled image is held, else 0 (a question, never an error). */
PT_API int pt_holds_upsampled(const pt_context *ctx);
/* The held upsampled image (rows x width float4, w = 1), its tonemap (pt_tonemap_denoised's arithmetic; RGBA8), the
 * two counts (2 x uint32: guided pixels that needed ring 2, guided pixels that took the nearest low pixel) and the
 * hipEvent times in ms of the two kernels (2 floats: the flat pass, upsample_kernel).  PT_ERR_STATE unless an upsampled
 * image is held. */
PT_API int pt_read_upsampled(pt_context *ctx, float *dst);
PT_API int pt_tonemap_upsampled(pt_context *ctx, uint8_t *dst);
PT_API int pt_read_upsample_counts(pt_context *ctx, uint32_t *dst);
PT_API int pt_read_upsample_timing(pt_context *ctx, float *dst);
/* Rule 8 on host arrays, without a context: color and lo_plane0..2 are lo_h x lo_w float4 (color's w is ignored),
 * hi_plane0..2 and out are hi_h x hi_w float4, out_counts (optional) 2 x uint32.  Errors: pt_last_error(NULL). */
PT_API int pt_upsample_image(int device, uint32_t lo_w, uint32_t lo_h, const float *color, const float *lo_plane0,
                             const float *lo_plane1, const float *lo_plane2, uint32_t hi_w, uint32_t hi_h,
                             const float *hi_plane0, const float *hi_plane1, const float *hi_plane2,
                             const pt_upsample_params *params, float *out, uint32_t *out_counts);

/* ---- Guided upsampling onto supersampled feature planes ---------------------------------------------
 * Rule 8's high planes are one first-hit sample per pixel, so its result is stair-stepped along every silhouette.
 * Rule 9 runs rule 8 onto the planes of an S-times larger frame of the same camera (S x S first-hit samples per
 * output pixel, each jittered inside its own sub-pixel by pt_render_features) and gives every output pixel the mean
 * of its S x S results; the S-times image is never written.  All float32, no contraction, + and / only beyond rule 8.
 * tests/upsample_resolve_model.py restates it.
 *
 * 9. A low image and its planes at w x h (rule 8's), planes at S W x S H, a factor S in {2, 3, 4}, pt_upsample_params.
 *    1 <= w <= W and 1 <= h <= H, and the S-times frame within rule 8's sizes (S W x S H < 2^30 pixels).
 *    rule8(x, y) below is rule 8 with its W, H = S W, S H: sx = (float)w / (float)(S W), and so on.
 *    The flat pass is rule 8's at the S-times size: F_q holds the S-times pixels whose nearest low pixel is q and that
 *    carry its id, so D_q is a mean over up to S^2 K^2 albedo samples at a ratio of K.
 *    Per output pixel (X, Y):
 *     sum = (0, 0, 0)
 *     for j = 0 .. S - 1 (outer), i = 0 .. S - 1 (inner):  sum = sum + rule8(S X + i, S Y + j).xyz      (per channel)
 *     out.xyz = sum / (float)(S * S);   out.w = 1
 *    The mean is of linear radiance, as an accumulation's is.  count_wide and count_nearest are rule 8's, summed over
 *    all S W x S H sub-pixels.  A sub-pixel that is not finite makes its output pixel not finite (inf and -inf give
 *    NaN); buffers compare as "words equal, or both NaN".
 *    The staged rectangle: an output tile of 32 x 8 covers the S-times pixels S X0 .. S X0 + 32 S - 1, whose u differ
 *    by (32 S - 1) * (w / (S W)) < 32 w / W <= 32; two reals less than 32 apart have floors at most 32 apart, so ring 1
 *    reaches at most 32 + 2 = 34 columns and likewise 8 + 2 = 10 rows: within rule 8's 35 x 11 and the same LDS.  (In
 *    float32 the coordinates of a frame wider than 2^24 are not exact; a rectangle that did not fit is read through
 *    the caches, the same words.)
 *    Two kernels: rule 8's flat pass, then upsample_resolve_kernel, one output pixel per lane on the 32 x 8 tile,
 *    the lane walking its S x S sub-pixels in the rule's order; staging as rule 8. */
/* Rule 9 from `lo`'s image and planes and `planes`' planes; the result is held by `hi` (hi's width x height float4) as
 * its upsampled image: pt_holds_upsampled, pt_read_upsampled, pt_tonemap_upsampled, pt_read_upsample_counts and
 * pt_read_upsample_timing (the flat pass, upsample_resolve_kernel) serve it as they serve pt_upsample's.  `hi` needs
 * neither planes nor a render.  Refused, naming the reason: PT_ERR_ARG for a null argument, the parameters, an unknown
 * source, contexts on different devices, a band partition on any of the three, a factor outside 2..4, a `planes` that
 * is not exactly factor x `hi` in both dimensions, a `lo` larger than `hi` in either dimension; PT_ERR_STATE when the
 * planes of `planes` or of `lo` are not current, or `lo` does not hold the source.  Errors are `hi`'s.  Nothing of any
 * render state is written, nothing at all of `lo` or `planes` changes, and a refused call changes nothing. */
PT_API int pt_upsample_resolve(pt_context *hi, pt_context *planes, pt_context *lo, uint32_t source, uint32_t frames,
                               uint32_t factor, const pt_upsample_params *params);
/* Rule 9 on host arrays, without a context: color and lo_plane0..2 are lo_h x lo_w float4, ss_plane0..2 are
 * ss_h x ss_w float4 (the S-times planes), out is (ss_h / factor) x (ss_w / factor) float4, out_counts (optional)
 * 2 x uint32.  PT_ERR_ARG also when factor does not divide ss_w and ss_h.  Errors: pt_last_error(NULL). */
PT_API int pt_upsample_resolve_image(int device, uint32_t lo_w, uint32_t lo_h, const float *color, const float *lo_plane0,
                                     const float *lo_plane1, const float *lo_plane2, uint32_t ss_w, uint32_t ss_h,
                                     const float *ss_plane0, const float *ss_plane1, const float *ss_plane2,
                                     uint32_t factor, const pt_upsample_params *params, float *out,
                                     uint32_t *out_counts);

/* ---- Moving objects in the temporal passes --------------------------------------------------------
 * Rule 3 (temporal reprojection) and rule 4's first part (the step with moments) project one world point with
 * two cameras: only the camera may move.  Rule 7 is the same step when the objects moved too: a per-primitive
 * affine map takes a surface point of the current scene to where that object point was in the scene the held
 * history was made from.  All float32, operation by operation, no contraction, + - x /, floor, compares and
 * selects only; every dot product as above.  tests/motion_model.py restates it.
 *
 * 7. The motion table, one entry per primitive i of the CURRENT scene (prim_count entries, at least 1):
 *     rows[i]        12 floats, a 3 x 4 row-major affine map T_i (T00 T01 T02 T03 | T10 .. | T20 ..): a world-space
 *                    point on primitive i now -> the world-space place that object point had in the earlier scene
 *     prev_index[i]  that primitive's index in the earlier scene, or 0xffffffff: "was not there, take no history
 *                    for its pixels"
 *    The table is meant to be rigid (a rotation and a translation).  Nothing checks that: under a scale or a shear
 *    Nm below is neither unit length nor the normal of the earlier surface, and the plane test's margin, which is
 *    relative to the current hit distance, no longer measures the earlier geometry.
 *    Per ok pixel p (rule 3's ok_p), with i = id_p (plane 0's w, as bits):
 *     i >= prim_count:  the pixel is treated as prev_index == 0xffffffff; the index is clamped (to 0) before the
 *                       load, as the taps' indices are clamped.  Only the _image forms can meet this.
 *     Pm.x = ((T00*P.x + T01*P.y) + T02*P.z) + T03,  Pm.y and Pm.z likewise with rows 1 and 2
 *     Nm.x = (T00*N.x + T01*N.y) + T02*N.z,          Nm.y and Nm.z likewise; Nm is not normalised
 *     (su0, sv0, z0) = project(cur, P_p);  (su1, sv1, z1) = project(prev, Pm);  fx, fy as in rule 3
 *     reproj = rule 3's condition && prev_index[i] != 0xffffffff       (a NaN in T_i fails the compares by itself)
 *     the taps are rule 3's with the moved quantities on the p side: a tap is skipped when  !(w > 0),  or q is
 *       outside the image,  or n_q < 1,  or a component of I_q is not finite,  or SAME_PRIMITIVE is set and
 *       id_q != prev_index[i],  or Nm . N_q < normal_cos_min,  or, with g = Nm . (P_q - Pm) and
 *       m = sigma_plane * t_p,  !(g*g <= m*m)
 *     everything else is rule 3 unchanged: the weights, the sums, n, the blend, demodulation, the !ok pass-through
 *     h1 = (N_p, id_p), h2 = (P_p, t_p): the CURRENT scene's words, so the new history is of the current scene
 *    The moments step (rule 4, part 1) takes the same substitution; its moment sums ride on the same taps, and the
 *    variance estimate (part 2) reads only the new history and is unchanged.
 *    With rows = the identity and prev_index[i] = i the words are rule 3's and rule 4's.
 *    Two kernels of their own, temporal_motion_kernel and temporal_moments_motion_kernel, on the same 32 x 8 tile;
 *    an entry is four float4 (the rows, then prev_index's bits), read in whole 16-byte loads through the caches.
 *
 * Not covered: device groups (pt_group_set_scene is unchanged and ends the history); the command-line tool (a
 * still has no previous frame); and lighting that a moving object changes on OTHER surfaces -- its shadow, its
 * bounce light -- which still fades over 1 / alpha_min frames. */
/* pt_set_scene with a motion table.  Everything pt_set_scene does: the same validation and the same refusals, the
 * previous scene intact on a refusal.  Also PT_ERR_ARG, naming the primitive, for a prev_index entry that is neither
 * 0xffffffff nor below the primitive count of the scene it replaces, and for a null table.  The history survives:
 * "a motion table is held that maps the current scene to the scene of the held history" from this call, made while
 * a history is held, until the next temporal pass begins (after it the history is of the current scene), a scene
 * or texture change, or a sky change to another handle.  One move per temporal step: a second pt_set_scene_moved
 * before the next pass would need the two tables composed, so it ends the history, its moments and the table.
 * Without a held history the call is pt_set_scene.  The feature planes end as with pt_set_scene. */
PT_API int pt_set_scene_moved(pt_context *ctx, const pt_bvh_node *nodes, uint32_t node_count, const pt_hittable *prims,
                              uint32_t prim_count, const float *motion_rows, const uint32_t *prev_index);
/* 1 while a motion table is held, else 0 (as pt_holds_despiked: a question, never an error).  While it is,
 * pt_temporal and pt_temporal_moments run rule 7 with the held table (they ask before the pass begins); in every
 * other case they run exactly what they ran before. */
PT_API int pt_holds_motion(const pt_context *ctx);
/* pt_temporal_image and pt_temporal_moments_image under rule 7: their arguments, then the table (motion_rows =
 * prim_count x 12 floats, prev_index = prim_count words; prim_count 1 .. 2^26 - 1).  prev_index is not checked
 * against anything: it is only compared with the history's ids.  For gathered frames and tests. */
PT_API int pt_temporal_motion_image(int device, uint32_t width, uint32_t height, const float *color, const float *plane0,
                                    const float *plane1, const float *plane2, const pt_camera *cur_cam,
                                    const float *hist0, const float *hist1, const float *hist2,
                                    const pt_camera *prev_cam, const pt_temporal_params *params, float *out_image,
                                    float *out_hist0, float *out_hist1, float *out_hist2, uint32_t prim_count,
                                    const float *motion_rows, const uint32_t *prev_index);
PT_API int pt_temporal_moments_motion_image(int device, uint32_t width, uint32_t height, const float *color,
                                            const float *plane0, const float *plane1, const float *plane2,
                                            const pt_camera *cur_cam, const float *hist0, const float *hist1,
                                            const float *hist2, const float *hist3, const pt_camera *prev_cam,
                                            const pt_temporal_params *params, const pt_variance_params *variance,
                                            float *out_image, float *out_hist0, float *out_hist1, float *out_hist2,
                                            float *out_hist3, float *out_variance, uint32_t prim_count,
                                            const float *motion_rows, const uint32_t *prev_index);

/* ---- Moving primitives without a rebuild: the refit -------------------------------------------------
 * pt_set_scene_moved replaces the whole scene: a new tree, four arrays freed, allocated and uploaded.  When the
 * objects only moved, the topology -- which node is whose child, which primitives a leaf holds, the leaf words of the
 * child-box records, the LDS stack rows, dfsOrder -- depends on no box value, and the tree can be REFITTED: the
 * moved primitives' records replaced, and the boxes of the nodes recomputed from the leaves up.  Rule 10 says what a
 * refit computes.  Compares and selects only, so the result is a function of (topology, boxes) alone;
 * tests/refit_model.py restates it.
 *
 * 10. The refit.  Inputs: the tree's topology as pt_set_scene accepted it; one box per primitive i,
 *     B_i = (min[3], max[3]), every word finite and min[k] <= max[k].  For every node reachable from the root:
 *      a leaf with first primitive f and count c:
 *        lo = B_f.min, hi = B_f.max;  then for k = 1 .. c - 1 in index order, with B = B_(f+k), per axis
 *        lo = B.min < lo ? B.min : lo,   hi = B.max > hi ? B.max : hi
 *      an interior node i with children a = i + 1 and b = offset, both done before it:  per axis
 *        lo = b.lo < a.lo ? b.lo : a.lo,   hi = b.hi > a.hi ? b.hi : a.hi
 *     Words written: the node's box takes (lo, hi); offset and primitive_count_axis keep their words.  Where the
 *     context holds child-box records, an interior node's record takes its children's new boxes; its fourth quad
 *     (the child words, the axis bit, the second child's first primitive) keeps its words.  A node that is not
 *     reachable from the root, and its record, keep every word.
 *     With the boxes a host build folded its nodes from, the refit reproduces that build's node boxes as float
 *     values; only the sign of a zero can differ, because the order of the fold differs.
 *     After a refit the tree is no longer the one a fresh build would make for the new poses: it is a valid tree over
 *     them, usually a slower one, and a render equals the oracle walking that same tree (the contract a caller's own
 *     BVH has always had: tie order and the rising-t_max rule depend on the tree).  A fresh pt_set_scene[_moved]
 *     returns to the build's tree.
 *     Kernels: motion_fill_kernel, move_scatter_kernel, refit_leaves_kernel, and refit_level_kernel launched once per
 *     depth of interior nodes, the deepest first (at most 32 launches).  Nothing waits inside a launch.
 *
 * Not covered: device groups (refused by name); adding or removing primitives or changing the topology (use
 * pt_set_scene_moved); two moves in one temporal step (the second ends the history, as with pt_set_scene_moved). */
/* The boxes of the current scene's primitives, prim_count x 6 floats (min xyz, max xyz), which pt_set_scene's
 * arguments do not carry: uploads them, reads the node topology back from the device once and keeps the lists of
 * reachable leaves and of reachable interior nodes by depth.  Nothing of the scene changes and no fact but "the boxes
 * are held" moves.  PT_ERR_ARG naming the primitive and the component for a word that is not finite or a min above
 * its max; PT_ERR_STATE without a scene, or on a context of a device group.  Held until the next pt_set_scene,
 * pt_set_scene_moved or pt_set_texture (a texture touches no box; ending the boxes there spares a second event and
 * costs one more call of this function). */
PT_API int pt_set_primitive_boxes(pt_context *ctx, const float *boxes);
/* 1 while the boxes are held, else 0 (a question, never an error). */
PT_API int pt_holds_primitive_boxes(const pt_context *ctx);
/* Move `count` primitives in place and refit the tree (rule 10).  index: distinct primitive indices of the scene (its
 * element order, as pt_set_scene took them); prims: their whole new records, checked as pt_set_scene checks a
 * primitive; boxes: count x 6, their new boxes, checked as above.
 * With motion_rows (count x 12) and prev_index (count; each its own index[j] or 0xffffffff): rule 7's table is made
 * on the device -- the identity and prev_index = i for every primitive not named, the given entry for the named ones
 * -- and the call raises what pt_set_scene_moved raises: over a held history the history, its moments and the table
 * are held for the next temporal pass; a second move before that pass ends all three.  Without them (both null) the
 * call is a scene change as pt_set_scene is.  Either way the feature planes end, and the boxes stay held.
 * Refused, naming the reason, with no word on the device changed and no event raised: PT_ERR_ARG for a null index,
 * prims or boxes, one of motion_rows and prev_index without the other, count == 0, an index given twice or not below
 * the primitive count, a primitive, box or prev_index that fails its check; PT_ERR_STATE when no boxes are held or
 * the context is part of a device group.
 * One packed host-to-device copy of 208 bytes per moved primitive, then kernels on the context's stream; the root's
 * new box is read back (32 bytes) for the trace kernel's by-value parameter, so the call returns with the work done.
 * A move that fails midway (a HIP error, PT_ERR_HIP) may have written part of its words.  With motion rows it then
 * raises a scene change: no history, no table, and the boxes not held.  Without them it already was a scene change;
 * the boxes stay held (the lists are of the topology, which no move touches).  Either way set the scene again.
 * Only the copy scales with `count`: the table's fill runs over every primitive and the refit over every reachable node.
 * The fast slab test stays chosen as pt_set_scene chose it (a tree that had an unordered reachable box keeps the exact
 * one after a refit has ordered its boxes; the words rendered are the same). */
PT_API int pt_move_primitives(pt_context *ctx, uint32_t count, const uint32_t *index, const pt_hittable *prims,
                              const float *boxes, const float *motion_rows, const uint32_t *prev_index);
/* What the device holds, for tests and diagnosis.  pt_read_bvh: the node_count nodes in pt_bvh_node's layout, and,
 * when records is not null and the context holds child-box records, max(interior nodes, 1) x 16 floats of them (a
 * context without records leaves the array as it was).  pt_read_primitive: dst[0..15] the primitive's four quads,
 * dst[16..27] its material's three. */
PT_API int pt_read_bvh(pt_context *ctx, pt_bvh_node *nodes, float *records);
PT_API int pt_read_primitive(pt_context *ctx, uint32_t index, float *dst);
/* Three floats about the last pt_move_primitives: dst[0] = hipEvent milliseconds of its kernels (the fill, the scatter,
 * the leaves, the levels); dst[1] = host milliseconds of the packing; dst[2] = hipEvent milliseconds of the one
 * host-to-device copy.  PT_ERR_STATE before the first move. */
PT_API int pt_read_refit_timing(pt_context *ctx, float *dst);

/* ---- Multi-device group (one process, one context per GPU, RCCL over xGMI) -------------------
 * Replaces the reference's hard-coded single device (Pathtracer.cpp:40: cudaSetDevice(0)) behind
 * the same Pathtracer interface: device i renders the row bands b = i, i + N, ... of the image
 * (pt_create_banded with band_offset = i, band_stride = N), and pt_group_gather assembles the
 * accumulation buffer on devices[0] with one grouped ncclSend/ncclRecv (communicators from
 * ncclCommInitAll) plus an unpermute kernel.  Seeds use global pixel indices, so the assembled
 * image is bit-identical to a single-device render.  Devices must be distinct. */
typedef struct pt_group pt_group;

PT_API int pt_group_create(int ndev, const int *devices, uint32_t width, uint32_t height, uint32_t band_rows,
                           pt_group **out);
PT_API void pt_group_destroy(pt_group *g);
PT_API int pt_group_size(const pt_group *g);
/* The context of device index i (for per-device calls such as pt_set_kernel_variant). */
PT_API pt_context *pt_group_context(pt_group *g, int index);
PT_API int pt_group_set_scene(pt_group *g, const pt_bvh_node *nodes, uint32_t node_count, const pt_hittable *prims,
                              uint32_t prim_count);
PT_API int pt_group_set_texture(pt_group *g, uint32_t handle, const float *rgba, uint32_t width, uint32_t height);
PT_API int pt_group_set_skybox(pt_group *g, uint32_t handle);
/* pt_render on every device concurrently (one host thread each); gpu_ms = the slowest device. */
PT_API int pt_group_render(pt_group *g, const pt_camera *camera, uint32_t spp, uint32_t chunks, int ignore_history,
                           float *gpu_ms);
/* RCCL gather of every device's accumulation rows to devices[0] + unpermute into the full image;
 * host_ms (optional) = wall time of the gather. */
PT_API int pt_group_gather(pt_group *g, float *host_ms);
/* Full-image raw accumulation (height x width float4, y-up) / tonemap (RGBA8), gathering first if
 * the image changed since the last gather. */
PT_API int pt_group_read_accum(pt_group *g, float *dst);
PT_API int pt_group_tonemap(pt_group *g, uint32_t frames, uint8_t *dst);
PT_API const char *pt_group_last_error(const pt_group *g);

#ifdef __cplusplus
}
#endif

#endif /* PT_HIP_H */
