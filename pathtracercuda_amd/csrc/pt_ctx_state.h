// pt_ctx_state.h -- what a context carries from one call to the next, and every rule that moves it:
// no HIP call, no context, plain values.  The C ABI functions (pt_kernels.hip, pt_denoise.h, pt_temporal.h, pt_svgf.h,
// pt_adaptive_variance.h, pt_despike.h, pt_upsample.h, pt_refit.h)
// raise the events below and ask the predicates; they assign none of these fields themselves.
// tools/ctx_state_check.cpp and tests/test_ctx_state.py run the same functions on the CPU.
//
// The facts, what each means and which events end it (DESIGN.md 5.8 has the host layer's flags):
//   order           the tile cost order (pt_launch_plan.h).  `stale`: it is not of this scene, textures,
//                   camera and schedule -- set by each of those changing and when its buffers are
//                   replaced or it is dropped, cleared when a launch sorts it.  Scheduling only.
//   stateEpoch      counts the changes of what a sample depends on besides the camera: scene, a texture,
//                   a changed sky, an RNG write, an adaptive render.  Never decreases.
//   launched, lastCam, lastState
//                   the camera and stateEpoch of the last render: the key of a run-ahead stash.
//   aheadValid      the last render made a run-ahead stash.  Every render and every adaptive render
//                   consumes or drops it; the next render uses it only under the same key.
//   aheadMisses     consecutive renders whose key had changed (at most 1000); from 2 on plan_launch
//                   stops making stashes.
//   adCountsValid   "the counts describe the buffer": set when an adaptive render is done, ended only by
//                   a launch that writes the accumulation (a render, the next adaptive render).  The
//                   adaptive reads, pt_denoise's per-pixel division and Pathtracer::adaptive() follow it.
//   adMomValid      "the moments can be continued": the former, and also ended by a scene, texture or
//                   sky change and an RNG write.  Implies adCountsValid; only reset = 0 asks for it.
//   featValid       the feature planes are of the current scene and textures: set when a features call
//                   is done, ended by its beginning and by a scene or texture change.
//   dnValid         a denoised image is held: ended when a denoise has passed its checks, set when it is
//                   done, so only a denoise that fails midway (a HIP error) leaves none.
//   tpValid         a temporal image is held (pt_read_temporal): ended when a temporal pass has passed its
//                   checks, set when it is done.
//   histValid       a history is held, which the next temporal pass may reproject: set when a temporal pass
//                   is done, ended by its beginning, by a scene or texture change and by a sky change to
//                   another handle (the colours it holds are of that scene and sky).  A camera change, a
//                   render and an RNG write end nothing: moving the camera is what the pass is for, and new
//                   samples of the same scene are what it blends in.  Implies tpValid.
//   tpOfPlanes      the temporal image was made from the planes the context holds now (pt_denoise_temporal's
//                   guide): set when a temporal pass is done, ended by its beginning and by the beginning
//                   of a features call.  Implies tpValid.
//   momValid        the held history has moments (a fourth plane, and the variance estimated from it:
//                   pt_temporal_moments, pt_read_temporal_variance, pt_denoise_variance): set when a moments
//                   step is done, ended by whatever ends the history -- a pt_temporal step included, which
//                   begins as every temporal pass and sets it no more.  Implies histValid.
//   avValid         "the held variance is of the counts" (pt_read_adaptive_variance and its timing): set when a
//                   pt_denoise_adaptive is done, ended by its beginning, by whatever ends adCountsValid (a launch
//                   that writes the accumulation) and by the beginning of a features call (it was made with the
//                   planes held then).  Implies adCountsValid.
//   dsValid         "a despiked image is held, of the accumulation and the planes the context holds" (pt_read_despiked,
//                   its tonemap, count and timing, pt_denoise_despiked): set when a pt_despike is done, ended by its
//                   beginning, by a launch that writes the accumulation (a render, an adaptive render), by the
//                   beginning of a features call, by a scene or texture change and by a sky change to another handle.
//                   An RNG write and a camera change end nothing: neither touches the image or the planes.
//   motionValid     "a motion table is held that maps the current scene to the scene of the held history" (rule 7 of
//                   include/pt_hip.h; pt_holds_motion, and pt_temporal / pt_temporal_moments run the motion kernels
//                   while it holds): set by scene_moved over a held history, ended by the beginning of a temporal pass
//                   (after it the history is of the current scene, or there is none), by a scene or texture change,
//                   by a sky change to another handle, and by a second scene_moved (one move per temporal step: the
//                   two tables would have to be composed, so the history ends with it).  A render, a camera change,
//                   an RNG write and a features call end nothing.  Implies histValid.
//   usValid         an upsampled image is held (pt_read_upsampled, its tonemap, counts and timing), by the context of the
//                   larger frame: ended when a pt_upsample has passed its checks, set when it is done (dnValid's rule: the
//                   image is a result handed out, and what it was made from may move on).  Nothing else ends it, and
//                   the context of the smaller frame raises no event.
//   boxValid        "the per-primitive boxes and the refit lists are of the current scene" (rule 10 of include/pt_hip.h;
//                   pt_holds_primitive_boxes, and pt_move_primitives asks for it): set by pt_set_primitive_boxes, ended
//                   by a scene or texture change, kept by a move (primitives_moved), which keeps the topology and
//                   replaces the boxes of what it moves.  A texture change ends it too although it touches no box:
//                   that costs one more pt_set_primitive_boxes and spares a second event.  Tied to no other fact.
//   epoch           counts the launches that wrote the accumulation (a device group's gather cache
//                   key, pt_group.h).  Never decreases.
// A call refused for its arguments or for the state raises no event (but for a render whose plan is a
// refusal: DESIGN.md 8).
#pragma once
#include <cstring>

#include "../../include/pt_hip.h"
#include "pt_launch_plan.h"

namespace pt {

struct CtxState {
    OrderState order;
    uint64_t stateEpoch = 0, lastState = 0;
    bool launched = false;
    pt_camera lastCam = {};
    bool aheadValid = false;
    uint32_t aheadMisses = 0;
    bool adMomValid = false, adCountsValid = false;
    bool featValid = false, dnValid = false;
    bool tpValid = false, histValid = false, tpOfPlanes = false;
    bool momValid = false;
    bool avValid = false;
    bool dsValid = false;
    bool motionValid = false;
    bool usValid = false;
    bool boxValid = false;
    uint64_t epoch = 0;
};

// ---- events ---------------------------------------------------------------------------------------
// pt_set_scene, pt_set_texture
inline void scene_or_texture_changed(CtxState& s)
{
    s.order.stale = true;
    s.adMomValid = false;
    s.featValid = false;
    s.histValid = false;
    s.momValid = false;
    s.dsValid = false;
    s.motionValid = false;
    s.boxValid = false;
    ++s.stateEpoch;
}

// pt_set_scene_moved: a scene change that comes with a motion table.  The history and its moments survive the first
// move after a temporal pass and the table is held beside them; a second move before the next pass ends all three
// (one move per temporal step).  Everything else is scene_or_texture_changed's.
inline void scene_moved(CtxState& s)
{
    const bool hist = s.histValid && !s.motionValid, mom = s.momValid && !s.motionValid;
    scene_or_texture_changed(s);
    s.histValid = hist;
    s.momValid = mom;
    s.motionValid = hist;
}

// pt_set_primitive_boxes
inline void boxes_set(CtxState& s) { s.boxValid = true; }

// pt_move_primitives: scene_moved when the move comes with a motion table, a scene change when it does not; either
// way the boxes stay, because the move has replaced those of what it moved and the topology is what it was
inline void primitives_moved(CtxState& s, bool with_table)
{
    const bool boxes = s.boxValid;
    if (with_table) scene_moved(s);
    else scene_or_texture_changed(s);
    s.boxValid = boxes;
}

// pt_set_skybox while `held` is set: only another handle changes anything (the planes hold first hits: no
// sky in them)
inline void sky_set(CtxState& s, uint32_t held, uint32_t handle)
{
    if (held == handle) return;
    ++s.stateEpoch;
    s.adMomValid = false;
    s.histValid = false;
    s.momValid = false;
    s.dsValid = false;
    s.motionValid = false;
}

// pt_write_rng: a stash and the moments continue the old streams
inline void rng_written(CtxState& s)
{
    ++s.stateEpoch;
    s.adMomValid = false;
}

inline void schedule_changed(CtxState& s) { s.order.stale = true; }

// the launch's K differs from the order's (LaunchPlan::dropOrder)
inline void order_dropped(CtxState& s)
{
    s.order.valid = false;
    s.order.stale = true;
}

// the order's buffers are replaced by ones of another size
inline void order_replaced(CtxState& s) { order_dropped(s); }

// the order was sorted from the tile costs of a launch of `samples` per pixel in units of `strip` tiles
inline void order_sorted(CtxState& s, uint64_t samples, uint32_t strip)
{
    s.order.samples = samples;
    s.order.strip = strip;
    s.order.valid = true;
    s.order.stale = false;
}

// those costs were measured under issue priority: the next launch rebuilds the order whatever it samples
inline void order_biased(CtxState& s) { s.order.samples = 0; }

// A render begins under `cam`.  The stash of the previous render matches when this one has its camera,
// scene, textures, sky and RNG state.
struct RenderStart {
    bool stashMatches;
    uint32_t aheadMisses;
};
inline RenderStart render_begins(CtxState& s, const pt_camera& cam)
{
    s.adMomValid = false;                 // the moments and counts of an adaptive render no longer describe the buffer
    s.adCountsValid = false;
    s.avValid = false;
    s.dsValid = false;
    const bool sameCam = memcmp(&s.lastCam, &cam, sizeof(pt_camera)) == 0;
    const bool sameKey = s.launched && sameCam && s.lastState == s.stateEpoch;
    s.aheadMisses = sameKey ? 0u : std::min(s.aheadMisses + 1u, 1000u);
    const bool stashMatches = s.aheadValid && sameKey;
    s.aheadValid = false;                 // consumed or dropped; a making launch sets it again
    s.launched = true;
    s.lastState = s.stateEpoch;
    if (!sameCam) {
        s.order.stale = true;
        s.lastCam = cam;
    }
    return {stashMatches, s.aheadMisses};
}

inline void accum_written(CtxState& s) { ++s.epoch; }

inline void stash_made(CtxState& s) { s.aheadValid = true; }

// the accumulation and the RNG streams move on: a stash of the old state is void; the cost order and
// the tile costs stay as they were (an adaptive render dispatches no tiles)
inline void adaptive_begins(CtxState& s)
{
    s.aheadValid = false;
    ++s.stateEpoch;
    accum_written(s);
    s.adMomValid = false;                 // until the render is complete
    s.adCountsValid = false;
    s.avValid = false;
    s.dsValid = false;
}

inline void adaptive_done(CtxState& s)
{
    s.adMomValid = true;
    s.adCountsValid = true;
}

inline void features_begin(CtxState& s)
{
    s.featValid = false;
    s.tpOfPlanes = false;
    s.avValid = false;
    s.dsValid = false;
}
inline void features_done(CtxState& s) { s.featValid = true; }
inline void denoise_begins(CtxState& s) { s.dnValid = false; }
inline void denoise_done(CtxState& s) { s.dnValid = true; }
inline void temporal_begins(CtxState& s)
{
    s.tpValid = false;
    s.histValid = false;
    s.tpOfPlanes = false;
    s.momValid = false;
    s.motionValid = false;
}
inline void temporal_done(CtxState& s)
{
    s.tpValid = true;
    s.histValid = true;
    s.tpOfPlanes = true;
}
// a moments step raises temporal_begins, temporal_done and then this
inline void moments_done(CtxState& s) { s.momValid = s.histValid; }
// pt_denoise_adaptive raises denoise_begins, this, denoise_done and then adaptive_variance_done
inline void adaptive_variance_begins(CtxState& s) { s.avValid = false; }
inline void adaptive_variance_done(CtxState& s) { s.avValid = s.adCountsValid; }
inline void despike_begins(CtxState& s) { s.dsValid = false; }
// (pt_despike has checked planes_current, and nothing between its two events can end the planes)
inline void despike_done(CtxState& s) { s.dsValid = s.featValid; }
inline void upsample_begins(CtxState& s) { s.usValid = false; }
inline void upsample_done(CtxState& s) { s.usValid = true; }

// ---- predicates -----------------------------------------------------------------------------------
inline bool counts_describe_buffer(const CtxState& s) { return s.adCountsValid; }
inline bool moments_continue(const CtxState& s) { return s.adMomValid; }
inline bool planes_current(const CtxState& s) { return s.featValid; }
inline bool holds_denoised(const CtxState& s) { return s.dnValid; }
inline bool holds_temporal(const CtxState& s) { return s.tpValid; }
inline bool history_held(const CtxState& s) { return s.histValid; }
inline bool temporal_of_planes(const CtxState& s) { return s.tpOfPlanes; }
inline bool history_has_moments(const CtxState& s) { return s.momValid; }
inline bool variance_of_counts(const CtxState& s) { return s.avValid; }
inline bool holds_despiked(const CtxState& s) { return s.dsValid; }
inline bool holds_motion(const CtxState& s) { return s.motionValid; }
inline bool holds_upsampled(const CtxState& s) { return s.usValid; }
inline bool holds_boxes(const CtxState& s) { return s.boxValid; }

} // namespace pt
