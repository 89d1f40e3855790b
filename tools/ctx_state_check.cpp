// Host view of what a context carries between calls (pathtracercuda_amd/csrc/pt_ctx_state.h), for
// tests/test_ctx_state.py.
//   g++ -O1 -std=c++17 -fsanitize=address,undefined -o ctx_state_check tools/ctx_state_check.cpp
// Reads one request per line on stdin and prints the whole state as one JSON object per request (flushed,
// so a test can decide its next request from the answer):
//   new                         a fresh context's state
//   <event> [key=value ...]     an event of the header by name; render_begins takes cam=ID (a small integer
//                               the tool turns into distinct pt_camera bytes) and adds "stashMatches" and
//                               "misses" to the object, order_sorted takes samples= and strip=, sky_set takes held= and
//                               handle=; primitives_moved(s, with_table) is primitives_moved_with_table and
//                               primitives_moved_without_table
//   <predicate>                 a predicate of the header by name; adds "result"
//   fuzz seed=S n=N             N seeded random events on a fresh state; adds "violations", the number of
//                               times one of the invariants of Fuzz::step did not hold
// Exit status 0 = every request understood.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <sstream>
#include <string>

#include "../pathtracercuda_amd/csrc/pt_ctx_state.h"

using namespace pt;

typedef std::map<std::string, unsigned long long> Row;

static unsigned long long get(Row& r, const char* key, unsigned long long dflt)
{
    auto it = r.find(key);
    if (it == r.end()) return dflt;
    const unsigned long long v = it->second;
    r.erase(it);
    return v;
}

static pt_camera camera_of(unsigned long long id)
{
    pt_camera c = {};
    c.origin[0] = (float)id;
    return c;
}

// primitives_moved takes an argument: the lists below hold its two forms
static void primitives_moved_with_table(CtxState& s) { primitives_moved(s, true); }
static void primitives_moved_without_table(CtxState& s) { primitives_moved(s, false); }

static void (*const kEventFns[])(CtxState&) = {
    scene_or_texture_changed, rng_written, schedule_changed, order_dropped, order_replaced, order_biased,
    accum_written, stash_made, adaptive_begins, adaptive_done, features_begin, features_done, denoise_begins, denoise_done,
    temporal_begins, temporal_done, moments_done, adaptive_variance_begins, adaptive_variance_done, despike_begins,
    despike_done, scene_moved, upsample_begins, upsample_done, boxes_set, primitives_moved_with_table,
    primitives_moved_without_table};
static const char* const kEventNames[] = {
    "scene_or_texture_changed", "rng_written", "schedule_changed", "order_dropped", "order_replaced",
    "order_biased", "accum_written", "stash_made", "adaptive_begins", "adaptive_done", "features_begin", "features_done",
    "denoise_begins", "denoise_done", "temporal_begins", "temporal_done", "moments_done", "adaptive_variance_begins",
    "adaptive_variance_done", "despike_begins", "despike_done", "scene_moved", "upsample_begins",
    "upsample_done", "boxes_set", "primitives_moved_with_table", "primitives_moved_without_table"};
constexpr int kEvents = sizeof(kEventFns) / sizeof(kEventFns[0]);
// the tool's own list of the events after which a sample is no longer what the last render's was
static bool moves_epoch(void (*event)(CtxState&))
{
    return event == scene_or_texture_changed || event == rng_written || event == adaptive_begins || event == scene_moved ||
           event == primitives_moved_with_table || event == primitives_moved_without_table;
}
static_assert(kEvents == sizeof(kEventNames) / sizeof(kEventNames[0]), "one name per event");

static bool (*const kPredicates[])(const CtxState&) = {counts_describe_buffer, moments_continue, planes_current, holds_denoised,
                                                       holds_temporal, history_held, temporal_of_planes, history_has_moments,
                                                       variance_of_counts, holds_despiked, holds_motion, holds_upsampled,
                                                       holds_boxes};
static const char* const kPredicateNames[] = {"counts_describe_buffer", "moments_continue", "planes_current", "holds_denoised",
                                              "holds_temporal", "history_held", "temporal_of_planes", "history_has_moments",
                                              "variance_of_counts", "holds_despiked", "holds_motion", "holds_upsampled",
                                              "holds_boxes"};
constexpr int kPredicateCount = sizeof(kPredicates) / sizeof(kPredicates[0]);
static_assert(kPredicateCount == sizeof(kPredicateNames) / sizeof(kPredicateNames[0]), "one name per predicate");

// The tool's own account of the stash, kept beside the state: a stash matches exactly when the previous
// render made one, this render has that render's camera id, and no epoch-moving event came in between.
struct Shadow {
    bool rendered = false, stash = false, moved = false;
    unsigned long long cam = 0;
};

struct Fuzz {
    CtxState s;
    Shadow sh;
    uint64_t rng;
    unsigned long long violations = 0;

    uint32_t next()                     // xorshift64*
    {
        rng ^= rng >> 12;
        rng ^= rng << 25;
        rng ^= rng >> 27;
        return (uint32_t)((rng * 2685821657736338717ull) >> 32);
    }
    void check(bool ok) { violations += ok ? 0 : 1; }
    void step()
    {
        const uint64_t stateEpoch = s.stateEpoch, epoch = s.epoch;
        const bool hist = s.histValid, mom = s.momValid;
        const bool av = s.avValid, counts = s.adCountsValid;
        const bool ds = s.dsValid, feat = s.featValid;
        const bool motion = s.motionValid;
        const bool us = s.usValid;
        const bool boxes = s.boxValid;
        const uint32_t e = next() % (kEvents + 6);       // (a render as likely as four other events)
        if (e < (uint32_t)kEvents) {
            kEventFns[e](s);
            if (kEventFns[e] == stash_made) sh.stash = sh.rendered;
            if (moves_epoch(kEventFns[e])) sh.moved = true;
        } else if (e == (uint32_t)kEvents) {
            order_sorted(s, next() % 4096, 1 + next() % 4);
        } else if (e == (uint32_t)kEvents + 1) {
            const uint32_t held = next() % 2, handle = next() % 2;
            sky_set(s, held, handle);
            if (held != handle) sh.moved = true;
            check(s.histValid == (hist && held == handle));
            check(s.momValid == (mom && held == handle));
            check(s.dsValid == (ds && held == handle));          // another sky: the image's colours are of the old one
            check(s.motionValid == (motion && held == handle));  // the table goes with the history
        } else {
            const unsigned long long cam = next() % 3;
            const RenderStart r = render_begins(s, camera_of(cam));
            check(r.stashMatches == (sh.stash && !sh.moved && sh.cam == cam));
            check(!s.aheadValid && s.launched && s.lastState == s.stateEpoch);
            check(r.aheadMisses == s.aheadMisses);
            check(!s.avValid);                           // a render writes the accumulation
            check(!s.dsValid);
            sh = {true, false, false, cam};
        }
        check(!s.adMomValid || s.adCountsValid);
        check((!s.histValid || s.tpValid) && (!s.tpOfPlanes || s.tpValid));
        check(!s.momValid || s.histValid);
        check(!s.avValid || s.adCountsValid);
        check(!s.dsValid || s.featValid);                // the despiked image is of the planes the context holds
        check(!s.motionValid || s.histValid);            // the table maps to the scene of a history that is held
        // the tool's own list of what ends a history and what does not
        if (e < (uint32_t)kEvents) {
            void (*const f)(CtxState&) = kEventFns[e];
            // a move of primitives is, for every fact but the boxes, the scene event it stands for
            const bool moved = f == scene_moved || f == primitives_moved_with_table;
            const bool changed = f == scene_or_texture_changed || f == primitives_moved_without_table;
            // (a move ends the history only when it is the second one since a temporal pass)
            const bool ends = changed || f == temporal_begins || (moved && motion);
            if (f != temporal_done) check(s.histValid == (hist && !ends));
            if (f == features_begin) check(!s.tpOfPlanes);
            // the moments end with the history (a plain temporal step begins as every step and sets them no more);
            // only a finished moments step over a held history sets them
            check(s.momValid == (f == moments_done ? hist : (mom && !ends)));
            // the tool's own list of what ends the variance of the counts: what writes the accumulation (a render is
            // checked above), a features call that begins, and the call that makes the next one; only a finished
            // pt_denoise_adaptive over counts that describe the buffer sets it
            const bool endsAv = f == adaptive_begins || f == features_begin || f == adaptive_variance_begins;
            check(s.avValid == (f == adaptive_variance_done ? counts : (av && !endsAv)));
            // the tool's own list of what ends the despiked image: its own beginning, what writes the accumulation (a
            // render is checked above), a features call that begins, a scene or texture change (another sky is checked
            // above); only a finished pt_despike over current planes sets it
            const bool endsDs = f == despike_begins || f == adaptive_begins || f == features_begin ||
                                changed || moved;
            check(s.dsValid == (f == despike_done ? feat : (ds && !endsDs)));
            // the tool's own list of what ends the motion table: a temporal pass that begins, a scene or texture change
            // (another sky is checked above), a second move; only a first move over a held history sets it
            const bool endsMotion = f == temporal_begins || changed;
            check(s.motionValid == (moved ? (hist && !motion) : (motion && !endsMotion)));
            // the tool's own list for the upsampled image: only the call's own two events move it
            check(s.usValid == (f == upsample_done ? true : (us && f != upsample_begins)));
            if (moved || changed) check(!s.featValid && s.stateEpoch == stateEpoch + 1 && s.order.stale);
            // the tool's own list for the boxes: set by their upload, ended by a scene or texture change and by a scene
            // that comes with a table; a move of primitives keeps them
            check(s.boxValid == (f == boxes_set ? true : (boxes && f != scene_or_texture_changed && f != scene_moved)));
        } else if (e != (uint32_t)kEvents + 1) {
            check(s.histValid == hist && s.momValid == mom);     // a sort of the order, a render
            check(s.motionValid == motion);
            check(s.usValid == us);                              // (a render ends no upsampled image)
            check(s.boxValid == boxes);
            if (e == (uint32_t)kEvents) check(s.avValid == av && s.dsValid == ds);
        } else {
            check(s.avValid == av);                              // a sky ends no variance of the counts
            check(s.usValid == us);                              // nor an upsampled image
            check(s.boxValid == boxes);                          // nor the boxes
        }
        check(s.stateEpoch >= stateEpoch && s.epoch >= epoch);
        check(s.aheadMisses <= 1000u);
    }
};

static void print_state(const CtxState& s, const std::string& extra)
{
    printf("{\"order\": {\"valid\": %d, \"stale\": %d, \"samples\": %llu, \"strip\": %u}, \"stateEpoch\": %llu, "
           "\"lastState\": %llu, \"launched\": %d, \"lastCam\": %d, \"aheadValid\": %d, \"aheadMisses\": %u, \"adMomValid\": %d, "
           "\"adCountsValid\": %d, \"featValid\": %d, \"dnValid\": %d, \"tpValid\": %d, \"histValid\": %d, "
           "\"tpOfPlanes\": %d, \"momValid\": %d, \"avValid\": %d, \"dsValid\": %d, \"motionValid\": %d, "
           "\"usValid\": %d, \"boxValid\": %d, \"epoch\": %llu%s}\n",
           (int)s.order.valid, (int)s.order.stale, (unsigned long long)s.order.samples, s.order.strip,
           (unsigned long long)s.stateEpoch, (unsigned long long)s.lastState, (int)s.launched, (int)s.lastCam.origin[0],
           (int)s.aheadValid, s.aheadMisses, (int)s.adMomValid, (int)s.adCountsValid, (int)s.featValid, (int)s.dnValid,
           (int)s.tpValid, (int)s.histValid, (int)s.tpOfPlanes, (int)s.momValid, (int)s.avValid, (int)s.dsValid,
           (int)s.motionValid, (int)s.usValid, (int)s.boxValid, (unsigned long long)s.epoch, extra.c_str());
    fflush(stdout);
}

int main()
{
    CtxState s;
    char buf[4096];
    while (fgets(buf, sizeof(buf), stdin)) {
        std::istringstream ss(buf);
        std::string what, tok, extra;
        if (!(ss >> what)) continue;
        Row r;
        while (ss >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) {
                fprintf(stderr, "ctx_state_check: '%s' is not key=value\n", tok.c_str());
                return 2;
            }
            r[tok.substr(0, eq)] = strtoull(tok.c_str() + eq + 1, nullptr, 10);
        }
        bool ok = false;
        for (int i = 0; i < kEvents && !ok; ++i)
            if ((ok = what == kEventNames[i])) kEventFns[i](s);
        for (int i = 0; i < kPredicateCount && !ok; ++i)
            if ((ok = what == kPredicateNames[i])) extra = std::string(", \"result\": ") + (kPredicates[i](s) ? "1" : "0");
        if (ok) {
        } else if ((ok = what == "new")) {
            s = CtxState{};
        } else if ((ok = what == "order_sorted")) {
            const uint64_t samples = get(r, "samples", 0);
            order_sorted(s, samples, (uint32_t)get(r, "strip", 1));
        } else if ((ok = what == "sky_set")) {
            const uint32_t held = (uint32_t)get(r, "held", 0);
            sky_set(s, held, (uint32_t)get(r, "handle", 0));
        } else if ((ok = what == "render_begins")) {
            const RenderStart b = render_begins(s, camera_of(get(r, "cam", 0)));
            extra = ", \"stashMatches\": " + std::to_string((int)b.stashMatches) + ", \"misses\": " + std::to_string(b.aheadMisses);
        } else if ((ok = what == "fuzz")) {
            Fuzz f = {CtxState{}, {}, (get(r, "seed", 1) * 0x9e3779b97f4a7c15ull) | 1, 0};
            for (unsigned long long n = get(r, "n", 0); n > 0; --n) f.step();
            s = f.s;
            extra = ", \"violations\": " + std::to_string(f.violations);
        }
        if (!ok || !r.empty()) {
            fprintf(stderr, "ctx_state_check: bad request '%s'%s%s\n", what.c_str(), r.empty() ? "" : ", unknown key ",
                    r.empty() ? "" : r.begin()->first.c_str());
            return 2;
        }
        print_state(s, extra);
    }
    return 0;
}
