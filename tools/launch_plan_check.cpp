// Host view of the launch policy (pathtracercuda_amd/csrc/pt_launch_plan.h) and the build table
// (pt_builds.h), for tests/test_launch_plan.py.
//   g++ -O1 -std=c++17 -fsanitize=address,undefined -o launch_plan_check tools/launch_plan_check.cpp
// Reads one request per line on stdin and prints one JSON object per request:
//   builds                      every row of the build table (one line each)
//   lds build=B nodes=.. records=.. prims=.. rows=.. hasRecords=..
//                               LDS bytes and staging level a launch of build B ends at
//   plan key=value ...          plan_launch of a launch; a key is a LaunchInputs field (scene sizes as
//                               nodes, records, prims, rows; prioBounds as prio0..prio2), the defaults
//                               are a fresh context's: every knob 0, no order, no stash
// Exit status 0 = every request understood.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>

#include "../pathtracercuda_amd/csrc/pt_launch_plan.h"

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

static SceneFacts scene_of(Row& r)
{
    SceneFacts sc = {};
    sc.size.nodes = (uint32_t)get(r, "nodes", 3);
    sc.size.records = (uint32_t)get(r, "records", 1);
    sc.size.prims = (uint32_t)get(r, "prims", 2);
    sc.size.stackRows = (uint32_t)get(r, "rows", 1);
    sc.hasRecords = get(r, "hasRecords", 1) != 0;
    sc.dfsOrder = get(r, "dfsOrder", 1) != 0;
    return sc;
}

// What a launch of build `b` ends at after launch_one's first two fallbacks (a child-box walk on a
// scene without records runs node at a time; a scene too large to stage is read through the caches).
struct LdsUse {
    size_t bytes;
    int SL;
};
static LdsUse launch_lds(const Build& b, bool hasRecords, const SceneSize& s)
{
    const bool cb = walks_child_boxes(b) && hasRecords;
    const size_t staged = lds_bytes(b.SL, b.WPB, cb, s);
    return staged > kLdsLimit && b.SL > 0 ? LdsUse{lds_bytes(0, b.WPB, cb, s), 0} : LdsUse{staged, b.SL};
}

static void print_builds()
{
    for (const Build& b : kBuilds)
        printf("{\"id\": %d, \"SL\": %d, \"WPB\": %d, \"WW\": %d, \"MINW\": %d, \"PERSIST\": %d, \"modes\": %u, \"settable\": %d, "
               "\"childBox\": %d}\n", b.id, b.SL, b.WPB, b.WW, b.MINW, (int)b.PERSIST, b.modes, (int)b.settable,
               (int)walks_child_boxes(b));
}

static bool print_lds(Row& r)
{
    const Build* b = find_build((int)get(r, "build", 0));
    if (!b) return false;
    const SceneFacts sc = scene_of(r);
    const LdsUse u = launch_lds(*b, sc.hasRecords, sc.size);
    printf("{\"bytes\": %zu, \"SL\": %d}\n", u.bytes, u.SL);
    return true;
}

static void print_plan(Row& r)
{
    LaunchInputs in = {};
    in.cus = (uint32_t)get(r, "cus", 256);
    in.tilesX = (uint32_t)get(r, "tilesX", 1);
    in.tilesY = (uint32_t)get(r, "tilesY", 1);
    in.spp = (uint32_t)get(r, "spp", 1);
    in.chunks = (uint32_t)get(r, "chunks", 1);
    in.instrumented = get(r, "instrumented", 0) != 0;
    in.scene = scene_of(r);
    in.knobs.variant = (int)get(r, "variant", 0);
    in.knobs.schedule = (int)get(r, "schedule", 0);
    in.knobs.stripMode = (int)get(r, "stripMode", 0);
    in.knobs.ssgMode = (int)get(r, "ssgMode", 0);
    in.knobs.aheadMode = (int)get(r, "aheadMode", 0);
    in.knobs.prioMode = (int)get(r, "prioMode", 0);
    in.knobs.prioBounds[0] = (uint32_t)get(r, "prio0", 0);
    in.knobs.prioBounds[1] = (uint32_t)get(r, "prio1", 0);
    in.knobs.prioBounds[2] = (uint32_t)get(r, "prio2", 0);
    in.knobs.prepassSpp = (uint32_t)get(r, "prepassSpp", 0);
    in.knobs.coldPriority = get(r, "coldPriority", 1) != 0;
    in.knobs.riseRepair = get(r, "riseRepair", 1) != 0;
    in.order.valid = get(r, "orderValid", 0) != 0;
    in.order.stale = get(r, "orderStale", 1) != 0;
    in.order.samples = get(r, "orderSamples", 0);
    in.order.strip = (uint32_t)get(r, "orderStrip", 1);
    in.stashMatches = get(r, "stashMatches", 0) != 0;
    in.aheadMisses = (uint32_t)get(r, "aheadMisses", 1);
    const LaunchPlan p = plan_launch(in);
    if (p.refusal) {
        printf("{\"refusal\": \"%s\"}\n", p.refusal);
        return;
    }
    static const char* const modes[] = {"plain", "instrumented", "strip", "ahead", "grouped"};
    static const char* const colds[] = {"none", "split", "prepass"};
    const LdsUse u = launch_lds(*find_build(p.build), in.scene.hasRecords, in.scene.size);
    printf("{\"refusal\": null, \"build\": %d, \"lds\": %zu, \"SL\": %d, \"mode\": \"%s\", \"K\": %u, \"units\": %u, \"G\": %u, "
           "\"ssgCap\": %u, \"aheadUse\": %d, \"aheadMake\": %d, \"dropOrder\": %d, \"costOrder\": %d, \"cold\": \"%s\", "
           "\"coldSpp\": %u, \"coldPairs\": %d, \"coldPrio\": [%u, %u, %u, %d], \"mainPrio\": [%u, %u, %u, %d], "
           "\"rebuildOrder\": %d, \"biasedOrder\": %d}\n",
           p.build, u.bytes, u.SL, modes[(int)p.mode], p.K, p.units, p.G, p.ssgCap, (int)p.aheadUse, (int)p.aheadMake,
           (int)p.dropOrder, (int)p.costOrder, colds[(int)p.cold], p.coldSpp, (int)p.coldPairs, p.coldPrio.prio[0],
           p.coldPrio.prio[1], p.coldPrio.prio[2], (int)p.coldPrio.dealt, p.mainPrio.prio[0], p.mainPrio.prio[1],
           p.mainPrio.prio[2], (int)p.mainPrio.dealt, (int)p.rebuildOrder, (int)p.biasedOrder);
}

int main()
{
    char buf[4096];
    while (fgets(buf, sizeof(buf), stdin)) {
        std::istringstream ss(buf);
        std::string what, tok;
        if (!(ss >> what)) continue;
        Row r;
        while (ss >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) {
                fprintf(stderr, "launch_plan_check: '%s' is not key=value\n", tok.c_str());
                return 2;
            }
            r[tok.substr(0, eq)] = strtoull(tok.c_str() + eq + 1, nullptr, 10);
        }
        bool ok = true;
        if (what == "builds") print_builds();
        else if (what == "lds") ok = print_lds(r);
        else if (what == "plan") print_plan(r);
        else ok = false;
        if (!ok || !r.empty()) {
            fprintf(stderr, "launch_plan_check: bad request '%s'%s%s\n", what.c_str(), r.empty() ? "" : ", unknown key ",
                    r.empty() ? "" : r.begin()->first.c_str());
            return 2;
        }
    }
    return 0;
}
