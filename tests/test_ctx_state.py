"""What a context carries from one call to the next, on the CPU.

pathtracercuda_amd/csrc/pt_ctx_state.h holds the carried state of a device context and one function per event
that moves it; the C ABI functions raise those events and assign nothing themselves.
tools/ctx_state_check.cpp (built with ASan/UBSan by the Makefile) runs the same functions.  Checked here:

  * the walks of tests/api_walk.py, replayed as events beside api_walk.Model: after every call the header's
    four predicates are the model's four device flags (the GPU suite compares the same model with a device);
  * the scheduling state no result depends on -- the run-ahead stash's key, the miss count, the cost
    order -- in directed cases written from DESIGN.md 5.3 and the header's statement of the facts;
  * the header's invariants over seeded random event sequences (the tool's `fuzz`).
"""
import json
import pathlib
import subprocess

import pytest

import api_walk as aw
from test_launch_plan import plan

ROOT = pathlib.Path(__file__).resolve().parents[1]
EXE = ROOT / "pathtracercuda_amd" / "lib" / "ctx_state_check"

PREDICATES = {"counts_describe_buffer": "counts_valid", "moments_continue": "moments_valid",
              "planes_current": "planes_valid", "holds_denoised": "denoised_valid"}
# What the C ABI functions behind each kind of call raise, in order, when the model lets the call through (a
# call the model refuses is refused before any of them).  A render's events follow its plan: see render().
EVENTS = {
    "adaptive": ("adaptive_begins", "adaptive_done"),
    "features": ("features_begin", "features_done"),
    "denoise": ("denoise_begins", "denoise_done"),
    "rng": ("rng_written",),
    # the loader: its textures (pt_set_texture), pt_set_scene, then the sky's handle, which is a new one
    # because handles grow from load to load (the sky event ends nothing the other two have not ended)
    "scene": ("scene_or_texture_changed", "scene_or_texture_changed", "sky_set held=1 handle=2"),
    "texture": ("scene_or_texture_changed",),
    "camera": (), "variant": (), "run_ahead": (), "groups": (),
}
ALL_EVENTS = ("scene_or_texture_changed", "sky_set", "rng_written", "schedule_changed", "order_replaced", "order_dropped",
              "order_sorted", "order_biased", "render_begins", "accum_written", "stash_made", "adaptive_begins",
              "adaptive_done", "features_begin", "features_done", "denoise_begins", "denoise_done")
RENDER_EVENTS = ("order_replaced", "render_begins", "accum_written", "stash_made", "order_sorted")
KNOB_EVENTS = {"schedule": ("schedule_changed",), "strip_units": (), "occupancy": (), "cold_start": ()}


def check_clean(returncode, stderr):
    assert returncode == 0, (returncode, stderr[-2000:])
    assert "ERROR: AddressSanitizer" not in stderr and "runtime error" not in stderr, stderr[-2000:]


def ask(lines):
    """The state after each request, from a fresh one; a sanitizer report or a rejected request fails."""
    run = subprocess.run([str(EXE)], input="".join(line + "\n" for line in ["new"] + list(lines)), capture_output=True,
                         text=True, timeout=120)
    check_clean(run.returncode, run.stderr)
    return [json.loads(line) for line in run.stdout.splitlines()][1:]


class Session:
    """One ctx_state_check process answering request by request."""

    def __init__(self):
        self.proc = subprocess.Popen([str(EXE)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                     text=True, bufsize=1)
        self.seen = set()
        self.state = self.ask("new")

    def ask(self, line):
        self.proc.stdin.write(line + "\n")
        self.proc.stdin.flush()
        answer = self.proc.stdout.readline()
        assert answer, self.proc.stderr.read()[-2000:]
        self.seen.add(line.split()[0])
        self.state = json.loads(answer)
        return self.state

    def close(self):
        _, err = self.proc.communicate(timeout=60)
        check_clean(self.proc.returncode, err)


# ---- the walks ------------------------------------------------------------------------------------
def render(ses, op, camera, model, knobs, cfg, first):
    """render_impl and run_plan as events: the plan is plan_launch's own (tools/launch_plan_check)."""
    a = op.args
    bands = range(cfg.row_offset, -(-cfg.height // cfg.band_rows), cfg.row_stride)
    rows = sum(min(cfg.band_rows, cfg.height - b * cfg.band_rows) for b in bands)
    tx, ty = (cfg.width + 7) // 8, (rows + 7) // 8
    begun = ses.ask(f"render_begins cam={camera}")
    if first:
        ses.ask("order_replaced")                # order_reserve: the frame's buffers
    o = ses.state["order"]
    prepass, priority = knobs["cold_start"]
    p = plan(tilesX=tx, tilesY=ty, spp=a["spp"], chunks=a["chunks"], variant=model.variant, aheadMode=model.run_ahead,
             ssgMode=model.groups, stripMode=knobs["strip_units"], schedule=knobs["schedule"], prepassSpp=prepass,
             coldPriority=priority, orderValid=o["valid"], orderStale=o["stale"], orderSamples=o["samples"],
             orderStrip=o["strip"], stashMatches=begun["stashMatches"], aheadMisses=begun["misses"])
    assert p["refusal"] is None and p["cold"] == "none"      # (no walk launch has the 16 samples of a cold start)
    if p["dropOrder"]:
        ses.ask("order_dropped")
    ses.ask("accum_written")
    if p["aheadMake"]:
        ses.ask("stash_made")
    if p["rebuildOrder"]:
        ses.ask(f"order_sorted samples={a['spp'] * a['chunks']} strip={p['K']}")


def replay(seed):
    """The walk of a seed as events beside the model; returns the events raised and every predicate's values."""
    cfg = aw.CONFIGS[seed]
    model, ses = aw.Model(cfg.band_rows == 1), Session()
    knobs = {"schedule": 0, "strip_units": 0, "occupancy": 0, "cold_start": (0, 1)}
    camera, first, values = 1, True, {name: set() for name in PREDICATES}
    for i, op in enumerate(aw.generate(seed)):
        if model.apply(op).code == aw.PT_OK:
            if op.kind in ("render", "render_raw"):
                render(ses, op, camera, model, knobs, cfg, first)
                first = False
            elif op.kind == "knob":
                knobs[op.args["which"]] = op.args["value"]
                for event in KNOB_EVENTS[op.args["which"]]:
                    ses.ask(event)
            else:
                for event in EVENTS[op.kind]:
                    ses.ask(event)
            if op.kind in ("camera", "scene"):   # a moved camera, or the loaded scene's own
                camera += 1
        for name, flag in PREDICATES.items():
            got = bool(ses.ask(name)["result"])
            assert got == getattr(model, flag), (seed, i, aw.describe(op), name, ses.state)
            values[name].add(got)
    ses.close()
    return ses.seen, values


def test_walks_agree_with_the_model():
    seen, values = set(), {name: set() for name in PREDICATES}
    for seed in aw.SEEDS:
        s, v = replay(seed)
        seen |= s
        for name in v:
            values[name] |= v[name]
    # not vacuous: every predicate was seen both ways, and every event a call of the walks raises occurred
    assert all(v == {False, True} for v in values.values()), values
    tables = list(EVENTS.values()) + list(KNOB_EVENTS.values()) + [RENDER_EVENTS]
    raised = {event.split()[0] for events in tables for event in events}
    assert raised <= seen, sorted(raised - seen)
    # (the other two follow plans no walk launch gets -- a cold start, which takes 16 samples, and a change of
    # the strip width K: the directed cases below have them)
    assert raised | {"order_biased", "order_dropped"} == set(ALL_EVENTS)


# ---- the run-ahead stash and the cost order -------------------------------------------------------
# a context that holds still under camera 1 (no misses), and whose last render made a stash
STASHED = ["render_begins cam=1", "accum_written", "render_begins cam=1", "accum_written", "stash_made"]


def test_a_stash_matches_the_next_render_of_the_same_camera():
    for between in ([], ["sky_set held=0 handle=0"], ["sky_set held=3 handle=3"]):       # the sky that is set, set again
        r = ask(STASHED + between + ["render_begins cam=1"])[-1]
        assert (r["stashMatches"], r["misses"], r["aheadValid"]) == (1, 0, 0), (between, r)


@pytest.mark.parametrize("between", [["rng_written"], ["scene_or_texture_changed"], ["sky_set held=0 handle=3"],
                                     ["adaptive_begins", "adaptive_done"]],
                         ids=["rng", "scene-or-texture", "sky", "adaptive"])
def test_a_change_of_what_a_sample_depends_on_voids_the_stash(between):
    r = ask(STASHED + between + ["render_begins cam=1"])[-1]
    assert (r["stashMatches"], r["misses"], r["aheadValid"]) == (0, 1, 0), r


def test_a_camera_change_voids_the_stash():
    r = ask(STASHED + ["render_begins cam=2"])[-1]
    assert (r["stashMatches"], r["misses"], r["lastCam"], r["order"]["stale"]) == (0, 1, 2, 1), r
    # and no stash, no match: a render that made none
    r = ask(STASHED[:2] + ["render_begins cam=1"])[-1]
    assert (r["stashMatches"], r["misses"]) == (0, 0), r


def test_misses_count_consecutive_renders_with_a_changed_key():
    first, second = ask(["render_begins cam=1", "render_begins cam=2"])
    assert (first["misses"], first["stashMatches"]) == (1, 0)            # a context's first render is a miss
    assert (second["misses"], second["aheadMisses"]) == (2, 2)
    # 2 is where plan_launch stops making stashes (a moving camera); a launch of 4 spp on a
    # grid whose tiles wait for a wave slot makes one below that
    assert plan(cus=1, tilesX=100, spp=4, aheadMisses=1)["aheadMake"] == 1
    assert plan(cus=1, tilesX=100, spp=4, aheadMisses=2)["aheadMake"] == 0
    # holding still ends the run, and the count saturates
    assert ask(["render_begins cam=1", "render_begins cam=2", "render_begins cam=2"])[-1]["misses"] == 0
    moving = ask([f"render_begins cam={1 + i % 2}" for i in range(1005)])
    assert [m["misses"] for m in moving[997:]] == [998, 999, 1000, 1000, 1000, 1000, 1000, 1000]


def test_the_cost_order():
    sorted_, biased, adaptive = ask(["order_sorted samples=8 strip=2", "order_biased", "adaptive_begins"])[:3]
    assert sorted_["order"] == {"valid": 1, "stale": 0, "samples": 8, "strip": 2}
    assert biased["order"] == {"valid": 1, "stale": 0, "samples": 0, "strip": 2}
    # an adaptive render dispatches no tiles: the order stays as it was
    done = ask(["order_sorted samples=8 strip=2", "adaptive_begins", "adaptive_done"])[-1]
    assert done["order"] == sorted_["order"] and adaptive["order"] == biased["order"]
    for event in ("scene_or_texture_changed", "schedule_changed", "render_begins cam=1"):
        assert ask(["order_sorted samples=8 strip=2", event])[-1]["order"] == {"valid": 1, "stale": 1, "samples": 8, "strip": 2}
    for event in ("order_dropped", "order_replaced"):
        after = ask(["order_sorted samples=8 strip=2", event])[-1]["order"]
        assert (after["valid"], after["stale"]) == (0, 1), event
    for event in ("sky_set held=1 handle=2", "rng_written"):                         # the tiles cost what they did
        assert ask(["order_sorted samples=8 strip=2", event])[-1]["order"] == sorted_["order"]


def test_unknown_requests_are_refused():
    for line in ("render cam=1", "render_begins camera=1", "new x=1", "stash_made 1"):
        run = subprocess.run([str(EXE)], input=line + "\n", capture_output=True, text=True, timeout=60)
        assert run.returncode == 2, (line, run.returncode, run.stderr[-500:])


# ---- the invariants -------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", (1, 2, 3))
def test_fuzz(seed):
    r = ask([f"fuzz seed={seed} n=1000000"])[-1]
    assert r["violations"] == 0, r
    assert r["epoch"] > 10000 and r["stateEpoch"] > r["epoch"]           # the events did move the state
