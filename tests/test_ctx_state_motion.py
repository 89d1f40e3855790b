""""A motion table is held that maps the current scene to the scene of the held history"
(pathtracercuda_amd/csrc/pt_ctx_state.h) on the CPU, through tools/ctx_state_check.cpp: what sets the fact, every
event that ends it, the double move, and what it implies.  The events a call raises:

  pt_set_scene_moved     scene_moved
  pt_set_scene           scene_or_texture_changed
  pt_temporal            temporal_begins, temporal_done
  pt_temporal_moments    temporal_begins, temporal_done, moments_done
  pt_render_features     features_begin, features_done
"""
import pytest

from test_ctx_state import ask

RENDER = ["render_begins cam=1", "accum_written"]
FEATURES = ["features_begin", "features_done"]
TEMPORAL = ["temporal_begins", "temporal_done"]
MOMENTS = TEMPORAL + ["moments_done"]
FRAME = RENDER + FEATURES + MOMENTS
HELD = FRAME + ["scene_moved"]


def predicate(lines, name="holds_motion"):
    return bool(ask(list(lines) + [name])[-1]["result"])


def test_a_move_over_a_held_history_sets_it():
    assert not predicate([])
    assert not predicate(["scene_moved"])                            # no history: the call is a plain scene change
    assert not predicate(RENDER + FEATURES + ["scene_moved"])
    assert not predicate(FRAME)
    assert predicate(HELD)
    assert predicate(RENDER + FEATURES + TEMPORAL + ["scene_moved"])  # a history without moments serves as well
    state = ask(HELD)[-1]
    assert (state["motionValid"], state["histValid"], state["momValid"], state["tpValid"]) == (1, 1, 1, 1)
    # everything else is a scene change's: the planes end, the order is stale, the samples are of another scene
    assert (state["featValid"], state["order"]["stale"]) == (0, 1)
    assert state["stateEpoch"] == ask(FRAME)[-1]["stateEpoch"] + 1
    plain = ask(RENDER + FEATURES + TEMPORAL + ["scene_moved"])[-1]
    assert (plain["motionValid"], plain["histValid"], plain["momValid"]) == (1, 1, 0)


@pytest.mark.parametrize("event", ["temporal_begins", "scene_or_texture_changed", "sky_set held=1 handle=2", "scene_moved"])
def test_what_ends_it(event):
    assert not predicate(HELD + [event])


def test_a_temporal_pass_ends_it_and_keeps_the_history():
    after = ask(HELD + RENDER + FEATURES + MOMENTS)[-1]
    assert (after["motionValid"], after["histValid"], after["momValid"]) == (0, 1, 1)
    assert predicate(HELD + RENDER + FEATURES + MOMENTS + ["scene_moved"])      # one move per temporal step


def test_the_double_move_ends_the_history():
    twice = ask(HELD + ["scene_moved"])[-1]
    assert (twice["motionValid"], twice["histValid"], twice["momValid"]) == (0, 0, 0)
    assert twice["tpValid"] == 1                                     # the image of the last pass can still be read
    # and a third move finds no history to keep
    assert not predicate(HELD + ["scene_moved", "scene_moved"])
    # the other ends take the history with them as before
    for event in ("scene_or_texture_changed", "sky_set held=1 handle=2"):
        s = ask(HELD + [event])[-1]
        assert (s["motionValid"], s["histValid"], s["momValid"]) == (0, 0, 0), event


@pytest.mark.parametrize("event", ["render_begins cam=1", "render_begins cam=2", "accum_written", "rng_written", "features_begin",
                                   "features_done", "sky_set held=1 handle=1", "denoise_begins", "denoise_done",
                                   "adaptive_begins", "adaptive_done", "despike_begins", "despike_done", "schedule_changed",
                                   "stash_made", "order_sorted samples=4 strip=1", "order_dropped", "moments_done",
                                   "adaptive_variance_begins", "adaptive_variance_done"])
def test_what_ends_nothing(event):
    assert predicate(HELD + [event])
    assert predicate(HELD + [event], "history_held")


def test_the_other_facts_are_what_they_were():
    # against a plain scene change, a move differs in the three facts of the history and nothing else
    moved, changed = ask(HELD)[-1], ask(FRAME + ["scene_or_texture_changed"])[-1]
    for key in moved:
        if key not in ("motionValid", "histValid", "momValid"):
            assert moved[key] == changed[key], key
    # and over no history it is a plain scene change in every fact
    a, b = ask(RENDER + FEATURES + ["scene_moved"])[-1], ask(RENDER + FEATURES + ["scene_or_texture_changed"])[-1]
    assert a == b
    # the double move is a plain scene change too
    assert ask(HELD + ["scene_moved"])[-1] == ask(HELD + ["scene_or_texture_changed"])[-1]
    # a context that never moves carries the facts it carried: the fact stays unset through a frame
    assert all(s["motionValid"] == 0 for s in ask(FRAME + FRAME))


def test_it_implies_a_held_history_in_the_random_walks():
    for seed in (41, 42):
        r = ask([f"fuzz seed={seed} n=300000"])[-1]
        assert r["violations"] == 0, r
