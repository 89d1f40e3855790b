""""The per-primitive boxes and the refit lists are of the current scene" (boxValid, pathtracercuda_amd/csrc/pt_ctx_state.h)
on the CPU, through tools/ctx_state_check.cpp: what sets the fact, what ends it, that a move of primitives keeps it, and
that such a move is, for every other fact, the scene event it stands for.  The events a call raises:

  pt_set_primitive_boxes                    boxes_set
  pt_move_primitives with motion rows       primitives_moved(s, true)   = scene_moved with boxValid carried over
  pt_move_primitives without                primitives_moved(s, false)  = scene_or_texture_changed with boxValid carried over
"""
import pytest

from test_ctx_state import ask

RENDER = ["render_begins cam=1", "accum_written"]
FEATURES = ["features_begin", "features_done"]
TEMPORAL = ["temporal_begins", "temporal_done"]
FRAME = RENDER + FEATURES + TEMPORAL
WITH, WITHOUT = "primitives_moved_with_table", "primitives_moved_without_table"


def predicate(lines, name="holds_boxes"):
    return bool(ask(list(lines) + [name])[-1]["result"])


def test_the_upload_sets_it_and_a_fresh_context_has_none():
    assert not predicate([])
    assert predicate(["boxes_set"])
    assert predicate(["boxes_set", "boxes_set"])
    before, after = ask(FRAME + ["moments_done"])[-1], ask(FRAME + ["moments_done", "boxes_set"])[-1]
    assert after["boxValid"] == 1 and before["boxValid"] == 0
    for key in before:                                   # it changes nothing of the scene: no other fact moves
        if key != "boxValid":
            assert before[key] == after[key], key


@pytest.mark.parametrize("event", ["scene_or_texture_changed", "scene_moved"])
def test_a_scene_or_texture_change_ends_it(event):
    assert not predicate(["boxes_set", event])
    assert not predicate(FRAME + ["boxes_set", event])
    assert predicate(["boxes_set", event, "boxes_set"])


@pytest.mark.parametrize("event", ["render_begins cam=1", "adaptive_begins", "adaptive_done", "features_begin", "features_done",
                                   "sky_set held=1 handle=2", "sky_set held=1 handle=1", "rng_written", "accum_written",
                                   "denoise_begins", "denoise_done", "temporal_begins", "temporal_done", "moments_done",
                                   "adaptive_variance_begins", "adaptive_variance_done", "despike_begins", "despike_done",
                                   "schedule_changed", "stash_made", "order_sorted samples=4 strip=1", "order_dropped",
                                   "upsample_begins", "upsample_done", WITH, WITHOUT])
def test_nothing_else_ends_it_and_a_move_keeps_it(event):
    assert predicate(["boxes_set", event])
    assert not predicate([event])                        # and none of them sets it


@pytest.mark.parametrize("move,scene", [(WITH, "scene_moved"), (WITHOUT, "scene_or_texture_changed")])
def test_a_move_is_the_scene_event_it_stands_for(move, scene):
    prefixes = ([], FRAME, FRAME + ["moments_done"], FRAME + ["scene_moved"], FRAME + [WITH], FRAME + ["despike_begins", "despike_done"],
                ["adaptive_begins", "adaptive_done"] + FEATURES, RENDER + ["stash_made"])
    for boxes in ([], ["boxes_set"]):
        for prefix in prefixes:
            a, b = ask(prefix + boxes + [move])[-1], ask(prefix + boxes + [scene])[-1]
            for key in a:
                if key != "boxValid":
                    assert a[key] == b[key], (prefix, key)
            assert a["boxValid"] == (1 if boxes else 0) and b["boxValid"] == 0
            assert a["featValid"] == 0 and a["order"]["stale"] == 1


def test_the_history_follows_set_scene_moveds_rules():
    held = lambda lines: ask(lines)[-1]
    s = held(FRAME + ["moments_done", "boxes_set", WITH])
    assert (s["histValid"], s["momValid"], s["motionValid"], s["boxValid"]) == (1, 1, 1, 1)
    s = held(FRAME + ["moments_done", "boxes_set", WITH, WITH])          # one move per temporal step
    assert (s["histValid"], s["momValid"], s["motionValid"], s["boxValid"]) == (0, 0, 0, 1)
    s = held(FRAME + ["boxes_set", "scene_moved", "boxes_set", WITH])    # a move of either kind counts
    assert (s["histValid"], s["motionValid"]) == (0, 0)
    s = held(FRAME + ["boxes_set", WITH] + FRAME + [WITH])               # the pass between them takes the table
    assert (s["histValid"], s["motionValid"], s["boxValid"]) == (1, 1, 1)
    s = held(FRAME + ["boxes_set", WITHOUT])
    assert (s["histValid"], s["motionValid"], s["boxValid"]) == (0, 0, 1)
    s = held(["boxes_set", WITH])                                        # without a history there is nothing to keep
    assert (s["histValid"], s["motionValid"], s["boxValid"]) == (0, 0, 1)


def test_its_rule_holds_in_the_random_walks():
    for seed in (51, 52):
        r = ask([f"fuzz seed={seed} n=300000"])[-1]
        assert r["violations"] == 0, r
        assert "boxValid" in r
