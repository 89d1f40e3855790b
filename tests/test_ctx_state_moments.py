""""The held history has moments" (pathtracercuda_amd/csrc/pt_ctx_state.h) on the CPU, through
tools/ctx_state_check.cpp: what sets the fact, what ends it, and what it implies.  The events a call raises:

  pt_temporal           temporal_begins, temporal_done
  pt_temporal_moments   temporal_begins, temporal_done, moments_done
"""
import pytest

from test_ctx_state import ask

PLAIN = ["temporal_begins", "temporal_done"]
MOMENTS = ["temporal_begins", "temporal_done", "moments_done"]
FEATURES = ["features_begin", "features_done"]


def predicate(lines, name="history_has_moments"):
    return bool(ask(list(lines) + [name])[-1]["result"])


def test_a_finished_moments_step_sets_it_and_a_fresh_context_has_none():
    assert not predicate([])
    assert not predicate(FEATURES)
    assert not predicate(FEATURES + MOMENTS[:2])             # not before the step is done
    assert predicate(FEATURES + MOMENTS)
    assert predicate(FEATURES + MOMENTS + FEATURES + MOMENTS)
    state = ask(FEATURES + MOMENTS)[-1]
    assert (state["momValid"], state["histValid"], state["tpValid"], state["tpOfPlanes"]) == (1, 1, 1, 1)


def test_a_plain_temporal_step_ends_it_and_keeps_the_colour_history():
    lines = FEATURES + MOMENTS + FEATURES + PLAIN
    assert not predicate(lines) and predicate(lines, "history_held")
    # the moments step after it meets a history without moments; once done, they are held again
    assert predicate(lines + FEATURES + MOMENTS)


@pytest.mark.parametrize("event", ["scene_or_texture_changed", "sky_set held=1 handle=2", "temporal_begins"])
def test_whatever_ends_the_history_ends_it(event):
    assert not predicate(FEATURES + MOMENTS + [event])
    assert not predicate(FEATURES + MOMENTS + [event], "history_held")


@pytest.mark.parametrize("event", ["sky_set held=1 handle=1", "rng_written", "render_begins cam=2", "accum_written",
                                   "features_begin", "features_done", "denoise_begins", "denoise_done", "adaptive_begins",
                                   "adaptive_done", "schedule_changed", "order_sorted samples=4 strip=1"])
def test_what_ends_no_history_ends_no_moments(event):
    assert predicate(FEATURES + MOMENTS + [event])


def test_features_take_the_planes_from_under_the_variance():
    # pt_denoise_variance asks both: the moments are still held, the image is no longer of the held planes
    lines = FEATURES + MOMENTS + FEATURES
    assert predicate(lines) and not predicate(lines, "temporal_of_planes")


def test_it_implies_a_held_history():
    # moments_done without a finished step sets nothing
    assert not predicate(["moments_done"])
    assert not predicate(FEATURES + ["temporal_begins", "moments_done"])
    for seed in (11, 12):
        r = ask([f"fuzz seed={seed} n=300000"])[-1]
        assert r["violations"] == 0, r
