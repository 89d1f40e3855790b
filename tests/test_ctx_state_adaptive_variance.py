""""The held variance is of the counts" (pathtracercuda_amd/csrc/pt_ctx_state.h) on the CPU, through
tools/ctx_state_check.cpp: what sets the fact, what ends it, and what it implies.  The events a call raises:

  pt_render_adaptive    adaptive_begins, adaptive_done
  pt_render_features    features_begin, features_done
  pt_denoise_adaptive   denoise_begins, adaptive_variance_begins, denoise_done, adaptive_variance_done
"""
import pytest

from test_ctx_state import ask

ADAPTIVE = ["adaptive_begins", "adaptive_done"]
FEATURES = ["features_begin", "features_done"]
DENOISE = ["denoise_begins", "adaptive_variance_begins", "denoise_done", "adaptive_variance_done"]
HELD = ADAPTIVE + FEATURES + DENOISE


def predicate(lines, name="variance_of_counts"):
    return bool(ask(list(lines) + [name])[-1]["result"])


def test_a_finished_call_sets_it_and_a_fresh_context_has_none():
    assert not predicate([])
    assert not predicate(ADAPTIVE + FEATURES)
    assert not predicate(ADAPTIVE + FEATURES + DENOISE[:3])          # not before the call is done
    assert predicate(HELD)
    assert predicate(HELD + DENOISE)
    assert not predicate(HELD + DENOISE[:2])                         # the next call overwrites it first
    state = ask(HELD)[-1]
    assert (state["avValid"], state["adCountsValid"], state["featValid"], state["dnValid"]) == (1, 1, 1, 1)


@pytest.mark.parametrize("event", ["render_begins cam=1", "adaptive_begins", "features_begin"])
def test_what_ends_the_counts_and_a_features_call_end_it(event):
    assert not predicate(HELD + [event])


def test_it_comes_back_only_with_a_new_call():
    assert not predicate(HELD + ADAPTIVE)
    assert not predicate(HELD + FEATURES)
    assert predicate(HELD + FEATURES + DENOISE)
    assert predicate(HELD + ADAPTIVE + DENOISE)                      # (the planes are still current)


@pytest.mark.parametrize("event", ["scene_or_texture_changed", "sky_set held=1 handle=2", "sky_set held=1 handle=1",
                                   "rng_written", "accum_written", "features_done", "denoise_begins", "denoise_done",
                                   "adaptive_done", "temporal_begins", "temporal_done", "moments_done", "schedule_changed",
                                   "stash_made", "order_sorted samples=4 strip=1", "order_dropped"])
def test_what_leaves_the_counts_alone_leaves_it_alone(event):
    # the variance describes the buffer the counts describe: a new scene, sky or RNG state changes neither
    assert predicate(HELD + [event])
    assert predicate(HELD + [event], "counts_describe_buffer")


def test_the_other_facts_are_what_they_were():
    # pt_denoise_adaptive is a denoise: it ends and sets "a denoised image is held", and touches nothing else
    before, after = ask(ADAPTIVE + FEATURES)[-1], ask(HELD)[-1]
    for key in before:
        if key not in ("avValid", "dnValid"):
            assert before[key] == after[key], key
    assert (before["dnValid"], after["dnValid"]) == (0, 1)


def test_it_implies_that_the_counts_describe_the_buffer():
    # adaptive_variance_done without counts sets nothing
    assert not predicate(["adaptive_variance_done"])
    assert not predicate(FEATURES + DENOISE)
    assert not predicate(["adaptive_begins"] + FEATURES + DENOISE)
    for seed in (21, 22):
        r = ask([f"fuzz seed={seed} n=300000"])[-1]
        assert r["violations"] == 0, r
