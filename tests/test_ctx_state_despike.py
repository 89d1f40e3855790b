""""A despiked image is held, of the accumulation and the planes the context holds"
(pathtracercuda_amd/csrc/pt_ctx_state.h) on the CPU, through tools/ctx_state_check.cpp: what sets the fact, what
ends it, and what it implies.  The events a call raises:

  pt_render             render_begins (then accum_written)
  pt_render_adaptive    adaptive_begins, adaptive_done
  pt_render_features    features_begin, features_done
  pt_despike            despike_begins, despike_done
  pt_denoise_despiked   denoise_begins, denoise_done
"""
import pytest

from test_ctx_state import ask

RENDER = ["render_begins cam=1", "accum_written"]
FEATURES = ["features_begin", "features_done"]
DESPIKE = ["despike_begins", "despike_done"]
HELD = RENDER + FEATURES + DESPIKE


def predicate(lines, name="holds_despiked"):
    return bool(ask(list(lines) + [name])[-1]["result"])


def test_a_finished_call_sets_it_and_a_fresh_context_has_none():
    assert not predicate([])
    assert not predicate(RENDER + FEATURES)
    assert not predicate(RENDER + FEATURES + DESPIKE[:1])           # not before the call is done
    assert predicate(HELD)
    assert predicate(HELD + DESPIKE)
    assert not predicate(HELD + DESPIKE[:1])                         # the next call overwrites it first
    state = ask(HELD)[-1]
    assert (state["dsValid"], state["featValid"], state["dnValid"]) == (1, 1, 0)


@pytest.mark.parametrize("event", ["render_begins cam=1", "render_begins cam=2", "adaptive_begins", "features_begin",
                                   "scene_or_texture_changed", "sky_set held=1 handle=2", "despike_begins"])
def test_what_ends_it(event):
    assert not predicate(HELD + [event])


def test_it_comes_back_only_with_a_new_call():
    assert not predicate(HELD + RENDER)
    assert not predicate(HELD + FEATURES)
    assert not predicate(HELD + ["adaptive_begins", "adaptive_done"])
    assert predicate(HELD + RENDER + DESPIKE)                        # (the planes are still current)
    assert predicate(HELD + FEATURES + DESPIKE)
    assert predicate(HELD + ["adaptive_begins", "adaptive_done"] + DESPIKE)
    # after a scene change the planes are void too: pt_despike is refused, and a done event alone sets nothing
    assert not predicate(HELD + ["scene_or_texture_changed"] + DESPIKE)
    assert predicate(HELD + ["scene_or_texture_changed"] + FEATURES + DESPIKE)
    # another sky ends the image but not the planes (first hits hold no sky)
    assert predicate(HELD + ["sky_set held=1 handle=2"], "planes_current")
    assert predicate(HELD + ["sky_set held=1 handle=2"] + DESPIKE)


@pytest.mark.parametrize("event", ["sky_set held=1 handle=1", "rng_written", "accum_written", "features_done", "denoise_begins",
                                   "denoise_done", "adaptive_done", "temporal_begins", "temporal_done", "moments_done",
                                   "adaptive_variance_begins", "adaptive_variance_done", "schedule_changed", "stash_made",
                                   "order_sorted samples=4 strip=1", "order_dropped", "despike_done"])
def test_what_leaves_the_image_and_the_planes_alone_leaves_it_alone(event):
    assert predicate(HELD + [event])
    assert predicate(HELD + [event], "planes_current")


def test_the_other_facts_are_what_they_were():
    # pt_despike touches no other fact; pt_denoise_despiked is a denoise and ends nothing of the despiked image
    before, after = ask(RENDER + FEATURES)[-1], ask(HELD)[-1]
    for key in before:
        if key != "dsValid":
            assert before[key] == after[key], key
    filtered = ask(HELD + ["denoise_begins", "denoise_done"])[-1]
    assert (filtered["dsValid"], filtered["dnValid"]) == (1, 1)
    # and it leaves an adaptive render's facts alone, as they leave it
    adaptive = ["adaptive_begins", "adaptive_done"] + FEATURES
    a, b = ask(adaptive)[-1], ask(adaptive + DESPIKE)[-1]
    assert (b["adCountsValid"], b["adMomValid"], b["dsValid"]) == (1, 1, 1)
    for key in a:
        if key != "dsValid":
            assert a[key] == b[key], key


def test_it_implies_current_planes_in_the_random_walks():
    assert not predicate(["despike_done"])                           # no planes: nothing is set
    assert not predicate(RENDER + DESPIKE)
    for seed in (31, 32):
        r = ask([f"fuzz seed={seed} n=300000"])[-1]
        assert r["violations"] == 0, r
