""""An upsampled image is held" (pathtracercuda_amd/csrc/pt_ctx_state.h) on the CPU, through tools/ctx_state_check.cpp:
what sets the fact, what ends it, and that it is tied to nothing else -- dnValid's rule: a result handed out, held until
the next call begins.  The events a call raises on the context of the larger frame:

  pt_upsample           upsample_begins, upsample_done        (nothing on the context of the smaller frame)
"""
import pytest

from test_ctx_state import ask

RENDER = ["render_begins cam=1", "accum_written"]
FEATURES = ["features_begin", "features_done"]
UPSAMPLE = ["upsample_begins", "upsample_done"]
HELD = FEATURES + UPSAMPLE                                   # the larger context needs planes and no render


def predicate(lines, name="holds_upsampled"):
    return bool(ask(list(lines) + [name])[-1]["result"])


def test_a_finished_call_sets_it_and_a_fresh_context_has_none():
    assert not predicate([])
    assert not predicate(FEATURES)
    assert not predicate(FEATURES + UPSAMPLE[:1])                    # not before the call is done
    assert predicate(HELD)
    assert predicate(HELD + UPSAMPLE)
    assert not predicate(HELD + UPSAMPLE[:1])                        # the next call overwrites it first
    state = ask(HELD)[-1]
    assert (state["usValid"], state["featValid"], state["dnValid"], state["dsValid"]) == (1, 1, 0, 0)


@pytest.mark.parametrize("event", ["render_begins cam=1", "adaptive_begins", "adaptive_done", "features_begin", "features_done",
                                   "scene_or_texture_changed", "scene_moved", "sky_set held=1 handle=2", "sky_set held=1 handle=1",
                                   "rng_written", "accum_written", "denoise_begins", "denoise_done", "temporal_begins",
                                   "temporal_done", "moments_done", "adaptive_variance_begins", "adaptive_variance_done",
                                   "despike_begins", "despike_done", "schedule_changed", "stash_made",
                                   "order_sorted samples=4 strip=1", "order_dropped", "upsample_done"])
def test_only_the_next_call_ends_it(event):
    assert predicate(HELD + [event])
    assert not predicate(HELD + [event, "upsample_begins"])


def test_the_other_facts_are_what_they_were():
    # on the larger context pt_upsample touches no other fact, whatever else it holds
    for prefix in (FEATURES, RENDER + FEATURES, RENDER + FEATURES + ["despike_begins", "despike_done", "denoise_begins", "denoise_done"],
                   ["adaptive_begins", "adaptive_done"] + FEATURES, RENDER + FEATURES + ["temporal_begins", "temporal_done", "moments_done"]):
        before, after = ask(prefix)[-1], ask(prefix + UPSAMPLE)[-1]
        assert after["usValid"] == 1
        for key in before:
            if key != "usValid":
                assert before[key] == after[key], key
    # and the held images a source is taken from are asked by their own predicates
    held = RENDER + FEATURES + ["despike_begins", "despike_done", "denoise_begins", "denoise_done", "temporal_begins", "temporal_done"]
    for name in ("planes_current", "holds_denoised", "temporal_of_planes", "holds_despiked"):
        assert predicate(held, name)
    assert not predicate(held + ["features_begin", "features_done"], "temporal_of_planes")
    assert not predicate(held + RENDER, "holds_despiked")


def test_its_rule_holds_in_the_random_walks():
    for seed in (41, 42):
        r = ask([f"fuzz seed={seed} n=300000"])[-1]
        assert r["violations"] == 0, r
        assert "usValid" in r
