"""The generator and the model of tests/api_walk.py on their own (no GPU): the walks are deterministic, cover
every ordered pair of operation kinds and the named sequences, meet every outcome the model can predict
without spending themselves in refusals, and the oracle's side of every walk is quick enough to run with
the suite.  These are conditions on the generator and its seeds, asserted here.
"""
import time

import numpy as np
import pytest

import api_walk as aw
import denoise_model as dm

WALKS = {seed: aw.generate(seed) for seed in aw.SEEDS}
INVALIDATES_STASH = ("camera", "rng", "scene", "texture", "adaptive")
INVALIDATES_MOMENTS = ("rng", "scene", "texture", "render_raw", "render")


def replay(seed):
    """The model along a walk: per step (op, outcome, the model's flags before the call)."""
    model = aw.Model(aw.CONFIGS[seed].band_rows == 1)
    out = []
    for op in WALKS[seed]:
        before = dict(vars(model))
        out.append((op, model.apply(op), before))
    return out


REPLAYS = {seed: replay(seed) for seed in aw.SEEDS}


def test_seeds_and_sizes():
    assert len(aw.SEEDS) >= 8 and len({s % 8 for s in aw.SEEDS}) == 8
    print("steps per seed:", {s: len(w) for s, w in WALKS.items()})
    assert all(aw.STEPS <= len(w) <= aw.STEPS + 10 for w in WALKS.values())      # "about 40"
    cfgs = [aw.CONFIGS[s] for s in aw.SEEDS]
    assert any((c.band_rows, c.row_offset, c.row_stride) == (8, 1, 2) for c in cfgs)
    assert any((c.width, c.height) == (7, 5) for c in cfgs)


def test_the_same_seed_gives_the_same_walk():
    assert aw.build_walks() == aw.build_walks() == WALKS
    assert len({tuple(aw.describe(op) for op in w) for w in WALKS.values()}) == len(aw.SEEDS)


def test_the_model_names_the_shipped_variants():
    from test_gpu_parity import SHIPPED_VARIANTS
    from test_gpu_adaptive import ADAPTIVE_VARIANTS
    assert aw.SHIPPED_VARIANTS == SHIPPED_VARIANTS and aw.ADAPTIVE_VARIANTS == (0,) + ADAPTIVE_VARIANTS


def test_every_argument_is_inside_the_documented_range():
    for w in WALKS.values():
        for op in w:
            a = op.args
            if op.kind in ("render", "render_raw"):
                assert a["spp"] in (1, 2, 4) and a["chunks"] in (1, 2, 3)
            elif op.kind == "adaptive":
                assert a["spp"] in (2, 4) and a["min_calls"] == 2 and a["max_calls"] in (3, 4, 6)
                assert a["tolerance"] in (0.0, 0.2, 1e9)
            elif op.kind == "variant":
                assert a["variant"] in (0,) + aw.SHIPPED_VARIANTS
            elif op.kind == "run_ahead":
                assert 0 <= a["mode"] <= 3
            elif op.kind == "groups":
                assert a["mode"] in (0, 1, 2, 4)
            elif op.kind == "knob":
                assert a["value"] in aw.KNOBS[a["which"]]
            elif op.kind == "scene":
                assert a["name"] in aw.SCENES
            elif op.kind == "camera":
                assert max(abs(a[k]) for k in "xyz") <= 0.05


def test_every_ordered_pair_of_kinds_occurs():
    # a refused call changes no state, so a pair counts only when its first call ran, and its second too --
    # unless the first is what voids the second (a scene or texture change, then denoise: refused by contract)
    seen = set()
    for r in REPLAYS.values():
        for (p, a, _), (q, b, _) in zip(r, r[1:]):
            inherent = p.kind in ("scene", "texture") and q.kind == "denoise"
            if a.code == 0 and (b.code == 0 or inherent):
                seen.add((p.kind, q.kind))
    missing = [(p, q) for p in aw.KINDS for q in aw.KINDS if (p, q) not in seen]
    assert not missing, missing
    knobs = {op.args["which"] for w in WALKS.values() for op in w if op.kind == "knob"}
    assert knobs == set(aw.KNOBS)


def triples():
    """Consecutive (step, step, step) of every walk, each step as (op, outcome, flags before)."""
    for r in REPLAYS.values():
        yield from zip(r, r[1:], r[2:])


def makes_stash(step):
    """By the contract of pt_set_run_ahead: mode 2 makes a stash at every launch of 3..64 samples per pixel.
    The device reports neither that a stash was made nor that one was used or dropped (pt_last_launch has
    no such word, and the launch plan also asks for a scene with child-box records and a build with the
    run-ahead mode), so these triples are a condition on the sequence only: on the GPU they assert that the
    results are the oracle's whether or not the stash existed."""
    op, out, before = step
    return op.kind in ("render", "render_raw") and op.args["spp"] == 4 and before["run_ahead"] == 2 and out.code == 0


def test_named_triples_occur():
    found = {("stash", k): False for k in INVALIDATES_STASH}
    found.update({("continue", k): False for k in INVALIDATES_MOMENTS})
    found.update({("read", k): False for k in ("rng", "scene", "texture")})
    found.update({("denoise", k): False for k in ("scene", "texture")})
    for a, b, c in triples():
        ok = all(s[1].code == 0 for s in (a, b))
        if makes_stash(a) and ok and b[0].kind in INVALIDATES_STASH and c[0].kind in ("render", "render_raw") and c[1].code == 0:
            found[("stash", b[0].kind)] = True
        if a[0].kind == "adaptive" and ok and b[0].kind in INVALIDATES_MOMENTS and c[0].kind == "adaptive" \
                and not c[0].args["reset"]:
            # the invalidating call really was one: the continuation is refused as pt_hip.h documents
            assert c[1] == aw.Outcome(aw.PT_ERR_STATE, "reset")
            found[("continue", b[0].kind)] = True
        if a[0].kind == "features" and ok and b[0].kind in ("scene", "texture") and c[0].kind == "denoise":
            assert c[1].code != 0
            found[("denoise", b[0].kind)] = True
    # adaptive -> invalidating operation -> image read: the images are read after every step
    for r in REPLAYS.values():
        for a, b in zip(r, r[1:]):
            if a[0].kind == "adaptive" and a[1].code == 0 and b[0].kind in ("rng", "scene", "texture") and b[1].code == 0:
                found[("read", b[0].kind)] = True
    assert all(found.values()), [k for k, v in found.items() if not v]
    # sample groups on -> plain -> groups on with a larger G, over consecutive renders of one walk
    grown = False
    for r in REPLAYS.values():
        g = [before["groups"] for op, out, before in r if op.kind in ("render", "render_raw") and out.code == 0]
        grown |= any(x >= 2 and y == 1 and z > x for x, y, z in zip(g, g[1:], g[2:]))
    assert grown


def test_denoise_runs():
    """The denoiser's transitions are walked, not only refused."""
    ran = {seed: [i for i, (op, out, _) in enumerate(r) if op.kind == "denoise" and out.code == 0] for seed, r in REPLAYS.items()}
    tried = sum(op.kind == "denoise" for r in REPLAYS.values() for op, _, _ in r)
    print(f"denoise: {sum(map(len, ran.values()))} of {tried} run; by seed {ran}")
    small = [s for s in aw.SEEDS if aw.CONFIGS[s].width == 7]
    assert all(ran[s] for s in small), "no denoise runs on the frame of less than one wave"
    assert sum(map(len, ran.values())) >= tried // 2
    # adaptive -> scene | texture | rng -> features -> denoise: the filter must still divide by the counts
    found = {k: False for k in ("scene", "texture", "rng")}
    ended = False
    for r in REPLAYS.values():
        for a, b, c, d in zip(r, r[1:], r[2:], r[3:]):
            if (a[0].kind, c[0].kind, d[0].kind) == ("adaptive", "features", "denoise") and b[0].kind in found \
                    and all(s[1].code == 0 for s in (a, b, c, d)) and d[2]["counts_valid"] and not d[2]["moments_valid"]:
                found[b[0].kind] = True
        # a scene load while the image calls return the denoised image ends that
        for a, b in zip(r, r[1:]):
            ended |= a[0].kind == "denoise" and a[1].code == 0 and a[0].args["host"] and b[0].kind == "scene" and b[2]["denoised"]
    assert all(found.values()) and ended, (found, ended)
    # both layers and both sigmas run; some denoise filters the plain arithmetic and some the per-pixel counts
    done = [(op.args["host"], op.args["sigma"] is None, before["counts_valid"])
            for r in REPLAYS.values() for op, out, before in r if op.kind == "denoise" and out.code == 0]
    assert {h for h, _, _ in done} == {s for _, s, _ in done} == {c for _, _, c in done} == {False, True}


def test_model_outcomes():
    outcomes = [out for r in REPLAYS.values() for _, out, _ in r]
    predicted = {aw.Outcome(aw.PT_ERR_STATE, "adaptive"), aw.Outcome(aw.PT_ERR_STATE, "reset"),
                 aw.Outcome(aw.PT_ERR_ARG, "adaptive build"), aw.Outcome(aw.PT_ERR_STATE, "feature"),
                 aw.Outcome(aw.PT_ERR_ARG, "whole frame")}
    assert predicted <= set(outcomes), predicted - set(outcomes)
    share = sum(o.code == 0 for o in outcomes) / len(outcomes)
    print(f"{len(outcomes)} steps, {share:.1%} succeed")
    assert share >= 0.8
    for seed, r in REPLAYS.items():
        assert sum(o.code == 0 for _, o, _ in r) >= 0.7 * len(r), seed
    # every arithmetic of the image reads is met, and the reads after an adaptive render survive a change
    model_images = set()
    for seed in aw.SEEDS:
        model = aw.Model(aw.CONFIGS[seed].band_rows == 1)
        for op in WALKS[seed]:
            was = model.image()
            out = model.apply(op)
            model_images.add(model.image())
            if out.code == 0 and op.kind in ("rng", "scene", "texture", "camera", "features", "variant", "knob") and was != "denoised":
                assert model.image() == was, (seed, aw.describe(op))
            assert not model.adaptive or model.counts_valid
    assert model_images == {"frames", "counts", "denoised"}


def test_a_refused_call_changes_nothing():
    model = aw.Model(False)
    model.apply(aw.Op("adaptive", dict(reset=True)))
    before = dict(vars(model))
    for op in (aw.Op("render", dict(spp=1, chunks=1, ignore=False)), aw.Op("denoise", dict(sigma=0.4, host=True)),
               aw.Op("denoise", dict(sigma=None, host=False))):
        assert model.apply(op).code != 0 and vars(model) == before
    model.apply(aw.Op("rng", {}))
    assert model.adaptive and model.image() == "counts" and not model.moments_valid
    assert model.apply(aw.Op("adaptive", dict(reset=False))) == aw.Outcome(aw.PT_ERR_STATE, "reset")
    model.apply(aw.Op("render_raw", dict(spp=1, chunks=1, ignore=False)))
    assert not model.adaptive and model.image() == "frames" and model.frames == 0


@pytest.mark.parametrize("seed", aw.SEEDS)
def test_oracle_replay_is_quick(scenes, seed):
    cfg = aw.CONFIGS[seed]
    t0 = time.perf_counter()
    model, walk = aw.Model(cfg.band_rows == 1), aw.OracleWalk(scenes, cfg)
    rows = walk.accum.shape[0]
    planes = dm.make_inputs(cfg.width, rows, seed)[1:]       # stand-ins: the oracle has no normal or position plane
    for op in WALKS[seed]:
        if model.apply(op).code != 0:
            continue
        walk.apply(op)
        if op.kind == "features":
            prim, hit, _ = walk.first_hit()
            assert prim.shape == (rows, cfg.width) and ((prim != 0xffffffff) == hit).all()
        if op.kind == "denoise":
            hdr, _ = walk.image(model.color(), model.frames)
            walk.denoise(hdr, planes, aw.DENOISE_SIGMA)
        if model.image() != "denoised":
            hdr, ldr = walk.image(model.image(), model.frames)
            assert hdr.shape == walk.accum.shape and ldr.dtype == np.uint8
    seconds = time.perf_counter() - t0
    print(f"seed {seed} ({cfg.width}x{cfg.height}, {rows} rows): oracle replay of {len(WALKS[seed])} steps in {seconds:.2f} s")
    assert seconds < 5.0                     # "a few seconds"; measured: at most 0.3 s
