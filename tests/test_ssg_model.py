"""The sample-group guess, lane and fold code restated (tests/ssg_model.py) on synthetic streams: whatever the
schedule of the lanes, the fold of their logs equals the serial fold of the stream.  Also that the case list
reaches every named path (ssg_model.REGIONS), and that each restated one-token mutation of the device text
breaks one of these checks.  CPU only; tests/test_gpu_ssg_stages.py runs the same inputs through the device
code."""
import collections

import numpy as np
import pytest

import ssg_model as sm

CASES = [c.name for c in sm.cases()] + ["g2_10000"]
RUNS = [(c, s) for c in CASES for s in sm.schedules_of(c)]


def test_seeded_sets_are_deterministic():
    assert np.array_equal(sm.guess_grid(), sm.guess_grid(), equal_nan=True)
    for name in CASES:
        cs = sm.case_named(name)
        a, b = sm.Pixels(cs), sm.Pixels(cs)
        for f in ("seed64", "tseed", "cls", "s0", "s1", "accum0", "rng0"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        assert (a.pairs is None and b.pairs is None) or np.array_equal(a.pairs, b.pairs, equal_nan=True)
    cs, px, _, _ = sm.inputs("g3_64")
    one = sm.chain(cs, px, sm.sched_random, seed=9)
    two = sm.chain(cs, px, sm.sched_random, seed=9)
    assert len(one) == len(two)
    for (s1, l1, _, f1), (s2, l2, _, f2) in zip(one, two):
        assert np.array_equal(s1, s2) and np.array_equal(l1.end, l2.end) and np.array_equal(l1.bits, l2.bits)
        assert np.array_equal(f1.fold, f2.fold) and np.array_equal(f1.accum.view(np.uint32), f2.accum.view(np.uint32))


def test_toy_stream_classes():
    """Lengths 1..6 of every class as described, colours finite with magnitudes 2^-12 .. 2^13."""
    o = np.arange(20000, dtype=np.uint32)
    seed = np.uint32(12345)
    want = {0: {1}, 1: {2}, 2: {2, 3, 4}, 3: {3}, 4: {6}, 5: {1, 2, 3, 4, 5, 6}, 6: {1, 2}, 7: {6}}
    for cls, lens in want.items():
        L = sm.toy_len(seed, np.uint32(cls), np.uint32(0), np.uint32(0), o)
        assert set(L.tolist()) == lens, cls
    threes = (sm.toy_len(seed, np.uint32(2), np.uint32(0), np.uint32(0), o) == 3).mean()
    assert 0.005 < threes < 0.02
    assert abs(sm.toy_len(seed, np.uint32(6), np.uint32(0), np.uint32(0), o).mean() - 1.5) < 0.02
    L7 = sm.toy_len(seed, np.uint32(7), np.uint32(3), np.uint32(100), o[:101])
    assert L7[0] == 3 and L7[2] == 1 and L7[3] == 6 and L7[94] == 6 and L7[95] == 5 and L7[99] == 1 and L7[100] == 6
    c = sm.toy_colour(seed, o)
    assert np.isfinite(c).all() and (np.abs(c) >= 2.0**-12).all() and (np.abs(c) < 2.0**13).all()
    assert (c < 0).any() and (c > 0).any()


@pytest.mark.parametrize("name,sched", RUNS)
def test_fold_of_any_schedule_equals_the_serial_fold(name, sched):
    """After every round: finished pixels at the truth of d = total, dead ends at the truth of d = F_DONE."""
    cs, px, tr, lim = sm.inputs(name)
    rounds, _ = sm.run(name, sched)
    bad = []
    for r, (_, _, _, S) in enumerate(rounds):
        bad += sm.check_against_truth(cs, tr, lim, S, f"round {r}")
    assert not bad, "\n".join(bad[:12])
    # the case asks for what it says: the plan's capacity, an order that is a permutation
    assert cs.cap == min(cs.total, 2 * cs.n + 64, 10000) and len(set(cs.order)) == len(cs.order)


def test_big_case_holds_the_end_offset_bound():
    """Item 0 of the 10,000-sample case logs cap samples of six pairs: its last end offset is 60,000."""
    cs, _, _, lim = sm.inputs("g2_10000")
    (_, L, _, S), = sm.run("g2_10000", "earliest")[0][:1]
    assert cs.cap == 10000 and (L.count[0] == 10000).all() and (L.end[0, 9999] == 60000).all() and S.dead == 0


def test_every_region_is_reached():
    reg = collections.Counter()
    for name, sched in RUNS:
        reg.update(sm.run(name, sched)[1])
    print("\n".join(f"{reg[k]:7d}  {k}" for k in sm.REGIONS))
    missing = [k for k in sm.REGIONS if reg[k] < 1]
    assert not missing, f"no pixel reaches: {missing}"
    assert set(reg) <= set(sm.REGIONS), set(reg) - set(sm.REGIONS)


def test_statistics_of_finished_pixels():
    """pairs[0..2] of a finished pixel: mean, odd fraction and variance of its toy lengths, from len(p, .)."""
    f = np.float32
    for name in CASES[:-1]:
        cs, px, tr, lim = sm.inputs(name)
        S = sm.run(name, "random")[0][-1][3]
        lens = tr.lens.astype(np.uint64)
        tot, odd, sq = lens.sum(axis=0), (lens & 1).sum(axis=0), (lens * lens).sum(axis=0)
        mean = tot.astype(f) / f(cs.total)
        var = np.maximum(sq.astype(f) / f(cs.total) - mean * mean, f(0))
        fin = np.zeros(cs.npix, bool)
        fin[lim[lim >= 0]] = True
        fin &= (S.fold[sm.F_FLAG] & 1) == 0
        assert fin.any()
        for k, want in enumerate((mean, odd.astype(f) / f(cs.total), var)):
            assert np.array_equal(S.pairs[k][fin].view(np.uint32), want[fin].view(np.uint32)), (name, k)


@pytest.mark.parametrize("name", CASES)
def test_guess_offsets_increase_and_phase_b_is_one_pair_on(name):
    cs, px, _, lim = sm.inputs(name)
    check_start_records(cs, px, lim, sm.guess(cs, px, px.pairs, lim))


@pytest.mark.parametrize("G,spp,chunks", sm.GRID_CASES, ids=sm.GRID_IDS)
def test_guess_grid_offsets_increase_and_phase_b_is_one_pair_on(G, spp, chunks):
    """The directed grid around the seven constants, m < 1, > 6 and NaN, unknown parity, n = 1."""
    cs, px, lim = sm.grid_case(G, spp, chunks)
    check_start_records(cs, px, lim, sm.guess(cs, px, px.pairs, lim))


def check_start_records(cs, px, lim, start):
    pos, lane = np.nonzero(lim >= 0)
    li = lim[pos, lane]
    prev = np.zeros(li.size, np.uint64)
    for g in range(1, cs.G):
        a = start[pos * cs.J + 2 * g - 1, :, lane]
        b = start[pos * cs.J + 2 * g, :, lane]
        assert (a[:, 0] > prev).all(), f"group {g}: offsets not strictly increasing"
        assert np.array_equal(a[:, 1:7], px.states(li, a[:, 0])), f"group {g}: not the state at its offset"
        dual = b[:, 0] != sm.IDLE
        assert (b[dual, 0] == a[dual, 0] + 1).all(), f"group {g}: phase B not one pair later"
        assert np.array_equal(b[dual, 1:7], px.states(li[dual], a[dual, 0] + 1)), f"group {g}: phase B not two draws on"
        last = sm.IDLE if g + 1 < cs.G else None
        if last is not None:
            assert (a[:, 7] == sm.IDLE).all() and (b[dual, 7] == sm.IDLE).all()
        else:
            assert (a[:, 7] != sm.IDLE).all() and (b[dual, 7] == a[dual, 7]).all()
        prev = a[:, 0].astype(np.uint64)


def grid_offsets(m, podd, var, G, spp, chunks):
    cs = sm.Case("grid", G, spp, chunks, width=1, height=1, order=(0,), tiles=1)
    pairs = np.asarray([[m], [podd], [var]], np.float32)
    offs = [int(o[0]) for o in sm.guess_offsets(cs, pairs)]
    dual = bool(sm._guess_fields(cs, pairs, 1)[3][0])
    return offs, dual, int(sm._guess_fields(cs, pairs, 1)[4][0])


def test_guess_constants_by_hand():
    """Offsets worked out by hand at the branch constants (n = total / G)."""
    f, up, dn = np.float32, lambda x: np.nextafter(np.float32(x), np.float32(9)), lambda x: np.nextafter(np.float32(x), np.float32(-9))
    # n = 1, G = 4: m = 2.6, parity unknown: not stable (|m - 2| >= 0.25), q = 3 but |m - 3| >= 0.02: plain rounding
    assert grid_offsets(2.6, -1, 1, 4, 1, 4)[0] == [3, 5, 8]            # 2.6 + .5, 5.2 + .5, 7.8 + .5 (float32)
    # m = 1, no odd samples: the even lattice gives 2, 2, 4: the second is bumped past the first
    assert grid_offsets(1.0, 0.0, 0.0, 4, 1, 4) == ([2, 3, 4], False, 4 + 1 + 2)     # 3 sqrt(4 * 0.05) = 1.34
    # m > 1.5 decides the second phase; 1.5 itself has none
    assert grid_offsets(1.5, 0.0, 0.0, 3, 2, 3)[1] is False and grid_offsets(up(1.5), 0.0, 0.0, 3, 2, 3)[1] is True
    # podd < 0.06 decides parity stability; n = 5, m = 2.5: stable 2 * (uint)(5 * 1.25 + .5) = 12, else 13
    assert grid_offsets(2.5, f(0.06), 0.3, 2, 2, 5) == ([13], False, 25 + int(3 * np.sqrt(f(10) * f(0.3))) + 2)
    assert grid_offsets(2.5, dn(0.06), 0.3, 2, 2, 5)[:2] == ([12], True)
    # |m - 2| < 0.25 with parity unknown; |m - q| < 0.02 for q >= 3 (n = 50: 148.5 + .5 -> 149, lattice 3 * 50 = 150)
    assert grid_offsets(2.25, -1, 1, 2, 2, 5)[1] is False and grid_offsets(dn(2.25), -1, 1, 2, 2, 5)[1] is True
    assert grid_offsets(2.97, -1, 1, 2, 10, 10)[0] == [149] and grid_offsets(2.99, -1, 1, 2, 10, 10)[0] == [150]
    # m below 1, above 6 and NaN are 1, 6 and 1
    assert grid_offsets(0.5, -1, 1, 2, 2, 5)[0] == [5] and grid_offsets(7.0, -1, 1, 2, 2, 5)[0] == [30]
    assert grid_offsets(np.nan, -1, 1, 2, 2, 5)[0] == [5]
    # var below 0.05 counts as 0.05: 10 * 2 + 3 sqrt(10 * 0.05) + 2 = 24.12
    assert grid_offsets(2.0, 0.5, 0.0, 2, 2, 5)[2] == 24 and grid_offsets(2.0, 0.5, 0.0499, 2, 2, 5)[2] == 24


# ---- mutations: each restated one-token change must break a check above -------------------------------
MUTATION_CASES = {"ignore_c0": "g2_33", "fold_every": "g3_64", "state_plus2": "g3_64", "popc_mask": "g3_64", "join_nobit": "g3_64",
                  "win_ge": "g5_1001", "prevrel0": "g3_64", "h_one": "g5_1001", "fallback_base": "g8_128"}


def mutated_chain_failures(mut, name, sched="round-robin"):
    cs, px, tr, lim = sm.inputs(name)
    pick, look = sm.SCHEDULES[sched]
    sm.MUT.add(mut)
    try:
        rounds = sm.chain(cs, px, pick, look, sm.ROUNDS, seed=5)
    except sm.Bounds as e:
        return [f"bounds in the model: {e}"]
    finally:
        sm.MUT.discard(mut)
    bad = []
    for r, (_, _, _, S) in enumerate(rounds):
        bad += sm.check_against_truth(cs, tr, lim, S, f"round {r}")
    if not bad:       # statistics are part of the fold's result
        want = sm.run(name, sched)[0]
        if len(want) != len(rounds) or any(not np.array_equal(a[3].pairs, b[3].pairs) or a[3].dead != b[3].dead
                                           for a, b in zip(want, rounds)):
            bad.append("statistics or dead ends differ from the unmutated fold")
    return bad


# h set to 1 instead of min(F_H, G) in a later round changes nothing: the two rules at the top of the fold's
# loop bring h back from the offset alone, and the group the walk last joined refuses the join (kh == ch)
EQUIVALENT = ("h_one",)


@pytest.mark.parametrize("mut", [m for m in sm.FOLD_MUTATIONS if m not in EQUIVALENT])
def test_fold_mutation_is_caught(mut):
    bad = mutated_chain_failures(mut, MUTATION_CASES[mut])
    print(mut, "->", bad[:1])
    assert bad, f"the mutation {mut} passes every check of {MUTATION_CASES[mut]}"


@pytest.mark.parametrize("name", ["g2_33", "g8_128", "g5_1001"])
def test_restoring_h_as_1_is_equivalent(name):
    assert EQUIVALENT == ("h_one",) and not mutated_chain_failures("h_one", name)


@pytest.mark.parametrize("mut", sm.GUESS_MUTATIONS)
def test_guess_mutation_is_caught(mut):
    sm.MUT.add(mut)
    try:
        with pytest.raises(AssertionError):
            test_guess_constants_by_hand()
            for name in ("g8_128", "g2_33"):
                test_guess_offsets_increase_and_phase_b_is_one_pair_on(name)
    finally:
        sm.MUT.discard(mut)
