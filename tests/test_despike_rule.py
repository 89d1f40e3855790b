"""Rule 6 of include/pt_hip.h (despike) on the CPU: the two numpy restatements of tests/despike_model.py agree word
for word, and the rule has the properties the header states.  No GPU."""
import numpy as np
import pytest

import despike_model as km
from despike_model import F, U, bits, same_words

P = km.PARAMS
FLAGS = (0, km.DEMODULATE, km.SAME_PRIMITIVE, km.DEMODULATE | km.SAME_PRIMITIVE)


def both(inputs, flags=km.SAME_PRIMITIVE, **over):
    """model() and scalar() on the same inputs, held against each other; returns model()'s (out, count, stats)."""
    p = dict(P, **over)
    stats = {}
    out, count = km.model(*inputs, flags=flags, stats=stats, **p)
    out2, count2 = km.scalar(*inputs, flags=flags, **p)
    assert same_words(out, out2)
    assert count == count2
    return out, count, stats


def properties(inputs, out, count, stats):
    """What the rule promises whatever the input."""
    color = inputs[0]
    changed = (bits(out[..., :3]) != bits(color[..., :3])).any(-1)
    spike = stats["spike_mask"]
    assert not (changed & ~spike).any()                    # a pixel that is not a spike has its input words
    assert np.all(bits(out[..., 3]) == bits(np.ones_like(out[..., 3])))
    # a spike is scaled by s in [0, 1), and s < 1 changes at least one word of a pixel whose luminance is positive
    assert count == int(changed.sum()) == stats["spikes"]
    if count:
        assert 0.0 <= stats["s_min"] and stats["s_max"] < 1.0


def vacuity(stats, npix):
    assert stats["spikes"] >= 1
    assert 2 * stats["ok"] >= npix


@pytest.mark.parametrize("width,height", km.SIZES)
def test_the_two_restatements_agree_on_every_size(width, height):
    inputs = km.make_case(width, height, seed=width * 100 + height)
    # (the small images are one id stripe wide or less: their neighbours are taken across stripes)
    over = dict(normal_cos_min=-1.0, sigma_plane=0.3) if min(width, height) < 8 else {}
    flags = 0 if min(width, height) < 8 else km.SAME_PRIMITIVE
    out, count, stats = both(inputs, flags=flags, **over)
    properties(inputs, out, count, stats)
    if (width, height) == (1, 1):
        assert count == 0 and same_words(out[..., :3], inputs[0][..., :3])
    else:
        vacuity(stats, width * height)


def test_every_tap_test_rejects_something():
    inputs = km.make_case(48, 40, seed=4840)
    _, _, stats = both(inputs, flags=km.SAME_PRIMITIVE, min_neighbors=12)
    for name in ("outside", "not_ok", "by_normal", "by_plane", "by_id"):
        assert stats[name] > 0, name
    assert 0 < stats["few"] < stats["ok"] and stats["spikes"] > 0


@pytest.mark.parametrize("radius", (1, 2, 3))
@pytest.mark.parametrize("rank", (1, 2, 3, 4))
def test_every_radius_and_rank(radius, rank):
    inputs = km.make_case(33, 9, seed=339)
    out, count, stats = both(inputs, radius=radius, rank=rank, min_neighbors=rank, sigma_plane=0.3, normal_cos_min=0.0)
    properties(inputs, out, count, stats)
    vacuity(stats, 33 * 9)


@pytest.mark.parametrize("flags", FLAGS)
def test_the_four_flag_combinations(flags):
    inputs = km.make_case(48, 40, seed=4840)
    out, count, stats = both(inputs, flags=flags)
    properties(inputs, out, count, stats)
    vacuity(stats, 48 * 40)


def test_the_flags_matter():
    inputs = km.make_case(48, 40, seed=4840)
    outs = [km.model(*inputs, flags=f, **P)[0] for f in FLAGS]
    for a in range(4):
        for b in range(a + 1, 4):
            assert not same_words(outs[a], outs[b]), (a, b)


@pytest.mark.parametrize("width,height,radius", [(33, 9, 1), (7, 1, 3), (1, 7, 2)])
def test_min_neighbors_above_what_the_window_offers_changes_nothing(width, height, radius):
    inputs = km.make_case(width, height, seed=5)
    offers = km.window_offers(width, height, radius)
    accepted = (2 * radius + 1) ** 2 - 1
    if offers < accepted:                                  # a window the image clips: no pixel can have this many
        out, count, _ = both(inputs, flags=0, radius=radius, rank=1, min_neighbors=offers + 1, normal_cos_min=-1.0, sigma_plane=0.3)
        assert count == 0 and same_words(out[..., :3], inputs[0][..., :3])
    # the most the struct accepts: only an interior pixel whose whole window is accepted has that many
    out, count, stats = both(inputs, flags=0, radius=radius, rank=1, min_neighbors=accepted)
    properties(inputs, out, count, stats)
    assert stats["few"] > 0


# ---- planted cases on one flat surface ------------------------------------------------------------------
def planted(width=12, height=10, value=0.25, **spikes):
    color, p0, p1, p2 = km.flat_inputs(width, height, value)
    for (x, y), v in spikes.get("at", {}).items():
        color[y, x, :3] = v
    return color, p0, p1, p2


FLAT = dict(radius=2, rank=1, factor=2.0, floor=0.05, min_neighbors=1, sigma_plane=0.3, normal_cos_min=0.0)


def run_flat(inputs, flags=km.SAME_PRIMITIVE, **over):
    out, count, stats = both(inputs, flags=flags, **dict(FLAT, **over))
    properties(inputs, out, count, stats)
    return out, count, stats


def test_a_single_spike_is_clamped_to_the_limit():
    inputs = planted(at={(5, 4): 40.0})
    out, count, stats = run_flat(inputs)
    assert count == 1 and stats["spike_mask"][4, 5]
    limit = F(2.0) * F(0.25) + F(0.05)                     # flat_inputs' grey: lum(v, v, v) is v to a rounding
    assert abs(float(out[4, 5, 0]) - float(limit)) < 1e-5


def test_a_pair_survives_rank_1_and_is_clamped_at_rank_2():
    inputs = planted(at={(5, 4): 40.0, (6, 4): 40.0})
    _, count1, _ = run_flat(inputs, rank=1)
    assert count1 == 0
    out, count2, stats = run_flat(inputs, rank=2, min_neighbors=2)
    assert count2 == 2 and stats["spike_mask"][4, 5] and stats["spike_mask"][4, 6]


def test_a_2x2_cluster_needs_rank_4():
    inputs = planted(at={(5, 4): 40.0, (6, 4): 40.0, (5, 5): 40.0, (6, 5): 40.0})
    for rank, expected in ((1, 0), (2, 0), (3, 0), (4, 4)):
        _, count, _ = run_flat(inputs, rank=rank, min_neighbors=rank)
        assert count == expected, rank


@pytest.mark.parametrize("where", [(0, 0), (11, 9), (0, 9), (11, 0), (0, 4), (5, 0), (11, 5), (6, 9)])
def test_spikes_in_a_corner_and_on_an_edge(where):
    inputs = planted(at={where: 40.0})
    _, count, stats = run_flat(inputs)
    assert count == 1 and stats["spike_mask"][where[1], where[0]]


def test_a_spike_on_an_id_boundary_sees_only_its_own_side():
    color, p0, p1, p2 = planted(at={(6, 4): 40.0})
    ids = bits(p0[..., 3]).copy()
    ids[:, 6:] = 9
    p0[..., 3] = ids.view(F)
    color[:, :6, :3] = 30.0                                # the other surface is bright
    inputs = (color, p0, p1, p2)
    _, count, stats = run_flat(inputs, flags=km.SAME_PRIMITIVE)
    assert count == 1 and stats["spike_mask"][4, 6] and stats["by_id"] > 0
    _, count, _ = run_flat(inputs, flags=0)                # across the boundary its bright neighbours excuse it
    assert count == 0


def test_equal_luminances_are_no_spikes():
    inputs = planted()
    out, count, _ = run_flat(inputs, factor=1.0, floor=0.0)
    assert count == 0                                      # l_p > limit is strict
    assert same_words(out[..., :3], inputs[0][..., :3])


def test_signed_zero_neighbours():
    # black neighbours of both signs: the limit is floor, whichever zero top[] keeps, and a lit pixel is a spike;
    # the zeros themselves are left as they are, sign included
    color, p0, p1, p2 = planted(value=0.0, at={(5, 4): 1.0})
    color[::2, ::2, :3] = F(-0.0)
    inputs = (color, p0, p1, p2)
    out, count, stats = run_flat(inputs)
    assert count == 1 and stats["spike_mask"][4, 5]
    assert abs(float(out[4, 5, 0]) - 0.05) < 1e-6
    rest = ~stats["spike_mask"]
    assert np.all(bits(out[..., :3])[rest] == bits(color[..., :3])[rest])
    # -0 + floor 0 is a limit of +-0, which passes limit >= 0
    out, count, _ = run_flat(inputs, floor=0.0)
    assert count == 1 and float(out[4, 5, 0]) == 0.0


def test_the_strict_compare_and_the_tap_order_fix_which_zero_is_kept():
    # Which zero top[0] holds shows only through a floor of -0 (limit = 2 * M + -0 keeps M's sign, and the spike is
    # scaled to a zero of that sign).  The first accepted tap of (5, 4) at radius 2 is (3, 2), the last (7, 6).
    negative_zero = bits(np.array([-0.0], dtype=F))[0]
    color, p0, p1, p2 = planted(value=0.0, at={(5, 4): 1.0})
    color[2, 3, :3] = F(-0.0)                              # the first tap -0, every later one +0: the first stays
    out, count, _ = run_flat((color, p0, p1, p2), floor=-0.0)
    assert count == 1 and np.all(bits(out[4, 5, :3]) == negative_zero)
    color, p0, p1, p2 = planted(value=0.0, at={(5, 4): 1.0})
    color[6, 7, :3] = F(-0.0)                              # the last tap -0: it does not displace the +0 before it
    out, count, _ = run_flat((color, p0, p1, p2), floor=-0.0)
    assert count == 1 and np.all(bits(out[4, 5, :3]) == 0)


def test_a_negative_luminance_pixel_is_never_a_spike_and_a_negative_limit_clamps_nothing():
    inputs = planted(at={(5, 4): -3.0})
    out, count, _ = run_flat(inputs)
    assert count == 0 and same_words(out[..., :3], inputs[0][..., :3])
    # every neighbour negative and no floor: limit < 0, so even a lit pixel stays
    inputs = planted(value=-1.0, at={(5, 4): 2.0})
    out, count, _ = run_flat(inputs, floor=0.0)
    assert count == 0 and same_words(out[..., :3], inputs[0][..., :3])
    _, count, _ = run_flat(inputs, floor=5.0)              # factor * M + floor = 3 > 2: still none
    assert count == 0
    _, count, _ = run_flat(inputs, floor=2.5)              # limit 0.5 < 2
    assert count == 1


def test_a_lone_lit_pixel_among_black_ones_with_and_without_floor():
    inputs = planted(value=0.0, at={(5, 4): 1.0})
    out, count, _ = run_flat(inputs, floor=0.05)
    assert count == 1 and abs(float(out[4, 5, 1]) - 0.05) < 1e-6         # kept, at the floor
    out, count, _ = run_flat(inputs, floor=0.0)
    assert count == 1 and np.all(out[4, 5, :3] == 0)                     # scaled to zero


def test_demodulation_clamps_in_the_demodulated_units():
    inputs = planted(at={(5, 4): 40.0})
    out, count, _ = run_flat(inputs, flags=km.DEMODULATE)
    # albedo 0.5: I = 0.5 around and 80 at the spike; limit = 2 * 0.5 + 0.05 = 1.05; out = 1.05 * 0.5
    assert count == 1 and abs(float(out[4, 5, 0]) - 0.525) < 1e-5


def test_a_pixel_that_is_no_spike_keeps_its_input_words_and_not_I_times_D():
    # make_case's colours are products of their albedo and come back from (C / D) * D; these do not
    color, p0, p1, p2 = km.flat_inputs(12, 10)
    p0[..., :3] = F(0.3)
    color[..., :3] = (F(0.2) + F(0.001) * np.arange(120, dtype=F).reshape(10, 12))[..., None]
    color[4, 5, :3] = 40.0
    round_trip = ((color[..., :3] / F(0.3)) * F(0.3)).astype(F)
    assert (bits(round_trip) != bits(color[..., :3])).any(-1).sum() > 10           # the inputs tell the two apart
    out, count, stats = run_flat((color, p0, p1, p2), flags=km.DEMODULATE)         # (properties() holds the words)
    assert count == 1 and stats["spike_mask"][4, 5]


def test_a_1x1_image_is_unchanged():
    inputs = km.flat_inputs(1, 1, 100.0)
    for radius in (1, 2, 3):
        out, count, _ = run_flat(inputs, radius=radius)
        assert count == 0 and same_words(out[..., :3], inputs[0][..., :3])
