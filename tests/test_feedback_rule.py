"""The feedback rule (include/pt_hip.h, rule 4) on the CPU: its two numpy restatements (tests/feedback_model.py)
agree word for word over four chained frames, the filter's own output is svgf_model's, the feedback writes the
colours of fed pixels and nothing else, and the seeded sequence exercises what the device tests rely on.  Equality
is the project's: words equal, or both NaN.
"""
import numpy as np
import pytest

import feedback_model as fm
import svgf_model as sm
import temporal_model as tm

F = fm.F
NAMES = ("image", "fed h0", "h1", "h2", "h3", "variance", "out", "unfed h0")


def words_differ(a, b):
    return (fm.bits(a[..., :3]) != fm.bits(b[..., :3])).any(-1)


@pytest.fixture(scope="module")
def seq():
    return fm.make_sequence()


@pytest.fixture(scope="module")
def unfed(seq):
    """The chain without feedback, per (flags, min_temporal): computed once, never written."""
    return {(flags, mt): fm.run_chain(sm.model, None, seq, flags, 0, min_temporal=mt) for flags in (0, 1, 2, 3) for mt in (1, 4)}


@pytest.mark.parametrize("min_temporal", (1, 4))
@pytest.mark.parametrize("flags", (0, 1, 2, 3))
@pytest.mark.parametrize("level", (1, 2, 3))
def test_the_two_restatements_agree_over_four_chained_frames(seq, unfed, level, flags, min_temporal):
    stats = []
    whole = fm.run_chain(sm.model, fm.filter_feedback_model, seq, flags, level, min_temporal=min_temporal, stats=stats)
    pixel = fm.run_chain(sm.scalar, fm.filter_feedback_scalar, seq, flags, level, min_temporal=min_temporal, want_out=False)
    base = unfed[flags, min_temporal]
    assert len(whole) == 4
    for k in range(4):
        for j in (0, 1, 2, 3, 4, 5, 7):
            assert fm.same_words(whole[k][j], pixel[k][j]), f"frame {k}, {NAMES[j]}"
        image, fed, h1, h2, h3, var, out, h0 = whole[k]
        color, p0, p1, p2 = seq[k][1]
        # the filter's own output is svgf_model's: the feedback reads an iteration and steers nothing
        want = sm.filter_model(image, p0, p1, p2, var, 3, flags=flags, **fm.VPARAMS)
        assert fm.same_words(out, want), f"frame {k}: the filter's output is not svgf_model's"
        # n, and every pixel that is not kept, are the step's words
        keep = sm.vkeep_mask(image, p0, p1, p2, var, flags)
        assert np.array_equal(fm.bits(fed[..., 3]), fm.bits(h0[..., 3])), f"frame {k}: an n word changed"
        assert fm.same_words(fed[~keep], h0[~keep]), f"frame {k}: a pixel that is not kept changed"
        assert not words_differ(fed, h0)[~keep].any()
        ok_not_kept = (h0[..., 3] >= 1) & ~keep
        misses = (fm.bits(p2[..., 3]) & fm.HIT) == 0
        emissive = (fm.bits(p2[..., 3]) & fm.EMISSIVE) != 0
        bad_var = (h0[..., 3] >= 1) & ~emissive & ~((var >= 0) & np.isfinite(var))
        changed = words_differ(fed, h0)
        print(f"L {level}, flags {flags}, min_temporal {min_temporal}, frame {k}: fed {stats[k]['fed']}, changed "
              f"{int(changed.sum())}, ok but not kept {int(ok_not_kept.sum())} (emissive {int((emissive & ok_not_kept).sum())}), "
              f"misses {int(misses.sum())}, bad variance {int(bad_var.sum())}")
        assert misses.sum() >= 4 and (emissive & ok_not_kept).sum() >= 4 and ok_not_kept.sum() >= 4
        if k >= 1:
            assert changed.sum() >= 64, f"frame {k}: only {int(changed.sum())} pixels are fed and differ"
        # h1, h2, h3 and the variance are those of a chain step on the same history (nothing but h0 is written)
        hist = None if k == 0 else whole[k - 1][1:5]
        again = sm.model(color, p0, p1, p2, seq[k][0], hist, seq[max(k - 1, 0)][0], flags=flags, min_temporal=min_temporal, **tm.PARAMS)
        for j in (2, 3, 4, 5):
            assert fm.same_words(whole[k][j], again[j]), f"frame {k}: {NAMES[j]} is not the step's"
    # the scalar form's filter output, once (the last frame)
    image, fed, h1, h2, h3, var, out, h0 = whole[3]
    sout, sfed = fm.filter_feedback_scalar(image, *seq[3][1][1:], var, h0, level, 3, flags=flags, **fm.VPARAMS)
    assert fm.same_words(sout, out) and fm.same_words(sfed, fed)
    # frame 1 has no history: the step's outputs are the unfed chain's; later frames reproject fed colours
    for j in (0, 2, 3, 4, 5, 7):
        assert fm.same_words(whole[0][j], base[0][j])
    assert seq[3][0] is not seq[2][0] and not np.array_equal(seq[3][0]["origin"], seq[2][0]["origin"])
    have = (whole[3][0][..., 3] > 1) & (base[3][0][..., 3] > 1)
    from_fed = have & words_differ(whole[3][0], base[3][0])
    print(f"frame 3: {int(from_fed.sum())} of {int(have.sum())} history pixels reproject a fed colour")
    assert from_fed.sum() >= 4
    assert from_fed.sum() > have.sum() / 2, "the fed chain's temporal image differs on too few history pixels"
    # the history lengths are untouched by feedback at every frame
    for k in range(4):
        assert np.array_equal(fm.bits(whole[k][0][..., 3]), fm.bits(base[k][0][..., 3]))


def test_a_second_application_in_the_same_frame_is_the_identity(seq):
    chain = fm.run_chain(sm.model, fm.filter_feedback_model, seq[:2], 3, 1)
    image, fed, h1, h2, h3, var, out, h0 = chain[1]
    p = seq[1][1][1:]
    out2, fed2 = fm.filter_feedback_model(image, *p, var, fed, 1, 3, flags=3, **fm.VPARAMS)
    assert fm.same_words(fed2, fed) and fm.same_words(out2, out)
    assert words_differ(fed, h0).sum() >= 64


@pytest.mark.parametrize("level", (1, 2))
def test_a_kept_pixel_whose_filtered_colour_is_not_finite_keeps_its_history(level):
    color, p0, p1, p2, var, cls, big = fm.make_overflow_inputs(tm.WIDTH, tm.HEIGHT, 21)
    rng = np.random.default_rng(5)
    h0 = np.concatenate([rng.random((tm.HEIGHT, tm.WIDTH, 3), dtype=F), np.full((tm.HEIGHT, tm.WIDTH, 1), F(3))], -1)
    levels = []
    sm.filter_model(color, p0, p1, p2, var, 2, flags=0, levels=levels, **sm.VPARAMS)
    I, v, _ = levels[level]
    kept_not_finite = ~(v < 0) & ~np.isfinite(I).all(-1)
    print(f"level {level}: {int(kept_not_finite.sum())} kept pixels with a filtered colour that is not finite, "
          f"{int((big & ~(v < 0)).sum())} kept pixels with a colour of 3e38")
    assert kept_not_finite.sum() >= 1 and (kept_not_finite & big).sum() >= 1, "the case does not occur in the model"
    stats = {}
    out, fed = fm.filter_feedback_model(color, p0, p1, p2, var, h0, level, 2, flags=0, stats=stats, **sm.VPARAMS)
    assert stats["kept_not_finite"] == kept_not_finite.sum()
    assert fm.same_words(fed[kept_not_finite], h0[kept_not_finite])
    assert np.isfinite(fed[..., :3]).all() and words_differ(fed, h0).sum() > 100
    sout, sfed = fm.filter_feedback_scalar(color, p0, p1, p2, var, h0, level, 2, flags=0, **sm.VPARAMS)
    assert fm.same_words(sfed, fed) and fm.same_words(sout, out)
    # every class of the variance plane is there, and the classes that are not kept keep their history
    assert set(np.unique(cls)) == set(range(len(sm.CLASSES)))
    for name in ("inf", "nan", "negative"):
        m = (cls == sm.CLASSES.index(name)) & ~big
        assert m.sum() >= 1 and fm.same_words(fed[m], h0[m]), name
