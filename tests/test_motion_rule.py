"""Rule 7 of include/pt_hip.h (the temporal steps across moved objects) on the CPU: its two numpy restatements
(tests/motion_model.py) against each other word for word, both against rules 3 and 4 under an identity table, that
the seeded sequence holds every case rule 7 adds, and that the rule does what it is for: a moving object keeps its
history.  tests/test_gpu_motion.py holds the device against the same model.
"""
import numpy as np
import pytest

import motion_model as mm
import svgf_model as sm
import temporal_model as tm

F, U = mm.F, mm.U
SIZES = ((1, 1), (31, 7), (33, 9), (48, 40))
NAMES = ("image", "h0", "h1", "h2", "h3", "variance")


def assert_same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert mm.same_words(g, w), f"{what}: {name} differs"


@pytest.fixture(scope="module")
def sequences():
    return {size: mm.make_sequence(*size) for size in SIZES}


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("flags", (0, 1, 2, 3))
def test_model_equals_scalar_restatement(sequences, size, flags):
    seq = sequences[size]
    a, b = mm.run_sequence(mm.model, seq, flags), mm.run_sequence(mm.scalar, seq, flags)
    for k in range(mm.FRAMES):
        assert_same(a[k], b[k], f"{size}, flags {flags}, frame {k}")
    # the step with moments: scalar() gives the five planes, the estimate over them is rule 4's own
    a = mm.run_sequence(mm.model, seq, flags, min_temporal=4)
    hist, prev = None, None
    for k, (cam, frame, (rows, prev_index)) in enumerate(seq):
        p = mm.PARAMS
        got = mm.scalar(*frame, cam, hist, prev if prev is not None else cam, rows, prev_index, p["alpha_min"],
                        p["max_history"], p["sigma_plane"], p["normal_cos_min"], flags, min_temporal=4)
        assert_same(a[k][:5], got, f"{size}, flags {flags}, frame {k}, moments")
        hist, prev = a[k][1:5], cam
    if size == (48, 40):      # and the frames do differ from their inputs: history was used
        assert not mm.same_words(a[2][0][..., :3], seq[2][1][0][..., :3])


@pytest.mark.parametrize("flags", (0, 1, 2, 3))
def test_an_identity_table_gives_rules_3_and_4(flags):
    """rows = identity, prev_index[i] = i: rule 7 is rule 3 (and rule 4's step) word for word.  The frames are
    temporal_model's and svgf_model's own sequences, whose ids are 0 .. 2 and 1000 + pixel (the latter beyond the
    table: such a pixel takes no history under rule 7, so they are given an entry each)."""
    rows, prev_index = mm.identity_table(1000 + tm.WIDTH * tm.HEIGHT)
    seq = tm.make_sequence()
    want = tm.run_sequence(tm.model, seq, flags)
    got = mm.run_sequence(mm.model, [(c, f, (rows, prev_index)) for c, f in seq], flags)
    for k in range(len(seq)):
        assert_same(got[k], want[k], f"flags {flags}, frame {k}")
    got = mm.run_sequence(mm.scalar, [(c, f, (rows, prev_index)) for c, f in seq], flags)
    for k in range(len(seq)):
        assert_same(got[k], want[k], f"scalar, flags {flags}, frame {k}")
    seq = sm.make_sequence()
    want = sm.run_sequence(sm.model, seq, flags)
    got = mm.run_sequence(mm.model, [(c, f, (rows, prev_index)) for c, f in seq], flags, min_temporal=4)
    for k in range(len(seq)):
        assert_same(got[k], want[k], f"moments, flags {flags}, frame {k}")


def test_the_sequence_holds_every_case(sequences):
    """At 48 x 40 with normal_cos_min = 0.9: per frame, the pixels with a tap whose verdict in the normal test
    differs between Nm and N_p, in the plane test between Pm and P_p, in the id test between prev_index[id_p] and
    id_p; the pixels of the appearing object; the pixels whose reprojected place leaves the image."""
    assert mm.PARAMS["normal_cos_min"] == 0.9
    stats = []
    mm.run_sequence(mm.model, sequences[(48, 40)], mm.SAME_PRIMITIVE | mm.DEMODULATE, stats=stats)
    for k, s in enumerate(stats):
        print(k, s)
    for k in range(1, mm.FRAMES):                          # the objects move in every frame, and so does the camera
        for key in ("normal_differs", "plane_differs", "leaves"):
            assert stats[k][key] >= 16, (k, key, stats[k])
    assert stats[mm.APPEARS_IN]["appearing"] >= 16                      # the frame the fifth object appears in
    assert stats[mm.FRAMES - 1]["id_differs"] >= 16                     # the frame whose primitives are permuted
    assert all(stats[k]["id_differs"] == 0 for k in range(mm.FRAMES - 1))
    assert all(stats[k]["appearing"] == 0 for k in range(mm.FRAMES) if k != mm.APPEARS_IN)
    assert all(s["have"] > 48 * 40 // 3 for s in stats[1:]) and stats[0]["have"] == 0
    # the special pixels of temporal_model.make_frame are here too
    color, p0, p1, p2 = sequences[(48, 40)][1][1]
    fl = mm.bits(p2[..., 3])
    hit = (fl & mm.HIT) != 0
    assert np.isnan(color[..., :3]).any() and np.isposinf(color[..., :3]).any() and np.isneginf(color[..., :3]).any()
    assert np.isnan(p1[..., :3]).any() and (fl & mm.EMISSIVE).any() and (~hit).any()
    assert ((p0[..., :3] == 0).all(-1) & hit).any() and ((p0[..., 0] > 0) & (p0[..., 0] < 1 / 64)).any()
    # and frame 4's table is a permutation, frame 3's has the one entry without a previous index
    assert sorted(mm.table(4)[1].tolist()) == [0, 1, 2, 3, 4] and mm.table(4)[1].tolist() != [0, 1, 2, 3, 4]
    assert (mm.table(3)[1] == mm.NONE).sum() == 1


def interior(frame_planes, frame, obj):
    """The ok pixels of an object whose eight neighbours are pixels of the same object."""
    m = mm.object_mask(frame_planes, frame, obj)
    p = np.pad(m, 1)
    inner = np.ones_like(m)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            inner &= p[dy:dy + m.shape[0], dx:dx + m.shape[1]]
    return inner & tm.ok_mask(frame_planes[0], frame_planes[2], frame_planes[3])


def test_a_moving_object_keeps_its_history(sequences):
    """The reason for rule 7.  Frames 0 .. 3 (K = 4; frame 4's permuted ids would end every history under rule 3,
    which is not the comparison meant): on the interior pixels of the translating and of the rotating object rule 7's
    n is K; rule 3, camera only with SAME_PRIMITIVE, leaves it at 1 on at least half of them."""
    K = 4
    seq = sequences[(48, 40)][:K]
    flags = mm.SAME_PRIMITIVE | mm.DEMODULATE
    moved = mm.run_sequence(mm.model, seq, flags)[K - 1][0][..., 3]
    still = tm.run_sequence(tm.model, [(c, f) for c, f, _ in seq], flags)[K - 1][0][..., 3]
    for obj in (mm.TRANSLATING, mm.ROTATING):
        inner = interior(seq[K - 1][1], K - 1, obj)
        print(obj, int(inner.sum()), np.bincount(moved[inner].astype(int)), np.bincount(still[inner].astype(int)))
        assert inner.sum() >= 16
        assert np.all(moved[inner] == K), (obj, np.bincount(moved[inner].astype(int)))
        assert (still[inner] == 1).sum() * 2 >= inner.sum(), (obj, np.bincount(still[inner].astype(int)))


def test_the_new_history_is_of_the_current_scene(sequences):
    outs = mm.run_sequence(mm.model, sequences[(48, 40)], 3)
    for (cam, (color, p0, p1, p2), _), (image, h0, h1, h2) in zip(sequences[(48, 40)], outs):
        assert mm.same_words(h1[..., :3], p1[..., :3]) and mm.same_words(h1[..., 3], p0[..., 3])
        assert mm.same_words(h2[..., :3], p2[..., :3]) and mm.same_words(h2[..., 3], p1[..., 3])


def test_a_nan_row_and_an_unknown_id_restart_the_pixel(sequences):
    seq = sequences[(48, 40)]
    flags = mm.DEMODULATE
    outs = mm.run_sequence(mm.model, seq[:2], flags)
    cam, frame, (rows, prev_index) = seq[2]
    hist = outs[1][1:4]
    base = mm.model(*frame, cam, hist, seq[1][0], rows, prev_index, flags=flags, **mm.PARAMS)[0]
    ok = tm.ok_mask(frame[0], frame[2], frame[3])
    for obj in (mm.TRANSLATING, mm.ROTATING):
        mask = mm.object_mask(frame, 2, obj) & ok
        assert (base[..., 3][mask] > 1).sum() >= 16
        bad = rows.copy()
        bad[mm.order(2)[obj], 1, 2] = F(np.nan)            # one word of the entry: every word reaches Pm
        got = mm.model(*frame, cam, hist, seq[1][0], bad, prev_index, flags=flags, **mm.PARAMS)[0]
        assert np.all(got[..., 3][mask] == 1) and mm.same_words(got[~mask], base[~mask])
    # ids beyond the table: a shorter table leaves the last primitive without an entry
    last = len(prev_index) - 1
    mask = (mm.bits(frame[1][..., 3]) == U(last)) & ok
    stats = {}
    got = mm.model(*frame, cam, hist, seq[1][0], rows[:last], prev_index[:last], flags=flags, stats=stats, **mm.PARAMS)[0]
    assert stats["unknown_id"] == mask.sum() >= 16
    assert np.all(got[..., 3][mask] == 1) and mm.same_words(got[~mask], base[~mask])
