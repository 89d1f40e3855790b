"""pth_motion_table (include/pt_host.h): rule 7's per-object maps from the two scenes' world->object rows, against its
float64 restatement in tests/motion_model.py word for word.  Pure CPU: the call makes no HIP call.
"""
import numpy as np
import pytest

import motion_model as mm
import pathtracercuda_amd as pa

F = mm.F


def hittables(rows):
    out = []
    for r in np.asarray(rows, dtype=F).reshape(-1, 3, 4):
        h = pa.PtHittable()
        for i in range(3):
            for j in range(4):
                h.inv_transform_rows[i][j] = float(r[i, j])
        out.append(h)
    return out


def inverse_rows(linear, translation):
    """World -> object rows of the object -> world map x -> linear x + translation, float32."""
    inv = np.linalg.inv(np.asarray(linear, dtype=np.float64))
    return np.concatenate([inv, -(inv @ np.asarray(translation, dtype=np.float64))[:, None]], 1).astype(F)


def rot(axis, deg):
    a = np.radians(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m = np.eye(3)
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def check(prev_rows, cur_rows):
    rows, valid = pa.motion_table(hittables(prev_rows), hittables(cur_rows))
    want, want_valid = mm.table_model(prev_rows, cur_rows)
    assert mm.same_words(rows, want), (rows, want)
    assert np.array_equal(valid, want_valid)
    return rows, valid


def cases():
    rng = np.random.default_rng(7)
    out = {}
    t = [rng.uniform(-5, 5, 3) for _ in range(8)]
    out["translations"] = ([inverse_rows(np.eye(3), a) for a in t], [inverse_rows(np.eye(3), a + rng.uniform(-1, 1, 3)) for a in t])
    for axis in range(3):
        out[f"rotations-{'xyz'[axis]}"] = ([inverse_rows(rot(axis, 10.0 * k), t[k]) for k in range(8)],
                                           [inverse_rows(rot(axis, 10.0 * k + 30.0), t[k]) for k in range(8)])
    scales = [1e-3, 1e-2, 0.1, 1.0, 10.0, 100.0, 1e3]
    out["scales"] = ([inverse_rows(rot(1, 20.0) * s, t[0]) for s in scales],
                     [inverse_rows(rot(1, 50.0) * s, t[1]) for s in scales])
    out["scale-changes"] = ([inverse_rows(np.eye(3) * s, t[2]) for s in scales],
                            [inverse_rows(np.eye(3) * s, t[3]) for s in reversed(scales)])
    mirror = np.diag([-1.0, 2.0, 0.5])
    out["mirrored"] = ([inverse_rows(rot(2, 15.0) @ mirror, t[4])], [inverse_rows(rot(2, 45.0) @ mirror, t[5])])
    return out


CASES = cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_table_equals_its_restatement(name):
    prev_rows, cur_rows = (np.stack(a) for a in CASES[name])
    rows, valid = check(prev_rows, cur_rows)
    assert valid.all()
    # and the map is the one meant: a world point of the object now goes to where that object point was
    p = np.random.default_rng(3).uniform(-2, 2, (len(rows), 3))
    for k in range(len(rows)):
        a, c = prev_rows[k].astype(np.float64), cur_rows[k].astype(np.float64)
        obj = c[:, :3] @ p[k] + c[:, 3]
        before = np.linalg.solve(a[:, :3], obj - a[:, 3])
        got = rows[k].astype(np.float64)[:, :3] @ p[k] + rows[k].astype(np.float64)[:, 3]
        assert np.allclose(got, before, rtol=1e-4, atol=1e-4 * (1 + np.abs(before).max())), (name, k, got, before)


def test_the_same_scene_gives_the_restatements_words():
    """prev == cur: the identity within the rounding of the float64 inverse -- the words the restatement gives,
    which are the identity's wherever the products are exact."""
    rows = np.stack([inverse_rows(rot(a, 37.0 * k) * s, (k, -k, 0.5 * k)) for k, (a, s) in
                     enumerate([(0, 1.0), (1, 0.5), (2, 3.0), (1, 1e-3), (0, 1e3)])]
                    + [inverse_rows(np.eye(3), (1.0, 2.0, 3.0)), inverse_rows(np.eye(3) * 2.0, (0.0, 0.0, 0.0))])
    got, valid = check(rows, rows)
    assert valid.all()
    ident = mm.identity_table(len(rows))[0]
    assert np.allclose(got, ident, atol=1e-6)
    assert mm.same_words(got[-2:], ident[-2:])           # axis-aligned rows: every product is exact
    assert np.all(got[..., 3] == 0)                      # b_cur - b_prev is exactly 0 in every entry (of either sign)


def test_an_inverse_that_overflows_is_marked_invalid():
    tiny = np.zeros((3, 4), dtype=F)
    tiny[0, 0] = tiny[1, 1] = tiny[2, 2] = F(1e-30)      # its inverse is 1e30; times a row of 1e30 it leaves float32
    big = np.zeros((3, 4), dtype=F)
    big[0, 0] = big[1, 1] = big[2, 2] = F(1e30)
    singular = np.zeros((3, 4), dtype=F)
    singular[0, 0] = singular[1, 1] = F(1)               # det = 0: the division gives inf and NaN
    good = inverse_rows(np.eye(3), (1, 2, 3))
    rows, valid = check(np.stack([tiny, singular, good]), np.stack([big, good, good]))
    assert valid.tolist() == [False, False, True]
    assert not np.isfinite(rows[0]).all() and not np.isfinite(rows[1]).all()


def test_refusals():
    h = hittables(np.zeros((2, 3, 4)))
    with pytest.raises(pa.PathtracerError, match="motion_table: 2 previous objects and 1 current"):
        pa.motion_table(h, h[:1])
    rows, valid = pa.motion_table([], [])
    assert rows.shape == (0, 3, 4) and valid.shape == (0,)
    from pathtracercuda_amd import _native as N
    assert N.host().pth_motion_table(None, None, 1, None, None) == N.PT_ERR_ARG
    assert b"pth_motion_table" in N.host().pth_last_error()
