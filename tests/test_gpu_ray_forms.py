"""The slab test, the child-pair test and the object-space transform of the trace kernel against the
packed-FP32 forms they replaced, on the GPU.

pathtracercuda_amd/lib/ray_forms (tools/ray_forms.hip) holds the earlier forms of slab_lo_x, cb_pair and
to_local (register pairs, v_pk_add_f32 / v_pk_mul_f32) word for word as the reference and includes the
shipped headers for the forms under test; it makes its inputs on the device from the case index, runs both
forms in one thread and counts the differing output words on the device:

  slab      one axis at a time, (box low, box high, origin, reciprocal) over the whole of S^4 -- S = the 25
            values +-0, +-2^-149, +-2^-127, +-2^-126, +-2^-125, +-0.001, +-1, +-3, +-2^125, +-2^127, +-FLT_MAX,
            +-inf, NaN -- the other two axes benign: 3 x 25^4 cases, lo and X each;
  cb_pair   2^20 seeded records and rays, t_max over {FLT_MAX, 1, 0.001, 0, NaN}, all six fields of ChildPair;
  to_local  every pair of the 18 input words over S^2 (153 x 25^2 cases) and 2^20 seeded cases, six words each.

The forms are the same products, differences and sums in the same order, one rounding each, so the count
of differing words is exactly zero: there is no tolerance.  `--mutate` evaluates one product of a copy of
the form under test with an FMA and must find differences: the negative control of the comparison.  Each
run is one child process of well under a second; a run that ended with a non-zero status is not repeated."""
import json
import subprocess

import pytest

pytestmark = pytest.mark.gpu

S = 25
EXPECTED_CASES = {"slab": 3 * S ** 4, "cb_pair": 1 << 20, "to_local": 153 * S ** 2 + (1 << 20)}
_RUNS = {}


def run(root, *args):
    if args not in _RUNS:
        exe = root / "pathtracercuda_amd" / "lib" / "ray_forms"
        assert exe.exists(), f"{exe} missing: run make"
        _RUNS[args] = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=120)
    r = _RUNS[args]
    assert r.returncode == 0, f"ray_forms {' '.join(args)}: exit status {r.returncode}: {r.stderr.strip()} {r.stdout.strip()}"
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    return out


@pytest.mark.parametrize("part", sorted(EXPECTED_CASES))
def test_every_case_ran(root, part):
    assert run(root)[part]["cases"] == EXPECTED_CASES[part]


@pytest.mark.parametrize("part", sorted(EXPECTED_CASES))
def test_no_word_differs(root, part):
    out = run(root)
    assert out["mutate"] is False
    assert out[part]["diff_words"] == 0


@pytest.mark.parametrize("part", sorted(EXPECTED_CASES))
def test_mutated_form_is_caught(root, part):
    out = run(root, "--mutate")
    assert out["mutate"] is True
    assert out[part]["cases"] == EXPECTED_CASES[part]
    assert out[part]["diff_words"] > 0
