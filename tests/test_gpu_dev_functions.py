"""The kernel's device functions one by one against the oracle, bit for bit, over the input sets of
tests/dev_inputs.py: arguments that a render reaches only by chance (denormal powers and quotients,
texture coordinates off the usual range, any accumulation word with any frame count, 64-bit seeds).
pathtracercuda_amd/lib/dev_functions (tools/dev_functions.hip) evaluates every operation on the GPU in one
child process; float words must be equal or both NaN, bytes, integers and XORWOW words strictly equal.
There is no tolerance in this file."""
import subprocess

import numpy as np
import pytest

import dev_inputs as di

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device_dir(root, tmp_path_factory):
    exe = root / "pathtracercuda_amd" / "lib" / "dev_functions"
    assert exe.exists(), f"{exe} missing: run make"
    di.check_tex2d_taps()         # no input may read outside a texture on the device
    d = tmp_path_factory.mktemp("dev_functions")
    di.write_inputs(d)
    run = subprocess.run([str(exe), str(d)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, f"dev_functions exit status {run.returncode}: {run.stderr.strip()} {run.stdout.strip()}"
    return d


def input_words(dev_op, i, n):
    """Input i of the operation as hex words."""
    name, _, planes, _ = di.DEVICE_OPS[dev_op]
    inp = di.inputs(name)
    if planes is None:
        return ", ".join(f"{k} = {int(v[i]):#x}" for k, v in inp.items())
    return ", ".join(f"{p} = {int(np.ascontiguousarray(inp[p]).view(np.uint32)[i]):#010x}" for p in planes)


def compare(device_dir, dev_op, per_input, floats, layout="planes"):
    """per_input result words per input, stored as planes or as records."""
    name = di.DEVICE_OPS[dev_op][0]
    want = di.oracle_words(dev_op)
    got = di.read_output(device_dir, dev_op)
    assert got.shape == want.shape, f"{dev_op}: {got.size} result words, expected {want.size}"
    n = want.size // per_input
    shape = (per_input, n) if layout == "planes" else (n, per_input)
    got, want = got.reshape(shape), want.reshape(shape)
    bad = got != want
    if floats:
        bad &= ~(np.isnan(got.view(np.float32)) & np.isnan(want.view(np.float32)))
    bad = bad.any(axis=0 if layout == "planes" else 1)
    if not bad.any():
        return
    lines = []
    for i in np.flatnonzero(bad)[:8]:
        g = got[:, i] if layout == "planes" else got[i]
        w = want[:, i] if layout == "planes" else want[i]
        where = di.regions_at(name, di.inputs(name), int(i)) if name in di.REGION_OPS else []
        lines.append(f"  input {int(i)}: {input_words(dev_op, int(i), n)} -> device "
                     f"{' '.join(f'{int(x):#010x}' for x in g)}, oracle {' '.join(f'{int(x):#010x}' for x in w)}; "
                     f"regions: {', '.join(where) if where else '-'}")
    raise AssertionError(f"{dev_op}: {int(bad.sum())} of {n} inputs differ from the oracle\n" + "\n".join(lines))


def test_sincos_pos(device_dir):
    compare(device_dir, "sincos_pos", 2, floats=True)


@pytest.mark.parametrize("dev_op", ["acos_", "acos_sel", "atan2_", "atan2_sel", "log_", "exp_", "pow_"])
def test_transcendental(device_dir, dev_op):
    compare(device_dir, dev_op, 1, floats=True)


def test_f2i_x86(device_dir):
    compare(device_dir, "f2i_x86", 1, floats=False)


def test_tonemap_pixel(device_dir):
    compare(device_dir, "tonemap_pixel", 1, floats=False)


def test_tex2d(device_dir):
    compare(device_dir, "tex2d", 3, floats=True)


def test_xorwow_init(device_dir):
    compare(device_dir, "xorwow_init", 6, floats=False, layout="records")


def test_xorwow_skip(device_dir):
    compare(device_dir, "xorwow_skip", 6, floats=False, layout="records")


def test_xorwow_stream(device_dir):
    """n words of xorwow_next, then n of uniform, per seed: every word strictly equal (a uniform value is
    never NaN)."""
    want = di.oracle_words("xorwow_stream")
    got = di.read_output(device_dir, "xorwow_stream")
    assert got.shape == want.shape
    n = di.XORWOW_STREAM
    seeds = di.inputs("xorwow_stream")["seed"]
    got, want = got.reshape(len(seeds), 2, n), want.reshape(len(seeds), 2, n)
    bad = np.argwhere(got != want)
    if len(bad):
        lines = [f"  seed {int(seeds[s]):#x}, {'uniform' if k else 'xorwow_next'} draw {int(i)}: device "
                 f"{int(got[s, k, i]):#010x}, oracle {int(want[s, k, i]):#010x}" for s, k, i in bad[:8]]
        raise AssertionError(f"xorwow_stream: {len(bad)} of {want.size} words differ from the oracle\n" + "\n".join(lines))
