"""The exact model of the two 8-bit conversions (tests/gamma_model.py: the byte of the correctly rounded power, by `decimal` at 80 digits) against everything on the CPU
that claims the same bytes: the oracle's restatements (glibc's pow and powf), and the bytes the reference's own progressive kernel wrote into
tests/golden/ref_realtime.npz.  tests/test_gpu_gamma_bytes.py then holds the two device kernels to the same model on the same inputs.

The inputs: T_k - 4 ... T_k + 3 in floats around every threshold T_k of each path (the least binary32 whose byte is >= k), the special values, and 4096 log-uniform
values in [1e-6, 4e5]."""
import numpy as np
import pytest

from . import gamma_model as gm
from .conftest import load_golden


@pytest.fixture(scope="module")
def ref():
    return load_golden("ref_realtime.npz")


def inputs(thresholds):
    return np.concatenate([gm.edge_values(thresholds).ravel(), gm.exact_root_values(), gm.SPECIALS, gm.log_uniform()])


def oracle_bytes_d(oracle, values):
    rgba = np.zeros((len(values), 4), np.float32)
    rgba[:, 0] = values
    return oracle.tonemap(rgba)[:, 0]


def oracle_bytes_f(oracle, values):
    """or_progressive_accumulate at frame number 1 on accum = 0: the display value is the input itself (0 + c, times 1.0f), except that -0 becomes +0: byte 0 either way"""
    accum = np.zeros((len(values), 4), np.float32)
    frame = np.zeros_like(accum)
    frame[:, 0] = values
    disp, rgb8 = oracle.progressive_accumulate(accum, frame, 1)
    shown, given = disp[:, 0].view(np.uint32), np.asarray(values, np.float32).view(np.uint32)
    assert np.array_equal(shown[given != 0x80000000], given[given != 0x80000000])
    return rgb8[:, 0]


def differing(values, got, exp):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(exp))
    return [(float(values[i]), hex(int(np.asarray(values, np.float32).view(np.uint32)[i])), int(got[i]), int(exp[i])) for i in bad[:8]], len(bad)


def test_exponents_are_the_c_expressions():
    assert gm.EXP_D == 1 / 2.2
    assert np.float32(gm.EXP_F) == gm.EXP_F == float(np.float32(1) / np.float32(2.2))
    assert f"{gm.EXP_F:.10f}" == "0.4545454383"


def test_exact_roots_truncate_below_their_code():
    """2048 = 32^2.2 and 177147 = 243^2.2 exactly, but the exponent is fl(1/2.2) < 1/2.2: the power is 1.04 and 1.56 binary64 ulps below the code"""
    assert gm.byte_d(2048.0) == 31 and gm.byte_d(177147.0) == 242
    assert gm.byte_d(float(np.nextafter(np.float32(2048), np.float32(np.inf)))) == 32
    assert gm.byte_d(float(np.nextafter(np.float32(177147), np.float32(np.inf)))) == 243


def test_special_values():
    exp_d = dict(zip(range(15), [0, 0, 0, 0, 0, 0, 1, 254, 255, 255, 255, 0, 0, 255, 0]))
    exp_f = dict(zip(range(15), [0, 0, 0, 0, 0, 0, 1, 254, 255, 255, 255, 255, 255, 255, 255]))
    for i, v in enumerate(gm.SPECIALS):
        assert gm.byte_d(v) == exp_d[i], (i, v)
        assert gm.byte_f(v) == exp_f[i], (i, v)


@pytest.mark.parametrize("path", ["d", "f"])
def test_thresholds_rise_and_split_their_neighbours(path):
    t = gm.thresholds_d() if path == "d" else gm.thresholds_f()
    fn = gm.byte_d if path == "d" else gm.byte_f
    assert len(t) == 255 and all(a < b for a, b in zip(t, t[1:]))
    for k, b in enumerate(t, start=1):
        assert fn(gm.f32_of_bits(b)) == k and fn(gm.f32_of_bits(b - 1)) == k - 1, k
    ev = gm.edge_values(t)
    assert gm.edges_are_covered(np.concatenate([ev.ravel(), gm.SPECIALS]), gm.bytes_of(fn, np.concatenate([ev.ravel(), gm.SPECIALS])), t)


def test_the_two_paths_have_their_own_edges():
    """1 / 2.2f is below 1./2.2, so the binary32 path's thresholds sit higher, by up to 6 floats: a fixture built on fl(k^2.2) +- 2 floats does not reach them"""
    d, f = np.array(gm.thresholds_d()), np.array(gm.thresholds_f())
    assert f[0] == d[0] - 1                                            # the float below 1: its power rounds to 1 in binary32, not in binary64
    assert (f[1:] >= d[1:]).all() and (f - d).max() >= 5
    b = (np.arange(1, 256, dtype=np.float64) ** 2.2).astype(np.float32).view(np.uint32).astype(np.int64)
    assert (np.abs(f - b) > 2).sum() > 100


def test_many_float_inputs_sit_within_an_ulp_of_a_code():
    """of the binary32 path's 2040 edge inputs, those whose exact power lies within one binary32 ulp of a code: the ones a powf that is not correctly rounded may flip
    (1074 with the ulp taken on the power's own side of the code, which halves below a power of two)"""
    near = sum(1 for v in gm.edge_values(gm.thresholds_f()).ravel() if gm.ulps_from_a_code(v) <= 1.0)
    print(f"{near} of 2040 edge inputs within one binary32 ulp of a code")
    assert near >= 1000


def test_model_equals_the_oracle_double_path(oracle):
    for t in (gm.thresholds_d(), gm.thresholds_f()):
        v = inputs(t)
        got, exp = oracle_bytes_d(oracle, v), gm.bytes_of(gm.byte_d, v)
        bad, n = differing(v, got, exp)
        assert n == 0, f"{n} bytes differ (value, bits, oracle, model): {bad}"


def test_model_equals_the_oracle_float_path(oracle):
    for t in (gm.thresholds_d(), gm.thresholds_f()):
        v = inputs(t)
        got, exp = oracle_bytes_f(oracle, v), gm.bytes_of(gm.byte_f, v)
        bad, n = differing(v, got, exp)
        assert n == 0, f"{n} bytes differ (value, bits, oracle, model): {bad}"


def test_model_equals_the_fixture(ref):
    """every prog_<n>_bytes row: what the reference's own kernel wrote for the display values it recorded"""
    for n in ref["prog_frames"]:
        disp, exp = ref[f"prog_{n}_display"], ref[f"prog_{n}_bytes"][:, :3]
        got = gm.bytes_of(gm.byte_f, disp)
        bad, cnt = differing(disp.ravel(), got.ravel(), exp.ravel())
        assert cnt == 0, f"frame {n}: {cnt} bytes differ (value, bits, model, fixture): {bad}"


# ---- the committed table of the binary32 path (raytracinggpu_amd/csrc/rt_gamma.h) and the function that reads it, through the host library
def committed_tables():
    """{path: [255 bit patterns]} as the header's text holds them"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "raytracinggpu_amd", "csrc", "rt_gamma.h")) as f:
        text = f.read()
    blocks = re.findall(r"// gamma-table-begin (\w)\n(.*?)// gamma-table-end", text, re.S)
    return {path: [int(x, 16) for x in re.findall(r"0x([0-9a-f]{8})u", body)] for path, body in blocks}


def test_committed_table_is_the_models():
    """the header holds the table of the path whose kernel needed it -- the binary32 one -- and its text is what the model gives today"""
    tables = committed_tables()
    assert sorted(tables) == ["f"]
    assert tuple(tables["f"]) == gm.thresholds_f()


def test_host_function_splits_every_threshold():
    """rth_gamma_byte, the text accumulate_kernel compiles: T_k gives k and the float below it k - 1, for every k of the committed table"""
    from raytracinggpu_amd import hostlib
    t = np.array(committed_tables()["f"], np.uint32)
    assert len(t) == 255
    assert np.array_equal(hostlib.gamma_byte(t.view(np.float32)), np.arange(1, 256, dtype=np.uint8))
    assert np.array_equal(hostlib.gamma_byte((t - 1).view(np.float32)), np.arange(0, 255, dtype=np.uint8))


def test_host_function_equals_the_model():
    from raytracinggpu_amd import hostlib
    more = np.array([0x00000001, 0x007fffff, 0x00800000, 0x7f7fffff, 0x7f800001, 0x7fffffff, 0x80000001, 0x80800000, 0xff7fffff, 0xff800001, 0xffc00000,
                     0xffffffff], np.uint32).view(np.float32)
    for t in (gm.thresholds_d(), gm.thresholds_f()):
        v = np.concatenate([inputs(t), more])
        got, exp = hostlib.gamma_byte(v), gm.bytes_of(gm.byte_f, v)
        bad, n = differing(v, got, exp)
        assert n == 0, f"{n} bytes differ (value, bits, rth_gamma_byte, model): {bad}"
