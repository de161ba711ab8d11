"""rt_upsample[_device] at the boundary, without a GPU: the library exports the two symbols, the header declares them with the argument lists the ctypes binding uses,
rt_upsample_params is 16 bytes for ctypes and for the compiler, the ABI number did not move, a NULL context is refused, the header states the formula, the Python layer
marshals what it is given, and SvgfSequence refuses the sizes and combinations it cannot run."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_upsample_device", "rt_upsample")


def _header():
    return open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()


def test_symbols_are_exported_declared_and_bound_alike():
    lib = _capi.load()
    hdr = _header()
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _capi.EXPORTS, n
        m = re.search(r"\bint %s\(([^;]*)\);" % n, hdr)
        assert m, f"{n} is not declared"
        args = [a.strip() for a in m.group(1).split(",")]
        assert args[0] == "rt_ctx *ctx", n
        assert len(getattr(lib, n).argtypes) == len(args), (n, args)
    assert len(lib.rt_upsample_device.argtypes) == 9 and len(lib.rt_upsample.argtypes) == 8


def test_struct_size_and_layout():
    u = _capi.UpsampleParams
    assert C.sizeof(u) == 16
    assert [u.factor.offset, u.n_planes.offset, u.k_normal.offset, u.k_position.offset] == [0, 4, 8, 12]
    src = ('#include "raytrace_hip.h"\n#include <stddef.h>\n'
           "_Static_assert(sizeof(rt_upsample_params) == 16, \"size\");\n"
           "_Static_assert(offsetof(rt_upsample_params, n_planes) == 4 && offsetof(rt_upsample_params, k_normal) == 8 && offsetof(rt_upsample_params, k_position) == 12, "
           "\"offsets\");\n")
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), "-"], input=src.encode(), check=True)


def test_abi_version_is_still_6():
    assert _capi.load().rt_abi_version() == 6
    assert "#define RT_ABI_VERSION 6" in _header()


def test_header_states_the_formula():
    hdr = _header()
    for word in ("gx = ((float)x + 0.5f) / (float)f - 0.5f", "q = (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1)", "w = b wn wp, multiplied left to right",
                 "a miss matches a miss", "the .w of the first counted tap", "plain bilinear", "takes the plain bilinear value", "A SPEED KNOB, not a quality feature",
                 "never fed back", "That is why the weights have no albedo term"):
        assert word in hdr, word


def test_null_context_is_refused():
    lib = _capi.load()
    fp = C.POINTER(C.c_float)
    low, laov, aov = np.zeros((2, 2, 4), np.float32), np.zeros((3, 2, 2, 4), np.float32), np.zeros((3, 4, 4, 4), np.float32)
    out = np.full((4, 4, 4), -7, np.float32)
    up = rt.make_upsample_params(2)
    assert lib.rt_upsample(None, low.ctypes.data_as(fp), laov.ctypes.data_as(fp), aov.ctypes.data_as(fp), 4, 4, C.byref(up), out.ctypes.data_as(fp)) == -1
    assert b"NULL" in lib.rt_last_error(None)
    assert lib.rt_upsample_device(None, None, None, None, 4, 4, C.byref(up), None, None) == -1
    assert (out == -7).all()


def test_default_parameters():
    u = rt.make_upsample_params(2)
    assert (u.factor, u.n_planes, u.k_normal, u.k_position) == (2, 1, 2.0, 0.25)
    assert rt.UPSAMPLE_DEFAULTS == dict(k_normal=2.0, k_position=0.25)
    u = rt.make_upsample_params(4, 2, k_normal=0.0, k_position=1.5)
    assert (u.factor, u.n_planes, u.k_normal, u.k_position) == (4, 2, 0.0, 1.5)
    assert isinstance(u, rt.UpsampleParams)


class _Recorder:
    """stands in for the loaded library: records every call with its arguments"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def _recording_context():
    c = rt.Context.__new__(rt.Context)
    c._L = _Recorder()
    c._h = C.c_void_p()
    return c


def test_python_marshals_frames_histories_and_parameters():
    c = _recording_context()
    laov, aov = np.zeros((3, 5, 7, 4), np.float32), np.zeros((3, 15, 21, 4))
    out = c.upsample(np.zeros((5, 7, 4)), laov, aov, 3)
    assert out.shape == (15, 21, 4) and out.dtype == np.float32
    out = c.upsample(np.zeros((2, 5, 7, 4), np.float32), laov, aov, 3, k_normal=0.0)
    assert out.shape == (2, 15, 21, 4)
    c.upsample_device(0x1000, 0x2000, 0x3000, 21, 15, 3, 0x4000, n_planes=2, stream=0x5000)
    assert [n for n, _ in c._L.calls] == ["rt_upsample", "rt_upsample", "rt_upsample_device"]
    a = c._L.calls[0][1]                                                # (ctx, low, low_aov, aov, width, height, params, out)
    assert (a[4], a[5]) == (21, 15) and (a[6]._obj.factor, a[6]._obj.n_planes, a[6]._obj.k_normal) == (3, 1, 2.0)
    a = c._L.calls[1][1]
    assert (a[6]._obj.n_planes, a[6]._obj.k_normal, a[6]._obj.k_position) == (2, 0.0, 0.25)
    a = c._L.calls[2][1]                                                # (ctx, low, low_aov, aov, width, height, params, out, stream)
    assert (a[1].value, a[2].value, a[3].value, a[4], a[5], a[7].value, a[8].value) == (0x1000, 0x2000, 0x3000, 21, 15, 0x4000, 0x5000) and a[6]._obj.n_planes == 2
    for bad in (lambda: c.upsample(np.zeros((5, 7, 4)), laov, aov, 2), lambda: c.upsample(np.zeros((3, 5, 7, 4)), laov, aov, 3),
                lambda: c.upsample(np.zeros((5, 7, 4)), laov[:2], aov, 3), lambda: c.upsample(np.zeros((5, 7, 4)), laov, aov, 3, out=np.zeros((15, 21, 4)))):
        with pytest.raises(rt.RtError) as e:
            bad()
        assert e.value.code == -1
    assert len(c._L.calls) == 3
    c._h = None


class _Allocator(_Recorder):
    def rt_device_alloc(self, h, p, n):
        self.calls.append(("rt_device_alloc", n))
        p._obj.value = 0x10000 * len(self.calls)
        return 0


def test_sequence_takes_the_option_and_refuses_what_it_cannot_run():
    c = _recording_context()
    c._L = _Allocator()
    with pytest.raises(rt.RtError):
        rt.SvgfSequence(c, 130, 128, upsample=4)                      # no multiple
    with pytest.raises(rt.RtError):
        rt.SvgfSequence(c, 128, 128, upsample=5)
    with pytest.raises(rt.RtError):
        rt.SvgfSequence(c, 128, 128, upsample=2, filter_at="both")
    with pytest.raises(rt.RtError):                                    # B never feeds its full-resolution history back
        rt.SvgfSequence(c, 128, 128, upsample=2, filter_at="full", svgf=rt.make_svgf_params(feedback_pass=0))
    assert not [x for x in c._L.calls if x[0] == "rt_device_alloc"]
    frame = 128 * 128 * 16
    seq = rt.SvgfSequence(c, 128, 128)
    assert (seq.upsample, seq.filter_at, seq.low_width, seq.low_height) == (1, "low", 128, 128)
    assert sorted(n for name, n in c._L.calls if name == "rt_device_alloc") == sorted(k * frame for k in (1, 1, 2, 2, 3, 3))
    c._L.calls.clear()
    seq = rt.SvgfSequence(c, 128, 128, upsample=2, filter_at="full")
    low = frame // 4
    assert (seq.low_width, seq.low_height) == (64, 64)
    assert sorted(n for name, n in c._L.calls if name == "rt_device_alloc") == sorted([low, 2 * low, 2 * low, 3 * low, 3 * low, frame, 3 * frame, 2 * frame])
    c._h = None
