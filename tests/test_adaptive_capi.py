"""Adaptive sampling at the boundary, without a GPU: the library exports the new symbols, the header declares them with the argument lists the ctypes binding uses,
rt_sample_count_params is 24 bytes for ctypes and for the compiler, the ABI number did not move, NULL and invalid arguments are refused before any device call, the
header states the contract and the formula, the Python layer marshals what it is given, and SvgfSequence takes the option only where it can run it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_render_counts_device", "rt_render_counts", "rt_render_counts_info", "rt_sample_counts_device", "rt_sample_counts", "rt_kat_sample_plan")


def _header():
    return open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()


def test_symbols_are_exported_declared_and_bound_alike():
    lib = _capi.load()
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)            # (a declaration may carry a comment between its arguments)
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _capi.EXPORTS, n
        m = re.search(r"\bint %s\(([^;]*)\);" % n, hdr)
        assert m, f"{n} is not declared"
        args = [a.strip() for a in m.group(1).split(",")]
        assert args[0] in ("rt_ctx *ctx", "const rt_ctx *ctx"), n
        assert len(getattr(lib, n).argtypes) == len(args), (n, args)
    assert len(lib.rt_render_counts_device.argtypes) == 7 and len(lib.rt_render_counts.argtypes) == 6
    assert len(lib.rt_sample_counts_device.argtypes) == 7 and len(lib.rt_sample_counts.argtypes) == 6 and len(lib.rt_kat_sample_plan.argtypes) == 9


def test_struct_size_and_layout():
    s = _capi.SampleCountParams
    assert C.sizeof(s) == 24
    assert [getattr(s, f).offset for f, _ in s._fields_] == [0, 4, 8, 12, 16, 20]
    assert [f for f, _ in s._fields_] == ["max_samples", "short_history", "new_surface_samples", "k_rel", "lum_floor", "reserved"]
    src = ('#include "raytrace_hip.h"\n#include <stddef.h>\n'
           "_Static_assert(sizeof(rt_sample_count_params) == 24, \"size\");\n"
           "_Static_assert(offsetof(rt_sample_count_params, short_history) == 4 && offsetof(rt_sample_count_params, new_surface_samples) == 8 && "
           "offsetof(rt_sample_count_params, k_rel) == 12 && offsetof(rt_sample_count_params, lum_floor) == 16 && offsetof(rt_sample_count_params, reserved) == 20, "
           "\"offsets\");\n_Static_assert(RT_MAX_SAMPLE_COUNT == 64, \"limit\");\n")
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), "-"], input=src.encode(), check=True)
    assert rt.MAX_SAMPLE_COUNT == 64


def test_abi_version_is_still_6():
    assert _capi.load().rt_abi_version() == 6
    assert "#define RT_ABI_VERSION 6" in _header()


def test_header_states_the_contract_and_the_formula():
    hdr = _header()
    for word in ("bit for bit and .w included", "p->num_rays = c", "inv_n = (float)(1. / c)", "With base == NULL a pixel with c == 0 is (0, 0, 0, 0)",
                 "p->num_rays is not read", "Counts above RT_MAX_SAMPLE_COUNT are read as RT_MAX_SAMPLE_COUNT", "Pixels with c <= 1 are copied from it",
                 "trace only samples 1 .. c - 1 and start their sum from base", "a one-sample frame stores (0 + a0) / 1", "out == base is allowed",
                 "Whole frames only", "RT_ERR_UNSUPPORTED", "rt_first_hit_cache_counts does not move", "THE ENTRY WAITS ON THE STREAM ONCE",
                 "n == 0 (a miss):  count = 1", "e_n   = (n < (float)short_history) ? (float)(new_surface_samples - 1) : 0", "rel   = V / (m1 m1 + lum_floor)",
                 "e_v   = floor(k_rel rel), taken as 0 unless it compares >= 1 (so a NaN gives 0)", "count = 1 + min((float)(max_samples - 1), max(e_n, e_v))",
                 "IEEE minNum / maxNum", "#define RT_MAX_SAMPLE_COUNT 64"):
        assert word in hdr, word


def test_null_and_invalid_arguments_are_refused_before_any_device_call():
    """(this machine has no GPU: a call that got as far as the device would answer RT_ERR_HIP or RT_ERR_NO_DEVICE, not RT_ERR_INVALID)"""
    lib = _capi.load()
    fp, u8 = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    p = rt.make_params(4, 4, 1, 1)
    counts = np.ones((4, 4), np.uint8)
    out = np.full((4, 4, 4), -7, np.float32)
    assert lib.rt_render_counts(None, C.byref(p), None, counts.ctypes.data_as(u8), None, out.ctypes.data_as(fp)) == -1
    assert b"NULL" in lib.rt_last_error(None)
    assert lib.rt_render_counts_device(None, C.byref(p), None, None, None, None, None) == -1
    hist = np.ones((2, 4, 4, 4), np.float32)
    cnt = np.full((4, 4), 9, np.uint8)
    cp = rt.make_sample_count_params()
    assert lib.rt_sample_counts(None, hist.ctypes.data_as(fp), 4, 4, C.byref(cp), cnt.ctypes.data_as(u8)) == -1
    assert lib.rt_sample_counts_device(None, None, 4, 4, C.byref(cp), None, None) == -1
    n = C.c_uint64(77)
    assert lib.rt_kat_sample_plan(None, counts.ctypes.data_as(u8), 4, 4, 0, None, None, C.byref(n), None) == -1
    assert lib.rt_render_counts_info(None, (C.c_uint64 * 4)()) == -1
    assert (out == -7).all() and (cnt == 9).all() and n.value == 77


def test_default_parameters():
    d = rt.make_sample_count_params()
    assert isinstance(d, rt.SampleCountParams) and d.reserved == 0
    assert {k: getattr(d, k) for k in rt.SAMPLE_COUNT_DEFAULTS} == pytest.approx(rt.SAMPLE_COUNT_DEFAULTS)
    assert 1 <= d.new_surface_samples <= d.max_samples <= rt.MAX_SAMPLE_COUNT and d.short_history >= 0
    d = rt.make_sample_count_params(max_samples=8, short_history=3, new_surface_samples=2, k_rel=1.5, lum_floor=0.25)
    assert (d.max_samples, d.short_history, d.new_surface_samples, d.k_rel, d.lum_floor) == (8, 3, 2, 1.5, 0.25)


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


def test_python_marshals_counts_frames_and_parameters():
    c = _recording_context()
    p = rt.make_params(7, 5, 1, 2)
    out = c.render_counts(p, np.ones((5, 7), np.uint8))
    assert out.shape == (5, 7, 4) and out.dtype == np.float32
    base = np.zeros((5, 7, 4), np.float32)
    assert c.render_counts(p, np.ones((5, 7), np.uint8), pose=rt.make_pose(), base=base, out=base) is base
    c.render_counts_device(p, 0x1000, 0x3000, base_ptr=0x2000, stream=0x5000)
    cnt = c.sample_counts(np.zeros((2, 5, 7, 4)), rt.make_sample_count_params(max_samples=9))
    assert cnt.shape == (5, 7) and cnt.dtype == np.uint8
    c.sample_counts_device(0x1000, 7, 5, 0x2000, stream=0x5000)
    assert [n for n, _ in c._L.calls] == ["rt_render_counts", "rt_render_counts", "rt_render_counts_device", "rt_sample_counts", "rt_sample_counts_device"]
    a = c._L.calls[0][1]                                                # (ctx, params, pose, counts, base, out)
    assert a[2] is None and a[4] is None
    a = c._L.calls[1][1]
    assert a[2] is not None and C.cast(a[4], C.c_void_p).value == C.cast(a[5], C.c_void_p).value == base.ctypes.data
    a = c._L.calls[2][1]                                                # (ctx, params, pose, counts, base, out, stream)
    assert (a[2], a[3].value, a[4].value, a[5].value, a[6].value) == (None, 0x1000, 0x2000, 0x3000, 0x5000)
    a = c._L.calls[3][1]                                                # (ctx, history, width, height, params, counts)
    assert (a[2], a[3], a[4]._obj.max_samples) == (7, 5, 9)
    a = c._L.calls[4][1]                                                # (ctx, history, width, height, params, counts, stream)
    assert (a[1].value, a[2], a[3], a[5].value, a[6].value) == (0x1000, 7, 5, 0x2000, 0x5000) and a[4]._obj.max_samples == rt.SAMPLE_COUNT_DEFAULTS["max_samples"]
    for bad in (lambda: c.render_counts(p, np.ones((5, 7), np.int32)), lambda: c.render_counts(p, np.ones((7, 5), np.uint8)),
                lambda: c.render_counts(p, np.ones((5, 7), np.uint8), base=np.zeros((5, 7, 3))), lambda: c.sample_counts(np.zeros((5, 7, 4))),
                lambda: c.kat_sample_plan(np.ones((5, 7), np.float32))):
        with pytest.raises(rt.RtError) as e:
            bad()
        assert e.value.code == -1
    assert len(c._L.calls) == 5
    c._h = None


class _Allocator(_Recorder):
    def rt_device_alloc(self, h, p, n):
        self.calls.append(("rt_device_alloc", n))
        p._obj.value = 0x10000 * len(self.calls)
        return 0


def test_sequence_takes_the_option_only_at_full_resolution():
    c = _recording_context()
    c._L = _Allocator()
    ad = rt.make_sample_count_params()
    with pytest.raises(rt.RtError):
        rt.SvgfSequence(c, 128, 128, adaptive=ad, upsample=2)
    assert not [x for x in c._L.calls if x[0] == "rt_device_alloc"]
    frame = 128 * 128 * 16
    seq = rt.SvgfSequence(c, 128, 128)
    assert seq.adaptive is None
    assert sorted(n for name, n in c._L.calls if name == "rt_device_alloc") == sorted(k * frame for k in (1, 1, 2, 2, 3, 3))
    c._L.calls.clear()
    seq = rt.SvgfSequence(c, 128, 128, adaptive=ad)
    assert sorted(n for name, n in c._L.calls if name == "rt_device_alloc") == sorted([128 * 128] + [k * frame for k in (1, 1, 2, 2, 3, 3)])
    # the frame's calls, in order: the one-sample frame, the planes, the accumulation, the counts, the extra samples in place, the accumulation again, the filter
    c._L.calls.clear()
    seq.frame(rt.make_params(128, 128, 1, 2))
    names = [n for n, _ in c._L.calls]
    assert names == ["rt_render_device", "rt_render_aov_device", "rt_temporal_accumulate_device", "rt_sample_counts_device", "rt_render_counts_device",
                     "rt_temporal_accumulate_device", "rt_svgf_filter_device"], names
    rc = c._L.calls[4][1]
    assert rc[3].value == seq.counts and rc[4].value == rc[5].value == seq.color
    assert [a.value if a is not None else None for a in c._L.calls[2][1][1:5]] == [a.value if a is not None else None for a in c._L.calls[5][1][1:5]]
    c._h = None
