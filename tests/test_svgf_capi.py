"""rt_svgf_filter[_device] at the boundary, without a GPU: the library exports the two symbols, the header declares them with the argument lists the ctypes binding
uses, rt_svgf_params is 32 bytes for ctypes and for the compiler, the ABI number did not move, a NULL context is refused, the header states the formula, the Python
layer marshals what it is given, and Renderer::svgf_filter compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_svgf_filter_device", "rt_svgf_filter")


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
    assert len(lib.rt_svgf_filter_device.argtypes) == 9 and len(lib.rt_svgf_filter.argtypes) == 8


def test_struct_size_and_layout():
    assert C.sizeof(_capi.SvgfParams) == 32
    assert [(_capi.SvgfParams.n_passes.offset), _capi.SvgfParams.feedback_pass.offset, _capi.SvgfParams.prefilter.offset, _capi.SvgfParams.k_normal.offset,
            _capi.SvgfParams.var_floor.offset] == [0, 4, 8, 12, 28]
    assert "typedef struct rt_svgf_params" in _header()
    src = ('#include "raytrace_hip.h"\n#include <stddef.h>\n'
           "_Static_assert(sizeof(rt_svgf_params) == 32, \"size\");\n"
           "_Static_assert(offsetof(rt_svgf_params, feedback_pass) == 4 && offsetof(rt_svgf_params, prefilter) == 8 && offsetof(rt_svgf_params, k_normal) == 12 && "
           "offsetof(rt_svgf_params, var_floor) == 28, \"offsets\");\n")
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), "-"], input=src.encode(), check=True)


def test_abi_version_is_still_6():
    assert _capi.load().rt_abi_version() == 6
    assert "#define RT_ABI_VERSION 6" in _header()


def test_header_states_the_formula():
    hdr = _header()
    for word in ("g = G[|dy|] * G[|dx|], G = {1/2, 1/4}", "SG += g V_q;   WG += g;", "Vg = SG / WG;   D = k_sigma Vg + var_floor", "V_out = SV / (W W) over the unfiltered V_q",
                 "plane 0 = (.rgb of pass", "plane 1 = the input history's plane 1, bit for bit", "out_history is NULL exactly when feedback_pass == -1",
                 "excludes no tap for a non-finite V_q", "a deviation from implementations that always use step 1", "the output is rt_denoise_var's bit for bit"):
        assert word in hdr, word


def test_null_context_is_refused():
    lib = _capi.load()
    fp = C.POINTER(C.c_float)
    aov = np.zeros((3, 4, 4, 4), np.float32)
    hist = np.zeros((2, 4, 4, 4), np.float32)
    out, outh = np.full((4, 4, 4), -7, np.float32), np.full((2, 4, 4, 4), -7, np.float32)
    sp = rt.make_svgf_params(feedback_pass=0)
    assert lib.rt_svgf_filter(None, hist.ctypes.data_as(fp), aov.ctypes.data_as(fp), 4, 4, C.byref(sp), out.ctypes.data_as(fp), outh.ctypes.data_as(fp)) == -1
    assert b"NULL" in lib.rt_last_error(None)
    assert lib.rt_svgf_filter_device(None, None, None, 4, 4, C.byref(sp), None, None, None) == -1
    assert (out == -7).all() and (outh == -7).all()


def test_default_parameters():
    s = rt.make_svgf_params()
    d, v = _capi.SVGF_DEFAULTS, _capi.DENOISE_VAR_DEFAULTS
    assert (s.n_passes, s.feedback_pass, s.prefilter) == (d["n_passes"], d["feedback_pass"], d["prefilter"])
    assert all(getattr(s, k) == np.float32(v[k]) for k in ("k_normal", "k_position", "k_albedo", "k_sigma", "var_floor")) and s.n_passes == v["n_passes"]
    s = rt.make_svgf_params(n_passes=5, feedback_pass=4, prefilter=0, var_floor=1.5)
    assert (s.n_passes, s.feedback_pass, s.prefilter, s.var_floor) == (5, 4, 0, 1.5)


class _Recorder:
    """stands in for the loaded library: records every call with its arguments"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def test_python_marshals_histories_and_parameters():
    c = rt.Context.__new__(rt.Context)
    c._L = _Recorder()
    c._h = C.c_void_p()
    hist, aov = np.zeros((2, 5, 7, 4)), np.zeros((3, 5, 7, 4), np.float32)
    out, fed = c.svgf_filter(hist, aov, params=rt.make_svgf_params(feedback_pass=-1))
    assert out.shape == (5, 7, 4) and out.dtype == np.float32 and fed is None
    out, fed = c.svgf_filter(hist, aov, params=rt.make_svgf_params(n_passes=2, feedback_pass=1, prefilter=0))
    assert fed.shape == (2, 5, 7, 4) and fed.dtype == np.float32
    c.svgf_filter_device(0x1000, 0x2000, 7, 5, 0x3000, 0x4000, params=rt.make_svgf_params(feedback_pass=0))
    c.svgf_filter_device(0x1000, 0x2000, 7, 5, 0x3000)
    assert [n for n, _ in c._L.calls] == ["rt_svgf_filter", "rt_svgf_filter", "rt_svgf_filter_device", "rt_svgf_filter_device"]
    a = c._L.calls[0][1]                                                # (ctx, history, aov, width, height, params, out, out_history)
    assert (a[3], a[4]) == (7, 5) and a[5]._obj.feedback_pass == -1 and a[7] is None
    a = c._L.calls[1][1]
    assert a[5]._obj.n_passes == 2 and a[5]._obj.feedback_pass == 1 and a[5]._obj.prefilter == 0 and a[7] is not None
    a = c._L.calls[2][1]                                                # (ctx, history, aov, width, height, params, out, out_history, stream)
    assert (a[1].value, a[2].value, a[3], a[4], a[6].value, a[7].value, a[8]) == (0x1000, 0x2000, 7, 5, 0x3000, 0x4000, None)
    a = c._L.calls[3][1]
    assert a[7] is None and a[5]._obj.feedback_pass == _capi.SVGF_DEFAULTS["feedback_pass"]
    for bad in (lambda: c.svgf_filter(hist, np.zeros((3, 5, 8, 4), np.float32)), lambda: c.svgf_filter(hist[0], aov),
                lambda: c.svgf_filter(hist, aov, params=rt.make_svgf_params(feedback_pass=0), out_history=np.zeros((2, 5, 8, 4), np.float32))):
        with pytest.raises(rt.RtError) as e:
            bad()
        assert e.value.code == -1
    assert len(c._L.calls) == 4
    c._h = None


def test_sequence_is_exported():
    assert rt.SvgfSequence.__module__ == "raytracinggpu_amd.svgf"
    for name in ("frame", "close"):
        assert callable(getattr(rt.SvgfSequence, name))


def test_renderer_member_compiles(tmp_path):
    src = tmp_path / "sv.cpp"
    src.write_text("""
#include "raytracer.hpp"
using namespace raytracer;
std::vector<float> use(Renderer &r, const RenderSettings &s) {
    std::vector<float> color = r.render_float(s), aov = r.render_aov(s), none;
    rt_temporal_params tp{32, 0.f, 0.9f, 0.5f};
    std::vector<float> h1 = r.temporal_accumulate(color, aov, none, none, s.W, s.H, tp, nullptr);
    rt_svgf_params sp{3, 0, 1, 2.0f, 0.25f, 16.0f, 16.0f, 0.f};
    std::vector<float> fed;
    std::vector<float> out = r.svgf_filter(h1, aov, s.W, s.H, sp, &fed);
    rt_reproject rp{};
    std::vector<float> h2 = r.temporal_accumulate(color, aov, aov, fed, s.W, s.H, tp, &rp);
    sp.feedback_pass = -1;
    return r.svgf_filter(h2, aov, s.W, s.H, sp);
}
""")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
