"""rt_temporal_accumulate_fast[_device] and rt_history_rectify[_device] at the boundary, without a GPU: the library exports the four symbols, the header declares them with
the argument lists the ctypes binding uses, rt_rectify_params is 8 bytes for ctypes and for the compiler, the ABI number did not move, a NULL context is refused, the
header states the formula, the Python layer marshals what it is given, and Renderer::history_rectify compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_temporal_accumulate_fast_device", "rt_temporal_accumulate_fast", "rt_history_rectify_device", "rt_history_rectify")


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
    assert [len(getattr(lib, n).argtypes) for n in NEW] == [14, 13, 9, 8]


def test_struct_size_and_layout():
    assert C.sizeof(_capi.RectifyParams) == 8
    assert (_capi.RectifyParams.radius.offset, _capi.RectifyParams.k_clamp.offset) == (0, 4)
    assert "typedef struct rt_rectify_params" in _header()
    src = ('#include "raytrace_hip.h"\n#include <stddef.h>\n'
           "_Static_assert(sizeof(rt_rectify_params) == 8, \"size\");\n"
           "_Static_assert(offsetof(rt_rectify_params, radius) == 0 && offsetof(rt_rectify_params, k_clamp) == 4, \"offsets\");\n")
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), "-"], input=src.encode(), check=True)


def test_abi_version_is_still_6():
    assert _capi.load().rt_abi_version() == 6
    assert "#define RT_ABI_VERSION 6" in _header()


def test_header_states_the_formula():
    hdr = _header()
    for word in ("n_f = min(F_q.w + 1, (float)fast_history)", "a_f = max(1 / n_f, alpha_min)", "F = F_q.rgb + a_f (C_p.rgb - F_q.rgb)", "takes the SAME tap q",
                 "H1_p.z <= F_p.w", "the pixel itself always counts", "s1_c += F_q.c;   s2_c += F_q.c F_q.c;   cnt += 1",
                 "sg_c = sqrt(max(0, e2_c - mu_c mu_c))", "lo_c = mu_c - k_clamp sg_c;   hi_c = mu_c + k_clamp sg_c;   H'_c = min(max(H_c, lo_c), hi_c)",
                 "If no channel moved (H'_c == H_c for all three):  a copy, every word", "n' = F_p.w", "m2' = m2 + (m1' m1' - m1 m1)",
                 "out == history EXACTLY (in place) is allowed", "a NaN H_c is replaced by lo_c", "radius\n *     outside [1, 3]"):
        assert word in hdr, word


def test_null_context_is_refused():
    lib = _capi.load()
    fp = C.POINTER(C.c_float)
    frame, two = np.zeros((4, 4, 4), np.float32), np.zeros((2, 4, 4, 4), np.float32)
    out, outf = np.full((2, 4, 4, 4), -7, np.float32), np.full((4, 4, 4), -7, np.float32)
    tp, rp = rt.make_temporal_params(), rt.make_rectify_params()
    p = lambda a: a.ctypes.data_as(fp)
    assert lib.rt_temporal_accumulate_fast(None, p(frame), p(two), None, None, None, 4, 4, C.byref(tp), None, 4, p(out), p(outf)) == -1
    assert b"NULL" in lib.rt_last_error(None)
    assert lib.rt_temporal_accumulate_fast_device(None, None, None, None, None, None, 4, 4, C.byref(tp), None, 4, None, None, None) == -1
    assert lib.rt_history_rectify(None, p(two), p(frame), p(frame), 4, 4, C.byref(rp), p(out)) == -1
    assert lib.rt_history_rectify_device(None, None, None, None, 4, 4, C.byref(rp), None, None) == -1
    assert (out == -7).all() and (outf == -7).all()


def test_default_parameters():
    r = rt.make_rectify_params()
    assert (r.radius, r.k_clamp) == (_capi.RECTIFY_DEFAULTS["radius"], np.float32(_capi.RECTIFY_DEFAULTS["k_clamp"]))
    r = rt.make_rectify_params(radius=3, k_clamp=0.5)
    assert (r.radius, r.k_clamp) == (3, 0.5)
    assert rt.RectifyParams is _capi.RectifyParams and rt.RECTIFY_DEFAULTS is _capi.RECTIFY_DEFAULTS and rt.FAST_HISTORY_DEFAULT == 4


class _Recorder:
    """stands in for the loaded library: records every call with its arguments"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def test_python_marshals_planes_and_parameters():
    c = rt.Context.__new__(rt.Context)
    c._L = _Recorder()
    c._h = C.c_void_p()
    color, aov, hist = np.zeros((5, 7, 4)), np.zeros((3, 5, 7, 4), np.float32), np.zeros((2, 5, 7, 4), np.float32)
    h, f = c.temporal_accumulate_fast(color, aov)
    assert h.shape == (2, 5, 7, 4) and f.shape == (5, 7, 4) and h.dtype == f.dtype == np.float32
    c.temporal_accumulate_fast(color, aov, aov, hist, f, reproject=rt.make_reproject(), fast_history=2)
    out = c.history_rectify(hist, f, aov, params=rt.make_rectify_params(radius=2, k_clamp=3.0))
    assert out.shape == hist.shape and out is not hist
    assert c.history_rectify(hist, f, aov[:1], out=hist) is hist       # in place
    c.temporal_accumulate_fast_device(0x1000, 0x2000, None, None, None, 7, 5, 0x3000, 0x4000)
    c.history_rectify_device(0x3000, 0x4000, 0x2000, 7, 5, 0x3000)
    names = [n for n, _ in c._L.calls]
    assert names == ["rt_temporal_accumulate_fast"] * 2 + ["rt_history_rectify"] * 2 + ["rt_temporal_accumulate_fast_device", "rt_history_rectify_device"]
    a = c._L.calls[0][1]                # (ctx, color, aov, prev_aov, prev_history, prev_fast, width, height, tp, rp, fast_history, out, out_fast)
    assert a[3] is None and a[4] is None and a[5] is None and (a[6], a[7]) == (7, 5) and a[9] is None and a[10] == 4
    a = c._L.calls[1][1]
    assert a[3] is not None and a[4] is not None and a[5] is not None and a[9] is not None and a[10] == 2
    a = c._L.calls[2][1]                # (ctx, history, fast, aov, width, height, params, out)
    assert (a[4], a[5]) == (7, 5) and a[6]._obj.radius == 2 and a[6]._obj.k_clamp == 3.0
    a = c._L.calls[4][1]
    assert (a[1].value, a[2].value, a[3], a[4], a[5], a[6], a[7], a[10], a[11].value, a[12].value, a[13]) == (0x1000, 0x2000, None, None, None, 7, 5, 4, 0x3000, 0x4000, None)
    a = c._L.calls[5][1]
    assert (a[1].value, a[7].value) == (0x3000, 0x3000) and a[6]._obj.radius == _capi.RECTIFY_DEFAULTS["radius"]
    for bad in (lambda: c.history_rectify(hist, f[:4], aov), lambda: c.history_rectify(hist[0], f, aov), lambda: c.temporal_accumulate_fast(color, aov, aov, hist, f[:, :6]),
                lambda: c.history_rectify(hist, f, aov, out=np.zeros((2, 5, 8, 4), np.float32))):
        with pytest.raises(rt.RtError) as e:
            bad()
        assert e.value.code == -1
    assert len(c._L.calls) == 6
    c._h = None


def test_sequence_takes_the_option():
    import inspect
    sig = inspect.signature(rt.SvgfSequence.__init__).parameters
    assert sig["rectify"].default is None and sig["fast_history"].default == 4


def test_renderer_members_compile(tmp_path):
    src = tmp_path / "rc.cpp"
    src.write_text("""
#include "raytracer.hpp"
using namespace raytracer;
std::vector<float> use(Renderer &r, const RenderSettings &s) {
    std::vector<float> color = r.render_float(s), aov = r.render_aov(s), none, fast, fast2;
    rt_temporal_params tp{32, 0.f, 0.9f, 0.5f};
    std::vector<float> h1 = r.temporal_accumulate_fast(color, aov, none, none, none, s.W, s.H, tp, nullptr, 4, fast);
    rt_rectify_params rc{1, 1.0f};
    h1 = r.history_rectify(h1, fast, aov, s.W, s.H, rc);
    rt_reproject rp{};
    std::vector<float> h2 = r.temporal_accumulate_fast(color, aov, aov, h1, fast, s.W, s.H, tp, &rp, 4, fast2);
    return r.history_rectify(h2, fast2, aov, s.W, s.H, rc);
}
""")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
