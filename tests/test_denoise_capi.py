"""First-hit planes and the denoiser at the boundary, without a GPU: the library exports rt_render_aov[_device] and rt_denoise[_device], the header declares them with
the argument lists the ctypes binding uses, the ABI number did not move, a NULL context is refused, the Python methods marshal shapes and parameters, and the C++
Renderer members compile."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_render_aov_device", "rt_render_aov", "rt_denoise_device", "rt_denoise")


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
    assert C.sizeof(_capi.DenoiseParams) == 20
    assert "typedef struct rt_denoise_params" in hdr and "int32_t n_passes;" in hdr
    for word in ("plane 0", "plane 1", "plane 2", "FIRST hit"):      # the layout and the caveat are stated where a caller reads them
        assert word in hdr, word


def test_abi_version_is_still_6():
    assert _capi.load().rt_abi_version() == 6
    assert "#define RT_ABI_VERSION 6" in _header()


def test_null_context_is_refused():
    lib = _capi.load()
    fp = C.POINTER(C.c_float)
    p = rt.make_params(4, 4)
    buf = np.zeros((3, 4, 4, 4), np.float32)
    col, out = np.zeros((4, 4, 4), np.float32), np.zeros((4, 4, 4), np.float32)
    dp = rt.make_denoise_params()
    assert lib.rt_render_aov(None, C.byref(p), None, None, buf.ctypes.data_as(fp)) == -1
    assert b"NULL" in lib.rt_last_error(None)
    assert lib.rt_render_aov_device(None, C.byref(p), None, None, None, None) == -1
    assert lib.rt_denoise(None, col.ctypes.data_as(fp), buf.ctypes.data_as(fp), 4, 4, C.byref(dp), out.ctypes.data_as(fp)) == -1
    assert b"NULL" in lib.rt_last_error(None)
    assert lib.rt_denoise_device(None, None, None, 4, 4, C.byref(dp), None, None) == -1
    assert not out.any()


def test_default_parameters():
    d = rt.make_denoise_params()
    assert (d.n_passes, d.k_normal, d.k_position, d.k_albedo) == (3, 2.0, 0.25, 16.0) and d.k_color == np.float32(5e-12)
    d = rt.make_denoise_params(n_passes=5, k_color=0.0)
    assert d.n_passes == 5 and d.k_color == 0.0 and d.k_normal == 2.0


class _Recorder:
    """stands in for the loaded library: records every call with its arguments"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def _fake_context():
    c = rt.Context.__new__(rt.Context)
    c._L = _Recorder()
    c._h = C.c_void_p()
    return c


def test_python_marshals_planes_and_parameters():
    c = _fake_context()
    p = rt.make_params(7, 5)
    aov = c.render_aov(p)
    assert aov.shape == (3, 5, 7, 4) and aov.dtype == np.float32
    rows, idx = rt.interleaved_rows(5, 2, 1, 2)
    assert c.render_aov(p, pose=rt.make_pose(), rows=rows).shape == (3, len(idx), 7, 4)
    c.render_aov_device(p, 0x1000)
    color = np.zeros((5, 7, 4))
    out = c.denoise(color, aov, n_passes=2, k_color=0.0)
    assert out.shape == (5, 7, 4) and out.dtype == np.float32
    c.denoise_device(0x1000, 0x2000, 7, 5, 0x3000, k_normal=1.5)
    names = [n for n, _ in c._L.calls]
    assert names == ["rt_render_aov", "rt_render_aov", "rt_render_aov_device", "rt_denoise", "rt_denoise_device"]
    assert c._L.calls[0][1][2] is None and c._L.calls[0][1][3] is None        # no pose, whole frame
    assert c._L.calls[1][1][2] is not None and c._L.calls[1][1][3]._obj.n_rows == len(idx)
    a = c._L.calls[2][1]                                                        # (ctx, params, pose, rows, out, stream)
    assert a[3]._obj.n_rows == 5 and a[4].value == 0x1000 and a[5] is None
    a = c._L.calls[3][1]                                                        # (ctx, color, aov, width, height, params, out)
    assert (a[3], a[4]) == (7, 5) and a[5]._obj.n_passes == 2 and a[5]._obj.k_color == 0.0 and a[5]._obj.k_albedo == 16.0
    a = c._L.calls[4][1]                                                        # (ctx, color, aov, width, height, params, out, stream)
    assert (a[1].value, a[2].value, a[3], a[4], a[6].value) == (0x1000, 0x2000, 7, 5, 0x3000) and a[5]._obj.k_normal == 1.5
    # planes of another frame size never reach the library
    with pytest.raises(rt.RtError) as e:
        c.denoise(color, np.zeros((3, 5, 8, 4), np.float32))
    assert e.value.code == -1 and len(c._L.calls) == 5
    c._h = None


def test_renderer_members_compile(tmp_path):
    src = tmp_path / "dn.cpp"
    src.write_text("""
#include "raytracer.hpp"
using namespace raytracer;
std::vector<float> use(Renderer &r, const RenderSettings &s, const rt_camera_pose &pose) {
    std::vector<float> color = r.render_float(s);
    std::vector<float> aov = r.render_aov(s), posed = r.render_aov(s, &pose);
    rt_denoise_params dp{3, 2.0f, 0.25f, 16.0f, 5e-12f};
    return r.denoise(color, aov, s.W, s.H, dp);
}
""")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
