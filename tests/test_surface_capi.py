"""The surface planes and the demodulate / modulate pair at the boundary, without a GPU: the library exports the six symbols, the header declares them with the
argument lists the ctypes binding uses, the ABI number did not move, a NULL context is refused by each, the Python methods marshal shapes, and the C++ Renderer
members compile."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_render_aov_surface_device", "rt_render_aov_surface", "rt_demodulate_device", "rt_demodulate", "rt_modulate_device", "rt_modulate")


def _header():
    return open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()


def test_symbols_are_exported_declared_and_bound_alike():
    lib = _capi.load()
    hdr = _header()
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _capi.EXPORTS, n
        m = re.search(r"\bint %s\s*\(([^;]*)\);" % n, hdr)
        assert m, f"{n} is not declared"
        args = [a.strip() for a in m.group(1).split(",")]
        assert args[0] == "rt_ctx *ctx", n
        assert len(getattr(lib, n).argtypes) == len(args), (n, args)
    for word in ("PATH CODE", "id + 16 first_id + 256 k", "max(A.c, albedo_floor)", "k_albedo = 0", "FIRST-HIT planes"):   # the contracts are stated where a caller reads them
        assert word in hdr, word


def test_abi_version_is_still_6():
    assert _capi.load().rt_abi_version() == 6
    assert "#define RT_ABI_VERSION 6" in _header()


def test_null_context_is_refused_by_each():
    lib = _capi.load()
    fp = C.POINTER(C.c_float)
    p = rt.make_params(4, 4)
    buf = np.zeros((3, 4, 4, 4), np.float32)
    col, out = np.ones((4, 4, 4), np.float32), np.zeros((4, 4, 4), np.float32)
    assert lib.rt_render_aov_surface(None, C.byref(p), None, None, 4, buf.ctypes.data_as(fp)) == -1
    assert b"NULL" in lib.rt_last_error(None)
    assert lib.rt_render_aov_surface_device(None, C.byref(p), None, None, 4, None, None) == -1
    for name in ("rt_demodulate", "rt_modulate"):
        assert getattr(lib, name)(None, col.ctypes.data_as(fp), buf.ctypes.data_as(fp), 16, 0.0, out.ctypes.data_as(fp)) == -1, name
        assert b"NULL" in lib.rt_last_error(None)
        assert getattr(lib, name + "_device")(None, None, None, 16, 0.0, None, None) == -1, name
    assert not out.any() and not buf.any()


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
    aov = c.render_aov_surface(p, 8)
    assert aov.shape == (3, 5, 7, 4) and aov.dtype == np.float32
    rows, idx = rt.interleaved_rows(5, 2, 1, 2)
    assert c.render_aov_surface(p, 3, pose=rt.make_pose(), rows=rows).shape == (3, len(idx), 7, 4)
    c.render_aov_surface_device(p, 2, 0x1000)
    color = np.zeros((5, 7, 4))
    out = c.demodulate(color, aov)
    assert out.shape == (5, 7, 4) and out.dtype == np.float32
    out = c.modulate(color, aov, albedo_floor=1e-3)
    assert out.shape == (5, 7, 4) and out.dtype == np.float32
    c.demodulate_device(0x1000, 0x2000, 35, 0x1000, albedo_floor=0.5)
    c.modulate_device(0x1000, 0x2000, 35, 0x3000)
    names = [n for n, _ in c._L.calls]
    assert names == ["rt_render_aov_surface", "rt_render_aov_surface", "rt_render_aov_surface_device", "rt_demodulate", "rt_modulate", "rt_demodulate_device",
                     "rt_modulate_device"]
    a = c._L.calls[0][1]                                                        # (ctx, params, pose, rows, max_specular, out)
    assert a[2] is None and a[3] is None and a[4] == 8
    a = c._L.calls[1][1]
    assert a[2] is not None and a[3]._obj.n_rows == len(idx) and a[4] == 3
    a = c._L.calls[2][1]                                                        # (ctx, params, pose, rows, max_specular, out, stream)
    assert a[3]._obj.n_rows == 5 and a[4] == 2 and a[5].value == 0x1000 and a[6] is None
    a = c._L.calls[3][1]                                                        # (ctx, color, aov, n_pixels, albedo_floor, out)
    assert a[3] == 35 and a[4] == 0.0
    a = c._L.calls[4][1]
    assert a[3] == 35 and a[4] == 1e-3
    a = c._L.calls[5][1]                                                        # (ctx, color, aov, n_pixels, albedo_floor, out, stream)
    assert (a[1].value, a[2].value, a[3], a[4], a[5].value) == (0x1000, 0x2000, 35, 0.5, 0x1000) and a[6] is None
    a = c._L.calls[6][1]
    assert (a[3], a[4], a[5].value) == (35, 0.0, 0x3000)
    # planes of another frame size never reach the library
    with pytest.raises(rt.RtError) as e:
        c.demodulate(color, np.zeros((3, 5, 8, 4), np.float32))
    assert e.value.code == -1 and len(c._L.calls) == 7
    with pytest.raises(rt.RtError):
        c.modulate(color, aov, out=np.zeros((5, 7, 4), np.float64))
    assert len(c._L.calls) == 7
    c._h = None


def test_decode_path_on_scalars_and_arrays():
    assert rt.Context.decode_path(5) == (5, 5, 0)
    assert rt.Context.decode_path(np.float32(3 + 16 * 7 + 256 * 2)) == (3, 7, 2)
    assert rt.Context.decode_path(-1.0) == (-1, -1, 0)
    i, f, k = rt.Context.decode_path(np.array([[4095.0, 0.0], [-1.0, 256.0 + 16.0]], np.float32))
    assert i.tolist() == [[15, 0], [-1, 0]] and f.tolist() == [[15, 0], [-1, 1]] and k.tolist() == [[15, 0], [0, 1]]


def test_renderer_members_compile(tmp_path):
    src = tmp_path / "surf.cpp"
    src.write_text("""
#include "raytracer.hpp"
using namespace raytracer;
std::vector<float> use(Renderer &r, const RenderSettings &s, const rt_camera_pose &pose) {
    std::vector<float> color = r.render_float(s);
    std::vector<float> aov = r.render_aov_surface(s, 8), posed = r.render_aov_surface(s, 4, &pose);
    rt_denoise_params dp{3, 2.0f, 0.25f, 0.0f, 5e-12f};
    std::vector<float> irr = r.demodulate(color, aov);
    return r.modulate(r.denoise(irr, aov, s.W, s.H, dp), aov, 1e-3f);
}
""")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
