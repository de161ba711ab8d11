"""Temporal accumulation and the variance-guided filter at the boundary, without a GPU: the library exports rt_temporal_accumulate[_device] and
rt_denoise_var[_device], the header declares them with the argument lists the ctypes binding uses, the structs have the sizes the header gives them, the ABI number did
not move, a NULL context is refused, the header states the history layout and the posed-camera caveat, the Python helpers build the motion records the header
describes, and the C++ Renderer members compile."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_temporal_accumulate_device", "rt_temporal_accumulate", "rt_denoise_var_device", "rt_denoise_var")


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


def test_struct_sizes_and_layout():
    hdr = _header()
    assert C.sizeof(_capi.TemporalParams) == 16
    assert C.sizeof(_capi.Motion) == 48
    assert C.sizeof(_capi.DenoiseVarParams) == 24
    assert C.sizeof(_capi.Reproject) == 56 and _capi.Reproject.motion.offset == 48 and _capi.Reproject.pose.offset == 20 and _capi.Reproject.no_history_mask.offset == 44
    assert _capi.MAX_OBJECTS == 16 and "#define RT_MAX_OBJECTS 16" in hdr
    for word in ("typedef struct rt_temporal_params", "typedef struct rt_motion", "typedef struct rt_reproject", "typedef struct rt_denoise_var_params", "int32_t max_history;"):
        assert word in hdr, word
    # the compiler agrees with ctypes
    src = ('#include "raytrace_hip.h"\n#include <stddef.h>\n'
           "_Static_assert(sizeof(rt_temporal_params) == 16 && sizeof(rt_motion) == 48 && sizeof(rt_denoise_var_params) == 24 && sizeof(rt_reproject) == 56, \"sizes\");\n"
           "_Static_assert(offsetof(rt_reproject, pose) == 20 && offsetof(rt_reproject, no_history_mask) == 44 && offsetof(rt_reproject, motion) == 48, \"offsets\");\n")
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), "-"], input=src.encode(), check=True)


def test_header_states_the_history_layout_and_the_posed_camera_caveat():
    hdr = _header()
    for word in ("history plane 0", "history plane 1", "(m1, m2, n, V)", "POSED CAMERA adds its", "INTO the ray direction", "FIRST valid one wins", "Nearest, not bilinear",
                 "D = k_sigma V_p + var_floor", "V_out = SV / (W W)"):
        assert word in hdr, word


def test_abi_version_is_still_6():
    assert _capi.load().rt_abi_version() == 6
    assert "#define RT_ABI_VERSION 6" in _header()


def test_null_context_is_refused():
    lib = _capi.load()
    fp = C.POINTER(C.c_float)
    aov = np.zeros((3, 4, 4, 4), np.float32)
    col = np.zeros((4, 4, 4), np.float32)
    hist = np.full((2, 4, 4, 4), -7, np.float32)
    out = np.full((4, 4, 4), -7, np.float32)
    tp, vp, rp = rt.make_temporal_params(), rt.make_denoise_var_params(), rt.make_reproject()
    assert lib.rt_temporal_accumulate(None, col.ctypes.data_as(fp), aov.ctypes.data_as(fp), None, None, 4, 4, C.byref(tp), C.byref(rp), hist.ctypes.data_as(fp)) == -1
    assert b"NULL" in lib.rt_last_error(None)
    assert lib.rt_temporal_accumulate_device(None, None, None, None, None, 4, 4, C.byref(tp), None, None, None) == -1
    assert lib.rt_denoise_var(None, hist.ctypes.data_as(fp), aov.ctypes.data_as(fp), 4, 4, C.byref(vp), out.ctypes.data_as(fp)) == -1
    assert b"NULL" in lib.rt_last_error(None)
    assert lib.rt_denoise_var_device(None, None, None, 4, 4, C.byref(vp), None, None) == -1
    assert (hist == -7).all() and (out == -7).all()


def test_default_parameters():
    t = rt.make_temporal_params()
    assert (t.max_history, t.alpha_min) == (32, 0.0) and t.min_normal_dot == np.float32(0.9) and t.max_plane_dist == 0.5
    assert rt.make_temporal_params(max_history=4, alpha_min=0.25).max_history == 4
    v = rt.make_denoise_var_params()
    d = _capi.DENOISE_VAR_DEFAULTS
    assert (v.n_passes, v.k_normal, v.k_position, v.k_albedo) == (d["n_passes"], 2.0, 0.25, 16.0) and v.k_sigma == np.float32(d["k_sigma"]) and v.var_floor == np.float32(d["var_floor"])
    assert rt.make_denoise_var_params(n_passes=5, var_floor=1.5).var_floor == 1.5


def test_motion_helpers():
    m = rt.static_motion()
    assert m.shape == (16, 12) and m.dtype == np.float32
    np.testing.assert_array_equal(m[3], [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])
    prev = [((0, 0, 0), 1.0, (1, 1, 1)), ((1.5, 2, 3), 2.0, (1, 1, 1))]
    cur = [((0, 0, 0), 1.0, (1, 1, 1)), ((2.5, 2, 1), 2.0, (1, 1, 1))]
    m = rt.motion_from_spheres(prev, cur)
    np.testing.assert_array_equal(m[1, 9:], [-1, 0, 2])              # previous centre - current centre
    np.testing.assert_array_equal(m[0], rt.static_motion()[0])
    with pytest.raises(rt.RtError):
        rt.motion_from_spheres(prev, cur[:1])
    # a mesh moved by v' = R v + T: the record takes v' back to v
    a = 0.3
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    T = np.array([1.0, -2.0, 0.5], np.float32)
    m = rt.motion_from_mesh_transform(R, T, 6, motion=m)
    np.testing.assert_array_equal(m[1, 9:], [-1, 0, 2])              # the table given is filled in, not replaced
    v = np.array([3.0, 4.0, -5.0])
    back = m[6, :9].reshape(3, 3).astype(np.float64) @ (R.astype(np.float64) @ v + T) + m[6, 9:]
    np.testing.assert_allclose(back, v, atol=1e-5)
    r = rt.make_reproject(motion=m, no_history_mask=0b101)
    assert r.posed == 0 and r.no_history_mask == 5 and r.camera.fov == np.float32(np.pi / 3) and list(r.camera.position) == [0.0, 0.0, 55.0]
    assert list(r.motion[6].translation) == list(m[6, 9:]) and list(r.motion[6].rotation) == list(m[6, :9])
    r = rt.make_reproject(pose=rt.make_pose(yaw=0.25))
    assert r.posed == 1 and r.pose.yaw == 0.25 and not r.motion
    with pytest.raises(rt.RtError):
        rt.make_reproject(motion=np.zeros((4, 12), np.float32))


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
    color, aov = np.zeros((5, 7, 4)), np.zeros((3, 5, 7, 4), np.float32)
    h1 = c.temporal_accumulate(color, aov)
    assert h1.shape == (2, 5, 7, 4) and h1.dtype == np.float32
    rp = rt.make_reproject(no_history_mask=2)
    c.temporal_accumulate(color, aov, aov, h1, reproject=rp, params=rt.make_temporal_params(max_history=8))
    c.temporal_accumulate_device(0x1000, 0x2000, 0, 0, 7, 5, 0x3000)
    out = c.denoise_var(h1, aov, n_passes=2, k_sigma=9.0)
    assert out.shape == (5, 7, 4) and out.dtype == np.float32
    c.denoise_var_device(0x1000, 0x2000, 7, 5, 0x3000, var_floor=0.5)
    assert [n for n, _ in c._L.calls] == ["rt_temporal_accumulate", "rt_temporal_accumulate", "rt_temporal_accumulate_device", "rt_denoise_var", "rt_denoise_var_device"]
    a = c._L.calls[0][1]                                                # (ctx, color, aov, prev_aov, prev_history, width, height, params, reproject, out)
    assert a[3] is None and a[4] is None and (a[5], a[6]) == (7, 5) and a[7]._obj.max_history == 32 and a[8] is None
    a = c._L.calls[1][1]
    assert a[3] is not None and a[4] is not None and a[7]._obj.max_history == 8 and a[8]._obj.no_history_mask == 2
    a = c._L.calls[2][1]                                                # (ctx, color, aov, prev_aov, prev_history, width, height, params, reproject, out, stream)
    assert (a[1].value, a[2].value, a[3], a[4], a[5], a[6], a[9].value, a[10]) == (0x1000, 0x2000, None, None, 7, 5, 0x3000, None)
    a = c._L.calls[3][1]                                                # (ctx, history, aov, width, height, params, out)
    assert (a[3], a[4]) == (7, 5) and a[5]._obj.n_passes == 2 and a[5]._obj.k_sigma == 9.0 and a[5]._obj.k_albedo == 16.0
    a = c._L.calls[4][1]
    assert (a[1].value, a[2].value, a[3], a[4], a[6].value) == (0x1000, 0x2000, 7, 5, 0x3000) and a[5]._obj.var_floor == 0.5
    # arrays of another frame size never reach the library
    for bad in (lambda: c.temporal_accumulate(color, np.zeros((3, 5, 8, 4), np.float32)), lambda: c.temporal_accumulate(color, aov, aov, h1[:1]),
                lambda: c.denoise_var(h1, np.zeros((3, 5, 8, 4), np.float32)), lambda: c.denoise_var(h1[0], aov)):
        with pytest.raises(rt.RtError) as e:
            bad()
        assert e.value.code == -1
    assert len(c._L.calls) == 5
    c._h = None


def test_renderer_members_compile(tmp_path):
    src = tmp_path / "tp.cpp"
    src.write_text("""
#include "raytracer.hpp"
using namespace raytracer;
std::vector<float> use(Renderer &r, const RenderSettings &s) {
    std::vector<float> color = r.render_float(s), aov = r.render_aov(s), none;
    rt_temporal_params tp{32, 0.f, 0.9f, 0.5f};
    std::vector<float> h1 = r.temporal_accumulate(color, aov, none, none, s.W, s.H, tp, nullptr);
    rt_motion motion[RT_MAX_OBJECTS] = {};
    rt_reproject rp{};
    rp.motion = motion;
    rp.no_history_mask = 1u << 3;
    std::vector<float> h2 = r.temporal_accumulate(color, aov, aov, h1, s.W, s.H, tp, &rp);
    rt_denoise_var_params vp{3, 2.0f, 0.25f, 16.0f, 4.0f, 0.f};
    return r.denoise_var(h2, aov, s.W, s.H, vp);
}
""")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
