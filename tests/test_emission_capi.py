"""Emissive meshes at the boundary, without a GPU: the library exports the six entries, the header declares them and the package binds them alike; a NULL context is
refused and a refused call writes nothing; the Python methods marshal; the C++ Renderer members compile.  What needs a context needs a device: tests/test_gpu_emission.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_scene_set_emission", "rt_scene_get_emission", "rt_scene_set_emission_sampling", "rt_scene_get_emission_sampling", "rt_kat_emission_table",
       "rt_kat_emission_sample")
FP, UP = C.POINTER(C.c_float), C.POINTER(C.c_uint32)


def test_emission_symbols_are_exported_declared_and_bound():
    lib = _capi.load()
    hdr = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _capi.EXPORTS, n
        assert f"int {n}(" in hdr, n
        assert getattr(lib, n).argtypes is not None, n
    assert "int rt_scene_set_emission(rt_ctx *ctx, int object_slot, const float rgb[3]);" in hdr
    assert "int rt_scene_get_emission(const rt_ctx *ctx, int object_slot, float rgb[3]);" in hdr
    assert "int rt_scene_set_emission_sampling(rt_ctx *ctx, float share);" in hdr
    assert "int rt_scene_get_emission_sampling(const rt_ctx *ctx, float *share);" in hdr
    assert "int rt_kat_emission_table(rt_ctx *ctx, uint32_t *c_out, uint64_t *prefix_out, uint64_t *total, int32_t *n_triangles);" in hdr
    assert "int rt_kat_emission_sample(rt_ctx *ctx, int count, const uint32_t *hs, const int32_t *seg, uint32_t *tri_out, float *point_out);" in hdr
    assert lib.rt_scene_set_emission.argtypes[1:] == [C.c_int, FP] and lib.rt_scene_get_emission.argtypes[1:] == [C.c_int, FP]
    assert lib.rt_scene_set_emission_sampling.argtypes[1:] == [C.c_float] and lib.rt_scene_get_emission_sampling.argtypes[1:] == [FP]
    assert lib.rt_kat_emission_table.argtypes[1:] == [UP, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
    assert lib.rt_kat_emission_sample.argtypes[1:] == [C.c_int, UP, C.POINTER(C.c_int32), UP, FP]
    assert "#define RT_ABI_VERSION 6" in hdr and lib.rt_abi_version() == 6          # additive: the ABI number stays
    assert "EMISSIVE MESHES" in hdr
    for m in ("set_emission", "emission", "set_emission_sampling", "emission_sampling", "kat_emission_table", "kat_emission_sample"):
        assert callable(getattr(rt.Context, m)), m


def test_null_context_is_refused():
    lib = _capi.load()
    l = _capi.Light()
    share = C.c_float(-7.0)
    total, nt = C.c_uint64(7), C.c_int32(7)
    c = (C.c_uint32 * 1)(7)
    p = (C.c_uint64 * 1)(7)
    hs, seg = (C.c_uint32 * 1)(1), (C.c_int32 * 1)(0)
    rgb, q = (C.c_float * 3)(-7.0, -7.0, -7.0), (C.c_float * 3)(-7.0, -7.0, -7.0)
    for call in (lambda: lib.rt_scene_set_emission(None, 0, rgb), lambda: lib.rt_scene_get_emission(None, 0, rgb),
                 lambda: lib.rt_scene_set_emission_sampling(None, C.c_float(0.5)), lambda: lib.rt_scene_get_emission_sampling(None, C.byref(share)),
                 lambda: lib.rt_kat_emission_table(None, c, p, C.byref(total), C.byref(nt)), lambda: lib.rt_kat_emission_sample(None, 1, hs, seg, c, q)):
        lib.rt_light_orbit(C.byref(l), C.c_float(0), C.c_float(0), C.byref(l))       # (a success in between: the message below is this call's own)
        assert call() == -1
        assert b"NULL" in lib.rt_last_error(None)
    assert share.value == -7.0 and total.value == 7 and nt.value == 7 and c[0] == 7 and p[0] == 7 and list(rgb) == [-7.0] * 3 and list(q) == [-7.0] * 3


class _Recorder:
    """stands in for the loaded library: records every call with its arguments"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name == "rt_scene_get_emission":
                args[2][0], args[2][1], args[2][2] = 1.0, 2.0, 3.0
            if name == "rt_scene_get_emission_sampling":
                args[1]._obj.value = 0.25
            if name == "rt_kat_emission_table":
                args[3]._obj.value = 1 << 40
                args[4]._obj.value = 4
                if args[1] is not None:
                    for k in range(4):
                        args[1][k], args[2][k] = k + 1, 10 * (k + 1)
            if name == "rt_kat_emission_sample":
                for k in range(args[1]):
                    args[4][k] = args[2][k] + args[3][k]
                    args[5][3 * k + 2] = 1.0
            return 0
        return fn


def test_python_routes_and_marshals_the_emission_calls():
    c = rt.Context.__new__(rt.Context)
    c._L, c._h = _Recorder(), C.c_void_p()
    c.set_emission(3, np.array([0.5, 1.5, 2.5]))
    assert c.emission(3) == (1.0, 2.0, 3.0)
    c.set_emission_sampling(0.75)
    assert c.emission_sampling() == 0.25
    cc, prefix, total = c.kat_emission_table()
    tri, point = c.kat_emission_sample(np.array([5, 6, 7], np.int64), 2)             # (any integer type; one segment for all)
    t2, _ = c.kat_emission_sample([1, 2], [3, 4])
    names = [n for n, _ in c._L.calls]
    assert names == ["rt_scene_set_emission", "rt_scene_get_emission", "rt_scene_set_emission_sampling", "rt_scene_get_emission_sampling", "rt_kat_emission_table",
                     "rt_kat_emission_table", "rt_kat_emission_sample", "rt_kat_emission_sample"]
    assert c._L.calls[0][1][1] == 3 and list(c._L.calls[0][1][2]) == [0.5, 1.5, 2.5]
    assert c._L.calls[1][1][1] == 3
    assert c._L.calls[2][1][1].value == 0.75
    assert c._L.calls[4][1][1] is None and c._L.calls[4][1][2] is None              # the count alone
    assert cc.dtype == np.uint32 and cc.tolist() == [1, 2, 3, 4] and prefix.dtype == np.uint64 and prefix.tolist() == [10, 20, 30, 40] and total == 1 << 40
    assert c._L.calls[6][1][1] == 3
    assert tri.dtype == np.uint32 and tri.tolist() == [7, 8, 9] and point.shape == (3, 3) and point[:, 2].tolist() == [1.0] * 3
    assert t2.tolist() == [4, 6]
    c._h = None


def test_the_panel_helper_is_a_two_triangle_mesh():
    v, t = rt.scenes.panel((1, 2, 3), (4, 0, 0), (0, 0, 2))
    assert v.dtype == np.float32 and t.dtype == np.int32 and v.shape == (4, 3) and t.tolist() == [[0, 1, 2], [0, 2, 3]]
    assert v.tolist() == [[1, 2, 3], [5, 2, 3], [5, 2, 5], [1, 2, 5]]
    area = sum(np.linalg.norm(np.cross(v[b] - v[a], v[c] - v[a])) / 2 for a, b, c in t)
    assert area == 8.0


def test_renderer_emission_members_compile(tmp_path):
    src = tmp_path / "emission.cpp"
    src.write_text("""
#include "raytracer.hpp"
using namespace raytracer;
float use(Renderer &r) {
    r.set_emission(3, Vector(1.f, 2.f, 3.f));
    r.set_emission_sampling(0.5f);
    return r.emission(3)[0] + r.emission_sampling();
}
""")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
