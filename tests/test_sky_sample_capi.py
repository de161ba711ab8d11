"""Sky sampling at the boundary, without a GPU: the library exports the four entries, the header declares them and the package binds them alike; a NULL context is
refused and a refused call writes nothing; the Python methods marshal; the C++ Renderer members compile.  What needs a context needs a device: tests/test_gpu_sky_sample.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_scene_set_environment_sampling", "rt_scene_get_environment_sampling", "rt_kat_environment_table", "rt_kat_environment_sample")
FP, UP = C.POINTER(C.c_float), C.POINTER(C.c_uint32)


def test_sampling_symbols_are_exported_declared_and_bound():
    lib = _capi.load()
    hdr = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _capi.EXPORTS, n
        assert f"int {n}(" in hdr, n
        assert getattr(lib, n).argtypes is not None, n
    assert "int rt_scene_set_environment_sampling(rt_ctx *ctx, float share);" in hdr
    assert "int rt_scene_get_environment_sampling(const rt_ctx *ctx, float *share);" in hdr
    assert "int rt_kat_environment_table(rt_ctx *ctx, uint32_t *c_out, uint64_t *prefix_out, uint64_t *total);" in hdr
    assert "int rt_kat_environment_sample(rt_ctx *ctx, int count, const uint32_t *hs, const int32_t *seg, uint32_t *texel_out, float *dir_out, float *g_out);" in hdr
    assert lib.rt_scene_set_environment_sampling.argtypes[1:] == [C.c_float] and lib.rt_scene_get_environment_sampling.argtypes[1:] == [FP]
    assert lib.rt_kat_environment_table.argtypes[1:] == [UP, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    assert lib.rt_kat_environment_sample.argtypes[1:] == [C.c_int, UP, C.POINTER(C.c_int32), UP, FP, FP]
    assert "#define RT_ABI_VERSION 6" in hdr and lib.rt_abi_version() == 6          # additive: the ABI number stays
    assert "SKY SAMPLING" in hdr
    for m in ("set_environment_sampling", "environment_sampling", "kat_environment_table", "kat_environment_sample"):
        assert callable(getattr(rt.Context, m)), m
    assert callable(rt.environment.add_sun) and callable(rt.environment.texel_solid_angles)


def test_null_context_is_refused():
    lib = _capi.load()
    l = _capi.Light()
    share = C.c_float(-7.0)
    total = C.c_uint64(7)
    c = (C.c_uint32 * 1)(7)
    p = (C.c_uint64 * 1)(7)
    hs, seg = (C.c_uint32 * 1)(1), (C.c_int32 * 1)(0)
    d, g = (C.c_float * 3)(-7.0, -7.0, -7.0), (C.c_float * 1)(-7.0)
    for call in (lambda: lib.rt_scene_set_environment_sampling(None, C.c_float(0.5)), lambda: lib.rt_scene_get_environment_sampling(None, C.byref(share)),
                 lambda: lib.rt_kat_environment_table(None, c, p, C.byref(total)), lambda: lib.rt_kat_environment_sample(None, 1, hs, seg, c, d, g)):
        lib.rt_light_orbit(C.byref(l), C.c_float(0), C.c_float(0), C.byref(l))       # (a success in between: the message below is this call's own)
        assert call() == -1
        assert b"NULL" in lib.rt_last_error(None)
    assert share.value == -7.0 and total.value == 7 and c[0] == 7 and p[0] == 7 and list(d) == [-7.0] * 3 and g[0] == -7.0


class _Recorder:
    """stands in for the loaded library: records every call with its arguments"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name == "rt_scene_get_environment_sampling":
                args[1]._obj.value = 0.25
            if name == "rt_scene_get_environment":
                args[1]._obj.value = 2
            if name == "rt_kat_environment_table":
                for k in range(4):
                    args[1][k], args[2][k] = k + 1, 10 * (k + 1)
                args[3]._obj.value = 1 << 40
            if name == "rt_kat_environment_sample":
                for k in range(args[1]):
                    args[4][k] = args[2][k] + args[3][k]
                    args[5][3 * k + 2] = 1.0
                    args[6][k] = 2.0
            return 0
        return fn


def test_python_routes_and_marshals_the_sampling_calls():
    c = rt.Context.__new__(rt.Context)
    c._L, c._h = _Recorder(), C.c_void_p()
    c.set_environment_sampling(0.5)
    assert c.environment_sampling() == 0.25
    cc, prefix, total = c.kat_environment_table()
    texel, dirs, g = c.kat_environment_sample(np.array([5, 6, 7], np.int64), 2)       # (any integer type; one segment for all)
    t2, _, _ = c.kat_environment_sample([1, 2], [3, 4])
    names = [n for n, _ in c._L.calls]
    assert names == ["rt_scene_set_environment_sampling", "rt_scene_get_environment_sampling", "rt_scene_get_environment", "rt_kat_environment_table",
                     "rt_kat_environment_sample", "rt_kat_environment_sample"]
    assert c._L.calls[0][1][1].value == 0.5
    assert c._L.calls[2][1][2] is None                                               # the size alone
    assert cc.dtype == np.uint32 and cc.tolist() == [1, 2, 3, 4] and prefix.dtype == np.uint64 and prefix.tolist() == [10, 20, 30, 40] and total == 1 << 40
    assert c._L.calls[4][1][1] == 3
    assert texel.dtype == np.uint32 and texel.tolist() == [7, 8, 9] and dirs.shape == (3, 3) and dirs[:, 2].tolist() == [1.0] * 3 and g.tolist() == [2.0] * 3
    assert t2.tolist() == [4, 6]
    c._h = None


def test_renderer_sampling_members_compile(tmp_path):
    src = tmp_path / "sky_sample.cpp"
    src.write_text("""
#include "raytracer.hpp"
using namespace raytracer;
float use(Renderer &r) {
    r.set_environment_sampling(0.5f);
    return r.environment_sampling();
}
""")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
