"""The environment at the boundary, without a GPU: the library exports rt_scene_set_environment / rt_scene_get_environment / rt_kat_environment, the header declares
them and the package binds them alike; a NULL context is refused and a refused get writes nothing; the Python methods marshal the map; the C++ Renderer members compile.
What needs a context -- get after set, an upload that removes the map, every refused map leaving the state as it was -- needs a device: tests/test_gpu_sky.py."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_scene_set_environment", "rt_scene_get_environment", "rt_kat_environment")
FP = C.POINTER(C.c_float)


def test_environment_symbols_are_exported_declared_and_bound():
    lib = _capi.load()
    hdr = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _capi.EXPORTS, n
        assert f"int {n}(" in hdr, n
        assert getattr(lib, n).argtypes is not None, n
    assert "int rt_scene_set_environment(rt_ctx *ctx, int n, const float *rgb);" in hdr
    assert "int rt_scene_get_environment(const rt_ctx *ctx, int *n, float *rgb);" in hdr
    assert "int rt_kat_environment(rt_ctx *ctx, int n_dirs, const float *dirs, float *rgb_out);" in hdr
    assert lib.rt_scene_set_environment.argtypes[1:] == [C.c_int, FP] and lib.rt_scene_get_environment.argtypes[1:] == [C.POINTER(C.c_int), FP]
    assert lib.rt_kat_environment.argtypes[1:] == [C.c_int, FP, FP]
    assert "#define RT_MAX_ENVIRONMENT 1024" in hdr and rt.environment.MAX_N == 1024
    assert "#define RT_ABI_VERSION 6" in hdr and lib.rt_abi_version() == 6          # additive: the ABI number stays
    assert "ENVIRONMENT" in hdr
    for m in ("set_environment", "environment", "kat_environment"):
        assert callable(getattr(rt.Context, m)), m


def test_static_counts_name_the_four_kernels():
    keys = json.load(open(os.path.join(ROOT, "raytracinggpu_amd", "static_counts.json")))
    for k in ("wf_advance_sky", "wf_advance_tex_sky", "wf_advance_soft_sky", "wf_advance_tex_soft_sky"):
        assert keys[k]["whole_kernel"]["valu"] > 0, k
    assert keys["wf_advance_sky"]["whole_kernel"]["valu"] > keys["wf_advance"]["whole_kernel"]["valu"]     # the lookup is in it


def test_null_context_is_refused():
    lib = _capi.load()
    l = _capi.Light()
    rgb = (C.c_float * 3)(7.0, 7.0, 7.0)
    n = C.c_int(-7)
    d = (C.c_float * 3)(0.0, 1.0, 0.0)
    out = (C.c_float * 3)(-7.0, -7.0, -7.0)
    for call in (lambda: lib.rt_scene_set_environment(None, 1, rgb), lambda: lib.rt_scene_set_environment(None, 0, None),
                 lambda: lib.rt_scene_get_environment(None, C.byref(n), rgb), lambda: lib.rt_kat_environment(None, 1, d, out)):
        lib.rt_light_orbit(C.byref(l), C.c_float(0), C.c_float(0), C.byref(l))       # (a success in between: the message below is this call's own)
        assert call() == -1
        assert b"NULL" in lib.rt_last_error(None)
    assert n.value == -7 and list(rgb) == [7.0] * 3 and list(out) == [-7.0] * 3      # a refused get writes nothing


class _Recorder:
    """stands in for the loaded library: records every call with its arguments"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name == "rt_scene_get_environment":
                args[1]._obj.value = 2
                if args[2] is not None:
                    for k in range(12):
                        args[2][k] = float(k)
            return 0
        return fn


def test_python_routes_and_marshals_the_environment():
    c = rt.Context.__new__(rt.Context)
    c._L, c._h = _Recorder(), C.c_void_p()
    env = np.arange(27, dtype=np.float64).reshape(3, 3, 3)                            # (not binary32, and it need not be contiguous)
    c.set_environment(env)
    c.set_environment(np.ones((1, 1, 3), np.float32)[:, :, ::-1])
    c.set_environment()
    back = c.environment()
    assert [n for n, _ in c._L.calls] == ["rt_scene_set_environment"] * 3 + ["rt_scene_get_environment"] * 2
    _, (h, n, p) = c._L.calls[0]
    assert n == 3 and [p[k] for k in range(27)] == [float(k) for k in range(27)]     # row 0 first, rgb innermost
    assert c._L.calls[1][1][1] == 1 and [c._L.calls[1][1][2][k] for k in range(3)] == [1.0] * 3
    assert c._L.calls[2][1][1:] == (0, None)                                         # no map: n = 0 and NULL
    assert c._L.calls[3][1][2] is None                                               # the size first
    assert back.dtype == np.float32 and back.shape == (2, 2, 3) and back.ravel().tolist() == [float(k) for k in range(12)]
    for bad in (np.zeros((2, 3, 3)), np.zeros((2, 2, 4)), np.zeros((4, 3))):
        with pytest.raises(ValueError):
            c.set_environment(bad)
    assert len(c._L.calls) == 5                                                      # nothing reached the library
    c._h = None


def test_renderer_environment_members_compile(tmp_path):
    src = tmp_path / "sky.cpp"
    src.write_text("""
#include "raytracer.hpp"
using namespace raytracer;
void use(Renderer &r) {
    std::vector<float> rgb(2 * 2 * 3, 0.5f);
    r.set_environment(2, rgb);
    r.set_environment(2, rgb.data());
    std::pair<int, std::vector<float>> back = r.environment();
    r.clear_environment();
    (void)back;
}
""")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
