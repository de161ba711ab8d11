"""The shutter at the boundary, without a GPU: the library exports rt_scene_set_shutter / rt_scene_get_shutter, the header declares them and the package binds them alike;
a NULL context is refused and a refused get writes nothing; the Python methods marshal the motion; the C++ Renderer members compile.  What needs a context -- get after
set, an upload that closes the shutter, every refused value leaving the state as it was -- needs a device: tests/test_gpu_shutter.py."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_scene_set_shutter", "rt_scene_get_shutter")


def test_shutter_symbols_are_exported_declared_and_bound():
    lib = _capi.load()
    hdr = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _capi.EXPORTS, n
        assert f"int {n}(" in hdr, n
        assert getattr(lib, n).argtypes is not None, n
    assert "typedef struct { float light[3]; float object[RT_MAX_OBJECTS][3]; } rt_shutter;" in hdr
    assert "int rt_scene_set_shutter(rt_ctx *ctx, const rt_shutter *shutter);" in hdr
    assert "int rt_scene_get_shutter(const rt_ctx *ctx, rt_shutter *out);" in hdr
    assert lib.rt_scene_set_shutter.argtypes[1:] == [C.POINTER(_capi.Shutter)] and lib.rt_scene_get_shutter.argtypes[1:] == [C.POINTER(_capi.Shutter)]
    assert C.sizeof(_capi.Shutter) == 4 * 3 * (1 + _capi.MAX_OBJECTS) and _capi.Shutter.object.offset == 12 and "#define RT_MAX_OBJECTS 16" in hdr
    assert "#define RT_ABI_VERSION 6" in hdr and lib.rt_abi_version() == 6          # additive: the ABI number stays
    assert "SHUTTER" in hdr
    for m in ("set_shutter", "shutter"):
        assert callable(getattr(rt.Context, m)), m


def test_static_counts_name_the_four_kernels():
    keys = json.load(open(os.path.join(ROOT, "raytracinggpu_amd", "static_counts.json")))
    for k in ("wf_advance_shutter_first", "wf_advance_lens_shutter_first", "wf_advance_shutter", "wf_advance_tex_shutter"):
        assert keys[k]["whole_kernel"]["valu"] > 0, k


def test_null_context_is_refused():
    lib = _capi.load()
    s, l = _capi.Shutter(), _capi.Light()
    C.memset(C.byref(s), 7, C.sizeof(s))
    one = _capi.Shutter()
    one.light[0] = 1.0
    for call in (lambda: lib.rt_scene_set_shutter(None, C.byref(one)), lambda: lib.rt_scene_set_shutter(None, None), lambda: lib.rt_scene_get_shutter(None, C.byref(s))):
        lib.rt_light_orbit(C.byref(l), C.c_float(0), C.c_float(0), C.byref(l))       # (a success in between: the message below is this call's own)
        assert call() == -1
        assert b"NULL" in lib.rt_last_error(None)
    assert bytes(s) == b"\x07" * C.sizeof(s)                                         # a refused get writes nothing


class _Recorder:
    """stands in for the loaded library: records every call with its arguments"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name == "rt_scene_get_shutter":
                out = args[1]._obj
                out.light[:] = [1.0, 2.0, 3.0]
                out.object[5][:] = [0.5, 0.25, -1.0]
            return 0
        return fn


def test_python_routes_and_marshals_the_shutter():
    c = rt.Context.__new__(rt.Context)
    c._L, c._h = _Recorder(), C.c_void_p()
    c.set_shutter(light=(1.5, 0, -2), objects={2: (4, 0, 0), 15: (0, 0.5, 0)})
    c.set_shutter(objects={0: (1, 1, 1)})
    c.set_shutter()
    light, objs = c.shutter()
    assert [n for n, _ in c._L.calls] == ["rt_scene_set_shutter"] * 3 + ["rt_scene_get_shutter"]
    s = c._L.calls[0][1][1]._obj
    assert isinstance(s, _capi.Shutter) and list(s.light) == [1.5, 0.0, -2.0]
    assert [list(o) for o in s.object] == [[4.0, 0.0, 0.0] if k == 2 else [0.0, 0.5, 0.0] if k == 15 else [0.0, 0.0, 0.0] for k in range(16)]
    s = c._L.calls[1][1][1]._obj
    assert list(s.light) == [0.0, 0.0, 0.0] and list(s.object[0]) == [1.0, 1.0, 1.0]
    assert c._L.calls[2][1][1] is None                                               # no motion at all: NULL, the shutter is closed
    assert light.dtype == np.float32 and light.tolist() == [1.0, 2.0, 3.0]
    assert objs.shape == (16, 3) and objs[5].tolist() == [0.5, 0.25, -1.0] and not objs[:5].any() and not objs[6:].any()
    c._h = None


def test_renderer_shutter_members_compile(tmp_path):
    src = tmp_path / "shutter.cpp"
    src.write_text("""
#include "raytracer.hpp"
using namespace raytracer;
void use(Renderer &r) {
    rt_shutter m = {};
    m.light[0] = 1.5f;
    m.object[2][0] = 4.f;
    r.set_shutter(m);
    rt_shutter back = r.shutter();
    r.close_shutter();
    (void)back;
}
""")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
