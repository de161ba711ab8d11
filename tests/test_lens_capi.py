"""The thin lens at the boundary, without a GPU: the library exports rt_camera_set_lens / rt_camera_get_lens, the header declares them and the package binds them; a NULL
context is refused and a refused get writes nothing; the Python methods marshal radius and focus; the C++ Renderer members compile.  What needs a context -- get after set,
an upload that leaves a pinhole, every refused value leaving the lens as it was -- needs a device: tests/test_gpu_lens.py."""
import ctypes as C
import os
import subprocess

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_camera_set_lens", "rt_camera_get_lens")


def test_lens_symbols_are_exported_declared_and_bound():
    lib = _capi.load()
    hdr = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _capi.EXPORTS, n
        assert f"int {n}(" in hdr, n
        assert getattr(lib, n).argtypes is not None, n
    assert "int rt_camera_set_lens(rt_ctx *ctx, float aperture_radius, float focus_distance);" in hdr
    assert "int rt_camera_get_lens(const rt_ctx *ctx, float *aperture_radius, float *focus_distance);" in hdr
    assert len(lib.rt_camera_set_lens.argtypes) == 3 and lib.rt_camera_set_lens.argtypes[1:] == [C.c_float, C.c_float]
    assert len(lib.rt_camera_get_lens.argtypes) == 3 and lib.rt_camera_get_lens.argtypes[1:] == [C.POINTER(C.c_float)] * 2
    assert "#define RT_ABI_VERSION 6" in hdr and lib.rt_abi_version() == 6          # additive: the ABI number stays
    assert "THIN LENS" in hdr
    for m in ("set_lens", "lens"):
        assert callable(getattr(rt.Context, m)), m


def test_null_context_is_refused():
    lib = _capi.load()
    r, f, l = C.c_float(-7.0), C.c_float(-7.0), _capi.Light()
    for call in (lambda: lib.rt_camera_set_lens(None, C.c_float(1.0), C.c_float(30.0)), lambda: lib.rt_camera_get_lens(None, C.byref(r), C.byref(f))):
        lib.rt_light_orbit(C.byref(l), C.c_float(0), C.c_float(0), C.byref(l))       # (a success in between: the message below is this call's own)
        assert call() == -1
        assert b"NULL" in lib.rt_last_error(None)
    assert (r.value, f.value) == (-7.0, -7.0)                                        # a refused get writes nothing


class _Recorder:
    """stands in for the loaded library: records every call with its arguments"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name == "rt_camera_get_lens":
                args[1]._obj.value, args[2]._obj.value = 2.5, 40.0
            return 0
        return fn


def test_python_routes_and_marshals_the_lens():
    c = rt.Context.__new__(rt.Context)
    c._L, c._h = _Recorder(), C.c_void_p()
    c.set_lens(1.5, 45)
    got = c.lens()
    assert [n for n, _ in c._L.calls] == ["rt_camera_set_lens", "rt_camera_get_lens"]
    _, a = c._L.calls[0]
    assert isinstance(a[1], C.c_float) and isinstance(a[2], C.c_float) and (a[1].value, a[2].value) == (1.5, 45.0)
    assert got == (2.5, 40.0)
    c._h = None


def test_renderer_lens_members_compile(tmp_path):
    src = tmp_path / "lens.cpp"
    src.write_text("""
#include "raytracer.hpp"
using namespace raytracer;
void use(Renderer &r) {
    r.set_lens(1.5f, 45.f);
    std::pair<float, float> back = r.lens();
    r.set_lens(0.f, back.second);
}
""")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
