"""Several point lights at the boundary, without a GPU: the library exports rt_scene_set_lights / get_lights / set_light_at / move_light_at, the header declares them
and the package binds them; a NULL context is refused; the Python methods marshal the list, the index and MoveLightSource's default dt; the C++ Renderer members compile."""
import ctypes as C
import os
import subprocess

import numpy as np

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_scene_set_lights", "rt_scene_get_lights", "rt_scene_set_light_at", "rt_scene_move_light_at")


def test_lights_symbols_are_exported_declared_and_bound():
    lib = _capi.load()
    hdr = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _capi.EXPORTS, n
        assert f"int {n}(" in hdr, n
        assert getattr(lib, n).argtypes is not None, n
    assert "#define RT_ABI_VERSION 6" in hdr and lib.rt_abi_version() == 6          # additive: the ABI number stays
    assert _capi.MAX_LIGHTS == 16 and "#define RT_MAX_LIGHTS 16" in hdr
    assert C.sizeof(_capi.Light) == 16
    for m in ("set_lights", "lights", "set_light_at", "move_light_at"):
        assert callable(getattr(rt.Context, m)), m


def test_null_context_is_refused():
    lib = _capi.load()
    arr, l, n = (_capi.Light * 3)(), _capi.Light(), C.c_int(-7)
    calls = [lambda: lib.rt_scene_set_lights(None, arr, 3), lambda: lib.rt_scene_get_lights(None, arr, 3, C.byref(n)),
             lambda: lib.rt_scene_set_light_at(None, 0, C.byref(l)), lambda: lib.rt_scene_move_light_at(None, 0, C.c_float(1.0), C.c_float(0.02))]
    for f in calls:
        lib.rt_light_orbit(C.byref(l), C.c_float(0), C.c_float(0), C.byref(l))       # (a success in between: the message below is this call's own)
        assert f() == -1
        assert b"NULL" in lib.rt_last_error(None)
    assert n.value == -7                                                             # a refused get writes nothing


class _Recorder:
    """stands in for the loaded library: records every call with its arguments"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name == "rt_scene_get_lights":                                        # answers a list of two
                args[1][0].position[:] = (1.0, 2.0, 3.0)
                args[1][0].intensity = 4.0
                args[1][1].position[:] = (-1.0, -2.0, -3.0)
                args[1][1].intensity = 0.5
                args[3]._obj.value = 2
            return 0
        return fn


def _fake_context():
    c = rt.Context.__new__(rt.Context)
    c._L = _Recorder()
    c._h = C.c_void_p()
    return c


def test_python_routes_and_marshals_the_list():
    c = _fake_context()
    c.set_lights([((1.0, 2.0, 3.0), 2.5e10), ((-4.0, 5.0, 6.5), 0.0), ((7.0, 8.0, 9.0), 1e9)])
    c.set_lights([((0.5, 0.25, 0.125), 3.0)])
    c.set_light_at(2, (1.5, -2.0, 3.25), 7.0)
    c.move_light_at(1, 0.75)
    c.move_light_at(3, -2.0, dt=0.5)
    got = c.lights()
    names = [n for n, _ in c._L.calls]
    assert names == ["rt_scene_set_lights", "rt_scene_set_lights", "rt_scene_set_light_at", "rt_scene_move_light_at", "rt_scene_move_light_at", "rt_scene_get_lights"]
    _, a = c._L.calls[0]
    assert a[2] == 3
    assert [list(a[1][k].position) for k in range(3)] == [[1.0, 2.0, 3.0], [-4.0, 5.0, 6.5], [7.0, 8.0, 9.0]]
    assert [a[1][k].intensity for k in range(3)] == [np.float32(2.5e10), 0.0, np.float32(1e9)]
    _, a = c._L.calls[1]
    assert a[2] == 1 and list(a[1][0].position) == [0.5, 0.25, 0.125] and a[1][0].intensity == 3.0
    _, a = c._L.calls[2]
    l = a[2]._obj
    assert a[1] == 2 and list(l.position) == [1.5, -2.0, 3.25] and l.intensity == 7.0
    _, a = c._L.calls[3]
    assert a[1] == 1 and [x.value for x in a[2:]] == [0.75, np.float32(2e-2)]        # MoveLightSource's default dt
    _, a = c._L.calls[4]
    assert a[1] == 3 and [x.value for x in a[2:]] == [-2.0, 0.5]
    _, a = c._L.calls[5]
    assert a[2] == _capi.MAX_LIGHTS
    assert got == [((1.0, 2.0, 3.0), 4.0), ((-1.0, -2.0, -3.0), 0.5)]
    c._h = None


def test_renderer_lights_members_compile(tmp_path):
    src = tmp_path / "lights.cpp"
    src.write_text("""
#include "raytracer.hpp"
using namespace raytracer;
void use(Renderer &r, Scene &scene) {
    std::vector<rt_light> l{{{1.f, 2.f, 3.f}, 2e10f}, {{scene.L[0], scene.L[1], scene.L[2]}, scene.intensity}};
    r.set_lights(l);
    std::vector<rt_light> back = r.lights();
    r.set_light_at(1, Vector(1.f, 2.f, 3.f), back[0].intensity);
    r.set_light_at(0, scene.L, scene.intensity);
    r.move_light_at(1, 0.5f);
    r.move_light_at(0, 0.5f, 0.1f);
    static_assert(RT_MAX_LIGHTS == 16, "");
}
""")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
