"""Animated scenes at the boundary, without a GPU: the library exports rt_scene_get / set / move_*, rt_light_orbit and rt_render_device_batch_scenes and refuses a NULL
context, the structures have the sizes raytrace_hip.h gives them, the Python methods marshal slots, spheres, lights and the per-frame scene array, the C++ Renderer members
compile, and rt_light_orbit (the host function behind rt_scene_move_light) follows MoveLightSource's formula (realtime_render.cu:1072-1090)."""
import ctypes as C
import os
import subprocess

import numpy as np

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_scene_get_light", "rt_scene_set_light", "rt_scene_get_sphere", "rt_scene_set_sphere", "rt_scene_move_light", "rt_scene_move_sphere", "rt_light_orbit",
       "rt_render_device_batch_scenes")


def test_scene_edit_symbols_are_exported_and_declared():
    lib = _capi.load()
    hdr = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _capi.EXPORTS, n
        assert f"int {n}(" in hdr, n
    assert "#define RT_ABI_VERSION 6" in hdr and lib.rt_abi_version() == 6          # additive: the ABI number stays
    assert _capi.MAX_SPHERES == 16 and "#define RT_MAX_SPHERES 16" in hdr
    assert C.sizeof(_capi.SpherePose) == 16
    assert C.sizeof(_capi.FrameScene) == 16 + 16 * _capi.MAX_SPHERES


def test_null_context_is_refused():
    lib = _capi.load()
    l, s = _capi.Light(), _capi.Sphere()
    v = (C.c_float * 3)(1, 0, 0)
    calls = [lambda: lib.rt_scene_get_light(None, C.byref(l)), lambda: lib.rt_scene_set_light(None, C.byref(l)),
             lambda: lib.rt_scene_get_sphere(None, 0, C.byref(s)), lambda: lib.rt_scene_set_sphere(None, 0, C.byref(s)),
             lambda: lib.rt_scene_move_light(None, C.c_float(1.0), C.c_float(0.02)), lambda: lib.rt_scene_move_sphere(None, 0, v, C.c_float(0.2))]
    p, rows = rt.make_params(64, 64), _capi.Rows(0, 64, 64, 1)
    fd, fs = (_capi.FrameDesc * 1)(), (_capi.FrameScene * 1)()
    calls.append(lambda: lib.rt_render_device_batch_scenes(None, C.byref(p), C.byref(rows), fd, fs, 0, 1, None))
    for f in calls:
        lib.rt_light_orbit(C.byref(l), C.c_float(0), C.c_float(0), C.byref(l))       # (a success in between: the message below is this call's own)
        assert f() == -1
        assert b"NULL" in lib.rt_last_error(None)
    assert lib.rt_light_orbit(None, C.c_float(1.0), C.c_float(0.02), C.byref(l)) == -1
    assert b"NULL" in lib.rt_last_error(None)


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


def test_python_marshals_the_edits():
    c = _fake_context()
    c.set_light((1.0, 2.0, 3.0), 2.5e10)
    c.set_sphere(4, ((1.5, -2.0, 3.25), 7.0, (0.25, 0.5, 0.75), 1, 1.5, 1.25))
    c.set_sphere(2, ((0, 0, 0), 3, (1, 1, 1)))                          # the short form scene_upload takes: diffuse, indices 1 / 1
    c.move_light(0.75)
    c.move_light(-2.0, dt=0.5)
    c.move_sphere(5, (1, 2, 3))
    c.move_sphere(1, np.float64([0.5, 0, -1]), dt=0.125)
    c.light()
    c.sphere(3)
    names = [n for n, _ in c._L.calls]
    assert names == ["rt_scene_set_light", "rt_scene_set_sphere", "rt_scene_set_sphere", "rt_scene_move_light", "rt_scene_move_light", "rt_scene_move_sphere",
                     "rt_scene_move_sphere", "rt_scene_get_light", "rt_scene_get_sphere"]
    l = c._L.calls[0][1][1]._obj
    assert list(l.position) == [1.0, 2.0, 3.0] and l.intensity == np.float32(2.5e10)
    _, a = c._L.calls[1]
    s = a[2]._obj
    assert a[1] == 4 and list(s.center) == [1.5, -2.0, 3.25] and s.radius == 7.0 and list(s.albedo) == [0.25, 0.5, 0.75]
    assert (s.mirror, s.in_refraction_index, s.out_refraction_index) == (1, 1.5, 1.25)
    _, a = c._L.calls[2]
    s = a[2]._obj
    assert a[1] == 2 and (s.mirror, s.in_refraction_index, s.out_refraction_index) == (0, 1.0, 1.0)
    assert [x.value for x in c._L.calls[3][1][1:]] == [0.75, np.float32(2e-2)]       # MoveLightSource's default dt
    assert [x.value for x in c._L.calls[4][1][1:]] == [-2.0, 0.5]
    _, a = c._L.calls[5]
    assert a[1] == 5 and np.ctypeslib.as_array(a[2], shape=(3,)).tolist() == [1.0, 2.0, 3.0] and a[3].value == np.float32(0.2)   # MoveObject's default dt
    _, a = c._L.calls[6]
    assert a[1] == 1 and np.ctypeslib.as_array(a[2], shape=(3,)).tolist() == [0.5, 0.0, -1.0] and a[3].value == 0.125
    assert c._L.calls[8][1][1] == 3
    c._h = None


def test_python_marshals_the_per_frame_scenes():
    c = _fake_context()
    p, rows = rt.make_params(64, 64), _capi.Rows(0, 64, 64, 1)
    frames = [(4096 * (k + 1), (0.5 * k, 0.0, 55.0), None, 100 + k) for k in range(3)]
    scenes = [(((-10.0 + k, 20.0, 40.0 - k), 3e10 + k * 1e9), [((k, 1.0, -1000.0), 940.0 + k), ((0.0, -1000.0 - k, 0.0), 990.0)]) for k in range(3)]
    c.render_device_batch(p, rows, frames)
    c.render_device_batch(p, rows, frames, scenes=scenes)
    (n0, a0), (n1, a1) = c._L.calls
    assert n0 == "rt_render_device_batch" and a0[4] == 3
    assert n1 == "rt_render_device_batch_scenes"                         # (ctx, params, rows, frames, scenes, n_spheres, n_frames, stream)
    assert a1[5] == 2 and a1[6] == 3 and a1[7] is None
    for k in range(3):
        assert a1[3][k].out_rgba_dev == 4096 * (k + 1) and a1[3][k].seed == 100 + k
        fs = a1[4][k]
        assert list(fs.light.position) == [-10.0 + k, 20.0, 40.0 - k] and fs.light.intensity == np.float32(3e10 + k * 1e9)
        assert list(fs.spheres[0].center) == [k, 1.0, -1000.0] and fs.spheres[0].radius == 940.0 + k
        assert list(fs.spheres[1].center) == [0.0, -1000.0 - k, 0.0] and fs.spheres[1].radius == 990.0
        assert fs.spheres[2].radius == 0.0
    for bad in (scenes[:2], [scenes[0], scenes[1], (scenes[2][0], scenes[2][1][:1])]):   # a frame without a scene; a frame that poses fewer spheres
        try:
            c.render_device_batch(p, rows, frames, scenes=bad)
        except ValueError:
            pass
        else:
            raise AssertionError("accepted")
    assert len(c._L.calls) == 2
    c._h = None


def test_renderer_scene_edit_members_compile(tmp_path):
    src = tmp_path / "edit.cpp"
    src.write_text("""
#include "raytracer.hpp"
using namespace raytracer;
void use(Renderer &r, Scene &scene, const Sphere &s) {
    r.set_light(Vector(1.f, 2.f, 3.f), 2e10f);
    r.set_light(scene.L, scene.intensity);
    r.set_sphere(s);
    r.move_light(0.5f);
    r.move_light(0.5f, 0.1f);
    r.move_object(s.id, Vector(1.f, 0.f, 0.f));
    r.move_object(3, Vector(1.f, 0.f, 0.f), 0.5f);
}
""")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_light_orbit_follows_the_reference_formula():
    """rt_light_orbit: y and the intensity come back bit for bit; x and z agree with MoveLightSource's formula evaluated in binary64 within 16 * 2^-24 * radius -- a handful of
    binary32 roundings of C-library functions good to an ulp, the angle's error scaled by the radius (a numpy float32 restatement stays within 6.3 of these units over 2e5
    lights of this range).  (Bit for bit against MoveLightSource itself: tests/test_realtime_pinned.py.)"""
    rng = np.random.default_rng(5)
    n = 20000
    pos = rng.uniform(-100, 100, (n, 3)).astype(np.float32)
    inten = rng.uniform(1e9, 5e10, n).astype(np.float32)
    speed = rng.uniform(-10, 10, n).astype(np.float32)
    dt = np.float32(0.02)
    lib = _capi.load()
    got = np.zeros((n, 4), np.float32)
    a, b = _capi.Light(), _capi.Light()
    for k in range(n):
        a.position[:] = pos[k].tolist()
        a.intensity = float(inten[k])
        assert lib.rt_light_orbit(C.byref(a), C.c_float(float(speed[k])), C.c_float(float(dt)), C.byref(b)) == 0
        got[k] = (*b.position, b.intensity)
    np.testing.assert_array_equal(got[:, 1].view(np.uint32), pos[:, 1].view(np.uint32))
    np.testing.assert_array_equal(got[:, 3].view(np.uint32), inten.view(np.uint32))
    x, z = pos[:, 0].astype(np.float64), pos[:, 2].astype(np.float64)
    radius = np.sqrt(x * x + z * z)
    ang = np.arctan2(z, x) + speed.astype(np.float64) * np.float64(dt)
    err = np.maximum(np.abs(got[:, 0] - radius * np.cos(ang)), np.abs(got[:, 2] - radius * np.sin(ang))) / (2.0 ** -24 * radius)
    print(f"rt_light_orbit: max error {err.max():.2f} units of 2^-24 * radius over {n} lights")
    assert err.max() <= 16.0
    # in place, and the package's wrapper
    assert lib.rt_light_orbit(C.byref(a), C.c_float(float(speed[-1])), C.c_float(float(dt)), C.byref(a)) == 0
    assert list(a.position) == list(b.position)
    p2, i2 = rt.light_orbit((tuple(float(v) for v in pos[-1]), float(inten[-1])), float(speed[-1]), float(dt))
    assert list(np.float32(p2)) == list(b.position) and np.float32(i2) == b.intensity
    # a quarter turn of a light on the x axis
    (x1, y1, z1), _ = rt.light_orbit(((10.0, 5.0, 0.0), 1.0), np.pi / 2, 1.0)
    assert y1 == 5.0 and abs(x1) < 1e-5 and abs(z1 - 10.0) < 1e-5
