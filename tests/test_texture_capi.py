"""Textured meshes at the boundary, without a GPU: the library exports rt_mesh_set_texture[_of] and rt_kat_surface and refuses a NULL context, the Python methods
marshal strides, slots, the texture record and the decode table, the C++ Renderer members compile, and the numpy model (tests/texture_model.py) that the GPU tests
hold the device to follows the rules of raytrace_hip.h."""
import ctypes as C
import os
import subprocess

import numpy as np

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi
from . import texture_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_mesh_set_texture", "rt_mesh_set_texture_of", "rt_kat_surface")


def test_texture_symbols_are_exported_and_declared():
    lib = _capi.load()
    hdr = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _capi.EXPORTS, n
        assert f"int {n}(rt_ctx *ctx" in hdr, n
    assert C.sizeof(_capi.Texture) == 40


def test_null_context_is_refused():
    lib = _capi.load()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    uv = np.zeros((3, 2), np.float32)
    ix = np.zeros((1, 3), np.int32)
    px = np.zeros((2, 2, 3), np.uint8)
    tex = _capi.Texture(px.ctypes.data_as(C.POINTER(C.c_uint8)), 2, 2, 3, 0, 0, None)
    assert lib.rt_mesh_set_texture(None, uv.ctypes.data_as(fp), 3, ix.ctypes.data_as(ip), 3, 1, C.byref(tex)) == -1
    assert b"NULL" in lib.rt_last_error(None)
    assert lib.rt_mesh_set_texture_of(None, 6, uv.ctypes.data_as(fp), 3, ix.ctypes.data_as(ip), 3, 1, C.byref(tex)) == -1
    assert b"NULL" in lib.rt_last_error(None)
    rays = np.zeros((1, 6), np.float32)
    out = np.zeros((1, 8), np.float32)
    assert lib.rt_kat_surface(None, rays.ctypes.data_as(fp), 1, C.c_float(1e-4), out.ctypes.data_as(fp)) == -1
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


def test_python_marshals_the_texture():
    c = _fake_context()
    uvs = np.arange(10, dtype=np.float64).reshape(5, 2)
    uvidx = np.array([[0, 1, 2], [2, 3, 4]])
    px = np.arange(2 * 3 * 4, dtype=np.uint8).reshape(2, 3, 4)
    dec = np.linspace(0, 2, 256).astype(np.float32)
    c.mesh_set_texture(uvs, uvidx, px)
    c.mesh_set_texture(uvs, uvidx, px, filter="bilinear", wrap="clamp", decode=dec, object_slot=3)
    c.mesh_set_texture(None, None, None, object_slot=7)
    c.mesh_set_texture(None, None, None)
    out = c.kat_surface(np.zeros((4, 6)), tri_tmin=0.0)
    assert out.shape == (4, 8) and out.dtype == np.float32
    names = [n for n, _ in c._L.calls]
    assert names == ["rt_mesh_set_texture", "rt_mesh_set_texture_of", "rt_mesh_set_texture_of", "rt_mesh_set_texture", "rt_kat_surface"]
    _, a = c._L.calls[0]                                                 # (ctx, uvs, n_uvs, uvidx, stride, n_triangles, &tex)
    assert a[2] == 5 and a[4] == 3 and a[5] == 2
    assert np.ctypeslib.as_array(a[1], shape=(10,)).tolist() == list(range(10))
    assert np.ctypeslib.as_array(a[3], shape=(6,)).tolist() == [0, 1, 2, 2, 3, 4]
    t = a[6]._obj
    assert (t.width, t.height, t.channels, t.filter, t.wrap) == (3, 2, 4, 0, 0) and not t.decode
    assert np.ctypeslib.as_array(t.texels, shape=(24,)).tolist() == list(range(24))
    _, a = c._L.calls[1]                                                 # (ctx, slot, uvs, n_uvs, uvidx, stride, n_triangles, &tex)
    assert a[1] == 3 and a[3] == 5 and a[5] == 3 and a[6] == 2
    t = a[7]._obj
    assert (t.filter, t.wrap) == (1, 1)
    np.testing.assert_array_equal(np.ctypeslib.as_array(t.decode, shape=(256,)), dec.astype(np.float32))
    _, a = c._L.calls[2]
    assert a[1] == 7 and a[2] is None and a[-1] is None                 # NULL: slot 7 untextured again
    _, a = c._L.calls[3]
    assert a[1] is None and a[-1] is None
    _, a = c._L.calls[4]
    assert a[2] == 4 and abs(a[3].value) == 0.0
    c._h = None


def test_renderer_texture_members_compile(tmp_path):
    src = tmp_path / "tex.cpp"
    src.write_text("""
#include "raytracer.hpp"
using namespace raytracer;
void use(Renderer &r, const TriangleMesh &m, const std::vector<uint8_t> &px, const float *dec) {
    r.use_texture(m, px.data(), 512, 1024, 4);
    r.use_texture(m, px.data(), 512, 1024, 4, RT_TEX_BILINEAR, RT_TEX_CLAMP, dec);
    r.use_texture_of(m, px.data(), 512, 1024, 3, RT_TEX_NEAREST, RT_TEX_REPEAT);
    r.use_untextured_of(m);
    r.use_untextured();
}
""")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def _img(w, h, ch, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, ch), dtype=np.uint8)


def test_model_nearest_wraps():
    px = _img(5, 3, 3)
    dec = tm.default_decode()
    # u = -0.1 -> x = floor(-0.5) = -1: repeat -> 4, clamp -> 0; v = 1.2 -> (1 - v) H = -0.6 -> y = -1: repeat -> 2, clamp -> 0
    for mode, x, y in ((tm.REPEAT, 4, 2), (tm.CLAMP, 0, 0)):
        got = tm.sample(px, dec, tm.NEAREST, mode, np.float32([-0.1]), np.float32([1.2]))
        np.testing.assert_array_equal(got[0], dec[px[y, x, :3]])
    # u = 2.5 -> x = 12: repeat -> 2, clamp -> 4; v = 0 -> y = 3 (one past the bottom row): repeat -> 0, clamp -> 2
    for mode, x, y in ((tm.REPEAT, 2, 0), (tm.CLAMP, 4, 2)):
        got = tm.sample(px, dec, tm.NEAREST, mode, np.float32([2.5]), np.float32([0.0]))
        np.testing.assert_array_equal(got[0], dec[px[y, x, :3]])
    # the top row is v just below 1, the first column u = 0; alpha is never read
    px4 = _img(5, 3, 4, seed=1)
    got = tm.sample(px4, dec, tm.NEAREST, tm.REPEAT, np.float32([0.0]), np.float32([0.99]))
    np.testing.assert_array_equal(got[0], dec[px4[0, 0, :3]])


def test_model_out_of_range_coordinates_sample_index_zero():
    px = _img(4, 4, 3, seed=2)
    dec = tm.default_decode()
    for u in (np.nan, np.inf, -np.inf, 3e9, -3e9):
        for mode in (tm.REPEAT, tm.CLAMP):
            got = tm.sample(px, dec, tm.NEAREST, mode, np.float32([u]), np.float32([0.9]))     # y = floor(0.4) = 0
            np.testing.assert_array_equal(got[0], dec[px[0, 0, :3]])
            got = tm.sample(px, dec, tm.BILINEAR, mode, np.float32([u]), np.float32([0.875]))  # t = 0.5 - 0.5 = 0: row 0 alone
            exp = (dec[px[0, 0, :3]] * np.float32(1) + dec[px[0, 1, :3]] * np.float32(0)) * np.float32(1) + \
                  (dec[px[1, 0, :3]] * np.float32(1) + dec[px[1, 1, :3]] * np.float32(0)) * np.float32(0)
            np.testing.assert_array_equal(got[0], exp)
    i, f = tm.tex_floor(np.float32([-2.0 ** 31, 2.0 ** 31, -0.0, 7.25, -7.25]))
    assert i.tolist() == [-2 ** 31, 0, 0, 7, -8] and f.tolist() == [0.0, 0.0, 0.0, 0.25, 0.75]


def test_model_bilinear_edges():
    px = _img(4, 2, 3, seed=3)
    dec = np.random.default_rng(4).random(256).astype(np.float32)
    # texel centres give that texel alone: u = (x + 0.5) / W, v = 1 - (y + 0.5) / H
    for x in range(4):
        for y in range(2):
            u, v = np.float32((x + 0.5) / 4), np.float32(1 - (y + 0.5) / 2)
            got = tm.sample(px, dec, tm.BILINEAR, tm.CLAMP, np.float32([u]), np.float32([v]))
            np.testing.assert_array_equal(got[0], dec[px[y, x, :3]])
    # between the last and the first column: repeat blends them, clamp keeps the last
    u, v = np.float32([1.0]), np.float32([0.75])                        # s = 3.5 -> x0 = 3, fx = 0.5; t = 0 -> row 0
    half = np.float32(0.5)
    rep = tm.sample(px, dec, tm.BILINEAR, tm.REPEAT, u, v)[0]
    np.testing.assert_array_equal(rep, ((dec[px[0, 3]] * half + dec[px[0, 0]] * half) * np.float32(1) + (dec[px[1, 3]] * half + dec[px[1, 0]] * half) * np.float32(0)))
    cl = tm.sample(px, dec, tm.BILINEAR, tm.CLAMP, u, v)[0]
    np.testing.assert_array_equal(cl, ((dec[px[0, 3]] * half + dec[px[0, 3]] * half) * np.float32(1) + (dec[px[1, 3]] * half + dec[px[1, 3]] * half) * np.float32(0)))
    # negative coordinates: s = -0.5 - 0.5 = -1 -> x0 = -1 (repeat: 3, clamp: 0), fraction 0
    got = tm.sample(px, dec, tm.BILINEAR, tm.REPEAT, np.float32([-0.125]), np.float32([0.75]))[0]
    exp = (dec[px[0, 3]] * np.float32(1) + dec[px[0, 0]] * np.float32(0)) * np.float32(1) + (dec[px[1, 3]] * np.float32(1) + dec[px[1, 0]] * np.float32(0)) * np.float32(0)
    np.testing.assert_array_equal(got, exp)


def test_model_barycentrics_and_uv():
    """a ray through a known point of a triangle: the barycentrics reproduce it, the UVs interpolate linearly, the albedo multiplies"""
    v = np.float32([[0, 0, 0], [4, 0, 0], [0, 4, 0]])
    uvs = np.float32([[0, 0], [1, 0], [0, 1]])
    O = np.float32([[1, 1, 5]])
    u = np.float32([[0, 0, -1]])
    px = np.full((2, 2, 3), 255, np.uint8)
    uv, alb = tm.surface(v, [[0, 1, 2]], [[0, 1, 2]], uvs, px, tm.default_decode(), tm.NEAREST, tm.REPEAT, (0.5, 0.25, 1.0), [0], O, u)
    np.testing.assert_array_equal(uv[0], np.float32([0.25, 0.25]))
    np.testing.assert_array_equal(alb[0], np.float32([0.5, 0.25, 1.0]))
