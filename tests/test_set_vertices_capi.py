"""The entries that give a mesh new vertex positions in place (rt_mesh_set_vertices / _of / _device) at the boundary, without a GPU: the library exports them, the header
declares them and Python binds them alike, the ABI version stays 6, a NULL context is refused with RT_ERR_INVALID and a message, the Python method routes object_slot and
the device form, and the C++ Renderer's members compile with the host compiler."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLS = {"rt_mesh_set_vertices": "int rt_mesh_set_vertices(rt_ctx *ctx, const float *xyz_host, int n_vertices);",
         "rt_mesh_set_vertices_of": "int rt_mesh_set_vertices_of(rt_ctx *ctx, int object_slot, const float *xyz_host, int n_vertices);",
         "rt_mesh_set_vertices_device": "int rt_mesh_set_vertices_device(rt_ctx *ctx, int object_slot, const void *xyz_dev, int stride_floats, int n_vertices);"}
fp = C.POINTER(C.c_float)


def test_symbols_are_exported_declared_and_bound_alike():
    lib = _capi.load()
    hdr = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n, decl in DECLS.items():
        assert hasattr(lib, n), n
        assert n in _capi.EXPORTS, n
        assert decl in code, n
    assert lib.rt_mesh_set_vertices.argtypes == [C.c_void_p, fp, C.c_int]
    assert lib.rt_mesh_set_vertices_of.argtypes == [C.c_void_p, C.c_int, fp, C.c_int]
    assert lib.rt_mesh_set_vertices_device.argtypes == [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
    assert lib.rt_abi_version() == 6
    assert "#define RT_ABI_VERSION 6\n" in hdr


def test_null_context_is_refused():
    lib = _capi.load()
    v = np.zeros((3, 3), np.float32)
    for call in (lambda: lib.rt_mesh_set_vertices(None, v.ctypes.data_as(fp), 3),
                 lambda: lib.rt_mesh_set_vertices_of(None, 0, v.ctypes.data_as(fp), 3),
                 lambda: lib.rt_mesh_set_vertices_device(None, -1, C.c_void_p(v.ctypes.data), 3, 3)):
        lib.rt_last_error(None)
        assert call() == -1
        assert b"NULL" in lib.rt_last_error(None)


class _Recorder:
    """stands in for the loaded library: records which entry a method called and with what arguments"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args[1:]))
            return 0
        return fn


def test_python_method_routes_object_slot_and_the_device_form():
    c = rt.Context.__new__(rt.Context)
    c._L = _Recorder()
    c._h = C.c_void_p()
    v = np.arange(12, dtype=np.float64).reshape(4, 3)
    c.mesh_set_vertices(v)
    c.mesh_set_vertices(v.tolist(), object_slot=7)
    c.mesh_set_vertices(device_ptr=4096, n_vertices=4)
    c.mesh_set_vertices(device_ptr=8192, stride=4, n_vertices=5, object_slot=3)
    (n0, a0), (n1, a1), (n2, a2), (n3, a3) = c._L.calls
    assert (n0, a0[1]) == ("rt_mesh_set_vertices", 4)
    assert (n1, a1[0], a1[2]) == ("rt_mesh_set_vertices_of", 7, 4)
    np.testing.assert_array_equal(np.ctypeslib.as_array(a1[1], (12,)), np.arange(12, dtype=np.float32))   # float32, row-major xyz
    assert n2 == "rt_mesh_set_vertices_device" and (a2[0], a2[1].value, a2[2], a2[3]) == (-1, 4096, 3, 4)
    assert n3 == "rt_mesh_set_vertices_device" and (a3[0], a3[1].value, a3[2], a3[3]) == (3, 8192, 4, 5)
    with pytest.raises(ValueError):
        c.mesh_set_vertices(v, device_ptr=4096, n_vertices=4)
    with pytest.raises(ValueError):
        c.mesh_set_vertices(device_ptr=4096)
    c._h = None                                                         # (nothing to destroy)


def test_renderer_members_compile(tmp_path):
    src = tmp_path / "set_vertices.cpp"
    src.write_text("""
#include "raytracer.hpp"
using namespace raytracer;
void use(Renderer &r, TriangleMesh &m) {
    for (Vector &v : m.vertices) v = v + Vector(0, 0.5, 0);
    r.set_mesh_vertices(m);
    r.set_mesh_vertices_of(m);
    r.use_smooth_normals_of(m);
}
""")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
