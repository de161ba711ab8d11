"""The per-mesh entries of a multi-mesh scene (rt_mesh_transform_of / rt_mesh_set_normals_of / rt_mesh_rebuild_of) at the boundary, without a GPU: the library exports
them, a NULL context is refused with RT_ERR_INVALID and a message, the Python methods route object_slot to them (and keep the plain entries without it), and the C++
Renderer's members that address one TriangleMesh compile with the host compiler."""
import ctypes as C
import os
import subprocess

import numpy as np

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_mesh_transform_of", "rt_mesh_set_normals_of", "rt_mesh_rebuild_of")


def test_per_mesh_symbols_are_exported_and_declared():
    lib = _capi.load()
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _capi.EXPORTS, n
    hdr = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for n in NEW:
        assert f"int {n}(rt_ctx *ctx, int object_slot" in hdr, n


def test_null_context_is_refused():
    lib = _capi.load()
    fp = C.POINTER(C.c_float)
    r = np.eye(3, dtype=np.float32).reshape(9)
    t = np.zeros(3, np.float32)
    lib.rt_last_error(None)
    assert lib.rt_mesh_transform_of(None, 0, r.ctypes.data_as(fp), t.ctypes.data_as(fp)) == -1
    assert b"NULL" in lib.rt_last_error(None)
    n = np.zeros((3, 3), np.float32)
    ix = np.zeros((1, 3), np.int32)
    assert lib.rt_mesh_set_normals_of(None, 0, n.ctypes.data_as(fp), 3, ix.ctypes.data_as(C.POINTER(C.c_int32)), 3, 1) == -1
    assert b"NULL" in lib.rt_last_error(None)
    arr = np.zeros((4, 10), np.float32)
    order = np.zeros(1, np.int32)
    nn = C.c_int32(7)
    assert lib.rt_mesh_rebuild_of(None, 0, 0, arr.ctypes.data_as(fp), order.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nn)) == -1
    assert b"NULL" in lib.rt_last_error(None)


class _Recorder:
    """stands in for the loaded library: records which entry a method called and with what slot"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args[1] if len(args) > 1 else None))
            return 0
        return fn


def _fake_context():
    c = rt.Context.__new__(rt.Context)
    c._L = _Recorder()
    c._h = C.c_void_p()
    return c


def test_python_methods_route_object_slot():
    c = _fake_context()
    R, t = np.eye(3), (1.0, 2.0, 3.0)
    vn, nidx = np.zeros((4, 3), np.float32), np.zeros((2, 3), np.int32)
    c.mesh_transform(R, t)
    c.mesh_transform(R, t, object_slot=3)
    c.mesh_set_normals(vn, nidx)
    c.mesh_set_normals(vn, nidx, object_slot=7)
    c.mesh_set_normals(None, None, object_slot=7)
    c.mesh_set_normals(None, None)
    arr, order = c.mesh_rebuild(5, "lbvh", object_slot=3)
    assert arr.shape == (0, 10) and order.shape == (5,)
    c.mesh_rebuild(5)
    names = [n for n, _ in c._L.calls]
    assert names == ["rt_mesh_transform", "rt_mesh_transform_of", "rt_mesh_set_normals", "rt_mesh_set_normals_of", "rt_mesh_set_normals_of",
                     "rt_mesh_set_normals", "rt_mesh_rebuild_of", "rt_mesh_rebuild_mode"]
    assert [s for n, s in c._L.calls if n.endswith("_of")] == [3, 7, 7, 3]
    c._h = None                                                         # (nothing to destroy)


def test_renderer_members_for_one_mesh_compile(tmp_path):
    src = tmp_path / "per_mesh.cpp"
    src.write_text("""
#include "raytracer.hpp"
using namespace raytracer;
void use(Renderer &r, const TriangleMesh &m) {
    const float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    r.transform_mesh_of(m, R, Vector(1, 2, 3));
    r.use_smooth_normals_of(m);
    r.use_flat_normals_of(m);
    std::vector<int32_t> order;
    std::vector<float> arr = r.rebuild_mesh_of(m, RT_BVH_LBVH, &order);
    (void)arr;
}
""")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
