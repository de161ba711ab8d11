"""Device vertex normals and normal snapshots at the boundary, without a GPU (rt_mesh_compute_normals[_of], rt_mesh_get_vertex_normals, rt_mesh_snapshot_normals,
rt_mesh_normal_snapshot_mask): the library exports the five entries, the header declares them and Python binds them alike, the ABI version stays 6, a NULL context is
refused with RT_ERR_INVALID and a message, the Python methods route object_slot (None = the plain form) and keep, the C++ Renderer's members compile with the host
compiler, and SvgfSequence(deforming=True) issues exactly the calls it issued before."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi

from .test_motion_capi import _Recorder, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLS = {
    "rt_mesh_compute_normals": "int rt_mesh_compute_normals(rt_ctx *ctx);",
    "rt_mesh_compute_normals_of": "int rt_mesh_compute_normals_of(rt_ctx *ctx, int object_slot);",
    "rt_mesh_get_vertex_normals": "int rt_mesh_get_vertex_normals(rt_ctx *ctx, int object_slot, float *out_xyz, int n_vertices);",
    "rt_mesh_snapshot_normals": "int rt_mesh_snapshot_normals(rt_ctx *ctx, int object_slot, int keep);",
    "rt_mesh_normal_snapshot_mask": "int rt_mesh_normal_snapshot_mask(const rt_ctx *ctx, uint32_t *mask);"}
fp = C.POINTER(C.c_float)
vp = C.c_void_p


def test_symbols_are_exported_declared_and_bound_alike():
    lib = _capi.load()
    hdr = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n, decl in DECLS.items():
        assert hasattr(lib, n), n
        assert n in _capi.EXPORTS, n
        assert decl in code, n
    assert lib.rt_mesh_compute_normals.argtypes == [vp]
    assert lib.rt_mesh_compute_normals_of.argtypes == [vp, C.c_int]
    assert lib.rt_mesh_get_vertex_normals.argtypes == [vp, C.c_int, fp, C.c_int]
    assert lib.rt_mesh_snapshot_normals.argtypes == [vp, C.c_int, C.c_int]
    assert lib.rt_mesh_normal_snapshot_mask.argtypes == [vp, C.POINTER(C.c_uint32)]
    assert lib.rt_abi_version() == 6
    assert "#define RT_ABI_VERSION 6\n" in hdr
    # the header no longer lists the two gaps
    assert "SMOOTH NORMALS ARE NOT RECOMPUTED" not in hdr and "the previous shading normals of a smooth deforming mesh" not in hdr


def test_null_context_is_refused():
    lib = _capi.load()
    out = np.full((5, 3), -7, np.float32)
    mask = C.c_uint32(0xABCD)
    for call in (lambda: lib.rt_mesh_compute_normals(None),
                 lambda: lib.rt_mesh_compute_normals_of(None, 6),
                 lambda: lib.rt_mesh_get_vertex_normals(None, -1, out.ctypes.data_as(fp), 5),
                 lambda: lib.rt_mesh_snapshot_normals(None, -1, 1),
                 lambda: lib.rt_mesh_normal_snapshot_mask(None, C.byref(mask))):
        assert call() == -1
        msg = lib.rt_last_error(None)
        assert b"NULL" in msg or b"bad arguments" in msg
    assert (out == -7).all() and mask.value == 0xABCD


def test_python_methods_route_slot_and_keep():
    c = rt.Context.__new__(rt.Context)
    c._L = _Recorder()
    c._h = C.c_void_p()
    c.mesh_compute_normals()
    c.mesh_compute_normals(object_slot=7)
    c.mesh_compute_normals(object_slot=0)                               # slot 0 is a slot, not "none"
    assert c._L.calls == [("rt_mesh_compute_normals", ()), ("rt_mesh_compute_normals_of", (7,)), ("rt_mesh_compute_normals_of", (0,))]
    c._L.calls.clear()
    c.mesh_snapshot_normals()
    c.mesh_snapshot_normals(object_slot=7)
    c.mesh_snapshot_normals(object_slot=3, keep=False)
    assert c._L.calls == [("rt_mesh_snapshot_normals", (-1, 1)), ("rt_mesh_snapshot_normals", (7, 1)), ("rt_mesh_snapshot_normals", (3, 0))]
    assert c.mesh_normal_snapshot_mask() == 0 and c._L.calls[-1][0] == "rt_mesh_normal_snapshot_mask"
    c._L.calls.clear()
    with pytest.raises(rt.RtError):                                     # this Context uploaded nothing: the count is the caller's to give
        c.mesh_vertex_normals()
    n = c.mesh_vertex_normals(n_vertices=11)
    assert n.shape == (11, 3) and n.dtype == np.float32
    c._mesh_nv = {3: 5, 7: 9}                                           # as scene_upload records them
    assert c.mesh_vertex_normals(object_slot=7).shape == (9, 3)
    with pytest.raises(rt.RtError):                                     # two meshes: name one
        c.mesh_vertex_normals()
    c._mesh_nv = {6: 4}
    assert c.mesh_vertex_normals().shape == (4, 3)
    names_slots_counts = [(name, a[0], a[2]) for name, a in c._L.calls]
    assert names_slots_counts == [("rt_mesh_get_vertex_normals", -1, 11), ("rt_mesh_get_vertex_normals", 7, 9), ("rt_mesh_get_vertex_normals", -1, 4)]
    c._h = None                                                         # (nothing to destroy)


def test_renderer_members_compile(tmp_path):
    src = tmp_path / "normals.cpp"
    src.write_text("""
#include "raytracer.hpp"
using namespace raytracer;
std::vector<float> use(Renderer &r, TriangleMesh &m, const RenderSettings &s) {
    r.snapshot_mesh_vertices_of(m);
    r.snapshot_mesh_normals_of(m);
    for (Vector &v : m.vertices) v = v + Vector(0, 0.5, 0);
    r.set_mesh_vertices_of(m);
    r.compute_mesh_normals_of(m);
    r.compute_mesh_normals();
    const std::vector<Vector> n = r.mesh_vertex_normals_of(m);
    const uint32_t mask = r.mesh_normal_snapshot_mask();
    (void)mask;
    std::vector<float> prev;
    std::vector<float> aov = r.render_aov_motion(s, &prev);
    r.forget_mesh_normal_snapshot_of(m);
    r.snapshot_mesh_normals();
    aov.push_back(n.empty() ? 0.f : n[0][0]);
    return aov;
}
""")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_deforming_sequence_issues_exactly_the_calls_it_issued_before():
    """svgf.py did not change: the normal snapshot reaches the chain through the context's mask inside render_aov_motion_device, not through a new call"""
    c, seq = _run(deforming=True)
    assert [n for n, _, _ in c.calls] == ["render_device", "render_aov_motion_device", "temporal_accumulate_device", "svgf_filter_device"] * 3
    for i in range(3):
        (_, aa, ak) = c.calls[4 * i + 1]
        assert len(aa) == 3 and set(ak) == {"pose", "motion", "stream"}
        assert aa[2] == seq.previous_frame_planes
    c, _ = _run()
    assert [n for n, _, _ in c.calls] == ["render_device", "render_aov_device", "temporal_accumulate_device", "svgf_filter_device"] * 3
    doc = rt.SvgfSequence.__doc__ + (rt.SvgfSequence.frame.__doc__ or "")
    for word in ("mesh_snapshot_vertices", "mesh_snapshot_normals", "mesh_compute_normals"):
        assert word in doc, word
