"""Reprojecting a deforming mesh at the boundary, without a GPU (rt_mesh_snapshot_vertices, rt_mesh_snapshot_mask, rt_render_aov_motion[_device]): the library exports
the four entries, the header declares them and Python binds them alike, the ABI version stays 6, a NULL context is refused with RT_ERR_INVALID and a message, the Python
methods route object_slot, keep, motion and the device form, the C++ Renderer's members compile with the host compiler, and SvgfSequence issues the calls it issued
before with deforming=False and the new chain with deforming=True."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLS = {
    "rt_mesh_snapshot_vertices": "int rt_mesh_snapshot_vertices(rt_ctx *ctx, int object_slot, int keep);",
    "rt_mesh_snapshot_mask": "int rt_mesh_snapshot_mask(const rt_ctx *ctx, uint32_t *mask);",
    "rt_render_aov_motion_device": "int rt_render_aov_motion_device(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, const rt_rows *rows, "
                                   "const rt_motion *motion, void *out_aov_dev, void *out_prev_dev, void *stream);",
    "rt_render_aov_motion": "int rt_render_aov_motion(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, const rt_rows *rows, const rt_motion *motion, "
                            "float *out_aov_host, float *out_prev_host);"}
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
    P = C.POINTER
    assert lib.rt_mesh_snapshot_vertices.argtypes == [vp, C.c_int, C.c_int]
    assert lib.rt_mesh_snapshot_mask.argtypes == [vp, P(C.c_uint32)]
    assert lib.rt_render_aov_motion_device.argtypes == [vp, P(_capi.Params), P(_capi.CameraPose), P(_capi.Rows), P(_capi.Motion), vp, vp, vp]
    assert lib.rt_render_aov_motion.argtypes == [vp, P(_capi.Params), P(_capi.CameraPose), P(_capi.Rows), P(_capi.Motion), fp, fp]
    assert lib.rt_abi_version() == 6
    assert "#define RT_ABI_VERSION 6\n" in hdr


def test_null_context_is_refused():
    lib = _capi.load()
    p = rt.make_params(4, 4, 1, 0)
    aov, prev = np.full((3, 4, 4, 4), -7, np.float32), np.full((2, 4, 4, 4), -7, np.float32)
    mask = C.c_uint32(0xABCD)
    for call in (lambda: lib.rt_mesh_snapshot_vertices(None, -1, 1),
                 lambda: lib.rt_mesh_snapshot_mask(None, C.byref(mask)),
                 lambda: lib.rt_render_aov_motion_device(None, C.byref(p), None, None, None, None, None, None),
                 lambda: lib.rt_render_aov_motion(None, C.byref(p), None, None, None, aov.ctypes.data_as(fp), prev.ctypes.data_as(fp))):
        assert call() == -1
        msg = lib.rt_last_error(None)
        assert b"NULL" in msg or b"bad arguments" in msg
    assert (aov == -7).all() and (prev == -7).all() and mask.value == 0xABCD


class _Recorder:
    """stands in for the loaded library: records which entry a method called and with what arguments"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args[1:]))
            return 0
        return fn


def test_python_methods_route_slot_keep_motion_and_the_device_form():
    c = rt.Context.__new__(rt.Context)
    c._L = _Recorder()
    c._h = C.c_void_p()
    c.mesh_snapshot_vertices()
    c.mesh_snapshot_vertices(object_slot=7)
    c.mesh_snapshot_vertices(object_slot=3, keep=False)
    assert c._L.calls == [("rt_mesh_snapshot_vertices", (-1, 1)), ("rt_mesh_snapshot_vertices", (7, 1)), ("rt_mesh_snapshot_vertices", (3, 0))]
    assert c.mesh_snapshot_mask() == 0 and c._L.calls[-1][0] == "rt_mesh_snapshot_mask"
    c._L.calls.clear()
    p = rt.make_params(7, 5, 1, 0)
    motion = rt.static_motion()
    motion[2, 9:] = (1, 2, 3)
    aov, prev = c.render_aov_motion(p)
    assert aov.shape == (3, 5, 7, 4) and prev.shape == (2, 5, 7, 4) and aov.dtype == prev.dtype == np.float32
    aov, prev = c.render_aov_motion(p, rows=_capi.Rows(1, 2, 2, 1), motion=motion.astype(np.float64), pose=rt.make_pose())
    assert aov.shape == (3, 2, 7, 4) and prev.shape == (2, 2, 7, 4)
    c.render_aov_motion_device(p, 0x1000, 0x2000)
    c.render_aov_motion_device(p, 0x1000, 0x2000, motion=motion, stream=0x30, rows=_capi.Rows(0, 3, 3, 1))
    (n0, a0), (n1, a1), (n2, a2), (n3, a3) = c._L.calls                 # (params, pose, rows, motion, out, prev[, stream])
    assert (n0, n1, n2, n3) == ("rt_render_aov_motion", "rt_render_aov_motion", "rt_render_aov_motion_device", "rt_render_aov_motion_device")
    assert a0[1] is None and a0[2] is None and a0[3] is None
    assert a1[1] is not None and a1[2]._obj.n_rows == 2
    np.testing.assert_array_equal(np.ctypeslib.as_array(C.cast(a1[3], fp), (16 * 12,)).reshape(16, 12), motion)   # float32, one record per object
    assert a2[3] is None and (a2[4].value, a2[5].value, a2[6]) == (0x1000, 0x2000, None)
    assert (a2[2]._obj.row0, a2[2]._obj.n_rows) == (0, 5)               # rows=None: the whole frame
    assert a3[3] is not None and a3[2]._obj.n_rows == 3 and a3[6].value == 0x30
    for bad in (lambda: c.render_aov_motion(p, motion=np.zeros((10, 12), np.float32)), lambda: c.render_aov_motion_device(p, 0x1000, 0x2000, motion=np.zeros((16, 9)))):
        with pytest.raises(rt.RtError) as e:
            bad()
        assert e.value.code == -1
    assert len(c._L.calls) == 4
    c._h = None                                                         # (nothing to destroy)


def test_renderer_members_compile(tmp_path):
    src = tmp_path / "motion.cpp"
    src.write_text("""
#include "raytracer.hpp"
using namespace raytracer;
std::vector<float> use(Renderer &r, TriangleMesh &m, const RenderSettings &s, const std::vector<float> &prev_planes, const std::vector<float> &prev_history) {
    r.snapshot_mesh_vertices_of(m);
    for (Vector &v : m.vertices) v = v + Vector(0, 0.5, 0);
    r.set_mesh_vertices_of(m);
    const uint32_t mask = r.mesh_snapshot_mask();
    (void)mask;
    std::vector<float> color = r.render_float(s), prev;
    rt_motion table[RT_MAX_OBJECTS] = {};
    std::vector<float> aov = r.render_aov_motion(s, &prev, table);
    rt_temporal_params tp{32, 0.f, 0.9f, 0.5f};
    rt_reproject rp{};                                                  // motion == nullptr: the motion is in the previous-frame planes
    std::vector<float> h = r.temporal_accumulate(color, prev, prev_planes, prev_history, s.W, s.H, tp, &rp);
    r.forget_mesh_snapshot_of(m);
    r.snapshot_mesh_vertices();
    return h;
}
""")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


class _Ctx:
    """stands in for a Context under SvgfSequence: hands out addresses, records every method call with its arguments"""

    def __init__(self):
        self.calls, self.next = [], 0x10000

    def device_alloc(self, n):
        self.next += 0x100000
        return self.next

    def device_free(self, p):
        pass

    @staticmethod
    def _rows_or_whole(params, rows):
        return rt.Context._rows_or_whole(params, rows)

    def __getattr__(self, name):
        def fn(*args, **kw):
            self.calls.append((name, args, kw))
        return fn


def _run(frames=3, **kw):
    c = _Ctx()
    seq = rt.SvgfSequence(c, 8, 6, **kw)
    motion = rt.static_motion()
    for i in range(frames):
        seq.frame(rt.make_params(8, 6, 1, 3, seed=i), motion=motion if i else None, no_history_mask=4)
    return c, seq


def test_sequence_without_deforming_issues_the_calls_it_always_issued():
    c, seq = _run()
    assert not hasattr(seq, "previous_frame_planes")
    assert [n for n, _, _ in c.calls] == ["render_device", "render_aov_device", "temporal_accumulate_device", "svgf_filter_device"] * 3
    for i in range(3):
        (_, ra, rk), (_, aa, ak), (_, ta, tk), (_, fa, fk) = c.calls[4 * i:4 * i + 4]
        planes = aa[1]
        assert ak == dict(pose=None, stream=None) and len(aa) == 2
        assert ta[0] == ra[2] and ta[1] == planes and fa[1] == planes  # the accumulation and the filter read the planes this frame rendered
        if i == 0:
            assert ta[2] is None and ta[3] is None and "reproject" not in tk
        else:
            assert ta[2] == c.calls[4 * (i - 1) + 1][1][1]             # the previous frame's planes
            assert tk["reproject"].motion and tk["reproject"].no_history_mask == 4   # the table rides in the record
    c, _ = _run(rectify=rt.make_rectify_params())
    assert [n for n, _, _ in c.calls] == ["render_device", "render_aov_device", "temporal_accumulate_fast_device", "history_rectify_device", "svgf_filter_device"] * 3


def test_deforming_sequence_reprojects_from_the_previous_frame_planes():
    c, seq = _run(deforming=True)
    assert [n for n, _, _ in c.calls] == ["render_device", "render_aov_motion_device", "temporal_accumulate_device", "svgf_filter_device"] * 3
    prevs = set()
    for i in range(3):
        (_, ra, rk), (_, aa, ak), (_, ta, tk), (_, fa, fk) = c.calls[4 * i:4 * i + 4]
        planes, source = aa[1], aa[2]
        prevs.add(source)
        assert source == seq.previous_frame_planes and source != planes
        assert (ak["motion"] is None) == (i == 0)                      # the table goes to the planes call ...
        assert ta[1] == source                                         # the accumulation reprojects from the previous-frame planes
        assert fa[1] == planes                                         # the filter keeps the current ones
        if i:
            assert ta[2] == c.calls[4 * (i - 1) + 1][1][1]             # prev_aov: the previous frame's CURRENT planes
            assert not tk["reproject"].motion and tk["reproject"].no_history_mask == 4   # ... and the record carries none
    assert len(prevs) == 1
    c, seq = _run(deforming=True, rectify=rt.make_rectify_params(), upsample=2, filter_at="full")
    names = [n for n, _, _ in c.calls]
    assert names[:7] == ["render_device", "render_aov_motion_device", "temporal_accumulate_fast_device", "history_rectify_device", "render_aov_device", "upsample_device",
                         "svgf_filter_device"]
    acc, rect, up = c.calls[2], c.calls[3], c.calls[5]
    planes = c.calls[1][1][1]
    assert acc[1][1] == seq.previous_frame_planes and rect[1][2] == planes and up[1][1] == planes   # the clamp and the upsample keep the current planes
    c, _ = _run(deforming=True, adaptive=rt.make_sample_count_params())
    assert [n for n, _, _ in c.calls][:7] == ["render_device", "render_aov_motion_device", "temporal_accumulate_device", "sample_counts_device", "render_counts_device",
                                              "temporal_accumulate_device", "svgf_filter_device"]
    assert c.calls[5][1][1] == c.calls[2][1][1] == c.calls[1][1][2]
