"""rt_mesh_rebuild_mode(RT_BVH_LBVH) against tests/lbvh_model.py, the numpy twin of the builder: the flat tree as bits, the triangle order and rt_build_stats on the
meshes of tests/lbvh_fixtures.py -- every size around a wave and a block, one cell, coincident triangles, zero-area boxes, a plane, the large-mesh triangle cost, and two
combs whose trees are as deep as the 63-bit code allows, one on either side of the device-side install's depth limit (rt_lbvh.hip.h, rt_host_mesh.hip.h rebuild_part).
Then the traversal kernels on those trees (explicit rays: the combs' triangles are too small for a frame to see) and the device-side install against the host's.  -m gpu."""
import os
import zlib

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import hostlib
from . import lbvh_fixtures as fx
from . import lbvh_model as lm
from .test_gpu_parity import values_equal

pytestmark = pytest.mark.gpu
KEYS = ("rays", "box_tests", "nodes", "tri_tests")
STATS = ("n_nodes", "n_leaves", "max_leaf_tris", "max_depth")
TRACE = ("wavefront_queue", "path", "wavefront")                         # the traversal kernels rt_trace_rays runs (lockstep renders frames only: see the frame test)
c_, s_ = np.float32(np.cos(0.4)), np.float32(np.sin(0.4))
R, T = np.array([[c_, 0, s_], [0, 1, 0], [-s_, 0, c_]], np.float32), (1.5, -0.5, 2.0)


class Case:
    """a fixture as a caller uploads it (the reference tree, its triangle order `up`), the model's tree on that order, and rays aimed at its triangles"""
    def __init__(self, name, v, t):
        self.name, self.v = name, v
        self.first = hostlib.build_mesh(v, t, albedo=rt.scenes.CAT_ALBEDO, object_slot=6)
        self.up = np.ascontiguousarray(self.first["indices"][:, :3])
        self.nt = len(self.up)
        self.model = lm.build(v, self.up)
        self.rays = _rays(v, self.up, seed=zlib.crc32(name.encode()))


def _rays(v, tris, seed):
    """one ray at the centroid of every triangle (of 2 000 drawn ones) from either side -- along the normal from close by, against it from half the mesh's size away --
    and 200 random ones through the mesh's box"""
    rng = np.random.default_rng(seed)
    P = np.asarray(v, np.float64)[tris if len(tris) <= 2000 else tris[rng.choice(len(tris), 2000, replace=False)]]
    C = P.mean(axis=1)
    nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    flat = np.linalg.norm(nrm, axis=1) == 0                              # zero area: any direction
    nrm[flat] = rng.normal(size=(int(flat.sum()), 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    lo, hi = np.asarray(v, np.float64).min(axis=0), np.asarray(v, np.float64).max(axis=0)
    size = float((hi - lo).max())
    near = np.maximum(3 * np.ptp(P, axis=1).max(axis=1), 1e-3)[:, None]   # (beyond tri_tmin = 1e-4)
    rays = [np.concatenate([C - near * nrm, nrm], 1), np.concatenate([C + 0.5 * size * nrm, -nrm], 1)]
    O = rng.uniform(lo - 0.25 * size, hi + 0.25 * size, (200, 3))
    d = rng.uniform(lo, hi, (200, 3)) - O
    rays.append(np.concatenate([O, d / np.linalg.norm(d, axis=1, keepdims=True)], 1))
    return np.concatenate(rays).astype(np.float32)


def _oracle_hits(om, rays):
    exp = np.zeros((len(rays), 5), np.float32)
    for i in range(len(rays)):
        h, t, N = om.intersect(rays[i, :3], rays[i, 3:], 1e-4)
        exp[i, 0] = 1.0 if h else 0.0
        exp[i, 1] = t; exp[i, 2:5] = N
    return exp


def _rays_equal(got, exp, what):
    hit = exp[:, 0] != 0
    np.testing.assert_array_equal(got[:, 0], exp[:, 0], err_msg=str(what))
    np.testing.assert_array_equal(got[hit].view(np.uint32), exp[hit].view(np.uint32), err_msg=str(what))


@pytest.fixture(scope="module")
def cases(cat_golden):
    meshes, made = fx.all_fixtures(cat_golden), {}

    def get(name):
        if name not in made:
            made[name] = Case(name, *meshes[name])
        return made[name]
    return get


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host_ctx():
    """a context that takes the host install after an LBVH build (knobs are read when the context is created)"""
    os.environ["RT_LBVH_HOST_INSTALL"] = "1"
    try:
        c = rt.Context(0)
    finally:
        del os.environ["RT_LBVH_HOST_INSTALL"]
    yield c
    c.close()


def _equals_model(ctx, got, model, on_device=None):
    arr, order = got
    m_arr, m_order, m_st = model
    st = ctx.build_stats()
    assert st["mode"] == 1 and {k: st[k] for k in STATS} == m_st
    np.testing.assert_array_equal(order, m_order)
    assert arr.shape == m_arr.shape
    np.testing.assert_array_equal(arr.view(np.uint32), m_arr.view(np.uint32))
    if on_device is not None:
        assert st["install_on_device"] == on_device


@pytest.mark.parametrize("name", fx.NAMES)
def test_tree_order_and_stats_equal_the_model_and_rays_the_oracle_on_the_models_tree(ctx, oracle, cases, name):
    k = cases(name)
    ctx.scene_upload(rt.scenes.spheres("cpu"), k.first)
    _equals_model(ctx, ctx.mesh_rebuild(k.nt, mode="lbvh"), k.model, on_device=0 if name == "comb_deep" else 1)
    m_arr, m_order, m_st = k.model
    om = oracle.Mesh.from_arrays(k.v, k.up).set_bvh(m_arr, m_order)
    exp = _oracle_hits(om, k.rays)
    aimed = exp[:len(k.rays) - 200, 0]
    print(f"{name}: {k.nt} triangles, {m_st}; {int(exp[:, 0].sum())} of {len(exp)} rays hit")
    if name in ("collinear_degenerate", "planar"):                       # a root box without thickness is never entered (the strict '>' of BoundingBox::intersect, cpu:156)
        assert exp[:, 0].sum() == 0
    else:
        assert aimed.mean() > 0.9
    for variant in TRACE:
        _rays_equal(ctx.trace_rays(k.rays, 1e-4, variant), exp, (name, variant))
    # a second build starts from the order the first one left: equal codes are now told apart by the NEW uploaded index
    _equals_model(ctx, ctx.mesh_rebuild(k.nt, mode="lbvh"), lm.build(k.v, k.up[m_order]), on_device=0 if name == "comb_deep" else 1)


@pytest.mark.parametrize("name", ["cat", "planar", "coincident_cluster"])
def test_frames_and_work_counters_on_the_models_tree(ctx, oracle, cases, name):
    k = cases(name)
    ctx.scene_upload(rt.scenes.spheres("cpu"), k.first)
    _equals_model(ctx, ctx.mesh_rebuild(k.nt, mode="lbvh"), k.model)
    osc = oracle.Scene.preset("cpu", oracle.Mesh.from_arrays(k.v, k.up).set_bvh(k.model[0], k.model[1]))
    W, H = 160, 100
    for b in (0, 2):
        exp, _, cnt = osc.render(W, H, 1, b, want_rgb8=False)
        for variant in ("auto", "wavefront", "lockstep") if b == 0 else ("auto",):
            p = rt.make_params(W, H, 1, b, variant=variant, **rt.scenes.CPU_LAUNCHER)
            got = ctx.render(p)
            assert values_equal(got[..., :3], exp[..., :3]).all(), (b, variant)
            np.testing.assert_array_equal(got[..., 3], exp[..., 3])
            assert ctx.count_work(p) == {key: cnt[key] for key in KEYS}, (b, variant)


def test_the_triangle_cost_override(cases, monkeypatch):
    """RT_LBVH_CT=4 (an A/B knob: honoured under RT_EXPERIMENT=1 only): the cut with a triangle test four times a box test"""
    k = cases("coincident_cluster")
    model4 = lm.build(k.v, k.up, ct=4.0)
    assert model4[0].shape != k.model[0].shape                           # another tree than the default's
    monkeypatch.setenv("RT_LBVH_CT", "4")
    stray = rt.Context(0)
    monkeypatch.setenv("RT_EXPERIMENT", "1")
    c = rt.Context(0)
    monkeypatch.delenv("RT_EXPERIMENT")
    monkeypatch.delenv("RT_LBVH_CT")
    try:
        for ctx_, model in ((c, model4), (stray, k.model)):             # a stray variable in a caller's environment moves nothing
            ctx_.scene_upload(rt.scenes.spheres("cpu"), k.first)
            _equals_model(ctx_, ctx_.mesh_rebuild(k.nt, mode="lbvh"), model, on_device=1)
    finally:
        c.close(); stray.close()


@pytest.mark.parametrize("name", ["cat", "planar"])
def test_the_builder_reads_the_vertices_the_device_holds(ctx, oracle, cases, name):
    """after mesh_transform: the model on the oracle's transformed vertices"""
    k = cases(name)
    ctx.scene_upload(rt.scenes.spheres("cpu"), k.first)
    ctx.mesh_transform(R, T)
    moved = oracle.Mesh.from_arrays(k.v, k.up).transform(R, T).vertices
    assert not np.array_equal(moved, k.v)
    _equals_model(ctx, ctx.mesh_rebuild(k.nt, mode="lbvh"), lm.build(moved, k.up), on_device=1)


def test_the_second_mesh_of_a_scene(ctx, cases):
    """rt_mesh_rebuild_of on the second part of a two-mesh scene (its triangles start behind the first mesh's, its vertex indices are global on the device):
    the model on that mesh's own arrays"""
    a, b = cases("sizes65"), cases("coincident_cluster")
    ctx.scene_upload(rt.scenes.spheres("cpu"), [dict(a.first, object_slot=6), dict(b.first, object_slot=7)])
    _equals_model(ctx, ctx.mesh_rebuild(b.nt, "lbvh", object_slot=7), b.model, on_device=0)
    _equals_model(ctx, ctx.mesh_rebuild(a.nt, "lbvh", object_slot=6), a.model, on_device=0)
    _equals_model(ctx, ctx.mesh_rebuild(b.nt, "lbvh", object_slot=7), lm.build(b.v, b.up[b.model[1]]), on_device=0)


@pytest.mark.parametrize("name", ["comb_shallow", "one_cell", "coincident_cluster", "sizes65"])
def test_device_install_equals_host_install(ctx, host_ctx, cases, name):
    """Both installs number the breadth-first pairs by one rule (root step most significant, right child first): the layouts' hashes, the rays through every traversal
    kernel and the work counters are equal, and after a mesh_transform -- the refit on device-built levels -- again."""
    k = cases(name)
    p = rt.make_params(160, 100, 1, 0, **rt.scenes.CPU_LAUNCHER)
    for c, on_device in ((ctx, 1), (host_ctx, 0)):
        c.scene_upload(rt.scenes.spheres("cpu"), k.first)
        _equals_model(c, c.mesh_rebuild(k.nt, mode="lbvh"), k.model, on_device=on_device)
    for step in ("built", "moved"):
        assert ctx.layout_hash() == host_ctx.layout_hash(), step
        assert ctx.layout_hash()["pairs"] != 0
        for variant in TRACE:
            np.testing.assert_array_equal(ctx.trace_rays(k.rays, 1e-4, variant).view(np.uint32), host_ctx.trace_rays(k.rays, 1e-4, variant).view(np.uint32), err_msg=f"{step} {variant}")
        if step == "built":
            assert ctx.count_work(p, detail=True) == host_ctx.count_work(p, detail=True)
            for c in (ctx, host_ctx):
                c.mesh_transform(R, T)


def test_a_tree_deeper_than_the_device_install_takes(ctx, oracle, cases):
    """comb_deep: depth 64, beyond the 56 of rebuild_part and the 58 path bits of the breadth-first sort key: the host install, no error, the oracle's hits;
    and the reference builder still works afterwards"""
    k = cases("comb_deep")
    ctx.scene_upload(rt.scenes.spheres("cpu"), k.first)
    arr, order = ctx.mesh_rebuild(k.nt, mode="lbvh")
    _equals_model(ctx, (arr, order), k.model, on_device=0)
    assert ctx.build_stats()["max_depth"] > 58
    exp = _oracle_hits(oracle.Mesh.from_arrays(k.v, k.up).set_bvh(arr, order), k.rays)
    assert exp[:, 0].sum() > 100
    for variant in TRACE:
        _rays_equal(ctx.trace_rays(k.rays, 1e-4, variant), exp, variant)
    arr2, order2 = ctx.mesh_rebuild(k.nt, mode="reference")
    assert ctx.build_stats()["mode"] == 0
    ref = hostlib.build_mesh(k.v, k.up[order], albedo=rt.scenes.CAT_ALBEDO, object_slot=6)
    np.testing.assert_array_equal(arr2.view(np.uint32), np.ascontiguousarray(ref["bvh_arr10"], np.float32).view(np.uint32))
    np.testing.assert_array_equal(k.up[order][order2], ref["indices"][:, :3])
