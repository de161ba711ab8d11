"""A mesh that changes shape in place (rt_mesh_set_vertices / _of / _device): new positions for every vertex, the triangle records and every box of the tree in use
refitted across the chip (rt_meshops.hip.h refit_up_kernel).  -m gpu.

Every expectation is something that existed before these entries: the CPU oracle walking the OLD tree refitted around the NEW vertices (Mesh.from_arrays(V_new, old
triangles).set_bvh(old tree).refit()), a fresh upload of exactly that, and rt_mesh_transform with its one-workgroup refit_kernel.  The deformation is a sine wave along one
axis with an amplitude of a few percent of the extent: no rigid motion explains it.  sigma == 0: frames are compared bit for bit in every channel and in .w."""
import ctypes
import os
from contextlib import contextmanager

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import hostlib

from . import material_scenes as ms
from .lbvh_fixtures import displaced_grid
from .test_gpu_forest_meshops import R1, R2, T1, T2, _check_rays, _vertex_normals
from .test_gpu_parity import TOL, _synthetic_mesh, linf, values_equal
from .test_gpu_tree_shapes import _big_leaf_mesh, _join, _soup

pytestmark = pytest.mark.gpu

A, B = 3, 7                                                             # the two cats' object slots in two_cats
SLOT = 6                                                                # the cat's in the cpu scene
W, H = 320, 200
VARIANTS = ("auto", "wavefront", "path", "lockstep")


@contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _context(**kw):
    with _env(**kw):                                                    # the knobs are read once, when the context is created
        return rt.Context(0)


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx2():
    c = rt.Context(0)
    yield c
    c.close()


def _params(b, variant="auto", n=1, w=W, h=H):
    return rt.make_params(w, h, n, b, variant=variant, **rt.scenes.CPU_LAUNCHER)


def _frames_equal(got, exp):
    np.testing.assert_array_equal(np.ascontiguousarray(got[..., :3]).view(np.uint32), np.ascontiguousarray(exp[..., :3]).view(np.uint32))
    np.testing.assert_array_equal(got[..., 3], exp[..., 3])


def _wave(v, axis=0, along=1, amp=0.04, periods=2.5):
    """v with coordinate `along` displaced by a sine of coordinate `axis`: amplitude amp * the extent along `along`, `periods` waves over the extent along `axis`"""
    v = np.asarray(v, np.float32)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    ext = np.maximum(hi - lo, 1e-6)
    out = v.copy()
    out[:, along] = (v[:, along].astype(np.float64) + amp * ext[along] * np.sin(2 * np.pi * periods * (v[:, axis] - lo[axis]) / ext[axis])).astype(np.float32)
    return out


def _tris(d):
    return np.ascontiguousarray(np.asarray(d["indices"])[:, :3], np.int32)


def _refitted(oracle, d, v_new, material=None):
    """the oracle's mesh of upload record d with the vertices v_new in d's tree: same triangles, same topology, every box refitted"""
    m = oracle.Mesh.from_arrays(v_new, _tris(d), albedo=tuple(d.get("albedo", (0.25, 0.25, 0.25))))
    if material:
        m.set_material(*material)
    return m.set_bvh(np.asarray(d["bvh_arr10"], np.float32).reshape(-1, 10)).refit()


def _as_upload(d, om):
    return dict(d, vertices=om.vertices, indices=om.triangles, bvh_arr10=om.bvh_array())


def _fresh(spheres, meshes):
    """(layout hashes, context) of a fresh upload"""
    c = rt.Context(0)
    try:
        c.scene_upload(spheres, meshes)
        return c.layout_hash(), c
    except Exception:
        c.close()
        raise


def _cat_record(cat_golden):
    return dict(vertices=np.asarray(cat_golden["vertices"], np.float32), indices=cat_golden["tri_bvh_order"], bvh_arr10=cat_golden["bvh_arr10"],
                albedo=rt.scenes.CAT_ALBEDO, object_slot=SLOT)


def _two_cats(cat_golden):
    spheres, meshes = ms.capi_scene("two_cats", cat_golden["vertices"], cat_golden["tri_obj_order"])
    mat = {pos: o[3:6] for pos, o in enumerate(ms.describe("two_cats", cat_golden["vertices"])) if o[0] == "mesh"}
    return spheres, meshes, mat


def _two_cats_oracle(oracle, cat_golden, meshes, mat, new):
    """two_cats in the oracle, mesh `slot` with the vertices new[slot] (else its own) in its uploaded tree, every mesh refitted -> (scene, {slot: mesh})"""
    osc, oms = oracle.Scene(), {}
    by_slot = {d["object_slot"]: d for d in meshes}
    for pos, o in enumerate(ms.describe("two_cats", cat_golden["vertices"])):
        if o[0] == "sphere":
            osc.add_sphere(o[1], o[2], o[3])
            continue
        d = by_slot[pos]
        oms[pos] = _refitted(oracle, d, new.get(pos, d["vertices"]), mat[pos])
        osc.add_mesh(oms[pos])
    return osc, oms


def _against_oracle(ctx, osc, tag):
    for b in (0, 2):
        exp, _, cnt = osc.render(W, H, 1, b, want_rgb8=False)
        for variant in VARIANTS:
            _frames_equal(ctx.render(_params(b, variant)), exp)
        work = ctx.count_work(_params(b))
        assert work["rays"] == cnt["rays"] and work["tri_tests"] == cnt["tri_tests"], (tag, b)


# ------------------------------------------------------------------------------------------------------------------------ 1, 2: the oracle and a fresh upload

def test_deformed_cat_equals_the_oracle_and_a_fresh_upload(ctx, oracle, cat_golden):
    d = _cat_record(cat_golden)
    spheres = rt.scenes.spheres("cpu")
    ctx.scene_upload(spheres, d)
    before = ctx.render(_params(0))
    vn = _wave(d["vertices"])
    assert np.abs(vn - d["vertices"]).max() > 0.5
    ctx.mesh_set_vertices(vn)
    om = _refitted(oracle, d, vn)
    _against_oracle(ctx, oracle.Scene.preset("cpu", om), "cat")
    assert (ctx.render(_params(0))[..., :3] != before[..., :3]).any()
    want, fresh = _fresh(spheres, _as_upload(d, om))
    try:
        assert ctx.layout_hash() == want
        _frames_equal(ctx.render(_params(2)), fresh.render(_params(2)))
    finally:
        fresh.close()
    ctx.mesh_set_vertices(_wave(vn, axis=2, along=0), object_slot=SLOT)   # a second deformation, through the per-mesh entry: the plain one on a scene of one mesh
    om2 = _refitted(oracle, d, _wave(vn, axis=2, along=0))
    exp, _, _ = oracle.Scene.preset("cpu", om2).render(W, H, 1, 2, want_rgb8=False)
    _frames_equal(ctx.render(_params(2)), exp)
    ctx.scene_upload([], dict(d, object_slot=0))                         # rays through the deformed mesh alone
    ctx.mesh_set_vertices(vn)
    _check_rays(ctx, oracle, [om], 71)


def test_two_cats_deformed_per_mesh_then_both(ctx, oracle, cat_golden):
    spheres, meshes, mat = _two_cats(cat_golden)
    by_slot = {d["object_slot"]: d for d in meshes}
    new = {A: _wave(by_slot[A]["vertices"]), B: _wave(by_slot[B]["vertices"], axis=1, along=2, amp=0.06)}
    for slots in ((A,), (B,), (A, B)):
        ctx.scene_upload(spheres, meshes)
        for s in slots:
            ctx.mesh_set_vertices(new[s], object_slot=s)
        osc, oms = _two_cats_oracle(oracle, cat_golden, meshes, mat, {s: new[s] for s in slots})
        _against_oracle(ctx, osc, slots)
        # the synthetic union above the two roots: one float step wider than its children, as an upload makes it
        want, fresh = _fresh(spheres, [_as_upload(d, oms[d["object_slot"]]) for d in meshes])
        fresh.close()
        assert ctx.layout_hash() == want, slots
    with pytest.raises(rt.RtError) as e:                                # the plain entry names no mesh of several
        ctx.mesh_set_vertices(new[A])
    assert e.value.code == -5
    ctx.scene_upload([], [dict(m, object_slot=j) for j, m in enumerate(meshes)])   # the rays: the meshes alone, A at 0, B at 1
    ctx.mesh_set_vertices(new[A], object_slot=0)
    ctx.mesh_set_vertices(new[B], object_slot=1)
    _, oms = _two_cats_oracle(oracle, cat_golden, meshes, mat, new)
    _check_rays(ctx, oracle, [oms[A], oms[B]], 72)


# ------------------------------------------------------------------------------------------------------------------------ 3: against refit_kernel

def _same_state(a, b, b_frame=2):
    assert a.layout_hash() == b.layout_hash()
    fa, fb = a.render(_params(b_frame)), b.render(_params(b_frame))
    np.testing.assert_array_equal(fa.view(np.uint32), fb.view(np.uint32))
    assert fa[..., 3].sum() > 0


def test_set_vertices_equals_transform_and_its_one_workgroup_refit(ctx, ctx2, oracle, cat_golden):
    """context A: rt_mesh_transform (transform_kernel + refit_kernel); context B: the oracle's transformed vertices (pinned to the device's, bit for bit) through
    rt_mesh_set_vertices (the climb); a third context under RT_REFIT_WIDE=0 sends the new entry through refit_kernel as well"""
    serial = _context(RT_REFIT_WIDE="0")
    try:
        d = _cat_record(cat_golden)
        spheres = rt.scenes.spheres("cpu")
        moved = oracle.Mesh.from_arrays(d["vertices"], _tris(d)).transform(R1, T1).vertices
        for c in (ctx, ctx2, serial):
            c.scene_upload(spheres, d)
        ctx.mesh_transform(R1, T1)
        ctx2.mesh_set_vertices(moved)
        serial.mesh_set_vertices(moved)
        _same_state(ctx, ctx2)
        _same_state(ctx, serial)
        # two_cats, one mesh at a time: the synthetic union is widened by both refits alike
        sp2, meshes, _ = _two_cats(cat_golden)
        by_slot = {m["object_slot"]: m for m in meshes}
        for slot, (R, T) in ((A, (R1, T1)), (B, (R2, T2))):
            mv = oracle.Mesh.from_arrays(by_slot[slot]["vertices"], _tris(by_slot[slot])).transform(R, T).vertices
            for c in (ctx, ctx2, serial):
                c.scene_upload(sp2, meshes)
            ctx.mesh_transform(R, T, object_slot=slot)
            ctx2.mesh_set_vertices(mv, object_slot=slot)
            serial.mesh_set_vertices(mv, object_slot=slot)
            _same_state(ctx, ctx2)
            _same_state(ctx, serial)
        # a displaced grid of 8 192 triangles on its LBVH tree: the level and child arrays both refits read were made by the device-side install
        v, t = displaced_grid(65)
        first = hostlib.build_mesh(v, t, albedo=rt.scenes.CAT_ALBEDO, object_slot=SLOT)
        mv = oracle.Mesh.from_arrays(v, _tris(first)).transform(R1, T1).vertices
        for c in (ctx, ctx2, serial):
            c.scene_upload(spheres, first)
            c.mesh_rebuild(len(t), mode="lbvh")
            assert c.build_stats()["install_on_device"] == 1
        ctx.mesh_transform(R1, T1)
        ctx2.mesh_set_vertices(mv)
        serial.mesh_set_vertices(mv)
        _same_state(ctx, ctx2)
        _same_state(ctx, serial)
        wv = _wave(v, axis=0, along=1, amp=0.2)                          # ... and a deformation of it, climb against refit_kernel
        ctx2.mesh_set_vertices(wv)
        serial.mesh_set_vertices(wv)
        _same_state(ctx2, serial)
    finally:
        serial.close()


# ------------------------------------------------------------------------------------------------------------------------ 4: tree shapes

def _signed_zero_faces(v):
    """every x >= 0 and every y <= 0, with vertices AT zero of both signs: -0 and +0 tie on the low x face and on the high y face of the root and of many leaves"""
    out = np.asarray(v, np.float32).copy()
    out[:, 0] = np.abs(out[:, 0]) + np.float32(0.25)
    out[:, 1] = -np.abs(out[:, 1]) - np.float32(0.25)
    k = np.arange(len(out))
    out[k % 5 == 0, 0] = np.float32(0.0)
    out[k % 10 == 0, 0] = np.float32(-0.0)
    out[k % 7 == 3, 1] = np.float32(-0.0)
    out[k % 14 == 3, 1] = np.float32(0.0)
    return out


def _shape(kind):
    """(vertices, triangles, deformed vertices, expected node count or None)"""
    rng = np.random.default_rng(90)
    if kind == "single_leaf":
        v, t = _synthetic_mesh("three_triangles", rng)
        return v, t, _wave(v), 1
    if kind == "two_leaves":
        v, t = _join(_soup(rng, 4, -12, -8, 2.0), _soup(rng, 4, 8, 12, 2.0))
        return v, t, _wave(v, amp=0.1), 3
    if kind in ("deep_strip", "geometric_chain"):
        v, t = _synthetic_mesh(kind, rng)
        return v, t, _wave(v, axis=0, along=2, amp=0.05), None
    if kind == "leaf_of_5000":
        v, t, _ = _big_leaf_mesh(5000, 6000)
        return v, t, _wave(v, amp=0.03), None
    if kind == "signed_zero_faces":
        v, t = _soup(rng, 300, -10, 10, 1.5)
        return v, t, _signed_zero_faces(v), None
    if kind == "flat":
        v, t = _soup(rng, 300, -12, 12, 2.0)
        vn = v.copy()
        vn[:, 2] = np.float32(3.0)
        return v, t, vn, None
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["single_leaf", "two_leaves", "deep_strip", "geometric_chain", "leaf_of_5000", "signed_zero_faces", "flat"])
def test_tree_shapes(ctx, oracle, kind):
    """root = leaf (no climb), one climb step, climbs far longer than a wave, one lane folding 15 000 corners, -0 / +0 on one face, zero half extents: the layout of a
    fresh upload of the oracle's refit, and a frame"""
    v, t, vn, n_nodes = _shape(kind)
    d = hostlib.build_mesh(v, t, albedo=rt.scenes.CAT_ALBEDO, object_slot=SLOT)
    arr = np.asarray(d["bvh_arr10"], np.float32).reshape(-1, 10)
    if n_nodes is not None:
        assert len(arr) == n_nodes
    if kind == "leaf_of_5000":
        leaves = arr[arr[:, 0] < 0]
        assert (leaves[:, 9] - leaves[:, 8]).max() == 5000
    spheres = rt.scenes.spheres("cpu")
    ctx.scene_upload(spheres, d)
    ctx.mesh_set_vertices(vn)
    om = _refitted(oracle, d, vn)
    box = om.bvh_array()
    if kind == "signed_zero_faces":
        assert box[0, 2] == 0 and box[0, 6] == 0                        # the root's low x and high y faces sit at zero
        assert len({np.signbit(b) for b in box[:, 2][box[:, 2] == 0]} | {np.signbit(b) for b in box[:, 6][box[:, 6] == 0]}) == 2   # and both signs occur among the boxes
    if kind == "flat":
        assert (box[:, 4] == box[:, 7]).all()
    want, fresh = _fresh(spheres, _as_upload(d, om))
    fresh.close()
    assert ctx.layout_hash() == want
    osc = oracle.Scene.preset("cpu", om)
    for b in (0, 2):
        exp, _, cnt = osc.render(W, H, 1, b, want_rgb8=False)
        _frames_equal(ctx.render(_params(b)), exp)
    work = ctx.count_work(_params(2))
    assert work["rays"] == cnt["rays"] and work["tri_tests"] == cnt["tri_tests"]


# ------------------------------------------------------------------------------------------------------------------------ 5: determinism

def test_the_same_call_twice_and_in_a_second_context(ctx, ctx2, cat_golden):
    spheres, meshes, _ = _two_cats(cat_golden)
    by_slot = {d["object_slot"]: d for d in meshes}
    va, vb = _wave(by_slot[A]["vertices"]), _wave(by_slot[B]["vertices"], axis=2, along=0)
    hashes = []
    for c in (ctx, ctx2):
        c.scene_upload(spheres, meshes)
        c.mesh_set_vertices(va, object_slot=A)
        c.mesh_set_vertices(vb, object_slot=B)
        hashes.append(c.layout_hash())
    for _ in range(3):                                                   # the counters are zeroed again; no box depends on which sibling arrived second
        ctx.mesh_set_vertices(vb, object_slot=B)
        hashes.append(ctx.layout_hash())
    assert all(h == hashes[0] for h in hashes), hashes
    assert hashes[0]["pairs"] != 0


# ------------------------------------------------------------------------------------------------------------------------ 6: the caches of a still view

def test_the_caches_are_emptied_and_refilled(cat_golden):
    on, off = _context(), _context(RT_FIRST_HIT_CACHE="0")
    try:
        d = _cat_record(cat_golden)
        vn = _wave(d["vertices"])
        p = _params(2, w=64, h=48)
        for c in (on, off):
            c.scene_upload(rt.scenes.spheres("cpu"), d)

        def frame():
            before = on.first_hit_cache_counts()
            got = on.render(p)
            after = on.first_hit_cache_counts()
            np.testing.assert_array_equal(got.view(np.uint32), off.render(p).view(np.uint32))   # word for word the frame of a context without the cache
            return got, {k: after[k] - before[k] for k in after}

        parts = None
        f0, d0 = frame()
        parts = on.stats()["parts"]
        assert d0["filled"] == parts and d0["skipped"] == 0
        _, d1 = frame()
        assert d1["skipped"] == parts and d1["filled"] == 0
        for c in (on, off):
            c.mesh_set_vertices(vn)
        f2, d2 = frame()
        assert d2["filled"] == parts and d2["skipped"] == 0 and d2["key_misses"] >= 1, d2
        assert (f2[..., :3] != f0[..., :3]).any()
        f3, d3 = frame()
        assert d3["skipped"] == parts and d3["filled"] == 0 and d3["key_misses"] == 0, d3
        np.testing.assert_array_equal(f3.view(np.uint32), f2.view(np.uint32))
        assert off.first_hit_cache_counts()["skipped"] == 0
    finally:
        on.close()
        off.close()


# ------------------------------------------------------------------------------------------------------------------------ 7: what is kept

def test_texture_uvs_and_normals_are_kept(ctx, oracle, cat_golden):
    """a smooth, textured, previously moved mesh: after set_vertices and the new normals its frame is that of a fresh upload of the deformed mesh given the same
    texture, UVs and normals; without the texture it meets the oracle as test_smooth_normals_on_one_mesh compares them"""
    rng = np.random.default_rng(17)
    d = _cat_record(cat_golden)
    tv = _tris(d)
    spheres = rt.scenes.spheres("cpu")
    vn = _wave(d["vertices"])
    t_obj = np.asarray(cat_golden["tri_obj_order"])
    n_old, n_new = _vertex_normals(d["vertices"], t_obj), _vertex_normals(vn, t_obj)
    uv = (rng.random((3 * len(tv), 2)) * 2 - 0.5).astype(np.float32)
    uvidx = np.arange(3 * len(tv), dtype=np.int32).reshape(-1, 3)
    px = rng.integers(0, 256, size=(23, 37, 3), dtype=np.uint8)
    ctx.scene_upload(spheres, d)
    ctx.mesh_transform(R1, T1)
    ctx.mesh_set_normals(n_old, tv)
    ctx.mesh_set_texture(uv, uvidx, px, filter="bilinear")
    ctx.mesh_set_vertices(vn)
    ctx.mesh_set_normals(n_new, tv)
    om = _refitted(oracle, d, vn)
    want, fresh = _fresh(spheres, _as_upload(d, om))
    try:
        fresh.mesh_set_normals(n_new, tv)
        fresh.mesh_set_texture(uv, uvidx, px, filter="bilinear")
        assert ctx.layout_hash() == want
        for b in (0, 2):
            np.testing.assert_array_equal(ctx.render(_params(b)).view(np.uint32), fresh.render(_params(b)).view(np.uint32))
        textured = ctx.render(_params(0))
    finally:
        fresh.close()
    ctx.mesh_set_texture(None, None, None)
    om.set_normals(n_new, tv)
    osc = oracle.Scene.preset("cpu", om)
    exp0, _, _ = osc.render(W, H, 1, 0, want_rgb8=False)
    got0 = ctx.render(_params(0))
    assert values_equal(got0[..., :3], exp0[..., :3]).all()
    np.testing.assert_array_equal(got0[..., 3], exp0[..., 3])
    assert (got0[..., :3] != textured[..., :3]).any()                   # (the texture was in the frames compared above)
    exp2, _, _ = osc.render(W, H, 2, 2, want_rgb8=False)
    got2 = ctx.render(_params(2, n=2))
    assert linf(oracle, got2, exp2) <= TOL
    np.testing.assert_array_equal(got2[..., 3], exp2[..., 3])


@pytest.mark.parametrize("mode", ["reference", "lbvh"])
def test_rebuild_after_set_vertices(ctx, ctx2, oracle, cat_golden, mode):
    d = _cat_record(cat_golden)
    spheres = rt.scenes.spheres("cpu")
    vn = _wave(d["vertices"], amp=0.1)
    ctx.scene_upload(spheres, d)
    ctx.mesh_set_vertices(vn)
    ctx2.scene_upload(spheres, _as_upload(d, _refitted(oracle, d, vn)))
    nt = len(_tris(d))
    (arr, order), (arr2, order2) = ctx.mesh_rebuild(nt, mode), ctx2.mesh_rebuild(nt, mode)
    assert len(arr) > 1
    np.testing.assert_array_equal(arr.view(np.uint32), arr2.view(np.uint32))
    np.testing.assert_array_equal(order, order2)
    _same_state(ctx, ctx2)


# ------------------------------------------------------------------------------------------------------------------------ 8: host and device entry

@pytest.mark.parametrize("stride", [3, 4])
def test_device_entry_equals_host_entry(ctx, ctx2, cat_golden, stride):
    import torch
    spheres, meshes, _ = _two_cats(cat_golden)
    by_slot = {d["object_slot"]: d for d in meshes}
    vn = _wave(by_slot[B]["vertices"], axis=2, along=1)
    rec = np.full((len(vn), stride), 7.5, np.float32)                   # (the fourth float of an xyzw record is never read into the scene)
    rec[:, :3] = vn
    dev = torch.from_numpy(rec).to("cuda")
    torch.cuda.synchronize()
    for c in (ctx, ctx2):
        c.scene_upload(spheres, meshes)
    ctx.mesh_set_vertices(vn, object_slot=B)
    ctx2.mesh_set_vertices(device_ptr=dev.data_ptr(), stride=stride, n_vertices=len(vn), object_slot=B)
    _same_state(ctx, ctx2)
    # object_slot -1 of the device entry: the scene's one mesh
    d = _cat_record(cat_golden)
    v1 = _wave(d["vertices"])
    rec = np.zeros((len(v1), stride), np.float32)
    rec[:, :3] = v1
    dev = torch.from_numpy(rec).to("cuda")
    torch.cuda.synchronize()
    for c in (ctx, ctx2):
        c.scene_upload(rt.scenes.spheres("cpu"), d)
    ctx.mesh_set_vertices(v1)
    ctx2.mesh_set_vertices(device_ptr=dev.data_ptr(), stride=stride, n_vertices=len(v1))
    _same_state(ctx, ctx2)


# ------------------------------------------------------------------------------------------------------------------------ 9: refusals

def test_refusals_leave_the_scene_untouched(ctx, cat_golden):
    import torch
    fresh = rt.Context(0)
    try:
        with pytest.raises(rt.RtError) as e:                            # before any upload
            fresh.mesh_set_vertices(np.zeros((3, 3), np.float32))
        assert e.value.code == -4
        with pytest.raises(rt.RtError) as e:
            fresh.mesh_set_vertices(np.zeros((3, 3), np.float32), object_slot=0)
        assert e.value.code == -4
    finally:
        fresh.close()
    spheres, meshes, _ = _two_cats(cat_golden)
    empty = dict(vertices=np.zeros((0, 3), np.float32), indices=np.zeros((0, 10), np.int32), bvh_arr10=np.zeros((0, 10), np.float32), object_slot=8)
    ctx.scene_upload(spheres, meshes + [empty])
    h0, f0 = ctx.layout_hash(), ctx.render(_params(1))
    va = _wave(meshes[0]["vertices"])
    nv = len(va)
    dev = torch.from_numpy(np.ascontiguousarray(va)).to("cuda")
    torch.cuda.synchronize()
    L, hnd = ctx._L, ctx._h
    fp = va.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    refused = [lambda: L.rt_mesh_set_vertices_of(hnd, A, None, nv),                                  # a NULL pointer
               lambda: L.rt_mesh_set_vertices_device(hnd, A, None, 3, nv),
               lambda: L.rt_mesh_set_vertices_of(hnd, A, fp, nv - 1),                                # a count that is not the mesh's
               lambda: L.rt_mesh_set_vertices_of(hnd, A, fp, nv + 1),
               lambda: L.rt_mesh_set_vertices_device(hnd, A, dev.data_ptr(), 3, nv - 1),
               lambda: L.rt_mesh_set_vertices_device(hnd, A, dev.data_ptr(), 2, nv),                 # a stride other than 3 or 4
               lambda: L.rt_mesh_set_vertices_device(hnd, A, dev.data_ptr(), 5, nv),
               lambda: L.rt_mesh_set_vertices_device(hnd, A, dev.data_ptr(), 0, nv)]
    for slot in (0, 5, -1, 9, 16):                                      # walls at 0 and 5; 9 objects in all
        refused.append(lambda slot=slot: L.rt_mesh_set_vertices_of(hnd, slot, fp, nv))
        if slot != -1:                                                   # (-1 of the device entry means the one mesh: refused on this forest as the plain entry is)
            refused.append(lambda slot=slot: L.rt_mesh_set_vertices_device(hnd, slot, dev.data_ptr(), 3, nv))
    for k, call in enumerate(refused):
        assert call() == -1, k
    assert L.rt_mesh_set_vertices(hnd, fp, nv) == -5                     # several meshes: the plain entry and slot -1 of the device entry name none
    assert L.rt_mesh_set_vertices_device(hnd, -1, dev.data_ptr(), 3, nv) == -5
    ctx.mesh_set_vertices(np.zeros((0, 3), np.float32), object_slot=8)   # a mesh without triangles: accepted, nothing happens
    assert ctx.layout_hash() == h0
    np.testing.assert_array_equal(ctx.render(_params(1)).view(np.uint32), f0.view(np.uint32))
    ctx.mesh_set_vertices(va, object_slot=A)                             # (and the call that is not refused does change both)
    assert ctx.layout_hash() != h0
