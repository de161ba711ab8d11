"""Vertex normals computed on the device and the previous shading normals of a smooth deforming mesh (rt_mesh_compute_normals[_of], rt_mesh_get_vertex_normals,
rt_mesh_snapshot_normals, rt_mesh_normal_snapshot_mask, the third form of rt_render_aov_motion's close kernel).  -m gpu.

Every comparison is bit for bit on uint32 views.  The vertex normals are held to the numpy model of tests/normals_model.py (the reference has no normal computation);
what the mesh then shades like is held to a SECOND context given mesh_set_normals(the model's normals, the triangles' vertex indices) -- the path the older tests hold to
the oracle; the previous-frame planes to tests/normals_model.py on top of tests/motion_model.py; the accumulation to tests/temporal_model.py.  Frames are 96 x 64 and
67 x 45 (a ragged last workgroup) and 1 x 1."""
import ctypes

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi, hostlib

from . import material_scenes as ms
from . import motion_model as mm
from . import normals_model as nm
from . import still_view as sv
from . import temporal_model as tm
from .test_normals_model import SEQ_H, SEQ_W, SLOT, TETRA_T, TETRA_V, kept, sequence_planes

pytestmark = pytest.mark.gpu

A, B = 3, 7                                                             # the two cats' object slots in two_cats
SIZES = ((96, 64), (67, 45))
VARIANTS = ("auto", "wavefront", "path")
R1 = np.float32([[0.9553365, 0, 0.29552022], [0, 1, 0], [-0.29552022, 0, 0.9553365]])
T1 = np.float32([0.5, 0.25, -0.5])


@pytest.fixture(scope="module")
def ctx():
    c_ = rt.Context(0)
    yield c_
    c_.close()


@pytest.fixture(scope="module")
def ctx2():
    c_ = rt.Context(0)
    yield c_
    c_.close()


def _bits_equal(a, b, msg=""):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, msg
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=msg)


def _params(w, h, b=0, variant="auto", **kw):
    return rt.make_params(w, h, 1, b, variant=variant, **dict(rt.scenes.CPU_LAUNCHER, **kw))


def _cat_record(cat_golden, slot=SLOT):
    return dict(vertices=np.asarray(cat_golden["vertices"], np.float32), indices=cat_golden["tri_bvh_order"], bvh_arr10=cat_golden["bvh_arr10"],
                albedo=rt.scenes.CAT_ALBEDO, object_slot=slot)


def _tris(d):
    return np.ascontiguousarray(np.asarray(d["indices"])[:, :3], np.int32)


def _refitted(oracle, d, v, material=None):
    m = oracle.Mesh.from_arrays(v, _tris(d), albedo=tuple(d.get("albedo", (0.25, 0.25, 0.25))))
    if material:
        m.set_material(*material)
    return m.set_bvh(np.asarray(d["bvh_arr10"], np.float32).reshape(-1, 10), None).refit()


def _same_pictures(c, ref, sizes=SIZES, tag="", frames=True, variants=VARIANTS):
    """the three planes and whole frames (b = 0 and 2, three pipelines, .w included) of context c are those of context ref"""
    for w, h in sizes:
        _bits_equal(c.render_aov(_params(w, h)), ref.render_aov(_params(w, h)), f"{tag}: planes at {w} x {h}")
        if not frames:
            continue
        for b in (0, 2):
            for variant in variants:
                p = _params(w, h, b, variant, seed=3)
                _bits_equal(c.render(p), ref.render(p), f"{tag}: frame {w} x {h}, b = {b}, {variant}")


def _two_cats(cat_golden):
    spheres, meshes = ms.capi_scene("two_cats", cat_golden["vertices"], cat_golden["tri_obj_order"])
    mat = {pos: o[3:6] for pos, o in enumerate(ms.describe("two_cats", cat_golden["vertices"])) if o[0] == "mesh"}
    return spheres, meshes, {m["object_slot"]: m for m in meshes}, mat


# ---------------------------------------------------------------------------------------------------------------- vertex normals against the model

def test_cat_normals_are_the_models_bits_and_shade_as_set_normals(ctx, ctx2, cat_golden):
    import torch
    d = _cat_record(cat_golden)
    v0, t = d["vertices"], _tris(d)
    assert len(v0) == 2247
    for c in (ctx, ctx2):
        c.scene_upload(rt.scenes.spheres("cpu"), d)
    flat = ctx.render_aov(_params(*SIZES[0]))
    ctx.mesh_compute_normals()
    vn0 = nm.vertex_normals(v0, t)
    _bits_equal(ctx.mesh_vertex_normals(), vn0, "the uploaded shape: all 2 247 vertices")
    ctx2.mesh_set_normals(vn0, t)
    _same_pictures(ctx, ctx2, tag="uploaded shape")
    assert (ctx.render_aov(_params(*SIZES[0]))[0] != flat[0]).any()     # (the mesh does shade smoothly now)
    # new vertices from the host
    v1 = mm.sine_deform(v0, 1)
    ctx.mesh_set_vertices(v1)
    ctx.mesh_compute_normals()
    vn1 = nm.vertex_normals(v1, t)
    _bits_equal(ctx.mesh_vertex_normals(), vn1, "deformed from the host")
    assert (vn1 != vn0).any()
    ctx2.mesh_set_vertices(v1)
    ctx2.mesh_set_normals(vn1, t)
    _same_pictures(ctx, ctx2, tag="deformed from the host")
    # ... and from device memory, with no host wait between the two calls
    v2 = mm.sine_deform(v0, 2)
    dev = torch.from_numpy(np.ascontiguousarray(v2)).to("cuda")
    torch.cuda.synchronize()
    ctx.mesh_set_vertices(device_ptr=dev.data_ptr(), stride=3, n_vertices=len(v2))
    ctx.mesh_compute_normals()
    vn2 = nm.vertex_normals(v2, t)
    _bits_equal(ctx.mesh_vertex_normals(), vn2, "deformed from device memory")
    ctx2.mesh_set_vertices(v2)
    ctx2.mesh_set_normals(vn2, t)
    _same_pictures(ctx, ctx2, sizes=SIZES[1:], tag="deformed from device memory")
    # the object slot of the one mesh names the same mesh
    _bits_equal(ctx.mesh_vertex_normals(object_slot=SLOT), vn2)
    ctx.mesh_compute_normals(object_slot=SLOT)
    _bits_equal(ctx.mesh_vertex_normals(), vn2)


def test_twice_and_in_a_second_context_the_same_bits(ctx, ctx2, cat_golden):
    d = _cat_record(cat_golden)
    v1 = mm.sine_deform(d["vertices"], 3)
    got = []
    for c in (ctx, ctx2):
        c.scene_upload(rt.scenes.spheres("cpu"), d)
        c.mesh_set_vertices(v1)
        c.mesh_compute_normals()
        got.append((c.mesh_vertex_normals(), c.render_aov(_params(*SIZES[1]))))
    for _ in range(2):
        ctx.mesh_compute_normals()
        got.append((ctx.mesh_vertex_normals(), ctx.render_aov(_params(*SIZES[1]))))
    for n, planes in got[1:]:
        _bits_equal(n, got[0][0])
        _bits_equal(planes, got[0][1])
    _bits_equal(got[0][0], nm.vertex_normals(v1, _tris(d)))


def test_two_cats_one_mesh_at_a_time_then_both(ctx, ctx2, cat_golden):
    w, h = SIZES[0]
    spheres, meshes, by_slot, _ = _two_cats(cat_golden)
    for c in (ctx, ctx2):
        c.scene_upload(spheres, meshes)
    ta, tb = _tris(by_slot[A]), _tris(by_slot[B])
    # B shades with an array of the caller's that no computation would give: its range of the normals must survive a computation on A
    own = np.tile(np.float32([[0.6, 0.0, 0.8]]), (len(by_slot[B]["vertices"]), 1))
    for c in (ctx, ctx2):
        c.mesh_set_normals(own, tb, object_slot=B)
    before = ctx.render_aov(_params(w, h))
    ctx.mesh_compute_normals(object_slot=A)
    vna = nm.vertex_normals(by_slot[A]["vertices"], ta)
    _bits_equal(ctx.mesh_vertex_normals(object_slot=A), vna)
    ctx2.mesh_set_normals(vna, ta, object_slot=A)
    _same_pictures(ctx, ctx2, sizes=SIZES[:1], tag="A computed, B the caller's")
    after = ctx.render_aov(_params(w, h))
    on_b = before[0, ..., 3] == B
    assert on_b.sum() > 50 and (before[0, ..., 3] == A).sum() > 100
    _bits_equal(after[:, on_b], before[:, on_b], "B's pixels are what they were")
    assert (after[0][before[0, ..., 3] == A] != before[0][before[0, ..., 3] == A]).any()
    with pytest.raises(rt.RtError) as e:                                # B was never computed
        ctx.mesh_vertex_normals(object_slot=B)
    assert e.value.code == -1
    # then both
    ctx.mesh_compute_normals(object_slot=B)
    vnb = nm.vertex_normals(by_slot[B]["vertices"], tb)
    _bits_equal(ctx.mesh_vertex_normals(object_slot=B), vnb)
    _bits_equal(ctx.mesh_vertex_normals(object_slot=A), vna)
    ctx2.mesh_set_normals(vnb, tb, object_slot=B)
    _same_pictures(ctx, ctx2, sizes=SIZES[:1], tag="both computed")
    # the plain entry names no mesh of a forest
    h0, f0 = ctx.layout_hash(), ctx.render(_params(w, h, 2))
    with pytest.raises(rt.RtError) as e:
        ctx.mesh_compute_normals()
    assert e.value.code == -5
    with pytest.raises(rt.RtError) as e:
        ctx.mesh_vertex_normals(n_vertices=len(vna))
    assert e.value.code == -5
    assert ctx.layout_hash() == h0
    _bits_equal(ctx.render(_params(w, h, 2)), f0)


# ---------------------------------------------------------------------------------------------------------------- small shapes

def _grid(n):
    """n x n vertices of a bumpy sheet, 2 (n - 1)^2 triangles"""
    k = np.arange(n)
    x, y = np.meshgrid(k, k, indexing="xy")
    v = np.stack([x * 0.5 - 4, y * 0.5 - 4, 20 + np.sin(x * 0.9) * np.cos(y * 0.7)], -1).reshape(-1, 3).astype(np.float32)
    i = (y[:-1, :-1] * n + x[:-1, :-1]).reshape(-1)
    t = np.concatenate([np.stack([i, i + 1, i + n], -1), np.stack([i + 1, i + n + 1, i + n], -1)]).astype(np.int32)
    return v, t


def _shape(kind):
    base = np.float32([[-3, -2, 20], [4, -1, 21], [-2, 5, 22], [5, 6, 19]])
    if kind == "one_triangle":
        return base[:3], np.int32([[0, 1, 2]])
    if kind == "quad":
        return base, np.int32([[0, 1, 2], [1, 3, 2]])
    if kind == "tetrahedron":
        return (TETRA_V + np.float32([-2, -2, 18])).astype(np.float32), TETRA_T
    if kind == "fan_of_5000":
        v, t = nm.fan()
        return (v * np.float32(2.0 ** -7) + np.float32([0, 0, 20])).astype(np.float32), t   # radii of 1/128 to 8 in front of the camera
    if kind == "repeated_index":
        return base, np.int32([[0, 1, 2], [3, 3, 1], [1, 3, 2]])
    if kind == "zero_area":
        v = np.concatenate([base, [[1, 2, 21.5]], [[1, 2, 21.5]]]).astype(np.float32)   # vertices 4 and 5 coincide: (2, 4, 5) has no area
        return v, np.int32([[0, 1, 2], [2, 4, 5], [1, 3, 2], [1, 4, 3]])
    if kind == "cancelling_faces":
        v = np.concatenate([base[:3], base[1:3]]).astype(np.float32)     # (0, 1, 2) and (0, 4, 3): the same triangle with the other winding, on vertices of its own
        return v, np.int32([[0, 1, 2], [0, 4, 3]])
    if kind == "minus_zero":
        # (2, 0, 3): e1 = (0, -1, 0), e2 = (1, 0, 0), N.x = -1 * 0 - 0 * 0 = -0: vertex 2 keeps it (its only face), vertices 0 and 3 add a +0 to it
        return np.float32([[0, 0, 20], [1, 0, 20], [0, 1, 20], [1, 1, 20]]), np.int32([[2, 0, 3], [0, 1, 3]])
    if kind == "nan_vertex":
        v = np.float32([[0, 0, 20], [1, 0, 20], [0, 1, 20], [np.nan, 0, 20], [1, 1, 20], [2, 1, 21]])
        return v, np.int32([[0, 1, 2], [1, 3, 4], [2, 1, 4], [4, 1, 5]])
    if kind == "nv_289":
        return _grid(17)                                                 # 289 vertices: one whole workgroup and a ragged one
    if kind == "nv_1":
        return np.float32([[0, 0, 20]]), np.int32([[0, 0, 0]])
    raise ValueError(kind)


SHAPES = ["one_triangle", "quad", "tetrahedron", "fan_of_5000", "repeated_index", "zero_area", "cancelling_faces", "minus_zero", "nan_vertex", "nv_289", "nv_1"]


@pytest.mark.parametrize("kind", SHAPES)
def test_small_shapes(ctx, ctx2, kind):
    v, t = _shape(kind)
    d = hostlib.build_mesh(v, t, albedo=(0.5, 0.5, 0.5), object_slot=SLOT)
    tu = _tris(d)                                                        # the uploaded order: the order of the sums
    assert len(tu) == len(t)
    ctx.scene_upload(rt.scenes.spheres("cpu"), d)
    ctx.mesh_compute_normals()
    exp = nm.vertex_normals(d["vertices"], tu)
    got = ctx.mesh_vertex_normals()
    _bits_equal(got, exp, kind)
    assert np.isfinite(got).all()                                        # zeros, never a NaN, where there is no normal
    if kind == "fan_of_5000":
        rev = nm.vertex_normals(d["vertices"], tu, order=np.arange(len(tu))[::-1])
        assert (rev[0].view(np.uint32) != exp[0].view(np.uint32)).any() and (got[0] != 0).any()   # the hub: the other order has other bits
    if kind == "cancelling_faces":
        np.testing.assert_array_equal(got[0], 0)
        assert (got[1:] != 0).any(1).all()
    if kind == "nan_vertex":
        np.testing.assert_array_equal(got[[1, 3, 4]], 0)
        assert (got[[0, 2, 5]] != 0).any(1).all()
        return                                                           # (no frame of a mesh with a NaN corner)
    if kind == "nv_1":
        np.testing.assert_array_equal(got, 0)
    if kind == "minus_zero":
        s, _ = nm.vertex_sums(d["vertices"], tu)
        assert np.signbit(s).any() and (s == 0).any()
        np.testing.assert_array_equal(np.signbit(got), np.signbit(exp))
    # what a pixel interpolates from them is what it interpolates from the model's (a zero corner normal drops out)
    ctx2.scene_upload(rt.scenes.spheres("cpu"), d)
    ctx2.mesh_set_normals(exp, tu)
    _same_pictures(ctx, ctx2, sizes=SIZES[:1], tag=kind, frames=kind in ("tetrahedron", "cancelling_faces", "nv_289"))
    if kind in ("quad", "cancelling_faces", "nv_289"):
        assert (ctx.render_aov(_params(*SIZES[0]))[0, ..., 3] == SLOT).sum() > 20   # (the shape is in the picture)


# ---------------------------------------------------------------------------------------------------------------- the other mesh operations

@pytest.mark.parametrize("mode", ["reference", "lbvh"])
def test_rebuild_carries_the_normals_and_a_fresh_computation_follows_the_new_order(cat_golden, mode):
    host = sv.context(RT_LBVH_HOST_INSTALL="1")
    ref = sv.context(RT_LBVH_HOST_INSTALL="1")
    try:
        d = _cat_record(cat_golden)
        v1, t = mm.sine_deform(d["vertices"], 2), _tris(d)
        vn = nm.vertex_normals(v1, t)
        for c in (host, ref):
            c.scene_upload(rt.scenes.spheres("cpu"), d)
            c.mesh_set_vertices(v1)
        host.mesh_compute_normals()
        ref.mesh_set_normals(vn, t)
        (arr, order), (arr2, order2) = host.mesh_rebuild(len(t), mode), ref.mesh_rebuild(len(t), mode)
        np.testing.assert_array_equal(order, order2)
        assert host.build_stats()["install_on_device"] == 0
        _same_pictures(host, ref, tag="carried through the rebuild")     # carried as the caller's own normals are
        _bits_equal(host.mesh_vertex_normals(), vn)                      # (vertices keep their order)
        assert (order != np.arange(len(t))).any()
        t_new = t[order]                                                 # the order the rebuild reported: the mesh's own triangle order from now on
        host.mesh_compute_normals()
        vn_new = nm.vertex_normals(v1, t_new)
        _bits_equal(host.mesh_vertex_normals(), vn_new, "the model fed the reported order")
        ref.mesh_set_normals(vn_new, t_new)
        _same_pictures(host, ref, sizes=SIZES[1:], tag="computed after the rebuild")
    finally:
        host.close()
        ref.close()


def test_after_the_device_side_install_the_adjacency_is_fetched_again(ctx, ctx2, cat_golden):
    d = _cat_record(cat_golden)
    t = _tris(d)
    for c in (ctx, ctx2):
        c.scene_upload(rt.scenes.spheres("cpu"), d)
    ctx.mesh_compute_normals()                                           # an adjacency of the OLD order exists ...
    ctx.mesh_set_normals(None, None)                                     # ... and the mesh is flat again: the install runs on the device
    (arr, order), _ = ctx.mesh_rebuild(len(t), "lbvh"), ctx2.mesh_rebuild(len(t), "lbvh")
    assert ctx.build_stats()["install_on_device"] == 1
    ctx.mesh_compute_normals()
    vn = nm.vertex_normals(d["vertices"], t[order])
    _bits_equal(ctx.mesh_vertex_normals(), vn)
    ctx2.mesh_set_normals(vn, t[order])
    _same_pictures(ctx, ctx2, sizes=SIZES[:1], tag="device-side install")


def test_transform_flat_again_replace_texture_and_uvs(ctx, ctx2, cat_golden):
    rng = np.random.default_rng(5)
    d = _cat_record(cat_golden)
    v, t = d["vertices"], _tris(d)
    uv = (rng.random((3 * len(t), 2)) * 2 - 0.5).astype(np.float32)
    uvidx = np.arange(3 * len(t), dtype=np.int32).reshape(-1, 3)
    px = rng.integers(0, 256, size=(23, 37, 3), dtype=np.uint8)
    for c in (ctx, ctx2):
        c.scene_upload(rt.scenes.spheres("cpu"), d)
    plain = ctx.render_aov(_params(*SIZES[0]))
    for c in (ctx, ctx2):
        c.mesh_set_texture(uv, uvidx, px, filter="bilinear")
    vn = nm.vertex_normals(v, t)
    ctx.mesh_compute_normals()
    ctx2.mesh_set_normals(vn, t)
    tex = ("auto", "wavefront")                                          # (the pipelines that take a textured mesh)
    _same_pictures(ctx, ctx2, sizes=SIZES[:1], tag="textured", variants=tex)   # texture and UVs are kept
    on = plain[0, ..., 3] == SLOT
    assert on.sum() > 150 and (ctx.render_aov(_params(*SIZES[0]))[2][on] != plain[2][on]).any()   # (the texture is in the planes compared above)
    # a transform rotates and translates them as it does the caller's
    for c in (ctx, ctx2):
        c.mesh_transform(R1, T1)
    _same_pictures(ctx, ctx2, sizes=SIZES[:1], tag="transformed", variants=tex)
    _bits_equal(ctx.mesh_vertex_normals(), vn, "the per-vertex array does not follow a transform")
    # flat again, and smooth again from the moved shape
    for c in (ctx, ctx2):
        c.mesh_set_normals(None, None, object_slot=SLOT)
    _same_pictures(ctx, ctx2, sizes=SIZES[:1], tag="flat again", frames=False)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]                                  # transform_kernel's arithmetic: products summed left to right, then the translation
    moved = np.stack([((R1[k, 0] * x + R1[k, 1] * y) + R1[k, 2] * z) + T1[k] for k in range(3)], -1)
    assert moved.dtype == np.float32
    ctx.mesh_compute_normals()
    got = ctx.mesh_vertex_normals()
    _bits_equal(got, nm.vertex_normals(moved, t), "the moved shape's normals")
    assert (got != vn).any()
    # the caller's own array replaces them
    own = np.tile(np.float32([[0.0, 0.6, 0.8]]), (len(v), 1))
    ctx.mesh_set_normals(own, t)
    ctx2.mesh_set_normals(own, t)
    _same_pictures(ctx, ctx2, sizes=SIZES[:1], tag="replaced", frames=False)
    for c in (ctx, ctx2):
        c.mesh_set_texture(None, None, None)


def test_the_shading_level_of_a_still_view_is_emptied(cat_golden):
    on, off = sv.context(), sv.context(RT_FIRST_HIT_CACHE="0", RT_FIRST_SHADOW_CACHE="0", RT_FIRST_SHADE_CACHE="0")
    try:
        sv.upload((on, off), cat_golden)
        p = sv.params()
        counts = lambda: (on.first_hit_cache_counts(), on.first_shadow_cache_counts(), on.first_shade_cache_counts())
        delta = lambda new, old: [{k: a[k] - b[k] for k in a} for a, b in zip(new, old)]
        for _ in range(5):                                               # a still view: the three levels fill and settle
            on.render(p)
        c0 = counts()
        flat = on.render(p)
        steady = delta(counts(), c0)
        assert steady[2]["resumed"] > 0 and all(s["key_misses"] == 0 and s["filled"] == 0 for s in steady), steady
        _bits_equal(flat, off.render(p))
        for c in (on, off):
            c.mesh_compute_normals()
        c1 = counts()
        smooth = on.render(p)
        hit, shadow, shade = delta(counts(), c1)
        assert hit["key_misses"] == 0 and hit["skipped"] > 0, hit       # the geometry did not change: the camera rays' hits are kept
        assert shadow["key_misses"] >= 1 and shadow["filled"] > 0 and shadow["skipped"] == 0, shadow
        assert shade["resumed"] == 0, shade
        _bits_equal(smooth, off.render(p))
        assert (smooth != flat).any()
        for _ in range(4):
            _bits_equal(on.render(p), smooth)
        c2 = counts()
        _bits_equal(on.render(p), smooth)
        assert delta(counts(), c2) == steady                             # ... and the view settles as before
        # a normal snapshot is nothing a render reads
        c3 = counts()
        on.mesh_snapshot_normals()
        on.mesh_snapshot_normals(keep=False)
        on.mesh_snapshot_normals(object_slot=SLOT)
        assert counts() == c3 and on.mesh_normal_snapshot_mask() == 1 << SLOT
        _bits_equal(on.render(p), smooth)
        assert delta(counts(), c3) == steady
    finally:
        on.close()
        off.close()


# ---------------------------------------------------------------------------------------------------------------- previous normals and the mask

def _check_prev(c, osc, w, h, snapshots, nsnap, motion=None, pose=None, tag=""):
    """one rt_render_aov_motion of the scene in use against rt_render_aov and the model -> (aov, prev, the trace)"""
    p = _params(w, h)
    aov, prev = c.render_aov_motion(p, pose=pose, motion=motion)
    _bits_equal(aov, c.render_aov(p, pose=pose), tag + ": the three planes are rt_render_aov's")
    cam = {} if pose is None else dict(cam=tuple(pose.position), fov=pose.fov, basis=rt.camera_basis(pose))
    meshes = {k: s["mesh"] for k, s in {**(snapshots or {}), **(nsnap or {})}.items()}
    tr = mm.trace(osc, w, h, meshes=meshes, **cam)
    _bits_equal(aov[:2], mm.planes(tr)[:2], tag + ": the model's own inputs")
    _bits_equal(prev, nm.previous_planes(tr, snapshots, motion, normal_snapshots=nsnap), tag + ": the previous-frame planes")
    return aov, prev, tr


@pytest.mark.parametrize("w,h", SIZES)
def test_previous_normals_of_the_deformed_smooth_cat(ctx, oracle, cat_golden, w, h):
    d = _cat_record(cat_golden)
    v0, t = d["vertices"], _tris(d)
    ctx.scene_upload(rt.scenes.spheres("cpu"), d)
    ctx.mesh_compute_normals()
    vn0 = nm.vertex_normals(v0, t)
    assert ctx.mesh_normal_snapshot_mask() == 0
    ctx.mesh_snapshot_vertices()
    ctx.mesh_snapshot_normals()
    assert ctx.mesh_normal_snapshot_mask() == 1 << SLOT and ctx.mesh_snapshot_mask() == 1 << SLOT
    v1 = mm.sine_deform(v0, 1)
    ctx.mesh_set_vertices(v1)
    ctx.mesh_compute_normals()
    vn1 = nm.vertex_normals(v1, t)
    om = _refitted(oracle, d, v1)
    om.set_normals(vn1, t)
    osc = oracle.Scene.preset("cpu", om)
    snap = {SLOT: dict(mesh=om, previous=v0, smooth=True)}
    ns = {SLOT: dict(mesh=om, normals=vn0, nidx=t)}
    aov, prev, tr = _check_prev(ctx, osc, w, h, snap, ns, tag="unposed")
    on = tr["id"] == SLOT
    assert on.sum() > 150
    assert (prev[0][on][:, :3] != aov[0][on][:, :3]).any(-1).mean() > 0.5          # N' is not N ...
    _bits_equal(prev[:, ~on], aov[:2][:, ~on])                                       # ... on the cat alone
    # the posed camera; a rigid table for everything else
    _check_prev(ctx, osc, w, h, snap, ns, pose=rt.make_pose((5.0, 3.0, 40.0), -0.4, 0.15, 1.2), tag="posed")
    motion = rt.static_motion()
    motion[:, 9:] = (0.25, -0.5, 0.125)
    motion[SLOT, :9] = R1.reshape(9)                                     # never read for the cat: both snapshots take precedence
    _, prev_m, _ = _check_prev(ctx, osc, w, h, snap, ns, motion=motion, tag="table")
    _bits_equal(prev_m[:, on], prev[:, on])
    # the normal snapshot alone: P' by the record, N' by the snapshot, ahead of the record's rotation
    ctx.mesh_snapshot_vertices(keep=False)
    _, prev_r, _ = _check_prev(ctx, osc, w, h, None, ns, motion=motion, tag="normal snapshot, rigid record")
    _bits_equal(prev_r[0][on], prev[0][on])
    assert (prev_r[1][on] != prev[1][on]).any()
    ctx.mesh_snapshot_vertices()                                         # (the current shape: P' = P from here on)
    # without the normal snapshot the planes are word for word what they were before the entry existed: N' = N
    ctx.mesh_snapshot_normals(keep=False)
    assert ctx.mesh_normal_snapshot_mask() == 0
    aov_o, prev_o, _ = _check_prev(ctx, osc, w, h, {SLOT: dict(mesh=om, previous=v1, smooth=True)}, None, tag="no normal snapshot")
    _bits_equal(prev_o[0][on], aov_o[0][on])


def test_two_cats_one_with_both_snapshots_one_moved_by_its_record(ctx, oracle, cat_golden):
    w, h = SIZES[0]
    spheres, meshes, by_slot, mat = _two_cats(cat_golden)
    ctx.scene_upload(spheres, meshes)
    ta = _tris(by_slot[A])
    va0 = by_slot[A]["vertices"]
    ctx.mesh_compute_normals(object_slot=A)
    vna0 = nm.vertex_normals(va0, ta)
    ctx.mesh_snapshot_vertices(object_slot=A)
    ctx.mesh_snapshot_normals()                                          # every SMOOTH mesh: A; B is flat and keeps its bit clear
    assert ctx.mesh_normal_snapshot_mask() == 1 << A
    ctx.mesh_snapshot_normals(object_slot=B)
    assert ctx.mesh_normal_snapshot_mask() == 1 << A
    va = mm.sine_deform(va0, 1)
    ctx.mesh_set_vertices(va, object_slot=A)
    ctx.mesh_compute_normals(object_slot=A)
    ctx.mesh_transform(R1, T1, object_slot=B)
    motion = rt.motion_from_mesh_transform(R1, T1, B)
    motion[A, 9:] = (9, 9, 9)                                            # never read: A holds a snapshot
    oma = _refitted(oracle, by_slot[A], va, mat[A])
    oma.set_normals(nm.vertex_normals(va, ta), ta)
    omb = _refitted(oracle, by_slot[B], by_slot[B]["vertices"], mat[B]).transform(R1, T1).refit()
    osc = oracle.Scene()
    for pos, o in enumerate(ms.describe("two_cats", cat_golden["vertices"])):
        if o[0] == "sphere":
            osc.add_sphere(o[1], o[2], o[3])
        else:
            osc.add_mesh(oma if pos == A else omb)
    aov, prev, tr = _check_prev(ctx, osc, w, h, {A: dict(mesh=oma, previous=va0, smooth=True)}, {A: dict(mesh=oma, normals=vna0, nidx=ta)}, motion=motion, tag="two cats")
    ids = aov[0, ..., 3]
    assert (ids == A).sum() > 100 and (ids == B).sum() > 50
    assert (prev[0][ids == A][:, :3] != aov[0][ids == A][:, :3]).any() and (prev[0][ids == B][:, :3] != aov[0][ids == B][:, :3]).any()


def test_host_form_device_form_rows_one_pixel_and_refusals(ctx, cat_golden):
    import torch
    w, h = SIZES[1]
    d = _cat_record(cat_golden)
    ctx.scene_upload(rt.scenes.spheres("cpu"), d)
    ctx.mesh_compute_normals()
    ctx.mesh_snapshot_vertices()
    ctx.mesh_snapshot_normals()
    ctx.mesh_set_vertices(mm.sine_deform(d["vertices"], 1))
    ctx.mesh_compute_normals()
    motion = rt.static_motion()
    motion[0, 9:] = (1, 2, 3)
    p = _params(w, h)
    exp, exp_prev = ctx.render_aov_motion(p, motion=motion)
    on = exp[0, ..., 3] == SLOT
    assert on.sum() > 100 and (exp_prev[0][on] != exp[0][on]).any()
    # interleaved rows and one pixel
    seen = np.zeros(h, bool)
    for rank in range(3):
        rows, idx = rt.interleaved_rows(h, 8, rank, 3)
        part, part_prev = ctx.render_aov_motion(p, rows=rows, motion=motion)
        _bits_equal(part, exp[:, idx])
        _bits_equal(part_prev, exp_prev[:, idx])
        seen[idx] = True
    assert seen.all()
    one, one_prev = ctx.render_aov_motion(_params(1, 1))
    assert one.shape == (3, 1, 1, 4) and one_prev.shape == (2, 1, 1, 4)
    # the device form, on a stream of the caller's and on the context's own
    st = torch.cuda.Stream()
    out = torch.full((3, h, w, 4), -7.0, dtype=torch.float32, device="cuda:0")
    prev = torch.full((2, h, w, 4), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.synchronize()
    ctx.render_aov_motion_device(p, out.data_ptr(), prev.data_ptr(), motion=motion, stream=st.cuda_stream)
    torch.cuda.synchronize()
    _bits_equal(out.cpu().numpy(), exp)
    _bits_equal(prev.cpu().numpy(), exp_prev)
    prev.fill_(-7.0)
    torch.cuda.synchronize()
    ctx.render_aov_motion_device(p, out.data_ptr(), prev.data_ptr(), motion=motion)
    ctx.synchronize()
    _bits_equal(prev.cpu().numpy(), exp_prev)
    # refusals: outputs untouched, masks, layout and frame as they were
    out.fill_(-7.0)
    prev.fill_(-7.0)
    torch.cuda.synchronize()
    masks = (ctx.mesh_snapshot_mask(), ctx.mesh_normal_snapshot_mask())
    h0, f0 = ctx.layout_hash(), ctx.render(_params(w, h, 2))
    ok = dict(params=p, out_ptr=out.data_ptr(), prev_ptr=prev.data_ptr(), motion=motion)
    for kw in (dict(prev_ptr=0), dict(out_ptr=0), dict(prev_ptr=out.data_ptr()), dict(params=_params(0, h)), dict(rows=_capi.Rows(h - 3, 8, 8, 1))):
        with pytest.raises(rt.RtError) as e:
            ctx.render_aov_motion_device(**dict(ok, **kw))
        assert e.value.code == -1, kw
    L, hnd = ctx._L, ctx._h
    nv = len(d["vertices"])
    buf = np.full((nv, 3), -7, np.float32)
    fp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    refused = [lambda: L.rt_mesh_snapshot_normals(hnd, SLOT, 2), lambda: L.rt_mesh_snapshot_normals(hnd, SLOT, -1),      # keep outside {0, 1}
               lambda: L.rt_mesh_snapshot_normals(hnd, 0, 1), lambda: L.rt_mesh_snapshot_normals(hnd, 99, 1), lambda: L.rt_mesh_snapshot_normals(hnd, -2, 1),
               lambda: L.rt_mesh_compute_normals_of(hnd, 0), lambda: L.rt_mesh_compute_normals_of(hnd, 99), lambda: L.rt_mesh_compute_normals_of(hnd, -1),
               lambda: L.rt_mesh_get_vertex_normals(hnd, SLOT, None, nv), lambda: L.rt_mesh_get_vertex_normals(hnd, SLOT, fp, nv - 1),
               lambda: L.rt_mesh_get_vertex_normals(hnd, -1, fp, nv + 1), lambda: L.rt_mesh_get_vertex_normals(hnd, 0, fp, nv),
               lambda: L.rt_mesh_normal_snapshot_mask(hnd, None)]
    for k, call in enumerate(refused):
        assert call() == -1, k
    ctx.synchronize()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and (prev.cpu().numpy() == -7.0).all() and (buf == -7).all()
    assert (ctx.mesh_snapshot_mask(), ctx.mesh_normal_snapshot_mask()) == masks
    assert ctx.layout_hash() == h0
    _bits_equal(ctx.render(_params(w, h, 2)), f0)
    again, again_prev = ctx.render_aov_motion(p, motion=motion)          # the context still works
    _bits_equal(again, exp)
    _bits_equal(again_prev, exp_prev)
    empty = rt.Context(0)                                                # no scene
    try:
        for call in (lambda: empty.mesh_compute_normals(), lambda: empty.mesh_compute_normals(object_slot=SLOT), lambda: empty.mesh_snapshot_normals(),
                     lambda: empty.mesh_snapshot_normals(object_slot=SLOT, keep=False), lambda: empty.mesh_vertex_normals(n_vertices=3)):
            with pytest.raises(rt.RtError) as e:
                call()
            assert e.value.code == -4                                    # RT_ERR_NO_SCENE
        assert empty.mesh_normal_snapshot_mask() == 0
        empty.scene_upload(rt.scenes.spheres("cpu"), d)
        with pytest.raises(rt.RtError) as e:                            # uploaded, never computed
            empty.mesh_vertex_normals()
        assert e.value.code == -1
    finally:
        empty.close()


def test_mask_life_cycle(cat_golden):
    c = sv.context(RT_LBVH_HOST_INSTALL="1")
    try:
        d = _cat_record(cat_golden)
        nt = len(_tris(d))
        bit = 1 << SLOT
        c.scene_upload(rt.scenes.spheres("cpu"), d)
        c.mesh_snapshot_normals()                                        # a flat mesh: a no-op, the bit stays clear
        c.mesh_snapshot_normals(object_slot=SLOT)
        assert c.mesh_normal_snapshot_mask() == 0
        c.mesh_compute_normals()
        c.mesh_snapshot_normals()
        c.mesh_snapshot_normals(object_slot=SLOT)                        # a second snapshot
        assert c.mesh_normal_snapshot_mask() == bit
        c.mesh_snapshot_normals(keep=False)
        assert c.mesh_normal_snapshot_mask() == 0
        for mode in ("reference", "lbvh"):                               # every rebuild clears the whole mask; the vertex snapshot survives
            c.mesh_snapshot_vertices()
            c.mesh_snapshot_normals()
            assert (c.mesh_snapshot_mask(), c.mesh_normal_snapshot_mask()) == (bit, bit)
            c.mesh_rebuild(nt, mode)
            assert (c.mesh_snapshot_mask(), c.mesh_normal_snapshot_mask()) == (bit, 0), mode
            aov, prev = c.render_aov_motion(_params(*SIZES[1]))          # N' = N again
            on = aov[0, ..., 3] == SLOT
            _bits_equal(prev[0][on], aov[0][on])
        c.mesh_snapshot_normals()
        c.mesh_set_normals(None, None)                                   # flat again under a snapshot: nothing reads it
        aov, prev = c.render_aov_motion(_params(*SIZES[1]))
        _bits_equal(prev[0], aov[0])
        c.mesh_compute_normals()
        c.mesh_snapshot_normals()
        assert c.mesh_normal_snapshot_mask() == bit
        c.scene_upload(rt.scenes.spheres("cpu"), d)                      # an upload clears both
        assert (c.mesh_snapshot_mask(), c.mesh_normal_snapshot_mask()) == (0, 0)
        with pytest.raises(rt.RtError):
            c.mesh_vertex_normals()
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------- a sequence that the feature decides

def test_the_rotating_cat_keeps_its_history_with_the_normal_snapshot(ctx, ctx2, oracle, cat_golden):
    """The smooth cat turned by 35 degrees a frame (cos = 0.819 < min_normal_dot = 0.9) through mesh_set_vertices, five one-sample frames.  ctx snapshots the normals,
    ctx2 does not.  Per frame both devices' planes and histories are the models' bit for bit; from frame 2 on strictly more cat pixels keep their history with the
    snapshot than without, and each side -- with, without, with only -- has at least 200 pixels (tests/test_normals_model.py asks the model alone the same)."""
    w, h = SEQ_W, SEQ_H
    seq = sequence_planes(oracle, cat_golden)
    d = _cat_record(cat_golden)
    state = {}
    for c, key in ((ctx, "with_"), (ctx2, "without")):
        c.scene_upload(rt.scenes.spheres("cpu"), d)
        c.mesh_compute_normals()
        p = _params(w, h, b=3, seed=60)
        color = c.render(p)
        aov, prev = c.render_aov_motion(p)
        _bits_equal(aov[:2], seq[0]["cur"][:2])
        hist = c.temporal_accumulate(color, prev, None, None, reproject=None)
        _bits_equal(hist, tm.accumulate(color, prev))
        state[key] = (aov, hist)
    for f in range(1, len(seq)):
        s = seq[f]
        cat = s["tr"]["id"] == SLOT
        n_kept = {}
        for c, key in ((ctx, "with_"), (ctx2, "without")):
            prev_aov, prev_hist = state[key]
            c.mesh_snapshot_vertices()
            if key == "with_":
                c.mesh_snapshot_normals()
            c.mesh_set_vertices(s["v"])
            c.mesh_compute_normals()
            _bits_equal(c.mesh_vertex_normals(), s["vn"], f"frame {f}: the vertex normals")
            p = _params(w, h, b=3, seed=60 + f)
            color = c.render(p)
            aov, prev = c.render_aov_motion(p)
            _bits_equal(aov[:2], s["cur"][:2], f"frame {f}, {key}: the current planes")
            _bits_equal(prev, s[key], f"frame {f}, {key}: the previous-frame planes")
            hist = c.temporal_accumulate(color, prev, prev_aov, prev_hist, reproject=rt.make_reproject())
            _bits_equal(hist, tm.accumulate(color, prev, prev_aov, prev_hist), f"frame {f}, {key}: the history")
            n_kept[key] = kept(hist, cat)
            state[key] = (aov, hist)
        kw, kwo = n_kept["with_"], n_kept["without"]
        print(f"frame {f}: cat pixels {int(cat.sum())}, history kept with the normal snapshot {int(kw.sum())}, without {int(kwo.sum())}, with only {int((kw & ~kwo).sum())}")
        if f >= 2:
            assert kw.sum() > kwo.sum()
            assert kw.sum() >= 200 and kwo.sum() >= 200 and (kw & ~kwo).sum() >= 200
