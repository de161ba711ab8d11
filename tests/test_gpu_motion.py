"""Reprojecting a deforming mesh on the device (rt_mesh_snapshot_vertices, rt_render_aov_motion[_device], SvgfSequence(deforming=True)).  -m gpu.

Every comparison is bit for bit on uint32 views.  The three planes are held to rt_render_aov's, the two previous-frame planes to the numpy model of
tests/motion_model.py (the CPU oracle's hits, tests/texture_model.py's barycentrics, tests/temporal_model.py's rigid motion), and the accumulation that is fed them
to what existed before: rt_temporal_accumulate on the current planes with a motion table, and tests/temporal_model.py.  Frames are 96 x 64, 67 x 45 (a ragged last
workgroup) and 1 x 1."""
import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi, hostlib

from . import denoise_model as dm
from . import material_scenes as ms
from . import motion_model as mm
from . import temporal_model as tm
from .test_gpu_aov import _vertex_normals

pytestmark = pytest.mark.gpu

SLOT = 6                                                                # the cat's object slot in the cpu scene
A, B = 3, 7                                                             # the two cats' in two_cats
SIZES = ((96, 64), (67, 45))


@pytest.fixture(scope="module")
def ctx():
    c_ = rt.Context(0)
    yield c_
    c_.close()


def _bits_equal(a, b, msg=""):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, msg                                      # no pixel is left out of the comparison
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=msg)


def _params(w, h, b=0, **kw):
    return rt.make_params(w, h, 1, b, **dict(rt.scenes.CPU_LAUNCHER, **kw))


def _cat_record(cat_golden, slot=SLOT):
    return dict(vertices=np.asarray(cat_golden["vertices"], np.float32), indices=cat_golden["tri_bvh_order"], bvh_arr10=cat_golden["bvh_arr10"],
                albedo=rt.scenes.CAT_ALBEDO, object_slot=slot)


def _tris(d):
    return np.ascontiguousarray(np.asarray(d["indices"])[:, :3], np.int32)


def _refitted(oracle, d, v, material=None, tree=None, order=None):
    """the oracle's mesh of upload record d with the vertices v in d's tree (or `tree`, with the triangles reordered by `order`): every box refitted"""
    m = oracle.Mesh.from_arrays(v, _tris(d), albedo=tuple(d.get("albedo", (0.25, 0.25, 0.25))))
    if material:
        m.set_material(*material)
    return m.set_bvh(np.asarray(d["bvh_arr10"] if tree is None else tree, np.float32).reshape(-1, 10), order).refit()


def _cat_scene(oracle, om):
    return oracle.Scene.preset("cpu", om)


def _check(ctx, osc, w, h, snapshots=None, motion=None, pose=None, tag=""):
    """one rt_render_aov_motion of the scene in use against rt_render_aov and the model -> (aov, prev, the branch of every pixel)"""
    p = _params(w, h)
    aov, prev = ctx.render_aov_motion(p, pose=pose, motion=motion)
    _bits_equal(aov, ctx.render_aov(p, pose=pose), tag + ": the three planes are rt_render_aov's")
    cam = {} if pose is None else dict(cam=tuple(pose.position), fov=pose.fov, basis=rt.camera_basis(pose))
    tr = mm.trace(osc, w, h, meshes={k: s["mesh"] for k, s in (snapshots or {}).items()}, **cam)
    _bits_equal(aov[:2], mm.planes(tr)[:2], tag + ": the model's own inputs")
    br = {}
    exp = mm.previous_planes(tr, snapshots, motion, branch=br)
    _bits_equal(prev, exp, tag + ": the previous-frame planes")
    return aov, prev, br["of"]


# ---------------------------------------------------------------------------------------------------------------- planes against the model

@pytest.mark.parametrize("w,h", SIZES)
def test_deformed_cat_flat_smooth_and_posed(ctx, oracle, cat_golden, w, h):
    d = _cat_record(cat_golden)
    ctx.scene_upload(rt.scenes.spheres("cpu"), d)
    assert ctx.mesh_snapshot_mask() == 0
    ctx.mesh_snapshot_vertices()
    assert ctx.mesh_snapshot_mask() == 1 << SLOT
    v1 = mm.sine_deform(d["vertices"], 1)
    ctx.mesh_set_vertices(v1)
    om = _refitted(oracle, d, v1)
    snap = {SLOT: dict(mesh=om, previous=d["vertices"])}
    aov, prev, of = _check(ctx, _cat_scene(oracle, om), w, h, snap, tag="flat")
    on = of == mm.SNAPSHOT
    assert on.sum() > 150 and (of == mm.STATIC).sum() > 1000
    assert (prev[1][on][:, :3] != aov[1][on][:, :3]).any(-1).mean() > 0.9          # the cat's points moved ...
    _bits_equal(prev[:, ~on], aov[:2][:, ~on])                                       # ... and nothing else
    # a snapshot takes precedence over the object's record; the walls follow theirs
    motion = rt.static_motion()
    motion[:, 9:] = (0.25, -0.5, 0.125)
    _, prev_m, of_m = _check(ctx, _cat_scene(oracle, om), w, h, snap, motion=motion, tag="flat + table")
    _bits_equal(prev_m[:, on], prev[:, on])
    assert (of_m == mm.RIGID).sum() > 1000
    # the posed camera
    pose = rt.make_pose((5.0, 3.0, 40.0), -0.4, 0.15, 1.2)
    _check(ctx, _cat_scene(oracle, om), w, h, snap, pose=pose, tag="posed")
    # interpolated normals: N' = N
    vn = _vertex_normals(v1, _tris(d))
    ctx.mesh_set_normals(vn, _tris(d))
    om.set_normals(vn, _tris(d))
    aov_s, prev_s, of_s = _check(ctx, _cat_scene(oracle, om), w, h, {SLOT: dict(snap[SLOT], smooth=True)}, tag="smooth")
    on_s = of_s == mm.SNAPSHOT
    _bits_equal(prev_s[0][on_s], aov_s[0][on_s])
    assert (aov_s[0][on_s] != aov[0][on_s]).any()
    _bits_equal(prev_s[1], prev[1])                                                  # the points do not depend on the shading
    ctx.mesh_set_normals(None, None)


def test_two_cats_one_snapshotted_one_moved_by_its_record(ctx, oracle, cat_golden):
    w, h = SIZES[0]
    v, t = cat_golden["vertices"], cat_golden["tri_obj_order"]
    spheres, meshes = ms.capi_scene("two_cats", v, t)
    mat = {pos: o[3:6] for pos, o in enumerate(ms.describe("two_cats", v)) if o[0] == "mesh"}
    by_slot = {m["object_slot"]: m for m in meshes}
    ctx.scene_upload(spheres, meshes)
    ctx.mesh_snapshot_vertices(object_slot=A)
    assert ctx.mesh_snapshot_mask() == 1 << A
    va = mm.sine_deform(by_slot[A]["vertices"], 1)
    ctx.mesh_set_vertices(va, object_slot=A)
    a = 0.12
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    T = np.array([-2.0, 1.0, 1.5], np.float32)
    ctx.mesh_transform(R, T, object_slot=B)
    motion = rt.motion_from_mesh_transform(R, T, B)
    motion[A, 9:] = (9, 9, 9)                                            # never read: A holds a snapshot
    oma = _refitted(oracle, by_slot[A], va, mat[A])
    omb = _refitted(oracle, by_slot[B], by_slot[B]["vertices"], mat[B]).transform(R, T).refit()
    osc = oracle.Scene()
    for pos, o in enumerate(ms.describe("two_cats", v)):
        if o[0] == "sphere":
            osc.add_sphere(o[1], o[2], o[3])
        else:
            osc.add_mesh(oma if pos == A else omb)
    aov, prev, of = _check(ctx, osc, w, h, {A: dict(mesh=oma, previous=by_slot[A]["vertices"])}, motion=motion, tag="two cats")
    ids = aov[0, ..., 3]
    assert ((of == mm.SNAPSHOT) == (ids == A)).all() and (ids == A).sum() > 100 and (ids == B).sum() > 50
    ctx.scene_upload(spheres, meshes)
    assert ctx.mesh_snapshot_mask() == 0                                 # a fresh upload holds no snapshot
    # B's previous points are where B was: on the pixels that show B before and after, the record takes its points back onto the old surface
    was = ctx.render_aov(_params(w, h))
    assert ((ids == B) & (was[0, ..., 3] == B)).sum() > 30


def test_demo10_sphere_moved_by_scene_move_sphere(ctx, oracle):
    w, h = SIZES[1]
    spheres = rt.scenes.spheres("demo10")
    ctx.scene_upload(spheres)
    ctx.mesh_snapshot_vertices()                                         # no mesh: nothing to keep
    assert ctx.mesh_snapshot_mask() == 0
    slot = 4
    before = [ctx.sphere(i) for i in range(len(spheres))]
    ctx.move_sphere(slot, (6.0, 3.0, -2.0), dt=0.5)
    after = [ctx.sphere(i) for i in range(len(spheres))]
    motion = rt.motion_from_spheres(before, after)
    osc = oracle.Scene()
    for s in after:
        osc.add_sphere(*s)
    aov, prev, of = _check(ctx, osc, w, h, motion=motion, tag="demo10")
    assert set(np.unique(of)) <= {mm.MISS, mm.RIGID}
    on = aov[0, ..., 3] == slot
    if on.any():
        _bits_equal(prev[0][on], aov[0][on])                            # a translation leaves the normal
        assert (prev[1][on][:, :3] != aov[1][on][:, :3]).any()
    _, prev0, of0 = _check(ctx, osc, w, h, tag="demo10, no table")
    _bits_equal(prev0, aov[:2])
    assert set(np.unique(of0)) <= {mm.MISS, mm.STATIC}


def _on_rays(w, h, pixels, depths):
    """points on the pixel-centre rays of `pixels` [(column, row)] at z = 55 - depth (binary64, narrowed once)"""
    O, u = dm.camera_rays(w, h)
    out = []
    for (c, r), depth in zip(pixels, depths):
        d = u[r, c].astype(np.float64)
        out.append(O.astype(np.float64) + d * (depth / -d[2]))
    return np.asarray(out, np.float32)


@pytest.mark.parametrize("shape", ["triangle", "quad"])
def test_single_triangle_and_quad_with_hits_on_edges_and_corners(ctx, oracle, shape):
    """the corners of the CURRENT shape lie on pixel-centre rays, so do points of its edges (the rows and columns between two corners, and the quad's diagonal)"""
    w, h = SIZES[0]
    px = [(30, 20), (62, 20), (30, 52), (62, 52)]
    cur = _on_rays(w, h, px, (33.0, 35.0, 37.0, 36.0))                # (not in one plane z = const: the reference's slab test rejects a box without depth)
    if shape == "triangle":
        cur, tris = cur[:3], np.array([[0, 2, 1]], np.int32)
    else:
        tris = np.array([[0, 2, 1], [1, 2, 3]], np.int32)
    prev_v = (cur + np.float32([[1.5, 0.25, -2.0], [-0.75, 1.0, 1.0], [0.5, -1.5, 3.0], [2.0, 2.0, -1.0]])[:len(cur)]).astype(np.float32)   # no rigid motion
    d = hostlib.build_mesh(prev_v, tris, albedo=(0.5, 0.5, 0.5), object_slot=SLOT)
    ctx.scene_upload(rt.scenes.spheres("cpu"), d)
    ctx.mesh_snapshot_vertices(object_slot=SLOT)
    ctx.mesh_set_vertices(cur)
    om = _refitted(oracle, d, cur)
    aov, prev, of = _check(ctx, _cat_scene(oracle, om), w, h, {SLOT: dict(mesh=om, previous=prev_v)}, tag=shape)
    on = of == mm.SNAPSHOT
    assert on.sum() > (400 if shape == "triangle" else 900)
    hit_corners = sum(bool(on[r, c]) for c, r in px[:len(cur)])
    print(shape, "pixels on the mesh:", int(on.sum()), "corner pixels hit:", hit_corners, "pixels of the top edge's row:", int(on[20, 30:63].sum()))
    assert hit_corners >= 1 and 0 < on[20, 30:63].sum() < 33 and not on[19].any()   # rays through corners and along an edge fall on both sides of it
    # the previous triangle's own normal, on every pixel of it
    n = np.cross((prev_v[tris[:, 1]] - prev_v[tris[:, 0]]).astype(np.float64), (prev_v[tris[:, 2]] - prev_v[tris[:, 0]]).astype(np.float64))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    got = prev[0][on][:, :3].astype(np.float64)
    assert np.min(np.max(np.abs(got[:, None, :] - n[None]), axis=-1), axis=1).max() < 1e-6


def test_one_pixel_frame_and_interleaved_rows(ctx, oracle, cat_golden):
    d = _cat_record(cat_golden)
    ctx.scene_upload(rt.scenes.spheres("cpu"), d)
    ctx.mesh_snapshot_vertices()
    v1 = mm.sine_deform(d["vertices"], 1)
    ctx.mesh_set_vertices(v1)
    om = _refitted(oracle, d, v1)
    snap = {SLOT: dict(mesh=om, previous=d["vertices"])}
    _check(ctx, _cat_scene(oracle, om), 1, 1, snap, tag="1 x 1")
    w, h = SIZES[1]
    motion = rt.static_motion()
    motion[:, 9] = 0.5
    p = _params(w, h)
    full, full_prev = ctx.render_aov_motion(p, motion=motion)
    seen = np.zeros(h, bool)
    for rank, world, tile in ((0, 3, 8), (1, 3, 8), (2, 3, 8), (1, 2, 5)):
        rows, idx = rt.interleaved_rows(h, tile, rank, world)
        part, part_prev = ctx.render_aov_motion(p, rows=rows, motion=motion)
        assert part.shape == (3, len(idx), w, 4) and part_prev.shape == (2, len(idx), w, 4)
        _bits_equal(part, full[:, idx])
        _bits_equal(part_prev, full_prev[:, idx])
        if world == 3:
            seen[idx] = True
    assert seen.all()                                                    # the three ranks' rows stitch to the full frame
    with pytest.raises(rt.RtError) as e:
        ctx.render_aov_motion(p, rows=_capi.Rows(h - 3, 8, 8, 1))
    assert e.value.code == -1


def test_device_form_equals_the_host_form_and_refusals_touch_nothing(ctx, cat_golden):
    import torch
    w, h = SIZES[1]
    d = _cat_record(cat_golden)
    ctx.scene_upload(rt.scenes.spheres("cpu"), d)
    ctx.mesh_snapshot_vertices()
    ctx.mesh_set_vertices(mm.sine_deform(d["vertices"], 1))
    motion = rt.static_motion()
    motion[0, 9:] = (1, 2, 3)
    p = _params(w, h)
    exp, exp_prev = ctx.render_aov_motion(p, motion=motion)
    st = torch.cuda.Stream()
    out = torch.full((3, h, w, 4), -7.0, dtype=torch.float32, device="cuda:0")
    prev = torch.full((3, h, w, 4), -7.0, dtype=torch.float32, device="cuda:0")   # (a third plane: room to slide an overlapping pair along)
    torch.cuda.synchronize()
    ctx.render_aov_motion_device(p, out.data_ptr(), prev.data_ptr(), motion=motion, stream=st.cuda_stream)
    torch.cuda.synchronize()
    _bits_equal(out.cpu().numpy(), exp)
    _bits_equal(prev.cpu().numpy()[:2], exp_prev)
    assert (prev.cpu().numpy()[2] == -7.0).all()
    ctx.render_aov_motion_device(p, out.data_ptr(), prev.data_ptr(), motion=motion)   # the context's own stream
    ctx.synchronize()
    _bits_equal(prev.cpu().numpy()[:2], exp_prev)
    out.fill_(-7.0)
    prev.fill_(-7.0)
    torch.cuda.synchronize()
    mask = ctx.mesh_snapshot_mask()
    plane = w * h * 16
    ok = dict(params=p, out_ptr=out.data_ptr(), prev_ptr=prev.data_ptr(), motion=motion)
    refused = [dict(prev_ptr=0), dict(out_ptr=0),                                                     # NULL outputs
               dict(prev_ptr=out.data_ptr()), dict(prev_ptr=out.data_ptr() + 3 * plane - 16), dict(out_ptr=prev.data_ptr() + 2 * plane - 16),   # overlap
               dict(prev_ptr=out.data_ptr() + plane + 64),
               dict(params=_params(0, h)), dict(params=_params(w, -1)),                               # what rt_render_aov refuses
               dict(rows=_capi.Rows(h - 3, 8, 8, 1)), dict(rows=_capi.Rows(0, 4, 0, 1)), dict(rows=_capi.Rows(-1, 4, 4, 1))]
    for kw in refused:
        with pytest.raises(rt.RtError) as e:
            ctx.render_aov_motion_device(**dict(ok, **kw))
        assert e.value.code == -1, kw
    for slot, keep in ((SLOT, 2), (SLOT, -1), (0, 1), (99, 1), (-2, 1)):  # keep outside {0, 1}; a sphere's slot; slots outside the scene
        with pytest.raises(rt.RtError) as e:
            ctx.mesh_snapshot_vertices(object_slot=slot, keep=keep)
        assert e.value.code == -1, (slot, keep)
    ctx.synchronize()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and (prev.cpu().numpy() == -7.0).all()
    assert ctx.mesh_snapshot_mask() == mask
    host, host_prev = np.full((3, h, w, 4), -7, np.float32), np.full((3, h, w, 4), -7, np.float32)
    lib, fp = _capi.load(), _capi.C.POINTER(_capi.C.c_float)
    for a, b in ((host, None), (None, host_prev), (host, host[1:]), (host_prev[1:], host_prev)):
        rc = lib.rt_render_aov_motion(ctx._h, _capi.C.byref(p), None, None, None, None if a is None else a.ctypes.data_as(fp), None if b is None else b.ctypes.data_as(fp))
        assert rc == -1
    assert (host == -7).all() and (host_prev == -7).all()
    again, again_prev = ctx.render_aov_motion(p, motion=motion)          # the context still works
    _bits_equal(again, exp)
    _bits_equal(again_prev, exp_prev)
    empty = rt.Context(0)                                                # no scene
    try:
        for call in (lambda: empty.mesh_snapshot_vertices(), lambda: empty.mesh_snapshot_vertices(object_slot=SLOT, keep=False), lambda: empty.render_aov_motion(p)):
            with pytest.raises(rt.RtError) as e:
                call()
            assert e.value.code == -4                                    # RT_ERR_NO_SCENE
        assert empty.mesh_snapshot_mask() == 0
    finally:
        empty.close()


# ---------------------------------------------------------------------------------------------------------------- existing behaviour as the yardstick

def _render(ctx, w, h, seed):
    p = _params(w, h, b=3, seed=seed)
    color, aov = ctx.render(p), ctx.render_aov(p)
    assert np.isfinite(color).all() and np.isfinite(aov).all()
    return color, aov


def _both_ways(ctx, color, motion, prev_aov, prev_hist, prev_fast, w, h):
    """with NO snapshot: accumulating from out_prev without a table == accumulating from the planes with the table, plain and fast, word for word"""
    assert ctx.mesh_snapshot_mask() == 0
    aov, prev = ctx.render_aov_motion(_params(w, h), motion=motion)
    table = ctx.temporal_accumulate(color, aov, prev_aov, prev_hist, reproject=rt.make_reproject(motion=motion))
    planes = ctx.temporal_accumulate(color, prev, prev_aov, prev_hist, reproject=rt.make_reproject())
    _bits_equal(planes, table, "rt_temporal_accumulate")
    ft, ff = ctx.temporal_accumulate_fast(color, aov, prev_aov, prev_hist, prev_fast, reproject=rt.make_reproject(motion=motion))
    pt, pf = ctx.temporal_accumulate_fast(color, prev, prev_aov, prev_hist, prev_fast, reproject=rt.make_reproject())
    _bits_equal(pt, ft, "rt_temporal_accumulate_fast, the history")
    _bits_equal(pf, ff, "rt_temporal_accumulate_fast, the fast plane")
    _bits_equal(ft, table)
    return aov, table


def test_previous_planes_without_a_table_equal_planes_with_the_table(ctx, cat_golden):
    w, h = SIZES[0]
    # the moved sphere of tests/test_gpu_temporal.py
    spheres = rt.scenes.spheres("cpu") + [((-14.0, -2.0, 18.0), 6.0, (0.8, 0.8, 0.8))]
    slot = len(spheres) - 1
    ctx.scene_upload(spheres, _cat_record(cat_golden, slot=len(spheres)))
    color0, aov0 = _render(ctx, w, h, 1)
    h0, f0 = ctx.temporal_accumulate_fast(color0, aov0)
    before = [ctx.sphere(i) for i in range(len(spheres))]
    ctx.move_sphere(slot, (20.0, 10.0, -8.0), dt=0.2)
    motion = rt.motion_from_spheres(before, [ctx.sphere(i) for i in range(len(spheres))])
    color1, _ = _render(ctx, w, h, 2)
    aov1, h1 = _both_ways(ctx, color1, motion, aov0, h0, f0, w, h)
    on = aov1[0, ..., 3] == slot
    assert on.sum() > 50 and (h1[1, ..., 2][on] == 2).mean() > 0.8      # the sphere's pixels follow it
    # the transformed cat
    sph, meshes = ms.capi_scene("two_cats", cat_golden["vertices"], cat_golden["tri_obj_order"])
    ctx.scene_upload(sph, meshes)
    color0, aov0 = _render(ctx, w, h, 11)
    h0, f0 = ctx.temporal_accumulate_fast(color0, aov0)
    a = 0.12
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    T = np.array([-2.0, 1.0, 1.5], np.float32)
    ctx.mesh_transform(R, T, object_slot=A)
    color1, _ = _render(ctx, w, h, 12)
    aov1, h1 = _both_ways(ctx, color1, rt.motion_from_mesh_transform(R, T, A), aov0, h0, f0, w, h)
    assert (h1[1, ..., 2][aov1[0, ..., 3] == A] == 2).sum() > 20


# ---------------------------------------------------------------------------------------------------------------- a deforming sequence

def test_deforming_sequence_of_five_frames(ctx, oracle, cat_golden):
    """per frame the device's history == tests/temporal_model.py on the model's planes; from frame 2 on the cat keeps history (n > 1 on at least 200 of its pixels: the
    model is asked first, so the condition is one the reference meets)"""
    w, h = SIZES[0]
    d = _cat_record(cat_golden)
    ctx.scene_upload(rt.scenes.spheres("cpu"), d)
    v_prev = d["vertices"]
    prev_aov = prev_hist = None
    for f in range(1, 6):
        ctx.mesh_snapshot_vertices()
        v = mm.sine_deform(d["vertices"], f)
        ctx.mesh_set_vertices(v)
        om = _refitted(oracle, d, v)
        color = ctx.render(_params(w, h, b=3, seed=40 + f))
        aov, prev, of = _check(ctx, _cat_scene(oracle, om), w, h, {SLOT: dict(mesh=om, previous=v_prev)}, tag=f"frame {f}")
        rp = None if prev_aov is None else rt.make_reproject()
        hist = ctx.temporal_accumulate(color, prev, prev_aov, prev_hist, reproject=rp)
        exp = tm.accumulate(color, prev, prev_aov, prev_hist)
        cat = of == mm.SNAPSHOT
        if f >= 2:
            kept = int((exp[1, ..., 2][cat] > 1).sum())
            print(f"frame {f}: cat pixels {int(cat.sum())}, with history {kept}")
            assert kept >= 200, (f, kept)
        _bits_equal(hist, exp, f"frame {f}: the history")
        v_prev, prev_aov, prev_hist = v, aov, hist


# ---------------------------------------------------------------------------------------------------------------- snapshot state

def test_snapshot_state_through_transform_rebuild_overwrite_and_release(ctx, oracle, cat_golden):
    w, h = SIZES[1]
    v, t = cat_golden["vertices"], cat_golden["tri_obj_order"]
    spheres, meshes = ms.capi_scene("two_cats_diffuse", v, t)
    by_slot = {m["object_slot"]: m for m in meshes}
    s0, s1 = sorted(by_slot)
    d = by_slot[s0]
    nt = len(_tris(d))
    R = np.float32([[0.9553365, 0, 0.29552022], [0, 1, 0], [-0.29552022, 0, 0.9553365]])
    T = np.float32([0.5, 0.25, -0.5])

    def scene_of(om0):
        osc = oracle.Scene()
        for pos, o in enumerate(ms.describe("two_cats_diffuse", v)):
            if o[0] == "sphere":
                osc.add_sphere(o[1], o[2], o[3])
            else:
                osc.add_mesh(om0 if pos == s0 else _refitted(oracle, by_slot[s1], by_slot[s1]["vertices"]))
        return osc

    ctx.scene_upload(spheres, meshes)
    ctx.mesh_snapshot_vertices(object_slot=s0)
    assert ctx.mesh_snapshot_mask() == 1 << s0
    # snapshot, then a transform: the previous corners are the pre-transform vertices
    ctx.mesh_transform(R, T, object_slot=s0)
    om = _refitted(oracle, d, d["vertices"]).transform(R, T).refit()
    v1 = om.vertices
    snap = {s0: dict(mesh=om, previous=d["vertices"])}
    _, prev_a, of = _check(ctx, scene_of(om), w, h, snap, tag="transform after snapshot")
    assert (of == mm.SNAPSHOT).sum() > 50
    # the snapshot survives a rebuild in both modes: the planes are the model's with the rebuilt order's triangles
    for mode in ("lbvh", "reference"):
        arr, order = ctx.mesh_rebuild(nt, mode=mode, object_slot=s0)
        assert ctx.mesh_snapshot_mask() == 1 << s0, mode
        omr = oracle.Mesh.from_arrays(v1, _tris(d), albedo=tuple(d["albedo"])).set_bvh(arr, order)
        d = dict(d, indices=omr.triangles, bvh_arr10=arr)               # the mesh as the device now holds it
        _check(ctx, scene_of(omr), w, h, {s0: dict(mesh=omr, previous=by_slot[s0]["vertices"])}, tag="rebuild " + mode)
    # a second snapshot overwrites the first: nothing moved since, so every point is its own previous one
    ctx.mesh_snapshot_vertices(object_slot=s0)
    aov, prev_b, _ = _check(ctx, scene_of(omr), w, h, {s0: dict(mesh=omr, previous=v1)}, tag="second snapshot")
    assert (prev_b != prev_a).any()
    # both meshes at once, then s0 handed back to the table
    ctx.mesh_snapshot_vertices()
    assert ctx.mesh_snapshot_mask() == (1 << s0) | (1 << s1)
    ctx.mesh_snapshot_vertices(object_slot=s1, keep=False)
    ctx.mesh_snapshot_vertices(object_slot=s0, keep=False)
    assert ctx.mesh_snapshot_mask() == 0
    motion = rt.motion_from_mesh_transform(R, T, s0)
    _, prev_c, of = _check(ctx, scene_of(omr), w, h, None, motion=motion, tag="keep = 0")
    assert not (of == mm.SNAPSHOT).any() and (prev_c != prev_b).any()
    # a single-mesh scene through the device-side LBVH install
    d1 = _cat_record(cat_golden)
    ctx.scene_upload(rt.scenes.spheres("cpu"), d1)
    assert ctx.mesh_snapshot_mask() == 0                                 # a fresh upload clears the mask
    ctx.mesh_snapshot_vertices()
    vd = mm.sine_deform(d1["vertices"], 2)
    ctx.mesh_set_vertices(vd)
    arr, order = ctx.mesh_rebuild(len(_tris(d1)), mode="lbvh")
    assert ctx.build_stats()["install_on_device"] == 1 and ctx.mesh_snapshot_mask() == 1 << SLOT
    oml = oracle.Mesh.from_arrays(vd, _tris(d1)).set_bvh(arr, order)
    _check(ctx, _cat_scene(oracle, oml), w, h, {SLOT: dict(mesh=oml, previous=d1["vertices"])}, tag="device-side install")


def test_a_snapshot_leaves_the_renderer_alone(ctx, cat_golden):
    w, h = SIZES[0]
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat_record(cat_golden))
    p = _params(w, h, b=2, seed=5)
    counts = lambda: (ctx.first_hit_cache_counts(), ctx.first_shadow_cache_counts(), ctx.first_shade_cache_counts())
    delta = lambda new, old: [{k: a[k] - b[k] for k in a} for a, b in zip(new, old)]
    for _ in range(4):                                                   # a still view: the three caches fill and settle
        ctx.render(p)
    c0 = counts()
    frame = ctx.render(p)
    c1 = counts()
    ctx.mesh_snapshot_vertices()
    ctx.mesh_snapshot_vertices(keep=False)
    ctx.mesh_snapshot_vertices(object_slot=SLOT)
    assert counts() == c1                                                # no key was replaced, no cache emptied
    again = ctx.render(p)
    _bits_equal(again, frame)
    steady = delta(c1, c0)
    assert delta(counts(), c1) == steady                                 # the frame after the snapshot was served by the caches as the frame before it
    assert all(d["filled"] == 0 and d["key_misses"] == 0 for d in steady) and steady[0]["skipped"] > 0


# ---------------------------------------------------------------------------------------------------------------- SvgfSequence

def _chain(ctx, w, h, frames, deforming, d=None, motion=None):
    """the sequence's chain issued call by call through the host entries -> the filtered frames"""
    sp = rt.make_svgf_params()
    outs, prev_aov, prev_hist = [], None, None
    for i in frames:
        if d is not None:
            ctx.mesh_snapshot_vertices()
            ctx.mesh_set_vertices(mm.sine_deform(d["vertices"], i))
        p = _params(w, h, b=3, seed=70 + i)
        color = ctx.render(p)
        if deforming:
            aov, source = ctx.render_aov_motion(p, motion=motion if prev_aov is not None else None)
            rp = rt.make_reproject()
        else:
            aov = source = ctx.render_aov(p)
            rp = rt.make_reproject(motion=motion)
        hist = ctx.temporal_accumulate(color, source, prev_aov, prev_hist, reproject=rp if prev_aov is not None else None)
        outs.append(ctx.svgf_filter(hist, aov, params=sp)[0])
        prev_aov, prev_hist = aov, hist
    return outs


def test_svgf_sequence_deforming_equals_the_calls_one_by_one(ctx, cat_golden):
    w, h = SIZES[0]
    d = _cat_record(cat_golden)
    motion = rt.static_motion()
    ctx.scene_upload(rt.scenes.spheres("cpu"), d)
    exp = _chain(ctx, w, h, range(1, 4), True, d, motion)
    ctx.scene_upload(rt.scenes.spheres("cpu"), d)
    with rt.SvgfSequence(ctx, w, h, deforming=True) as seq:
        for k, i in enumerate(range(1, 4)):
            ctx.mesh_snapshot_vertices()
            ctx.mesh_set_vertices(mm.sine_deform(d["vertices"], i))
            out = seq.frame(_params(w, h, b=3, seed=70 + i), motion=motion)
            _bits_equal(ctx.device_to_host(out, (h, w, 4)), exp[k], f"deforming=True, frame {i}")
        assert len(seq._ptrs) == 7                                       # the six buffers of a plain sequence and the previous-frame planes
    # deforming=False on a static scene: the chain of the entries that existed before
    ctx.scene_upload(rt.scenes.spheres("cpu"), d)
    exp = _chain(ctx, w, h, range(3), False, None, motion)
    with rt.SvgfSequence(ctx, w, h) as seq:
        for i in range(3):
            out = seq.frame(_params(w, h, b=3, seed=70 + i), motion=motion)
            _bits_equal(ctx.device_to_host(out, (h, w, 4)), exp[i], f"deforming=False, frame {i}")
        assert len(seq._ptrs) == 6
    # ... and on a static scene the two sequences agree
    with rt.SvgfSequence(ctx, w, h, deforming=True) as seq:
        for i in range(3):
            out = seq.frame(_params(w, h, b=3, seed=70 + i), motion=motion)
            _bits_equal(ctx.device_to_host(out, (h, w, 4)), exp[i], f"deforming=True on a static scene, frame {i}")
