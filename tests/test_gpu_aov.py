"""rt_render_aov on the device: the first-hit planes (normal | object id, hit point | hit flag, albedo) of the pixel-centre camera rays against the CPU oracle's
Scene::intersect_all, bit for bit as uint32 views.  -m gpu.

The rays are the model's (tests/denoise_model.py camera_rays: cpu_launcher.cpp:694-709 with sigma 0, realtime_render.cu:1115 for a pose); the oracle answers every one
of them (or_scene_intersect_all), so planes 0 and 1 are held to the reference's loop over the objects, ties and all."""
import numpy as np
import pytest

import raytracinggpu_amd as rt
from . import denoise_model as dm
from . import material_scenes as ms

pytestmark = pytest.mark.gpu

W, H = 203, 149                                                      # odd on purpose: no multiple of any tile
SLOT = 6


@pytest.fixture(scope="module")
def ctx():
    c_ = rt.Context(0)
    yield c_
    c_.close()


def _bits_equal(a, b, msg=""):
    np.testing.assert_array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32), err_msg=msg)


def _cat(cat_golden, slot=SLOT, albedo=rt.scenes.CAT_ALBEDO):
    return dict(vertices=cat_golden["vertices"], indices=cat_golden["tri_bvh_order"], bvh_arr10=cat_golden["bvh_arr10"], albedo=albedo, object_slot=slot)


def _params(w=W, h=H, b=0, **kw):
    d = dict(rt.scenes.CPU_LAUNCHER)
    d.update(kw)
    return rt.make_params(w, h, 1, b, **d)


def _vertex_normals(v, tv):
    v = np.asarray(v, np.float64)
    fn = np.cross(v[tv[:, 1]] - v[tv[:, 0]], v[tv[:, 2]] - v[tv[:, 0]])
    vn = np.zeros_like(v)
    for k in range(3):
        np.add.at(vn, tv[:, k], fn)
    return (vn / np.maximum(np.linalg.norm(vn, axis=1, keepdims=True), 1e-20)).astype(np.float32)


def _scene(name, ctx, oracle, cat_golden):
    """uploads scene `name`; -> (oracle scene, albedo by object id)"""
    v, t_obj = cat_golden["vertices"], cat_golden["tri_obj_order"]
    if name == "demo10":                                             # a glass sphere, a mirror, a nested pair, the walls
        ctx.scene_upload(rt.scenes.spheres("demo10"))
        return oracle.Scene.preset("demo10"), [s[2] for s in rt.scenes.spheres("demo10")]
    if name == "two_cats":
        spheres, meshes = ms.capi_scene("two_cats", v, t_obj)
        ctx.scene_upload(spheres, meshes)
        return ms.oracle_scene(oracle, "two_cats", v, t_obj), [o[3] if o[0] == "sphere" else o[2] for o in ms.describe("two_cats", v)]
    om = oracle.Mesh.from_arrays(v, t_obj)
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    if name == "cpu_smooth":
        vn = _vertex_normals(v, np.asarray(t_obj))
        om.set_normals(vn, t_obj)
        ctx.mesh_set_normals(vn, cat_golden["tri_bvh_order"])
    return oracle.Scene.preset("cpu", om.build_bvh()), [s[2] for s in rt.scenes.spheres("cpu")] + [rt.scenes.CAT_ALBEDO]


@pytest.mark.parametrize("name", ["cpu", "demo10", "two_cats", "cpu_smooth"])
def test_planes_equal_intersect_all(ctx, oracle, cat_golden, name):
    """every pixel of every plane: N, P and id are Scene::intersect_all's for the pixel-centre ray, the albedo is the hit object's, a miss is (0, 0, 0, -1), 0, 0"""
    osc, albedos = _scene(name, ctx, oracle, cat_golden)
    got = ctx.render_aov(_params())
    assert got.shape == (3, H, W, 4)
    exp = dm.oracle_aov(osc, albedos, W, H)
    ids = set(np.unique(got[0, ..., 3]).astype(int))
    print(name, "object ids seen:", sorted(ids))
    assert len(ids) >= 4, ids                                        # walls and the objects in front of them
    for k in range(3):
        _bits_equal(got[k], exp[k], f"{name}: plane {k}")
    if name == "cpu_smooth":                                         # interpolated normals are not the flat ones
        ctx.mesh_set_normals(None, None)
        flat = ctx.render_aov(_params())
        cat = got[0, ..., 3] == SLOT
        assert (flat[0][cat] != got[0][cat]).any()
        _bits_equal(flat[1], got[1])
    # what the parameters of a render call add is ignored: jitter, samples, bounces, seed
    again = ctx.render_aov(rt.make_params(W, H, 7, 5, sigma=0.4, seed=99, eps=1e-3, tri_tmin=1e-4))
    if name != "cpu_smooth":
        _bits_equal(again, got)


def test_first_hit_is_recorded_whatever_its_material(ctx, oracle, cat_golden):
    """the mirror and the glass spheres of the demo scene report themselves"""
    _scene("demo10", ctx, oracle, cat_golden)
    got = ctx.render_aov(_params())
    ids = set(np.unique(got[0, ..., 3]).astype(int))
    sph = rt.scenes.spheres("demo10")
    assert sph[0][4] != sph[0][5] and sph[1][3]                      # object 0 is glass, object 1 a mirror
    assert {0, 1} <= ids, ids
    for k in (0, 1):
        on = got[0, ..., 3] == k
        _bits_equal(got[2][on][:, :3], np.tile(np.float32(sph[k][2]), (int(on.sum()), 1)))


def test_posed_camera(ctx, oracle, cat_golden):
    """the camera of rt_render_pose: basis from or_camera_basis, u = normalize(C + bz z + bx X + by Y) (realtime_render.cu:1115)"""
    osc, albedos = _scene("cpu", ctx, oracle, cat_golden)
    for pos, yaw, pitch, fov in (((0.0, 0.0, 55.0), 0.0, 0.3, None), ((5.0, 3.0, 40.0), -0.4, 0.15, 1.2)):
        pose = rt.make_pose(pos, yaw, pitch, fov)
        got = ctx.render_aov(_params(), pose=pose)
        exp = dm.oracle_aov(osc, albedos, W, H, cam=pos, fov=pose.fov, basis=oracle.camera_basis(yaw, pitch))
        for k in range(3):
            _bits_equal(got[k], exp[k], f"pose {pos} {yaw} {pitch}: plane {k}")
    plain = ctx.render_aov(_params())
    assert (plain != got).any()


def test_textured_albedo_equals_kat_surface(ctx, cat_golden):
    """plane 2 on a textured cat: the value rt_kat_surface reports for the same rays (tex_albedo, the device function the shading kernel calls)"""
    rng = np.random.default_rng(5)
    v, tv = cat_golden["vertices"], np.asarray(cat_golden["tri_bvh_order"])[:, :3]
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden, albedo=(0.75, 0.5, 0.3)))
    lo, hi = np.asarray(v).min(0), np.asarray(v).max(0)
    uvs = (((np.asarray(v)[:, :2] - lo[:2]) / (hi[:2] - lo[:2])) * np.float32(2.6) - np.float32(0.8)).astype(np.float32)
    px = rng.integers(0, 256, size=(23, 37, 3), dtype=np.uint8)
    for filt in ("nearest", "bilinear"):
        ctx.mesh_set_texture(uvs, tv, px, filter=filt, wrap="repeat")
        got = ctx.render_aov(_params())
        O, u = dm.camera_rays(W, H)
        rays = np.concatenate([np.broadcast_to(O, u.shape), u], -1).reshape(-1, 6)
        kat = ctx.kat_surface(rays).reshape(H, W, 8)
        cat = got[0, ..., 3] == SLOT
        assert cat.sum() > 500 and (kat[cat][:, 0] == SLOT).all()
        _bits_equal(got[2][cat][:, :3], kat[cat][:, 5:8], filt)
        assert len(np.unique(got[2][cat][:, 0])) > 50               # a texture, not a constant
        walls = (got[0, ..., 3] >= 0) & ~cat
        exp = np.float32([s[2] for s in rt.scenes.spheres("cpu")])[got[0][walls][:, 3].astype(int)]
        _bits_equal(got[2][walls][:, :3], exp)
    ctx.mesh_set_texture(None, None, None)


def test_interleaved_rows_equal_the_full_frame(ctx, oracle, cat_golden):
    _scene("cpu", ctx, oracle, cat_golden)
    full = ctx.render_aov(_params())
    for rank, world, tile in ((0, 3, 8), (2, 3, 8), (1, 2, 5)):
        rows, idx = rt.interleaved_rows(H, tile, rank, world)
        part = ctx.render_aov(_params(), rows=rows)
        assert part.shape == (3, len(idx), W, 4)
        _bits_equal(part, full[:, idx])
    part = ctx.render_aov(_params(), rows=rt._capi.Rows(17, 40, 40, 1))
    _bits_equal(part, full[:, 17:57])
    with pytest.raises(rt.RtError) as e:
        ctx.render_aov(_params(), rows=rt._capi.Rows(H - 3, 8, 8, 1))
    assert e.value.code == -1


def test_misses_are_the_pixels_that_trace_one_ray(ctx, cat_golden):
    """a scene without its back wall: at sigma 0, b 0 a camera ray that hits nothing is the only ray of its pixel (.w == 1), a hit adds a shadow ray"""
    walls = [s for s in rt.scenes.spheres("cpu") if tuple(s[0]) != (0, 0, -1000)]
    assert len(walls) == len(rt.scenes.spheres("cpu")) - 1
    ctx.scene_upload(walls, _cat(cat_golden, slot=len(walls)))
    p = _params(b=0)
    frame = ctx.render(p)
    aov = ctx.render_aov(p)
    miss = aov[0, ..., 3] == -1
    assert 100 < miss.sum() < W * H - 100
    np.testing.assert_array_equal(miss, frame[..., 3] == 1)
    np.testing.assert_array_equal(aov[1, ..., 3], (~miss).astype(np.float32))
    assert not aov[:, miss, :3].any() and not aov[2, ..., 3].any()


def test_aov_between_renders_leaves_them_alone(ctx, oracle, cat_golden):
    """an AOV call between two frames -- host calls, progressive frames, pipelined device frames on one stream -- changes no frame: it has a queue of its own"""
    import torch
    _scene("cpu", ctx, oracle, cat_golden)
    w, h = 640, 360
    p = _params(w, h, b=3)
    ref = ctx.render(p)
    aov_ref = ctx.render_aov(p)
    _bits_equal(ctx.render(p), ref)
    ctx.render_aov(_params())                                        # another size in between
    _bits_equal(ctx.render(p), ref)
    # progressive accumulation
    pose = rt.make_pose()
    ctx.progressive_reset()
    a = [ctx.progressive_frame(p, pose)[0] for _ in range(3)]
    ctx.progressive_reset()
    b = []
    for _ in range(3):
        b.append(ctx.progressive_frame(p, pose)[0])
        ctx.render_aov(p, pose=pose)
    assert ctx.progressive_frames() == 3
    for x, y in zip(a, b):
        _bits_equal(x, y)
    # pipelined frames into alternating buffers, the planes of each rendered on the same stream in between
    st = torch.cuda.Stream()
    rows, _ = rt.interleaved_rows(h, 8, 0, 1)
    bufs = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    planes = [torch.zeros((3, h, w, 4), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()
    try:
        ctx.set_pipelining(True)
        for k in range(6):
            ctx.render_device(p, rows, bufs[k % 2].data_ptr(), st.cuda_stream)
            ctx.render_aov_device(p, planes[k % 2].data_ptr(), stream=st.cuda_stream)
        torch.cuda.synchronize()
    finally:
        ctx.set_pipelining(False)
    for k in range(2):
        _bits_equal(bufs[k].cpu().numpy(), ref)
        _bits_equal(planes[k].cpu().numpy(), aov_ref)
    ctx.selfcheck()
