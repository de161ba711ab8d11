"""rt_render_aov_surface on the device: the planes of the first diffuse surface behind mirrors and glass against tests/surface_model.py (the reference's specular
branches over the CPU oracle's Scene::intersect_all), bit for bit as uint32 views, and against the production render path's own ray counts.  -m gpu."""
import numpy as np
import pytest

import raytracinggpu_amd as rt
from . import denoise_model as dm
from . import material_scenes as ms
from . import surface_model as sm

pytestmark = pytest.mark.gpu

W, H = 203, 149                                                      # odd on purpose: no multiple of any tile
MIRROR_BALL = ((-24, 2, 12), 12, (0, 0, 0), 1, 1.0, 1.0)             # beside the cat, towards the camera: it shows the cat's flank
CAT_SLOT = 7                                                         # in the mirror_cat scenes: six walls, the ball, the cat


@pytest.fixture(scope="module")
def ctx():
    c_ = rt.Context(0)
    yield c_
    c_.close()


def _bits_equal(a, b, msg=""):
    np.testing.assert_array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32), err_msg=msg)


def _params(w=W, h=H, b=0, **kw):
    d = dict(rt.scenes.CPU_LAUNCHER)
    d.update(kw)
    return rt.make_params(w, h, 1, b, **d)


def _cat(cat_golden, slot, albedo=rt.scenes.CAT_ALBEDO):
    return dict(vertices=cat_golden["vertices"], indices=cat_golden["tri_bvh_order"], bvh_arr10=cat_golden["bvh_arr10"], albedo=albedo, object_slot=slot)


def _vertex_normals(v, tv):
    v = np.asarray(v, np.float64)
    fn = np.cross(v[tv[:, 1]] - v[tv[:, 0]], v[tv[:, 2]] - v[tv[:, 0]])
    vn = np.zeros_like(v)
    for k in range(3):
        np.add.at(vn, tv[:, k], fn)
    return (vn / np.maximum(np.linalg.norm(vn, axis=1, keepdims=True), 1e-20)).astype(np.float32)


def _upload(name, ctx, cat_golden):
    v, t_obj = cat_golden["vertices"], cat_golden["tri_obj_order"]
    if name == "demo10":
        ctx.scene_upload(rt.scenes.spheres("demo10"))
    elif name == "cpu":
        ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden, 6))
    elif name in ("mirror_cat", "mirror_cat_smooth"):
        ctx.scene_upload(rt.scenes.spheres("cpu") + [MIRROR_BALL], _cat(cat_golden, CAT_SLOT, albedo=(0.75, 0.5, 0.3)))
        if name == "mirror_cat_smooth":
            ctx.mesh_set_normals(_vertex_normals(v, np.asarray(t_obj)), cat_golden["tri_bvh_order"])
    else:
        ctx.scene_upload(*ms.capi_scene(name, v, t_obj))


def _oracle_scene(name, oracle, cat_golden):
    """-> (oracle scene, materials, albedos)"""
    v, t_obj = cat_golden["vertices"], cat_golden["tri_obj_order"]
    if name == "demo10":
        return (oracle.Scene.preset("demo10"),) + sm.sphere_tables(rt.scenes.spheres("demo10"))
    if name == "mirror_cat_smooth":
        sph = rt.scenes.spheres("cpu") + [MIRROR_BALL]
        s = oracle.Scene()
        for x in sph:
            s.add_sphere(*x)
        s.add_mesh(oracle.Mesh.from_arrays(v, t_obj).set_normals(_vertex_normals(v, np.asarray(t_obj)), t_obj).build_bvh())
        materials, albedos = sm.sphere_tables(sph)
        return s, materials + [(0, 1.0, 1.0)], albedos + [(0.75, 0.5, 0.3)]
    return (ms.oracle_scene(oracle, name, v, t_obj),) + sm.described_tables(ms.describe(name, v))


MAX_SPECULAR = {"demo10": 8, "cpu_mirror": 4, "cpu_glass": 8, "two_cats": 4, "mirror_cat_smooth": 4}
_models = {}


def _model(name, oracle, cat_golden):
    """the model's planes and chains of scene `name` at W x H, computed once"""
    if name not in _models:
        scene, materials, albedos = _oracle_scene(name, oracle, cat_golden)
        chains = {}
        planes = sm.oracle_aov_surface(scene, materials, albedos, W, H, MAX_SPECULAR[name], chains=chains)
        planes.setflags(write=False)
        _models[name] = (planes, chains)
    return _models[name]


# least distinct path codes: the walls a frame shows directly (at least 3) and the same seen through the scene's mirror or glass (another 3); demo10 has three
# specular objects in front of its walls
@pytest.mark.parametrize("name,least_codes", [("demo10", 9), ("cpu_mirror", 6), ("cpu_glass", 6), ("two_cats", 6), ("mirror_cat_smooth", 6)])
def test_planes_equal_the_model(ctx, oracle, cat_golden, name, least_codes):
    _upload(name, ctx, cat_golden)
    got = ctx.render_aov_surface(_params(), MAX_SPECULAR[name])
    assert got.shape == (3, H, W, 4)
    exp, chains = _model(name, oracle, cat_golden)
    codes = np.unique(got[0, ..., 3]).astype(int)
    print(name, "path codes seen:", len(codes), codes.tolist())
    for k in range(3):
        _bits_equal(got[k], exp[k], f"{name}: plane {k}")
    assert len(codes) >= least_codes, codes
    ident, first, ks = rt.Context.decode_path(got[0, ..., 3])
    exhausted = (got[2, ..., 3] == 0) & (got[0, ..., 3] >= 0)
    if name == "demo10":
        assert ks.max() >= 4, ks.max()
    if name == "cpu_glass":
        assert exhausted.sum() >= 1
    if name == "mirror_cat_smooth":                                  # an interpolated normal reached through a chain: not the flat one
        in_ball = (ident == CAT_SLOT) & (ks >= 1)
        assert in_ball.sum() > 100, in_ball.sum()
        ctx.mesh_set_normals(None, None)
        flat = ctx.render_aov_surface(_params(), MAX_SPECULAR[name])
        assert (flat[0][in_ball][:, :3] != got[0][in_ball][:, :3]).any()
        _bits_equal(flat[1], got[1])
        _bits_equal(flat[0, ..., 3], got[0, ..., 3])
    # what the parameters of a render call add is ignored: jitter, samples, bounces, seed
    if name == "demo10":
        _bits_equal(ctx.render_aov_surface(rt.make_params(W, H, 7, 5, sigma=0.4, seed=99, eps=1e-3, tri_tmin=1e-4), MAX_SPECULAR[name]), got)


@pytest.mark.parametrize("name", ["demo10", "cpu"])
def test_max_specular_0_is_render_aov(ctx, cat_golden, name):
    _upload(name, ctx, cat_golden)
    first = ctx.render_aov(_params())
    got = ctx.render_aov_surface(_params(), 0)
    _bits_equal(got[:2], first[:2])
    _bits_equal(got[2, ..., :3], first[2, ..., :3])
    hit = first[0, ..., 3] >= 0
    specular = np.isin(first[0, ..., 3], [0, 1, 2, 3]) if name == "demo10" else np.zeros_like(hit)
    np.testing.assert_array_equal(got[2, ..., 3], (hit & ~specular).astype(np.float32))
    assert not first[2, ..., 3].any()


def test_a_larger_bound_keeps_what_an_earlier_one_retired(ctx, cat_golden):
    _upload("demo10", ctx, cat_golden)
    frames = {m: ctx.render_aov_surface(_params(), m) for m in (0, 1, 2, 3)}
    n_exhausted = []
    for m in (0, 1, 2, 3):
        g = frames[m]
        exhausted = (g[2, ..., 3] == 0) & (g[0, ..., 3] >= 0)
        n_exhausted.append(int(exhausted.sum()))
        if m > 0:
            done = ~prev_exhausted                                   # retired at the earlier bound: a miss or a diffuse end
            _bits_equal(g[:, done], frames[m - 1][:, done], f"max_specular {m} against {m - 1}")
            assert (g[0, ..., 3][prev_exhausted] != frames[m - 1][0, ..., 3][prev_exhausted]).all()   # the others went on: another hit, another code
        prev_exhausted = exhausted
    print("exhausted pixels at max_specular 0..3:", n_exhausted)
    assert n_exhausted[0] > 1000 and all(a >= b for a, b in zip(n_exhausted, n_exhausted[1:])) and n_exhausted[3] < n_exhausted[0]


def test_textured_albedo_through_a_mirror_equals_kat_surface(ctx, oracle, cat_golden):
    """plane 2 on a textured cat seen in the mirror ball: what rt_kat_surface reports for the model's arriving rays (tex_albedo, with the arriving segment's barycentrics)"""
    rng = np.random.default_rng(5)
    _, chains = _model("mirror_cat_smooth", oracle, cat_golden)      # (the cat is diffuse: its normals do not change a chain's rays)
    _upload("mirror_cat", ctx, cat_golden)
    v, tv = cat_golden["vertices"], np.asarray(cat_golden["tri_bvh_order"])[:, :3]
    lo, hi = np.asarray(v).min(0), np.asarray(v).max(0)
    uvs = (((np.asarray(v)[:, :2] - lo[:2]) / (hi[:2] - lo[:2])) * np.float32(2.6) - np.float32(0.8)).astype(np.float32)
    px = rng.integers(0, 256, size=(23, 37, 3), dtype=np.uint8)
    where = [rc for rc, ch in chains.items() if ch.status == sm.DIFFUSE and ch.k >= 1 and ch.id == CAT_SLOT]
    assert len(where) > 100
    rays = np.array([np.concatenate([chains[rc].O, chains[rc].u]) for rc in where], np.float32)
    rr, cc = np.array(where).T
    for filt in ("nearest", "bilinear"):
        ctx.mesh_set_texture(uvs, tv, px, filter=filt, wrap="repeat")
        got = ctx.render_aov_surface(_params(), MAX_SPECULAR["mirror_cat_smooth"])
        kat = ctx.kat_surface(rays).reshape(-1, 8)
        assert (kat[:, 0] == CAT_SLOT).all()
        ident, first, ks = rt.Context.decode_path(got[0, rr, cc, 3])
        assert (ident == CAT_SLOT).all() and (first == 6).all() and (ks >= 1).all()
        _bits_equal(got[2, rr, cc, :3], kat[:, 5:8], filt)
        assert (got[2, rr, cc, 3] == 1).all()
        assert len(np.unique(got[2, rr, cc, 0])) > 50               # a texture, not a constant
    ctx.mesh_set_texture(None, None, None)


def test_chain_lengths_are_the_render_paths(ctx):
    """At sigma 0 with one ray the production frame counts its rays in .w.  A chain that ends on a diffuse surface after k specular segments traced k + 1 segments
    and one shadow ray when the frame is given exactly k bounces; one that leaves the scene after j segments traced j + 1 rays, however many bounces are left.
    No oracle: the chain lengths of the planes against the render kernels."""
    spheres = [s for s in rt.scenes.spheres("demo10") if tuple(s[0]) != (0, 0, -1000)]    # without the back wall: some chains leave the scene
    assert len(spheres) == len(rt.scenes.spheres("demo10")) - 1
    ctx.scene_upload(spheres)
    aov = ctx.render_aov_surface(_params(), 15)
    code = aov[0, ..., 3]
    _, _, ks = rt.Context.decode_path(code)
    diffuse = aov[2, ..., 3] == 1
    assert not ((aov[2, ..., 3] == 0) & (code >= 0)).any()          # nothing is exhausted at 15
    longest = int(ks.max())
    assert longest >= 4, longest
    miss = code == -1
    full = ctx.render(_params(b=15))[..., 3]
    # a miss does not carry its length in the code: the frame's own count gives j, and j segments are what the bounded planes need to find the miss
    j_of = full[miss].astype(int) - 1
    print("chain lengths:", np.bincount(ks[diffuse]).tolist(), "misses after j segments:", np.bincount(j_of).tolist())
    assert miss.sum() > 100 and j_of.min() == 0 and j_of.max() >= 1
    for k in range(longest + 1):
        frame = ctx.render(_params(b=k))[..., 3]
        at_k = diffuse & (ks == k)
        assert at_k.any() or k != 0
        np.testing.assert_array_equal(frame[at_k], np.float32(k + 2), err_msg=f"diffuse after {k} segments")
        bounded = ctx.render_aov_surface(_params(), k)
        found = bounded[0, ..., 3] == -1                             # chains that missed after at most k segments
        np.testing.assert_array_equal(found, miss & (full <= k + 1), err_msg=f"misses within {k} segments")
        np.testing.assert_array_equal(frame[found], full[found])


def test_posed_camera_and_rows(ctx, oracle, cat_golden):
    _upload("demo10", ctx, cat_golden)
    scene, materials, albedos = _oracle_scene("demo10", oracle, cat_golden)
    pos, yaw, pitch, fov = (5.0, 3.0, 40.0), -0.4, 0.15, 1.2
    pose = rt.make_pose(pos, yaw, pitch, fov)
    full = ctx.render_aov_surface(_params(), 8, pose=pose)
    some = [5, 74, 140]                                              # three rows against the model, every row against the full frame
    exp = sm.oracle_aov_surface(scene, materials, albedos, W, H, 8, cam=pos, fov=pose.fov, basis=oracle.camera_basis(yaw, pitch), rows=some)
    _bits_equal(full[:, some], exp)
    assert (rt.Context.decode_path(full[0, ..., 3])[2] >= 1).any()
    plain = ctx.render_aov_surface(_params(), 8)
    assert (plain != full).any()
    for pose_, ref in ((None, plain), (pose, full)):
        for rank, world, tile in ((0, 3, 8), (2, 3, 8), (1, 2, 5)):
            rows, idx = rt.interleaved_rows(H, tile, rank, world)
            part = ctx.render_aov_surface(_params(), 8, pose=pose_, rows=rows)
            assert part.shape == (3, len(idx), W, 4)
            _bits_equal(part, ref[:, idx])
    _bits_equal(ctx.render_aov_surface(_params(), 8, rows=rt._capi.Rows(17, 40, 40, 1)), plain[:, 17:57])
    with pytest.raises(rt.RtError) as e:
        ctx.render_aov_surface(_params(), 8, rows=rt._capi.Rows(H - 3, 8, 8, 1))
    assert e.value.code == -1


def test_max_specular_out_of_range_is_refused(ctx, cat_golden):
    import torch
    _upload("demo10", ctx, cat_golden)
    buf = torch.full((3, H, W, 4), 7.5, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    for bad in (-1, 16):
        with pytest.raises(rt.RtError) as e:
            ctx.render_aov_surface_device(_params(), bad, buf.data_ptr())
        assert e.value.code == -1
        with pytest.raises(rt.RtError):
            ctx.render_aov_surface(_params(), bad)
    ctx.synchronize()
    assert (buf.cpu().numpy() == 7.5).all()
    ctx.render_aov_surface_device(_params(), 15, buf.data_ptr())   # the largest bound is taken
    ctx.synchronize()
    _bits_equal(buf.cpu().numpy(), ctx.render_aov_surface(_params(), 15))


def test_surface_planes_between_renders_leave_them_alone(ctx, cat_golden):
    """a surface call between two frames -- host calls, progressive frames, pipelined device frames on one stream -- changes no frame: queue and state are its own"""
    import torch
    ctx.scene_upload(rt.scenes.spheres("cpu") + [MIRROR_BALL], _cat(cat_golden, CAT_SLOT))
    w, h = 640, 360
    p = _params(w, h, b=3)
    ref = ctx.render(p)
    aov_ref = ctx.render_aov_surface(p, 4)
    first_ref = ctx.render_aov(p)
    _bits_equal(ctx.render(p), ref)
    ctx.render_aov_surface(_params(), 2)                             # another size and bound in between
    _bits_equal(ctx.render(p), ref)
    _bits_equal(ctx.render_aov(p), first_ref)                        # (the first-hit call shares the queue: neither leaves the other anything)
    # progressive accumulation
    pose = rt.make_pose()
    ctx.progressive_reset()
    a = [ctx.progressive_frame(p, pose)[0] for _ in range(3)]
    ctx.progressive_reset()
    b = []
    for _ in range(3):
        b.append(ctx.progressive_frame(p, pose)[0])
        ctx.render_aov_surface(p, 4, pose=pose)
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
            ctx.render_aov_surface_device(p, 4, planes[k % 2].data_ptr(), stream=st.cuda_stream)
        torch.cuda.synchronize()
    finally:
        ctx.set_pipelining(False)
    for k in range(2):
        _bits_equal(bufs[k].cpu().numpy(), ref)
        _bits_equal(planes[k].cpu().numpy(), aov_ref)
    ctx.selfcheck()
