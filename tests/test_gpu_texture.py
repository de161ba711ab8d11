"""Textured meshes on the device (rt_mesh_set_texture[_of], rt_kat_surface) against the numpy model of tests/texture_model.py and the CPU oracle.  -m gpu.

The cat of the `cpu` preset (object slot 6) and two_cats of tests/material_scenes.py (the diffuse cat at slot 3 textured, the mirror cat at slot 7 not).  Textures are
procedural: random 37 x 23 RGB / RGBA images with random decode tables, constant ones and power-of-two checkers."""
import numpy as np
import pytest

import raytracinggpu_amd as rt
from . import material_scenes as ms
from . import texture_model as tm

pytestmark = pytest.mark.gpu

W, H = 320, 200
SLOT = 6
FILTERS = (("nearest", tm.NEAREST), ("bilinear", tm.BILINEAR))
WRAPS = (("repeat", tm.REPEAT), ("clamp", tm.CLAMP))


@pytest.fixture(scope="module")
def ctx():
    c_ = rt.Context(0)
    yield c_
    c_.close()


def _bits_equal(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _cat(cat_golden, albedo=rt.scenes.CAT_ALBEDO):
    return dict(vertices=cat_golden["vertices"], indices=cat_golden["tri_bvh_order"], bvh_arr10=cat_golden["bvh_arr10"], albedo=albedo, object_slot=SLOT)


def _params(b, spp=1, variant="auto", **kw):
    d = dict(rt.scenes.CPU_LAUNCHER)
    d.update(kw)
    return rt.make_params(W, H, spp, b, variant=variant, **d)


def _planar_uv(v):
    v = np.asarray(v, np.float32)
    lo, hi = v.min(0), v.max(0)
    return (((v[:, :2] - lo[:2]) / (hi[:2] - lo[:2])) * np.float32(2.6) - np.float32(0.8)).astype(np.float32)   # [-0.8, 1.8]: outside [0, 1] on purpose


def _spherical_uv(v):
    v = np.asarray(v, np.float64)
    c = v - v.mean(0)
    r = np.linalg.norm(c, axis=1) + 1e-9
    return np.stack([np.arctan2(c[:, 2], c[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(c[:, 1] / r, -1, 1)) / np.pi * 3 - 1], 1).astype(np.float32)


def _rays(rng, v, n):
    """rays from around the camera and from random directions at random points of the mesh's box"""
    v = np.asarray(v, np.float32)
    lo, hi = v.min(0), v.max(0)
    tgt = lo + rng.random((n, 3)) * (hi - lo)
    org = np.where(rng.random((n, 1)) < 0.5, np.float32([0, 0, 55]) + rng.normal(0, 5, (n, 3)), tgt + rng.normal(0, 1, (n, 3)) * 60)
    u = tgt - org
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return np.concatenate([org, u], 1).astype(np.float32)


def _check_kat(ctx, rays, verts, tri_vidx, uvs, uvidx, px, dec, filt, mode, albedo, slot):
    out = ctx.kat_surface(rays)
    hit = out[:, 0] == slot
    assert hit.sum() >= 200, hit.sum()
    tri = out[hit, 1].astype(np.int64)
    uv, alb = tm.surface(verts, tri_vidx, uvidx, uvs, px, dec, filt, mode, albedo, tri, rays[hit, :3], rays[hit, 3:])
    _bits_equal(out[hit, 3:5], uv)
    _bits_equal(out[hit, 5:8], alb)
    return out


def test_sampler_matches_the_model_bit_for_bit(ctx, cat_golden):
    """rt_kat_surface (production traversal, then the shading kernel's lookup) against the float32 model: planar / spherical / per-corner UVs, RGB and RGBA,
    random decode tables, both filters x both wraps; the cat alone and the diffuse cat of two_cats"""
    rng = np.random.default_rng(7)
    v, tv = cat_golden["vertices"], np.asarray(cat_golden["tri_bvh_order"])[:, :3]
    rays = _rays(rng, v, 4000)
    corner_uv = (rng.random((3 * len(tv), 2)) * 3 - 1).astype(np.float32)          # one UV per corner, -1 .. 2
    corner_idx = np.arange(3 * len(tv), dtype=np.int32).reshape(-1, 3)
    cases = [(_planar_uv(v), tv), (_spherical_uv(v), tv), (corner_uv, corner_idx)]
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden, albedo=(0.75, 0.5, 0.3)))
    k = 0
    for uvs, uvidx in cases:
        for ch in (3, 4):
            px = rng.integers(0, 256, size=(23, 37, ch), dtype=np.uint8)
            dec = rng.random(256).astype(np.float32)
            for fname, filt in FILTERS:
                for wname, mode in WRAPS:
                    k += 1
                    d = None if k % 4 == 0 else dec
                    ctx.mesh_set_texture(uvs, uvidx, px, filter=fname, wrap=wname, decode=d)
                    _check_kat(ctx, rays, v, tv, uvs, uvidx, px, tm.default_decode() if d is None else d, filt, mode, (0.75, 0.5, 0.3), SLOT)
    # two_cats: slot 3 textured, the mirror cat at slot 7 keeps its constant albedo
    spheres, meshes = ms.capi_scene("two_cats", v, cat_golden["tri_obj_order"])
    ctx.scene_upload(spheres, meshes)
    m3 = next(d for d in meshes if d["object_slot"] == 3)
    t3 = np.asarray(m3["indices"])[:, :3]
    px = rng.integers(0, 256, size=(23, 37, 4), dtype=np.uint8)
    dec = rng.random(256).astype(np.float32)
    uvs = _planar_uv(m3["vertices"])
    allv = np.concatenate([m["vertices"] for m in meshes])
    rays = _rays(rng, allv, 6000)
    for fname, filt in FILTERS:
        for wname, mode in WRAPS:
            ctx.mesh_set_texture(uvs, t3, px, filter=fname, wrap=wname, decode=dec, object_slot=3)
            out = _check_kat(ctx, rays, m3["vertices"], t3, uvs, t3, px, dec, filt, mode, (0.25, 0.25, 0.25), 3)
            mir = out[:, 0] == 7
            assert mir.sum() > 50
            _bits_equal(out[mir, 5:8], np.tile(np.float32([0.6, 0.3, 0.1]), (int(mir.sum()), 1)))


def _constant_texture(rng, c, ch=3):
    px = rng.integers(0, 256, size=(23, 37, ch), dtype=np.uint8)
    return px, np.full(256, c, np.float32)


def test_constant_texture_equals_the_untextured_oracle(ctx, oracle, cat_golden):
    """every texel decodes to c: the frame equals the oracle's untextured scene with mesh albedo fl(albedo c), every channel bit for bit (sigma 0, flat normals,
    b 0 / 1 / 3, one and four samples) -- the cat alone, and two_cats with the diffuse cat textured next to the untextured mirror cat"""
    rng = np.random.default_rng(11)
    c = np.float32(0.7)
    alb = tuple(float(np.float32(a) * c) for a in rt.scenes.CAT_ALBEDO)
    v, tv = cat_golden["vertices"], np.asarray(cat_golden["tri_bvh_order"])[:, :3]
    px, dec = _constant_texture(rng, c)
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    ctx.mesh_set_texture(_planar_uv(v), tv, px, decode=dec)
    om = oracle.Mesh.from_arrays(v, cat_golden["tri_obj_order"], albedo=alb).build_bvh()
    osc = oracle.Scene.preset("cpu", om)
    for b in (0, 1, 3):
        for spp in (1, 4):
            exp, _, _ = osc.render(W, H, spp, b, want_rgb8=False)
            _bits_equal(ctx.render(_params(b, spp)), exp)
    # two_cats
    t = cat_golden["tri_obj_order"]
    spheres, meshes = ms.capi_scene("two_cats", v, t)
    ctx.scene_upload(spheres, meshes)
    m3 = next(d for d in meshes if d["object_slot"] == 3)
    ctx.mesh_set_texture(_planar_uv(m3["vertices"]), np.asarray(m3["indices"])[:, :3], px, decode=dec, object_slot=3)
    osc = oracle.Scene()
    for o in ms.describe("two_cats", v):
        if o[0] == "sphere":
            osc.add_sphere(o[1], o[2], o[3])
        else:
            a = alb if o[3] == 0 else o[2]
            osc.add_mesh(oracle.Mesh.from_arrays(o[1], t, albedo=a).set_material(o[3], o[4], o[5]).build_bvh())
    for b in (0, 1, 3):
        for spp in (1, 4):
            exp, _, _ = osc.render(W, H, spp, b, want_rgb8=False)
            _bits_equal(ctx.render(_params(b, spp)), exp)


def test_constant_texture_equals_untextured_on_the_device(ctx, cat_golden):
    """where the oracle is not bit-exact (jitter) or not the point: the textured frame against the device's untextured frame with albedo fl(albedo c), bitwise --
    sigma 0.2, smooth normals, a batch of frames, a posed camera, progressive frames"""
    import torch
    rng = np.random.default_rng(12)
    c = np.float32(0.55)
    alb = tuple(float(np.float32(a) * c) for a in rt.scenes.CAT_ALBEDO)
    v, tv = cat_golden["vertices"], np.asarray(cat_golden["tri_bvh_order"])[:, :3]
    px, dec = _constant_texture(rng, c, ch=4)
    vn = np.zeros_like(np.asarray(v, np.float64))
    fn = np.cross(v[tv[:, 1]] - v[tv[:, 0]], v[tv[:, 2]] - v[tv[:, 0]])
    for k in range(3):
        np.add.at(vn, tv[:, k], fn)
    vn = (vn / np.maximum(np.linalg.norm(vn, axis=1, keepdims=True), 1e-20)).astype(np.float32)
    pose = rt.make_pose(yaw=0.2, pitch=0.1)
    rows = rt._capi.Rows(0, H, H, 1)

    def frames(textured):
        ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden, albedo=rt.scenes.CAT_ALBEDO if textured else alb))
        if textured:
            ctx.mesh_set_texture(_planar_uv(v), tv, px, decode=dec)
        out = [ctx.render(_params(2, 2, sigma=0.2))]
        ctx.mesh_set_normals(vn, tv)
        out.append(ctx.render(_params(3, 1)))
        out.append(ctx.render_pose(_params(2, 1), pose))
        bufs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
        ctx.render_device_batch(_params(2, 1), rows, [(bf.data_ptr(), (0.0, 0.0, 55.0 + k), None, 100 + k) for k, bf in enumerate(bufs)])
        ctx.synchronize()
        out += [bf.cpu().numpy() for bf in bufs]
        ctx.progressive_reset()
        for _ in range(3):
            disp, _ = ctx.progressive_frame(_params(1, 1), pose)
        out.append(disp)
        return out

    want = frames(False)
    got = frames(True)
    for g, w in zip(got, want):
        _bits_equal(g, w)


def _primary_rays(W_, H_, fov=None):
    """the camera rays of cpu:693-709 with sigma 0, as the device forms them"""
    f32 = np.float32
    fov = f32(np.pi / 3) if fov is None else f32(fov)
    z = f32(-f32(W_)) / (f32(2) * f32(np.tan(np.float64(fov / f32(2)))))
    px, row = np.meshgrid(np.arange(W_), np.arange(H_))
    ux = (np.float64(px.astype(f32) - f32(W_) / f32(2)) + 0.5).astype(f32)
    uy = (np.float64(f32(H_) / f32(2) - row.astype(f32)) - 0.5).astype(f32)
    uc = np.stack([ux, uy, np.full_like(ux, z)], -1).astype(f32)
    n = np.sqrt((uc[..., 0] * uc[..., 0] + uc[..., 1] * uc[..., 1]) + uc[..., 2] * uc[..., 2])
    u = uc / n[..., None]
    O = np.broadcast_to(f32([0, 0, 55]), u.shape)
    return np.concatenate([O, u], -1).reshape(-1, 6).astype(f32)


def test_checker_scales_each_pixel_exactly(ctx, cat_golden):
    """mesh albedo 1, a checker of power-of-two texels (other values per channel), b = 0: each pixel of the textured frame is texel(primary hit) (.) the same pixel
    of the untextured frame, bit for bit (scaling by a power of two commutes with every rounding); texel(primary hit) from rt_kat_surface on the frame's primary
    rays.  Bilinear filtering changes the frame too."""
    v, tv = cat_golden["vertices"], np.asarray(cat_golden["tri_bvh_order"])[:, :3]
    dec = np.zeros(256, np.float32)
    dec[[0, 1, 2, 3]] = [0.5, 0.25, 0.125, 2.0]
    check = ((np.arange(37)[None, :] // 4 + np.arange(23)[:, None] // 3) % 2).astype(np.uint8)
    px = np.stack([check, 1 + check, 3 - 2 * check], -1).astype(np.uint8)   # texel (a, b, c) channels: (0.5 | 0.25, 0.25 | 0.125, 2 | 0.25)
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden, albedo=(1.0, 1.0, 1.0)))
    base = ctx.render(_params(0))
    uvs = _planar_uv(v)
    ctx.mesh_set_texture(uvs, tv, px, decode=dec)
    got = ctx.render(_params(0))
    k = ctx.kat_surface(_primary_rays(W, H)).reshape(H, W, 8)
    on_cat = k[..., 0] == SLOT
    assert on_cat.mean() > 0.05
    texel = np.where(on_cat[..., None], k[..., 5:8], np.float32(1))
    assert set(np.unique(texel[on_cat])) <= {0.125, 0.25, 0.5, 2.0}
    _bits_equal(got[..., :3], (texel * base[..., :3]).astype(np.float32))
    np.testing.assert_array_equal(got[..., 3], base[..., 3])
    ctx.mesh_set_texture(uvs, tv, px, filter="bilinear", decode=dec)
    bil = ctx.render(_params(0))
    assert (bil[..., :3] != base[..., :3]).any() and (bil[..., :3] != got[..., :3]).any()


def test_untextured_frames_and_variants(ctx, cat_golden):
    """set then clear = never textured, word for word; every wf_advance variant gives the same textured frame; path / lockstep / global refuse; a re-upload clears"""
    rng = np.random.default_rng(13)
    v, tv = cat_golden["vertices"], np.asarray(cat_golden["tri_bvh_order"])[:, :3]
    px = rng.integers(0, 256, size=(23, 37, 3), dtype=np.uint8)
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    plain = {b: ctx.render(_params(b, 2)) for b in (1, 3)}
    ctx.mesh_set_texture(_spherical_uv(v), tv, px, filter="bilinear")
    tex = ctx.render(_params(3, 2))
    assert (tex[..., :3] != plain[3][..., :3]).any()
    for variant in ("wavefront", "wavefront_lds", "wavefront_queue", "lds_verts", "lds_top", "lds_all"):
        _bits_equal(ctx.render(_params(3, 2, variant=variant)), tex)
    for variant in ("path", "lockstep", "global"):
        with pytest.raises(rt.RtError) as e:
            ctx.render(_params(3, 2, variant=variant))
        assert e.value.code == -5
    ctx.mesh_set_texture(None, None, None)
    for b in (1, 3):
        _bits_equal(ctx.render(_params(b, 2)), plain[b])
    ctx.mesh_set_texture(_spherical_uv(v), tv, px, object_slot=SLOT)
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    _bits_equal(ctx.render(_params(3, 2)), plain[3])
    _bits_equal(ctx.render(_params(3, 2, variant="path")), plain[3])


def test_mesh_operations_keep_the_uvs(ctx, oracle, cat_golden):
    """two_cats, slot 3 textured with per-corner UVs: after rebuild_of (reference and LBVH) the uploaded triangle index reported by rt_kat_surface still names the
    UVs it had (rows permuted by the reported order); after transform_of the lookup follows the moved vertices"""
    rng = np.random.default_rng(14)
    v, t = cat_golden["vertices"], cat_golden["tri_obj_order"]
    spheres, meshes = ms.capi_scene("two_cats", v, t)
    m3 = next(d for d in meshes if d["object_slot"] == 3)
    verts, tv = np.asarray(m3["vertices"], np.float32), np.asarray(m3["indices"])[:, :3]
    nt = len(tv)
    corner_uv = (rng.random((3 * nt, 2)) * 2 - 0.5).astype(np.float32)
    uvidx = np.arange(3 * nt, dtype=np.int32).reshape(-1, 3)
    px = rng.integers(0, 256, size=(23, 37, 3), dtype=np.uint8)
    dec = rng.random(256).astype(np.float32)
    rays = _rays(rng, verts, 5000)
    for mode in ("reference", "lbvh"):
        ctx.scene_upload(spheres, meshes)
        ctx.mesh_set_texture(corner_uv, uvidx, px, wrap="clamp", decode=dec, object_slot=3)
        _check_kat(ctx, rays, verts, tv, corner_uv, uvidx, px, dec, tm.NEAREST, tm.CLAMP, (0.25, 0.25, 0.25), 3)
        _, order = ctx.mesh_rebuild(nt, mode, object_slot=3)
        assert sorted(order.tolist()) == list(range(nt))
        _check_kat(ctx, rays, verts, tv[order], corner_uv, uvidx[order], px, dec, tm.NEAREST, tm.CLAMP, (0.25, 0.25, 0.25), 3)
    R = np.array([[0.9553365, 0, 0.29552022], [0, 1, 0], [-0.29552022, 0, 0.9553365]], np.float32)
    T = (0.5, 0.25, -0.5)
    ctx.mesh_transform(R, T, object_slot=3)
    om = oracle.Mesh.from_arrays(verts, tv).transform(R, T)
    moved = om.vertices
    rays2 = _rays(rng, moved, 5000)
    _check_kat(ctx, rays2, moved, tv[order], corner_uv, uvidx[order], px, dec, tm.NEAREST, tm.CLAMP, (0.25, 0.25, 0.25), 3)
    # the one-mesh scene: the plain rebuild carries the UVs as well (the LBVH device-side install is skipped for a textured mesh)
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    cv, ct = cat_golden["vertices"], np.asarray(cat_golden["tri_bvh_order"])[:, :3]
    uvs = _planar_uv(cv)
    ctx.mesh_set_texture(uvs, ct, px, decode=dec)
    _, order = ctx.mesh_rebuild(len(ct), "lbvh")
    _check_kat(ctx, _rays(rng, cv, 3000), cv, ct[order], uvs, ct[order], px, dec, tm.NEAREST, tm.REPEAT, rt.scenes.CAT_ALBEDO, SLOT)


def test_errors_leave_the_state_unchanged(ctx, cat_golden):
    rng = np.random.default_rng(15)
    v, tv = cat_golden["vertices"], np.asarray(cat_golden["tri_bvh_order"])[:, :3]
    px = rng.integers(0, 256, size=(23, 37, 3), dtype=np.uint8)
    uvs = _planar_uv(v)
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    ctx.mesh_set_texture(uvs, tv, px)
    before = ctx.render(_params(2))
    bad_idx = tv.copy()
    bad_idx[5, 1] = len(uvs)
    cases = [dict(object_slot=99), dict(object_slot=0),                                     # outside the scene; a sphere
             dict(uvidx=bad_idx), dict(uvidx=tv[:-1]),                                      # UV index out of range; fewer triangles than the mesh
             dict(texels=np.zeros((0, 4, 3), np.uint8)), dict(texels=np.zeros((4, 0, 3), np.uint8)),
             dict(texels=np.zeros((4, 4, 2), np.uint8)), dict(texels=np.zeros((4, 4, 5), np.uint8)),
             dict(filter=2), dict(wrap=-1)]
    for case in cases:
        a = dict(uvs=uvs, uvidx=tv, texels=np.zeros((8, 8, 3), np.uint8), filter="nearest", wrap="repeat", object_slot=None)
        a.update(case)
        with pytest.raises(rt.RtError) as e:
            ctx.mesh_set_texture(a["uvs"], a["uvidx"], a["texels"], filter=a["filter"], wrap=a["wrap"], object_slot=a["object_slot"])
        assert e.value.code == -1, case
        _bits_equal(ctx.render(_params(2)), before)


def test_count_work_on_a_textured_scene(ctx, cat_golden):
    """rt_count_work with a textured mesh (wf_advance<kFormTex | kFormStats>, the one form no other test launches): a default counting run has any-hit and the
    dead-channel rule off, so a texture changes albedos and nothing else -- the reference's work is that of the same scene with the texture cleared.  64 x 48: 12 tiles,
    two sub-frames for the frames beside it; one sample, two bounces."""
    rng = np.random.default_rng(29)
    v, tv = cat_golden["vertices"], np.asarray(cat_golden["tri_bvh_order"])[:, :3]
    px = rng.integers(0, 256, size=(23, 37, 3), dtype=np.uint8)
    p = rt.make_params(64, 48, 1, 2, **rt.scenes.CPU_LAUNCHER)
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    plain_frame, plain = ctx.render(p), ctx.count_work(p)
    assert plain["rays"] > 64 * 48 and plain["tri_tests"] > 0, plain   # the cat is in the picture
    ctx.mesh_set_texture(_spherical_uv(v), tv, px, filter="bilinear")
    assert (ctx.render(p)[..., :3] != plain_frame[..., :3]).any()      # ... and the texture on it
    got = ctx.count_work(p)
    ctx.mesh_set_texture(None, None, None)
    assert {k: got[k] for k in ("rays", "box_tests", "nodes", "tri_tests")} == {k: plain[k] for k in ("rays", "box_tests", "nodes", "tri_tests")}
    assert ctx.count_work(p) == plain
