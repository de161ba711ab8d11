"""Frames of scenes in which a mesh emits (rt_scene_set_emission: every wf_advance launch after the opening one is a kFormEmit form; a ray that hits an emitter ends
there, a diffuse segment's one shadow ray may go to a point of one).  -m gpu.  Every case fails on a library without the entries.

Every comparison is on uint32 views, .w (the ray count) included.  References, none of them the code under test:
  what exists   no emission, and an emission set and removed, against a context that never heard of the calls: frames and all three still-view counters;
  the model     tests/emission_model.py Walker (held to the mathematics and to soft_lights_model.Walker by tests/test_emission_model.py), its intersections the oracle's:
                a panel over a floor with a diffuse, a mirror and a glass ball; the open cat under a panel, plain and textured; a room whose bumpy ceiling emits;
  closed forms  a camera ray that hits the panel is Le; a one-triangle emitter at share 1 over one diffuse sphere at b = 0;
  statistics    the frame mean at share 0.5 against the frame mean at share 0 over 8 seeds.
Frames are 67 x 45, 96 x 64 and 1 x 1.  The panels are tilted a little: a box without thickness is entered by no ray (the reference's strict box test)."""
import ctypes as C

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi
from . import emission_model as em
from . import lens_model as lnm
from . import lights_model as lm
from . import soft_lights_model as slm
from . import still_view as sv
from . import texture_model as tm
from .test_gpu_emission import _grid
from .test_gpu_sky import BALLS, LENS, NEAR, ROOM, WAVEFRONTS
from .test_gpu_soft_lights import COUNTS, POSE, THREE, _bits_equal, _differ, _moved, _params, _planar_uv, _texture

pytestmark = pytest.mark.gpu

f32 = np.float32
FP = C.POINTER(C.c_float)
RADII = [0.0, 2.0, 5.0]
LE = (4e5, 3e5, 2e5)                                                    # of the order of the direct term of rt.scenes.LIGHT at these distances: both kinds of light show
DIFFUSE_BALL = ((-2.0, -2.0, 18.0), 8.0, (0.7, 0.6, 0.3))
# name -> (spheres, [(kind, geometry arguments)], {mesh index: radiance}); the meshes take the object positions after the spheres
SCENES = {
    "balls": (BALLS + [DIFFUSE_BALL], [("panel", ((-30, 22, -20), (60, 2, 0), (0, 1, 50)))], {0: LE}),
    "cat": ([], [("cat", None), ("panel", ((-25, 32, -18), (50, 2, 0), (0, 1, 40)))], {1: LE}),
    "textured cat": ([], [("cat", "textured"), ("panel", ((-25, 32, -18), (50, 2, 0), (0, 1, 40)))], {1: (2e5, 4e5, 3e5)}),
    "room": (ROOM, [("grid", (8, 8, (-32, 45, -32), 8.0, 88))], {0: (3e5, 3e5, 2.5e5)}),
}


@pytest.fixture(scope="module")
def ctx():
    c_ = rt.Context(0)
    yield c_
    c_.close()


@pytest.fixture(scope="module")
def ref():
    c_ = rt.Context(0)
    yield c_
    c_.close()


_CACHE = {}


def _built(oracle, g, name):
    """-> (spheres, upload dicts, oracle meshes, {object slot: radiance}), built once"""
    if ("built", name) not in _CACHE:
        spheres, meshes, emit = SCENES[name]
        dicts, oms = [], []
        for k, (kind, arg) in enumerate(meshes):
            if kind == "cat":
                m = oracle.Mesh.from_arrays(g["vertices"], g["tri_obj_order"]).build_bvh()
            elif kind == "panel":
                m = oracle.Mesh.from_arrays(*rt.scenes.panel(*arg)).build_bvh()
            else:
                m = oracle.Mesh.from_arrays(*_grid(*arg)).build_bvh()
            oms.append(m)
            dicts.append(dict(vertices=m.vertices, indices=m.triangles, bvh_arr10=m.bvh_array(), albedo=rt.scenes.CAT_ALBEDO, object_slot=len(spheres) + k))
        _CACHE[("built", name)] = (spheres, dicts, oms, {len(spheres) + k: le for k, le in emit.items()})
    return _CACHE[("built", name)]


def _up(c, oracle, g, name, emit=True, **kw):
    spheres, dicts, _, emission = _built(oracle, g, name)
    c.scene_upload(spheres, dicts if len(dicts) > 1 else dicts[0], **kw)
    if SCENES[name][1][0][1] == "textured":
        texels, decode = _texture()
        c.mesh_set_texture(_planar_uv(g["vertices"]), np.asarray(dicts[0]["indices"])[:, :3], texels, filter="bilinear", decode=decode, object_slot=dicts[0]["object_slot"])
    if emit:
        for slot, le in emission.items():
            c.set_emission(slot, le)


def _table(dicts, emission):
    tris = [em.corners(d["vertices"], d["indices"], em.stored_order(d["bvh_arr10"])) for d in dicts]
    le = [np.broadcast_to(np.asarray(emission.get(d["object_slot"], (0, 0, 0)), f32), (len(t), 3)) for t, d in zip(tris, dicts)]
    return em.TriTable(np.concatenate(tris), np.concatenate(le))


def _oracle_scene(oracle, g, name):
    """-> (oracle scene, materials, table, surface hook or None), built once"""
    if ("scene", name) not in _CACHE:
        spheres, dicts, oms, emission = _built(oracle, g, name)
        osc = oracle.Scene()
        for s in spheres:
            osc.add_sphere(s[0], s[1], s[2], *(s[3:] if len(s) > 3 else ()))
        for m in oms:
            osc.add_mesh(m)
        surface = None
        if SCENES[name][1][0][1] == "textured":
            texels, decode = _texture()
            mesh, slot = oms[0], dicts[0]["object_slot"]
            verts, tris, uvs = mesh.vertices, mesh.triangles, _planar_uv(g["vertices"])

            def surface(oid, O, u, alb):
                if oid != slot:
                    return alb
                found, _, _, tri = mesh.intersect_tri(O, u, 1e-4)
                assert found and tri >= 0
                return tm.surface(verts, tris, tris, uvs, texels, decode, tm.BILINEAR, tm.REPEAT, alb, [tri], np.asarray(O, f32)[None], np.asarray(u, f32)[None])[1][0]
        _CACHE[("scene", name)] = (osc, lm.materials(spheres, dicts), _table(dicts, emission), surface)
    return _CACHE[("scene", name)]


class _LensWalker(em.Walker, lnm.Walker):
    """the emission walker's path behind the lens walker's camera rays"""


def _model(oracle, g, name, share, b, spp=1, w=67, h=45, pose=None, rows=None, lights=(rt.scenes.LIGHT,), radii=None, lens=None, cam=(0, 0, 55), seed=123456):
    """the model's frame at `share`, computed once"""
    key = ("frame", name, share, b, spp, w, h, pose, None if rows is None else tuple(rows), repr(lights), repr(radii), lens, cam, seed)
    if key not in _CACHE:
        osc, mats, tb, surface = _oracle_scene(oracle, g, name)
        kw = dict(fov=np.pi / 2) if pose is not None else {}
        if lens is not None:
            kw["lens"] = lens
        wk = (_LensWalker if lens is not None else em.Walker)(osc, mats, list(lights), radii, emission=_built(oracle, g, name)[3], table=tb, share=share, cam=cam, seed=seed, **kw)
        wk.surface = surface
        _CACHE[key] = wk.render(w, h, spp, b, pose=pose, rows=rows)
    return _CACHE[key]


# ---- exact against what exists ----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", ["cat", "room"])
def test_no_emission_and_an_emission_set_and_removed_are_the_context_that_never_heard_of_the_calls(oracle, cat_golden, scene):
    """frames and all three still-view counters, on new contexts"""
    a, b = rt.Context(0), rt.Context(0)
    try:
        for c_ in (a, b):
            _up(c_, oracle, cat_golden, scene, emit=False)
        slot = next(iter(_built(oracle, cat_golden, scene)[3]))
        a.set_emission_sampling(0.75)                                   # a share without an emitter: nothing to sample
        p = _params(2, w=96, h=64)
        before = [[getattr(c_, n)() for n in COUNTS] for c_ in (a, b)]
        for _ in range(4):                                              # fill, use, store the records, resume
            plain = b.render(p)
            _bits_equal(a.render(p), plain)
        assert _moved(a, before[0]) == _moved(b, before[1])
        # set, rendered twice, and removed: an emitting chain keeps out of the still view, so the levels a holds are the ones it stored -- from here on a's frames AND its
        # counters move as b's do, which rendered nothing in between (a refill would show as misses and fills that b does not have)
        a.set_emission(slot, LE)
        lit = a.render(p)
        assert _differ(lit, plain) > 100
        _bits_equal(a.render(p), lit)
        a.set_emission(slot, (0, 0, 0))
        before = [[getattr(c_, n)() for n in COUNTS] for c_ in (a, b)]
        for q in (p, p, _params(2, spp=4, w=96, h=64), p, _params(0, w=1, h=1)):
            _bits_equal(a.render(q), b.render(q))
        assert _moved(a, before[0]) == _moved(b, before[1])
        _bits_equal(a.render_pose(_params(2), rt.make_pose(**POSE)), b.render_pose(_params(2), rt.make_pose(**POSE)))
    finally:
        a.close()
        b.close()


def test_w_does_not_depend_on_the_share(ctx, oracle, cat_golden):
    for name in ("balls", "cat"):
        _up(ctx, oracle, cat_golden, name)
        frames = {}
        for share in (0.0, 0.5, 1.0):
            ctx.set_emission_sampling(share)
            frames[share] = ctx.render(_params(2, spp=4, w=96, h=64))
        _bits_equal(frames[0.5][..., 3], frames[0.0][..., 3], name)
        _bits_equal(frames[1.0][..., 3], frames[0.0][..., 3], name)
        assert _differ(frames[0.5], frames[0.0]) > 100 and _differ(frames[0.5], frames[1.0]) > 100


# ---- against the model, word for word --------------------------------------------------------------------------------------------------------------------------------------

CASES = [("balls", 0.5, 0, 1), ("balls", 0.5, 2, 1), ("balls", 0.25, 3, 1), ("balls", 1.0, 0, 4), ("balls", 0.5, 2, 4),
         ("cat", 0.25, 2, 1), ("cat", 0.5, 3, 1), ("cat", 0.0, 2, 1), ("textured cat", 0.5, 2, 1), ("textured cat", 1.0, 0, 4),
         ("room", 1.0, 2, 1), ("room", 0.5, 3, 1), ("room", 0.0, 0, 4), ("room", 0.25, 2, 4)]


@pytest.mark.parametrize("scene,share,b,spp", CASES)
def test_scenes_with_an_emitter_equal_the_model(ctx, oracle, cat_golden, scene, share, b, spp):
    _up(ctx, oracle, cat_golden, scene)
    ctx.set_emission_sampling(share)
    _bits_equal(ctx.render(_params(b, spp=spp)), _model(oracle, cat_golden, scene, share, b, spp), f"{scene} share {share} b={b} spp={spp}")


def test_intensity_0_a_light_list_and_radii_equal_the_model(ctx, oracle, cat_golden):
    for scene in ("balls", "textured cat"):
        _up(ctx, oracle, cat_golden, scene)
        dark = [(rt.scenes.LIGHT[0], 0.0)]
        ctx.set_light(*dark[0])                                         # intensity 0: the effective share is 1 whatever the positive share
        ctx.set_emission_sampling(0.25)
        exp = _model(oracle, cat_golden, scene, 0.25, 2, lights=dark)
        _bits_equal(ctx.render(_params(2)), exp, "intensity 0")
        _bits_equal(exp, _model(oracle, cat_golden, scene, 1.0, 2, lights=dark), "effective share 1")
        ctx.set_lights(THREE)
        _bits_equal(ctx.render(_params(2)), _model(oracle, cat_golden, scene, 0.25, 2, lights=THREE), "three lights")
        ctx.set_light_radii(RADII)
        _bits_equal(ctx.render(_params(2)), _model(oracle, cat_golden, scene, 0.25, 2, lights=THREE, radii=RADII), "radii")


def test_lens_posed_camera_row_shares_one_pixel_and_every_wavefront_variant_equal_the_model(ctx, oracle, cat_golden):
    import torch
    _up(ctx, oracle, cat_golden, "balls")
    p = _params(2)
    whole = _model(oracle, cat_golden, "balls", 0.5, 2)
    ctx.set_lens(*LENS)
    _bits_equal(ctx.render(p), _model(oracle, cat_golden, "balls", 0.5, 2, lens=LENS), "lens")
    ctx.set_lens(0.0, 1.0)
    near = ctx.render_pose(p, rt.make_pose(position=NEAR, **POSE))
    _bits_equal(near, _model(oracle, cat_golden, "balls", 0.5, 2, pose=(POSE["yaw"], POSE["pitch"]), cam=NEAR))
    share, image_rows = rt.interleaved_rows(45, 8, 1, 3)
    buf = torch.zeros((share.n_rows, 67, 4), dtype=torch.float32, device="cuda")
    ctx.render_device(p, share, buf.data_ptr())
    ctx.synchronize()
    _bits_equal(buf.cpu().numpy(), whole[list(image_rows)])
    _bits_equal(ctx.render(_params(2, w=1, h=1)), _model(oracle, cat_golden, "balls", 0.5, 2, w=1, h=1))
    for v in WAVEFRONTS:
        _bits_equal(ctx.render(_params(2, variant=v)), whole, v)


@pytest.mark.parametrize("knobs", [dict(RT_PARTS="1"), dict(RT_PARTS="3"), dict(RT_DEAD_CHANNELS="0"), dict(RT_TRAVQ_ANYHIT="0")])
def test_other_cuts_and_knobs_render_the_same_words(ctx, oracle, cat_golden, knobs):
    """the room's pure-colour walls kill channels of paths whose later shadow rays go to the ceiling"""
    c_ = sv.context(**knobs)
    try:
        for scene, share, b, spp in (("room", 0.5, 3, 1), ("balls", 0.5, 2, 4)):
            _up(c_, oracle, cat_golden, scene)
            c_.set_emission_sampling(share)
            got = c_.render(_params(b, spp=spp))
            _bits_equal(got, _model(oracle, cat_golden, scene, share, b, spp), f"{knobs} {scene}")
    finally:
        c_.close()


def test_a_batch_of_three_async_and_the_emitter_transformed_between_pipelined_frames(ctx, ref, oracle, cat_golden):
    import torch
    W, H = 67, 45
    _up(ctx, oracle, cat_golden, "balls")
    rows = _capi.Rows(0, H, H, 1)
    cams = [((0.5 * k, 0.0, 55.0 - 3 * k), 40 + k) for k in range(3)]
    bufs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in cams]
    ctx.render_device_batch(_params(2), rows, [(bf.data_ptr(), cam, None, seed) for bf, (cam, seed) in zip(bufs, cams)])
    ctx.synchronize()
    for bf, (cam, seed) in zip(bufs, cams):
        _up(ref, oracle, cat_golden, "balls", camera=(cam, None))
        _bits_equal(bf.cpu().numpy(), ref.render(_params(2, seed=seed)), str(cam))
    cam, seed = cams[1]
    _bits_equal(bufs[1].cpu().numpy(), _model(oracle, cat_golden, "balls", 0.5, 2, cam=cam, seed=seed))
    out = rt.PinnedArray((H, W, 4), np.float32)
    try:
        ctx.render_async(_params(2), out.array, slot=0)
        ctx.wait(0)
        _bits_equal(out.array, _model(oracle, cat_golden, "balls", 0.5, 2))
    finally:
        out.close()
    # the panel slides back and forth between pipelined frames: every frame is the one a fresh upload of the moved panel renders
    slot = next(iter(_built(oracle, cat_golden, "balls")[3]))
    eye = np.eye(3, dtype=f32)
    steps = [(4.0, 0.0, 0.0), (0.0, -2.0, 3.0), (-4.0, 2.0, -3.0), (0.0, 0.0, 0.0)]
    want = []
    _up(ref, oracle, cat_golden, "balls")
    for t in steps:
        ref.mesh_transform(eye, t, object_slot=slot)
        want.append(ref.render(_params(2, seed=77)))
    assert _differ(want[0], want[1]) > 100
    pair = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    got = []
    ctx.set_pipelining(True)
    try:
        for k, t in enumerate(steps):
            ctx.mesh_transform(eye, t, object_slot=slot)
            ctx.render_device(_params(2, seed=77), rows, pair[k % 2].data_ptr())
            if k % 2 == 1:
                ctx.synchronize()
                got.extend(b.cpu().numpy() for b in pair)
    finally:
        ctx.set_pipelining(False)
    for k, fr in enumerate(got):
        _bits_equal(fr, want[k], f"pipelined frame {k}")
    # ... and the model agrees with the last one: the panel is back where it was, up to the roundings of the three moves -- so against the model of the moved vertices
    moved = oracle.Mesh.from_arrays(*rt.scenes.panel(*SCENES["balls"][1][0][1])).build_bvh()
    for t in steps:
        moved.transform(eye, t)
    spheres, dicts, _, emission = _built(oracle, cat_golden, "balls")
    osc = oracle.Scene()
    for s in spheres:
        osc.add_sphere(s[0], s[1], s[2], *(s[3:] if len(s) > 3 else ()))
    moved.refit()
    osc.add_mesh(moved)
    d = dict(dicts[0], vertices=moved.vertices)
    wk = em.Walker(osc, lm.materials(spheres, [d]), [rt.scenes.LIGHT], None, emission=emission, table=_table([d], emission), share=0.5, seed=77)
    _bits_equal(got[3], wk.render(W, H, 1, 2), "the model of the moved panel")


# ---- closed forms ------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_a_camera_ray_that_hits_the_panel_is_le_exactly(ctx, oracle):
    m = oracle.Mesh.from_arrays(*rt.scenes.panel((-8, -5, 0), (16, 0.5, 0.5), (0, 12, 1))).build_bvh()
    ctx.scene_upload([((0, -1000, 0), 990, (0.5, 0.5, 0.5))], dict(vertices=m.vertices, indices=m.triangles, bvh_arr10=m.bvh_array(), albedo=(0.9, 0.9, 0.9), object_slot=1))
    le = np.array([3.5, 0.0, 2.0 ** 95], f32)
    ctx.set_emission(1, le)
    osc = oracle.Scene()
    osc.add_sphere((0, -1000, 0), 990, (0.5, 0.5, 0.5))
    osc.add_mesh(m)
    W, H = 67, 45
    for share, b in ((0.5, 0), (0.0, 2), (1.0, 3)):
        ctx.set_emission_sampling(share)
        got = ctx.render(_params(b))
        seen = 0
        for row in range(0, H, 2):
            for px in range(0, W, 2):
                hit, oid, _, _ = osc.intersect_all(np.array([0, 0, 55], f32), slm.camera_dir(W, H, row, px), 1e-4)
                if hit and oid == 1:
                    _bits_equal(got[row, px, :3], le, f"pixel {row},{px}")
                    assert got[row, px, 3] == 1
                    seen += 1
        assert seen > 20


def test_a_one_triangle_emitter_at_share_1_over_one_diffuse_sphere(ctx, oracle):
    """b = 0: one segment.  A pixel that hits the sphere (nothing blocks a ray that leaves a convex body, and the triangle lies beyond the ray's end) is
    fl(fl(l alb) / pi) + fl(alb (+0)) per channel with l = fl(w_emit fl(g Le)), w_emit = 1, g from the model's draw at the sphere's own normal"""
    alb = np.array([0.25, 0.5, 0.75], f32)
    sphere = ((0.0, 0.0, 0.0), 10.0, tuple(alb))
    v = np.array([[-20, 25, 5], [15, 30, 20], [5, 28, -25]], f32)
    m = oracle.Mesh.from_arrays(v, np.array([[0, 1, 2]], np.int32)).build_bvh()
    d = dict(vertices=m.vertices, indices=m.triangles, bvh_arr10=m.bvh_array(), albedo=(0.1, 0.1, 0.1), object_slot=1)
    ctx.scene_upload([sphere], d)
    le = np.array([7.0, 5.0, 3.0], f32)
    ctx.set_emission(1, le)
    ctx.set_emission_sampling(1.0)
    W, H, seed = 67, 45, 123456
    got = ctx.render(_params(0, seed=seed))
    tb = _table([d], {1: le})
    osc = oracle.Scene()
    osc.add_sphere(*sphere)
    osc.add_mesh(m)
    checked = lit = 0
    for row in range(H):
        for px in range(W):
            pixel = row * W + px
            if pixel % 5:
                continue
            ok, oid, P, N = osc.intersect_all(np.array([0, 0, 55], f32), slm.camera_dir(W, H, row, px), 1e-4)
            if not ok or oid != 0:
                continue
            t, Q = tb.sample(em.sample_key(seed, pixel, 0), 0)
            g, _, _ = tb.weight(t, Q, P, N)
            l3 = (f32(1) * (g[0] * le).astype(f32)).astype(f32)
            exp = ((l3 * alb).astype(f32) / f32(np.pi)).astype(f32) + (alb * f32(0)).astype(f32)
            _bits_equal(got[row, px, :3], exp, f"pixel {row},{px}")
            assert got[row, px, 3] == 2
            checked += 1
            lit += int(g[0] > 0)
    assert checked > 40 and lit > 10


# ---- unbiased on the device ----------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_frame_mean_at_share_half_is_the_frame_mean_at_share_0(ctx, oracle):
    """a diffuse floor with a diffuse ball under a ceiling panel of 100 x 100 at 24 above the floor, lights of intensity 0 (so share 0.5 takes every shadow ray to the
    panel and share 0 finds it by bounces alone), 24 x 16, b = 2, 64 samples, 8 seeds.  The panel's size, from the model on the CPU (24 x 16 x 4 paths): a sample's
    standard deviation inside its pixel is 0.36 of the frame mean at share 0 and 0.80 at share 0.5 (a wide panel close by is a poor target for sampling by area; a
    panel of 160 gives 0.28 and 1.10, one of 40 far more at share 0), so over 24 576 samples a frame and 8 frames five combined standard errors are about 1.0 % of
    the mean."""
    m = oracle.Mesh.from_arrays(*rt.scenes.panel((-50, 14, -50), (100, 1, 0), (0, 0.5, 100))).build_bvh()
    ctx.scene_upload([((0, -1000, 0), 990, (0.5, 0.5, 0.5)), DIFFUSE_BALL],
                     dict(vertices=m.vertices, indices=m.triangles, bvh_arr10=m.bvh_array(), albedo=(0.5, 0.5, 0.5), object_slot=2))
    ctx.set_light(rt.scenes.LIGHT[0], 0.0)
    ctx.set_emission(2, (10.0, 9.0, 8.0))
    means = {}
    for share in (0.0, 0.5):
        ctx.set_emission_sampling(share)
        means[share] = np.array([ctx.render(_params(2, spp=64, w=24, h=16, seed=1000 + k))[..., :3].astype(np.float64).mean() for k in range(8)])
    m0, m1 = means[0.0].mean(), means[0.5].mean()
    se = np.sqrt(means[0.0].var(ddof=1) / 8 + means[0.5].var(ddof=1) / 8)
    print(f"share 0: {m0:.6f}, share 0.5: {m1:.6f}, five combined standard errors {5 * se:.6f}")
    assert 5 * se <= 0.02 * m0                                           # a wrong constant cannot pass
    assert abs(m1 - m0) <= 5 * se


# ---- what refuses ----------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_what_cannot_render_an_emitter_refuses(ctx, oracle, cat_golden):
    """RT_ERR_UNSUPPORTED (-5), outputs as they were (filled with -7), "emission" in the error text"""
    import torch
    W, H = 67, 45
    _up(ctx, oracle, cat_golden, "balls")
    p = _params(2)
    frame = ctx.render(p)
    lib, h = ctx._L, ctx._h
    counts = np.full((H, W), 2, np.uint8)
    n_sph = len(SCENES["balls"][0])

    def refused():
        for v in ("path", "lockstep", "global"):
            out = np.full((H, W, 4), -7.0, f32)
            pv = _params(2, variant=v)
            yield v, lib.rt_render(h, C.byref(pv), 0, H, out.ctypes.data_as(FP)), bool((out == -7.0).all())
        work = _capi.Work()
        C.memset(C.byref(work), 7, C.sizeof(work))
        yield "rt_count_work", lib.rt_count_work(h, C.byref(p), 0, H, C.byref(work)), bytes(work) == b"\x07" * C.sizeof(work)
        out = np.full((H, W, 4), -7.0, f32)
        yield "rt_render_counts", lib.rt_render_counts(h, C.byref(p), None, counts.ctypes.data_as(C.POINTER(C.c_uint8)), None, out.ctypes.data_as(FP)), bool((out == -7.0).all())
        buf = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
        poses = [(s[0], s[1]) for s in SCENES["balls"][0]]
        try:
            ctx.render_device_batch(p, _capi.Rows(0, H, H, 1), [(buf.data_ptr(), (0.0, 0.0, 55.0), None, 1)], scenes=[(rt.scenes.LIGHT, poses)])
            rc = 0
        except rt.RtError as e:
            rc = e.code
        ctx.synchronize()
        yield "rt_render_device_batch_scenes", rc, bool((buf.cpu().numpy() == -7.0).all())

    seen = 0
    for what, rc, untouched in refused():
        assert rc == -5 and untouched, (what, rc, untouched)
        assert b"emission" in lib.rt_last_error(h), what
        seen += 1
    assert seen == 6 and n_sph == 5
    for turn_on, turn_off in ((lambda: ctx.set_shutter(light=(6.0, 0.0, -4.0)), lambda: ctx.set_shutter()),
                              (lambda: ctx.set_environment(np.ones((2, 2, 3), f32)), lambda: ctx.set_environment())):
        turn_on()
        out = np.full((H, W, 4), -7.0, f32)
        assert lib.rt_render(h, C.byref(p), 0, H, out.ctypes.data_as(FP)) == -5 and (out == -7.0).all()
        assert b"emission" in lib.rt_last_error(h)
        turn_off()
    _bits_equal(ctx.render(p), frame)
