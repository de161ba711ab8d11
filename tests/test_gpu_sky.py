"""The environment map on the device (rt_scene_set_environment: under a map every wf_advance launch after the opening one is a kFormSky form, and a path whose last
ray leaves the scene folds from what it met there).  -m gpu.  Every case fails on a library without the entry.

Every comparison is on uint32 views, .w (the ray count) included.  References, none of them the code under test:
  what exists   a map set and removed against a context that never heard of one: frames and all three still-view counters; an all-zero map against no map;
  the model     tests/sky_model.py (held to soft_lights_model.py, lights_model.py and the oracle by tests/test_sky_model.py) on scenes that are open: the cat alone, smooth
                and textured, a mirror and a hollow glass ball over a floor, the room with the wall in front of the camera removed;
  closed forms  a constant sky seen directly; one convex diffuse sphere under it.
sigma stays 0 in the model cases: the walkers the model rests on do not restate the jitter.  Frames are 67 x 45 (partial tiles both ways, two sub-frames), 96 x 64 and 1 x 1;
maps have n = 1, 2, 5 and 64.  The C-API cases that need a context live here too."""
import ctypes as C

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi
from raytracinggpu_amd import environment as envm
from . import lens_model as lnm
from . import lights_model as lm
from . import sky_model as sky
from . import still_view as sv
from . import texture_model as tm
from .test_gpu_soft_lights import COUNTS, POSE, THREE, _bits_equal, _differ, _moved, _params, _planar_uv, _texture, _upload, _vertex_normals

pytestmark = pytest.mark.gpu

f32 = np.float32
NEAR = (0.0, 0.0, 20.0)
LENS = (1.5, 45.0)
WAVEFRONTS = ("auto", "wavefront", "wavefront_lds", "wavefront_queue", "lds_verts", "lds_top", "lds_all")
SAMPLING = [(0, 1), (1, 1), (2, 1), (3, 1), (0, 4), (2, 4)]           # (four samples at 0 and 2 bounces: the model walks every path in Python)
RADII = [0.0, 2.0, 5.0]
FLOOR = ((0, -1000, 0), 990, (0.5, 0.5, 0.5))
BALLS = [FLOOR, rt.scenes.DEMO[1], rt.scenes.DEMO[2], rt.scenes.DEMO[3]]      # a diffuse floor, a mirror, a hollow glass ball (one sphere inside the other)
ROOM = rt.scenes.WALLS[1:]                                            # the room without the green wall the camera looks at
OPEN = ("open cat", "smooth open cat", "textured open cat", "balls", "room")
SPHERES = {"open cat": [], "smooth open cat": [], "textured open cat": [], "balls": BALLS, "room": ROOM}


def _maps():
    rng = np.random.default_rng(2112)
    noisy = envm.gradient_sky((0.2, 0.5, 2.0), (1.5, 1.5, 1.5), (0.3, 0.2, 0.1), 64) * rng.uniform(0.5, 1.5, (64, 64, 3)).astype(f32)
    return {1: np.array([[[0.5, 0.75, 1.25]]], f32), 2: rng.uniform(0.0, 2.0, (2, 2, 3)).astype(f32), 5: rng.uniform(0.0, 2.0, (5, 5, 3)).astype(f32) * f32(1e3),
            64: np.ascontiguousarray(noisy, f32)}


MAPS = _maps()


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


def _mesh(g, name):
    return dict(vertices=g["vertices"], indices=g["tri_bvh_order"], bvh_arr10=g["bvh_arr10"], albedo=rt.scenes.CAT_ALBEDO, object_slot=len(SPHERES[name]))


def _up(c, name, g, **kw):
    """one of the open scenes, with the one uploaded light rt.scenes.LIGHT"""
    if name == "balls":
        c.scene_upload(BALLS, None, **kw)
        return
    c.scene_upload(SPHERES[name], _mesh(g, name), **kw)
    v, tv = g["vertices"], np.asarray(g["tri_bvh_order"])[:, :3]
    if name == "smooth open cat":
        c.mesh_set_normals(_vertex_normals(v, tv), tv)
    if name == "textured open cat":
        texels, decode = _texture()
        c.mesh_set_texture(_planar_uv(v), tv, texels, filter="bilinear", decode=decode)


_MODEL = {}


def _oracle_scene(oracle, g, name):
    """-> (oracle scene, materials, surface hook or None), built once"""
    if ("scene", name) in _MODEL:
        return _MODEL[("scene", name)]
    osc = oracle.Scene()
    for s in SPHERES[name]:
        osc.add_sphere(s[0], s[1], s[2], *(s[3:] if len(s) > 3 else ()))
    surface = None
    if name == "balls":
        mats = lm.materials(BALLS)
    else:
        slot = len(SPHERES[name])
        mats = lm.materials(SPHERES[name], [_mesh(g, name)])
        mesh = oracle.Mesh.from_arrays(g["vertices"], g["tri_obj_order"]).build_bvh()
        if name == "smooth open cat":
            mesh.set_normals(_vertex_normals(g["vertices"], np.asarray(g["tri_bvh_order"])[:, :3]), mesh.triangles)
        if name == "textured open cat":
            texels, decode = _texture()
            verts, tris, uvs = mesh.vertices, mesh.triangles, _planar_uv(g["vertices"])

            def surface(oid, O, u, alb):
                if oid != slot:
                    return alb
                found, _, _, tri = mesh.intersect_tri(O, u, 1e-4)
                assert found and tri >= 0
                return tm.surface(verts, tris, tris, uvs, texels, decode, tm.BILINEAR, tm.REPEAT, alb, [tri], np.asarray(O, f32)[None], np.asarray(u, f32)[None])[1][0]
        osc.add_mesh(mesh)
    _MODEL[("scene", name)] = (osc, mats, surface)
    return _MODEL[("scene", name)]


class _LensWalker(sky.Walker, lnm.Walker):
    """the sky walker's path behind the lens walker's camera rays"""


def _model(oracle, g, name, n, b, spp=1, w=67, h=45, pose=None, rows=None, lights=(rt.scenes.LIGHT,), radii=None, lens=None, cam=(0, 0, 55), seed=123456):
    """the model's frame under MAPS[n] (n None: no map), computed once"""
    key = (name, n, b, spp, w, h, pose, None if rows is None else tuple(rows), repr(lights), repr(radii), lens, cam, seed)
    if key not in _MODEL:
        osc, mats, surface = _oracle_scene(oracle, g, name)
        kw = dict(fov=np.pi / 2) if pose is not None else {}
        if lens is not None:
            kw["lens"] = lens
        wk = (_LensWalker if lens is not None else sky.Walker)(osc, mats, list(lights), radii, env=None if n is None else MAPS[n], cam=cam, seed=seed, **kw)
        wk.surface = surface
        _MODEL[key] = wk.render(w, h, spp, b, pose=pose, rows=rows)
    return _MODEL[key]


# ---- the lookup ----------------------------------------------------------------------------------------------------------------------------------------------------------------

def _directions():
    rng = np.random.default_rng(4096)
    n = 1 << 16
    u = rng.standard_normal((n, 3)).astype(f32)
    axes = np.array([(0, 1, 0), (0, -1, 0), (-1, 0, 0), (1, 0, 0), (0, 0, -1), (0, 0, 1), (0, -0.0, 1), (-0.0, -1, -0.0)], f32)
    k = rng.integers(0, 4097, 2000).astype(np.float64)
    seam = np.stack([rng.choice([-1, 1], 2000) * k / 4096, rng.choice([0.0, -0.0, 1e-45, -1e-45, 1e-30, -1e-30], 2000), rng.choice([-1, 1], 2000) * (4096 - k) / 4096], -1).astype(f32)
    border = u[:4000].copy()
    border[:, 1] = -np.abs(border[:, 1]) * f32(1e-4)                  # just below the horizon: the border of the map, where the clamp acts
    border[:2000, 0] *= f32(1e-3)
    bad = np.array([(0, 0, 0), (-0.0, 0, 0), (np.nan, 1, 0), (0, np.nan, 0), (1, 0, np.nan), (np.inf, 0, 0), (0, -np.inf, 1), (3e38, 3e38, 0), (1e-45, 0, 0), (0, -1e-45, 0)], f32)
    scale = np.exp2(rng.uniform(-140, 120, (4000, 1)))
    wide = (rng.standard_normal((4000, 3)) * scale).astype(f32)       # denormal and huge components: the literal quotients
    head = np.concatenate([axes, seam, border, bad, wide])
    u[:len(head)] = head
    return u


@pytest.mark.parametrize("n", [1, 2, 5, 64])
def test_the_lookup_equals_the_model_on_65536_directions(ctx, cat_golden, n):
    _up(ctx, "balls", cat_golden)
    ctx.set_environment(MAPS[n])
    u = _directions()
    assert len(u) == 1 << 16
    exp = sky.sky_radiance(MAPS[n], u)
    _bits_equal(ctx.kat_environment(u), exp)
    assert (exp[:6] > 0).all() and (exp.view(np.uint32) == 0).all(-1).sum() >= 8       # the axes see the map; zero, NaN and overflowing directions see +0
    ctx.set_environment()
    with pytest.raises(rt.RtError):
        ctx.kat_environment(u[:4])                                    # no map: nothing to look up


# ---- exact against what exists -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", ["cat", "demo10", "textured cat"])
def test_a_map_set_and_removed_is_the_context_that_never_heard_of_it(cat_golden, scene):
    """frames and all three still-view counters, on new contexts (nothing cached before)"""
    a, b = rt.Context(0), rt.Context(0)
    try:
        p = _params(2, w=96, h=64)
        for c_ in (a, b):
            _upload(c_, scene, cat_golden)
        a.set_environment(MAPS[5])
        a.set_environment()
        assert a.environment() is None and b.environment() is None
        before = [[getattr(c_, n)() for n in COUNTS] for c_ in (a, b)]
        for _ in range(4):                                            # fill, use, store the records, resume
            _bits_equal(a.render(p), b.render(p))
        assert _moved(a, before[0]) == _moved(b, before[1])
        if scene == "cat":
            assert a.first_shade_cache_counts()["resumed"] > 0        # the shade level was reached: the comparison covers all three
        _bits_equal(a.render_pose(_params(2), rt.make_pose(**POSE)), b.render_pose(_params(2), rt.make_pose(**POSE)))
        _bits_equal(a.render(_params(2, spp=4)), b.render(_params(2, spp=4)))
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("scene", ["open cat", "room", "textured open cat"])
def test_an_all_zero_map_is_the_frame_without_one_and_w_never_changes(ctx, ref, cat_golden, scene):
    for c_ in (ctx, ref):
        _up(c_, scene, cat_golden)
    for n in (1, 5):
        ctx.set_environment(np.zeros((n, n, 3), f32))
        for p in (_params(2), _params(3, spp=4), _params(0, w=1, h=1)):
            _bits_equal(ctx.render(p), ref.render(p))
    ctx.set_environment(MAPS[5])                                      # a lit map: the colours change, the ray counts do not
    lit, dark = ctx.render(_params(3)), ref.render(_params(3))
    _bits_equal(lit[..., 3], dark[..., 3])
    assert _differ(lit, dark) > 300
    ctx.set_lights(THREE)                                             # the soft route: .w against the list without a map
    ref.set_lights(THREE)
    _bits_equal(ctx.render(_params(2))[..., 3], ref.render(_params(2))[..., 3])


# ---- against the model -------------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b,spp", SAMPLING)
@pytest.mark.parametrize("scene", OPEN)
def test_open_scenes_under_a_map_equal_the_model(ctx, oracle, cat_golden, scene, b, spp):
    n = (1, 2, 5, 64)[(OPEN.index(scene) + b + spp) % 4]              # every size meets every scene
    _up(ctx, scene, cat_golden)
    ctx.set_environment(MAPS[n])
    exp = _model(oracle, cat_golden, scene, n, b, spp)
    _bits_equal(ctx.render(_params(b, spp=spp)), exp, f"n = {n}")
    assert _differ(exp, _model(oracle, cat_golden, scene, None, b, spp)) > 300            # the map does reach the frame


def test_sky_only_a_light_list_and_radii_equal_the_model(ctx, oracle, cat_golden):
    for scene, n in (("open cat", 64), ("room", 5)):
        _up(ctx, scene, cat_golden)
        ctx.set_environment(MAPS[n])
        dark = [(rt.scenes.LIGHT[0], 0.0)]
        ctx.set_light(*dark[0])                                       # intensity 0: the sky alone lights the scene
        exp = _model(oracle, cat_golden, scene, n, 2, lights=dark)
        _bits_equal(ctx.render(_params(2)), exp, "sky only")
        assert (exp[..., :3] > 0).any()
        ctx.set_lights(THREE)                                         # a list without radii: the soft forms with radii 0, held to the walker that is lights_model's
        _bits_equal(ctx.render(_params(2)), _model(oracle, cat_golden, scene, n, 2, lights=THREE), "three lights")
        _bits_equal(ctx.render(_params(1, spp=4)), _model(oracle, cat_golden, scene, n, 1, 4, lights=THREE), "three lights, four samples")
        ctx.set_light_radii(RADII)
        soft = _model(oracle, cat_golden, scene, n, 2, lights=THREE, radii=RADII)
        _bits_equal(ctx.render(_params(2)), soft, "radii")
        assert _differ(soft, _model(oracle, cat_golden, scene, n, 2, lights=THREE)) > 100
    _up(ctx, "textured open cat", cat_golden)                         # tex | soft | sky
    ctx.set_environment(MAPS[2])
    ctx.set_lights(THREE)
    ctx.set_light_radii(RADII)
    _bits_equal(ctx.render(_params(2)), _model(oracle, cat_golden, "textured open cat", 2, 2, lights=THREE, radii=RADII), "textured, radii")


def test_lens_posed_camera_row_shares_one_pixel_and_every_wavefront_variant_equal_the_model(ctx, oracle, cat_golden):
    import torch
    _up(ctx, "open cat", cat_golden)
    ctx.set_environment(MAPS[64])
    p = _params(2)
    whole = _model(oracle, cat_golden, "open cat", 64, 2)
    ctx.set_lens(*LENS)                                               # the opening launch is the lens's own; the later ones meet the sky
    for spp in (1, 4):
        _bits_equal(ctx.render(_params(2, spp=spp)), _model(oracle, cat_golden, "open cat", 64, 2, spp, lens=LENS), f"lens, spp {spp}")
    assert _differ(_model(oracle, cat_golden, "open cat", 64, 2, lens=LENS), whole) > 300
    ctx.set_lens(0.0, 1.0)
    near = ctx.render_pose(p, rt.make_pose(position=NEAR, **POSE))
    _bits_equal(near, _model(oracle, cat_golden, "open cat", 64, 2, pose=(POSE["yaw"], POSE["pitch"]), cam=NEAR))
    _bits_equal(ctx.render(p, 13, 31), whole[13:31])                  # starts and ends inside an 8-row tile
    share, image_rows = rt.interleaved_rows(45, 8, 1, 3)              # tiles 1 and 4 of six: rows 8 .. 15 and 32 .. 39
    buf = torch.zeros((share.n_rows, 67, 4), dtype=torch.float32, device="cuda")
    ctx.render_device(p, share, buf.data_ptr())
    ctx.synchronize()
    _bits_equal(buf.cpu().numpy(), whole[list(image_rows)])
    _bits_equal(np.concatenate([ctx.render(p, 0, 20), ctx.render(p, 20, 45)]), whole)      # two row shares against the whole frame
    _bits_equal(ctx.render(_params(2, w=1, h=1)), _model(oracle, cat_golden, "open cat", 64, 2, w=1, h=1))
    for v in WAVEFRONTS:
        _bits_equal(ctx.render(_params(2, variant=v)), whole, v)
    _up(ctx, "balls", cat_golden)                                     # no mesh: auto is never lockstep under a map
    ctx.set_environment(MAPS[5])
    for v in ("auto", "wavefront", "wavefront_queue"):
        _bits_equal(ctx.render(_params(3, variant=v)), _model(oracle, cat_golden, "balls", 5, 3), v)


@pytest.mark.parametrize("knobs", [dict(RT_PARTS="1"), dict(RT_PARTS="3"), dict(RT_DEAD_CHANNELS="0"), dict(RT_TRAVQ_ANYHIT="0")])
def test_other_cuts_and_knobs_render_the_same_words(ctx, oracle, cat_golden, knobs):
    """the room with a wall removed: pure-colour walls kill channels of paths that then escape"""
    c_ = sv.context(**knobs)
    try:
        for scene, n, b, spp in (("room", 5, 3, 1), ("open cat", 2, 2, 4)):
            _up(c_, scene, cat_golden)
            c_.set_environment(MAPS[n])
            got = c_.render(_params(b, spp=spp))
            exp = _model(oracle, cat_golden, scene, n, b, spp)
            _bits_equal(got, exp, f"{knobs} {scene}")
            _up(ctx, scene, cat_golden)                               # ... and the default context's frame
            ctx.set_environment(MAPS[n])
            _bits_equal(got, ctx.render(_params(b, spp=spp)), f"{knobs} {scene} against the default")
        if "RT_PARTS" in knobs:
            assert c_.stats()["parts"] == int(knobs["RT_PARTS"])
    finally:
        c_.close()


def test_a_batch_of_three_cameras_async_and_pipelined_frames(ctx, ref, oracle, cat_golden):
    import torch
    W, H = 67, 45
    _up(ctx, "open cat", cat_golden)
    ctx.set_environment(MAPS[5])
    rows = _capi.Rows(0, H, H, 1)
    cams = [((0.5 * k, 0.0, 55.0 - 3 * k), 40 + k) for k in range(3)]
    bufs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in cams]
    ctx.render_device_batch(_params(2), rows, [(bf.data_ptr(), cam, None, seed) for bf, (cam, seed) in zip(bufs, cams)])
    ctx.synchronize()
    for bf, (cam, seed) in zip(bufs, cams):
        _up(ref, "open cat", cat_golden, camera=(cam, None))
        ref.set_environment(MAPS[5])
        _bits_equal(bf.cpu().numpy(), ref.render(_params(2, seed=seed)), str(cam))
    cam, seed = cams[1]
    _bits_equal(bufs[1].cpu().numpy(), _model(oracle, cat_golden, "open cat", 5, 2, cam=cam, seed=seed))
    out = rt.PinnedArray((H, W, 4), np.float32)
    try:
        ctx.render_async(_params(2), out.array, slot=0)
        ctx.wait(0)
        _bits_equal(out.array, _model(oracle, cat_golden, "open cat", 5, 2))
    finally:
        out.close()
    # pipelined frames into alternating buffers, the map replaced between them: frame k is the lone frame of its map
    order = [5, 2, None, 64, 2, 5]
    want = {}
    for n in set(order):
        ctx.set_environment(None if n is None else MAPS[n])
        want[n] = ctx.render(_params(2, seed=77))
    assert _differ(want[5], want[2]) > 100 and _differ(want[5], want[None]) > 100
    pair = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    got = []
    ctx.set_pipelining(True)
    try:
        for k, n in enumerate(order):
            ctx.set_environment(None if n is None else MAPS[n])
            ctx.render_device(_params(2, seed=77), rows, pair[k % 2].data_ptr())
            if k % 2 == 1:                                            # both buffers hold a frame: read them before the next two overwrite them
                ctx.synchronize()
                got.extend(b.cpu().numpy() for b in pair)
    finally:
        ctx.set_pipelining(False)
    for k, g in enumerate(got):
        _bits_equal(g, want[order[k]], f"pipelined frame {k}")


# ---- closed forms ----------------------------------------------------------------------------------------------------------------------------------------------------------

def test_a_constant_sky_seen_directly_and_one_diffuse_sphere_under_it(ctx, cat_golden):
    E = MAPS[1][0, 0]
    _up(ctx, "open cat", cat_golden)
    ctx.set_environment(MAPS[1])
    out = ctx.render(_params(0, w=96, h=64))
    miss = out[..., 3] == 1                                           # one ray: the camera ray found nothing
    assert miss.sum() > 1000 and (~miss).sum() > 100
    assert (out[miss][:, :3].view(np.uint32) == E.view(np.uint32)).all()
    # one convex diffuse sphere of albedo rho alone under E, the light dark: a pixel on it folds one segment, l = +0, from the E its bounce ray met
    rho = np.array([0.5, 0.25, 1.0], f32)
    ctx.scene_upload([((0, 0, 0), 10.0, tuple(float(x) for x in rho))], None, light=(rt.scenes.LIGHT[0], 0.0))
    ctx.set_environment(MAPS[1])
    want = (((f32(0) * rho).astype(f32) / f32(lm.PI)).astype(f32) + (rho * E).astype(f32)).astype(f32)
    for b in (1, 3):
        out = ctx.render(_params(b, w=96, h=64))
        on = out[..., 3] > 1
        assert on.sum() > 300 and (out[on][:, 3] == 3).all()          # camera ray, shadow ray, the bounce ray that escapes
        assert (out[on][:, :3].view(np.uint32) == want.view(np.uint32)).all()
        assert (out[~on][:, :3].view(np.uint32) == E.view(np.uint32)).all()


# ---- the still view ----------------------------------------------------------------------------------------------------------------------------------------------------------

def test_sky_frames_leave_the_still_view_alone_and_a_frame_without_a_map_again_is_cold(cat_golden):
    c_, cold = rt.Context(0), sv.context(RT_FIRST_HIT_CACHE="0")
    try:
        for x in (c_, cold):
            _upload(x, "cat", cat_golden)
        p = _params(2, w=96, h=64)
        exp = cold.render(p)
        for _ in range(4):                                            # the levels are full
            _bits_equal(c_.render(p), exp)
        c_.set_environment(MAPS[5])
        before = [getattr(c_, n)() for n in COUNTS]
        assert sum(len(b) for b in before) == 12                      # three levels, four counters each
        frames = [c_.render(p) for _ in range(3)]
        assert [getattr(c_, n)() for n in COUNTS] == before           # the twelve counters of all three levels, the ineligible chains' too
        for f in frames[1:]:
            _bits_equal(f, frames[0])
        cold.set_environment(MAPS[5])
        _bits_equal(cold.render(p), frames[0])
        # the map removed: the next frame is the cold frame, and its chains fill -- nothing stored before the map was set is used
        c_.set_environment()
        n = c_.stats()["parts"]
        _bits_equal(c_.render(p), exp)
        hit, sh, rec = _moved(c_, before)
        assert hit["filled"] == n and hit["skipped"] == 0 and sh["filled"] == n and sh["skipped"] == 0 and rec["resumed"] == 0, (hit, sh, rec)
        for _ in range(3):
            _bits_equal(c_.render(p), exp)
        assert _moved(c_, before)[2]["resumed"] > 0
    finally:
        c_.close()
        cold.close()


# ---- the boundary, on a context --------------------------------------------------------------------------------------------------------------------------------------------

def _state(c):
    e = c.environment()
    return b"" if e is None else bytes([e.shape[0] % 256]) + e.tobytes()


def test_get_after_set_edits_keep_it_uploads_remove_it_and_what_is_refused(ctx, ref, cat_golden):
    _up(ctx, "room", cat_golden)
    assert ctx.environment() is None
    for n in (1, 2, 5, 64):
        ctx.set_environment(MAPS[n])
        back = ctx.environment()
        assert back.shape == (n, n, 3)
        _bits_equal(back, MAPS[n])
    ctx.set_environment(MAPS[5])
    was = _state(ctx)
    frame = ctx.render(_params(2))
    # the sphere, light, lens and shutter edits keep the map
    ctx.move_sphere(0, (0.0, 2.0, 0.0), 0.5)
    ctx.set_sphere(0, ROOM[0])
    ctx.move_light(0.3, 0.5)
    ctx.set_light(*rt.scenes.LIGHT)
    ctx.set_lens(*LENS)
    ctx.set_lens(0.0, 1.0)
    ctx.set_shutter(light=(1.0, 0.0, 0.0))
    ctx.set_shutter()
    assert _state(ctx) == was
    _bits_equal(ctx.render(_params(2)), frame)
    lib, h = ctx._L, ctx._h
    fp = C.POINTER(C.c_float)
    ok = np.ascontiguousarray(MAPS[2])
    assert lib.rt_scene_set_environment(h, -1, ok.ctypes.data_as(fp)) == -1 and b"environment" in lib.rt_last_error(h) and _state(ctx) == was
    assert lib.rt_scene_set_environment(h, 1025, ok.ctypes.data_as(fp)) == -1 and _state(ctx) == was
    assert lib.rt_scene_set_environment(h, 2, None) == -1 and _state(ctx) == was
    for bad in (np.nan, np.inf, -np.inf, -1.0, -0.0, 2.0 ** 96, -1e-45):
        for at in (0, 7, 11):
            m = ok.copy()
            m.reshape(-1)[at] = bad
            assert lib.rt_scene_set_environment(h, 2, m.ctypes.data_as(fp)) == -1, (bad, at)
            assert b"environment" in lib.rt_last_error(h)
            assert _state(ctx) == was
    m = ok.copy()
    m.reshape(-1)[3] = np.nextafter(f32(2.0 ** 96), f32(0))          # the largest texel there is, and the smallest
    m.reshape(-1)[4] = 1e-45
    assert lib.rt_scene_set_environment(h, 2, m.ctypes.data_as(fp)) == 0
    _bits_equal(ctx.environment(), m)
    ctx.set_environment(MAPS[5])
    assert lib.rt_scene_get_environment(h, None, None) == -1 and _state(ctx) == was
    _bits_equal(ctx.render(_params(2)), frame)                        # nothing that was refused reached the frame
    _up(ctx, "room", cat_golden)                                      # an upload removes the map: it belongs to the scene
    assert ctx.environment() is None
    _up(ref, "room", cat_golden)
    _bits_equal(ctx.render(_params(2)), ref.render(_params(2)))
    fresh = rt.Context(0)                                             # no upload: RT_ERR_NO_SCENE, and the get writes nothing
    try:
        n = C.c_int(-7)
        out = np.full(12, -7.0, f32)
        assert fresh._L.rt_scene_get_environment(fresh._h, C.byref(n), out.ctypes.data_as(fp)) == -4 and n.value == -7 and (out == -7.0).all()
        assert fresh._L.rt_scene_set_environment(fresh._h, 2, ok.ctypes.data_as(fp)) == -4 and fresh._L.rt_scene_set_environment(fresh._h, 0, None) == -4
    finally:
        fresh.close()


def test_what_cannot_render_an_environment_refuses(ctx, cat_golden):
    """RT_ERR_UNSUPPORTED (-5), outputs as they were (filled with -7), "environment" in the error text, the state and a following frame unchanged; without the map each works"""
    import torch
    W, H = 67, 45
    _upload(ctx, "cat", cat_golden)
    ctx.set_environment(MAPS[5])
    p = _params(2)
    frame = ctx.render(p)
    was = _state(ctx)
    lib, h = ctx._L, ctx._h
    fp = C.POINTER(C.c_float)
    rows = _capi.Rows(0, H, H, 1)
    poses = [((s[0]), float(s[1])) for s in rt.scenes.spheres("cpu")]
    counts = np.full((H, W), 2, np.uint8)
    dcounts = torch.full((H, W), 2, dtype=torch.uint8, device="cuda")

    def after(what):
        assert _state(ctx) == was, what
        _bits_equal(ctx.render(p), frame, what)

    def refused():
        for v in ("path", "lockstep", "global"):
            out = np.full((H, W, 4), -7.0, f32)
            pv = _params(2, variant=v)
            yield v, lib.rt_render(h, C.byref(pv), 0, H, out.ctypes.data_as(fp)), bool((out == -7.0).all())
        work = _capi.Work()
        C.memset(C.byref(work), 7, C.sizeof(work))
        yield "rt_count_work", lib.rt_count_work(h, C.byref(p), 0, H, C.byref(work)), bytes(work) == b"\x07" * C.sizeof(work)
        out = np.full((H, W, 4), -7.0, f32)
        yield "rt_render_counts", lib.rt_render_counts(h, C.byref(p), None, counts.ctypes.data_as(C.POINTER(C.c_uint8)), None, out.ctypes.data_as(fp)), bool((out == -7.0).all())
        dout = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
        rc = lib.rt_render_counts_device(h, C.byref(p), None, C.c_void_p(dcounts.data_ptr()), None, C.c_void_p(dout.data_ptr()), None)
        ctx.synchronize()
        yield "rt_render_counts_device", rc, bool((dout == -7.0).all())
        bufs = [torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda") for _ in range(2)]
        frames = [(bf.data_ptr(), (0.0, 0.0, 55.0), None, 123456) for bf in bufs]
        try:
            ctx.render_device_batch(p, rows, frames, scenes=[(THREE[0], poses), (THREE[1], poses)])
            rc = 0
        except rt.RtError as e:
            rc = e.code
        ctx.synchronize()
        yield "rt_render_device_batch_scenes", rc, all(bool((bf == -7.0).all()) for bf in bufs)

    seen = []
    for what, rc, untouched in refused():
        assert rc == -5 and untouched, (what, rc, untouched)
        assert b"environment" in lib.rt_last_error(h), what
        after(what)
        seen.append(what)
    assert len(seen) == 7
    # the shutter on under a map: no form takes both, whatever the variant
    ctx.set_shutter(light=(6.0, 0.0, -4.0))
    for v in ("auto", "wavefront"):
        out = np.full((H, W, 4), -7.0, f32)
        pv = _params(2, variant=v)
        assert lib.rt_render(h, C.byref(pv), 0, H, out.ctypes.data_as(fp)) == -5 and (out == -7.0).all(), v
        assert b"environment" in lib.rt_last_error(h), v
    assert _state(ctx) == was
    ctx.set_environment()                                             # without the map the shutter frame renders
    assert _differ(ctx.render(p), frame) > 100
    ctx.set_shutter()
    ctx.set_environment(MAPS[5])
    after("the shutter closed again")
    ctx.set_environment()                                             # removed: each of them works
    for what, rc, untouched in refused():
        assert rc == 0 and not untouched, (what, rc, untouched)
    assert ctx.count_work(p)["rays"] > 0


def test_a_progressive_frame_and_the_svgf_sequence(ctx, cat_golden):
    W, H = 96, 64
    _up(ctx, "open cat", cat_golden)
    pose = rt.make_pose(position=NEAR, **POSE)
    ctx.progressive_reset()
    dark, _ = ctx.progressive_frame(_params(2), pose)
    ctx.set_environment(MAPS[64])
    ctx.progressive_reset()
    lit, _ = ctx.progressive_frame(_params(2), pose)
    assert np.isfinite(lit).all() and _differ(lit, dark) > 300
    ctx.set_environment()

    def run():
        outs = []
        with rt.SvgfSequence(ctx, W, H) as seq:
            for i in range(3):
                ptr = seq.frame(_params(2, w=W, h=H, seed=100 + i))
                ctx.synchronize()
                outs.append(ctx.device_to_host(ptr, (H, W, 4)))
        return outs

    plain = run()
    ctx.set_environment(MAPS[5])
    ctx.set_environment()
    for a, b in zip(run(), plain):                                    # set and removed: the sequence is itself
        _bits_equal(a, b)
    ctx.set_environment(MAPS[5])
    on = run()
    assert all(np.isfinite(o).all() for o in on)
    assert _differ(on[2], plain[2]) > 100
