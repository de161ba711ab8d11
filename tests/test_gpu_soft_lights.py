"""Point lights with a radius on the device (rt_scene_set_light_radii: one point of the picked light's shell per shadow ray).  -m gpu.

Every comparison is on uint32 views, .w (the ray count) included.  References, none of them the code under test:
  what exists   radii set explicitly to 0 against the same context type without the call; one soft light against three co-located ones of the same radius;
  the model     tests/soft_lights_model.py (held to lights_model.py and to the oracle by tests/test_soft_lights_model.py): segments, samples, a posed camera, row shares,
                smooth normals, a texture (tests/texture_model.py), a shell that reaches through a wall and into spheres.
Frames are 96 x 64, 67 x 45 (partial tiles both ways, two sub-frames) and 1 x 1."""
import ctypes as C
import functools

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi
from . import lights_model as lm
from . import material_scenes as ms
from . import soft_lights_model as sm
from . import still_view as sv
from . import texture_model as tm

pytestmark = pytest.mark.gpu

SLOT = 6
I0 = 3e10                                                             # rt.scenes.LIGHT's intensity: I0 / 4 and I0 / 2 are exact
P_A, P_B, P_C = (-10.0, 20.0, 40.0), (15.0, 25.0, 30.0), (0.0, 35.0, 5.0)
ONE, ONE_R = [(P_B, I0)], [3.0]
THREE, THREE_R = [(P_A, 1e10), (P_B, 2e10), (P_C, 5e10)], [0.0, 2.0, 5.0]
LISTS = {"one": (ONE, ONE_R), "three": (THREE, THREE_R)}
POSE = dict(yaw=0.2, pitch=0.1)
COUNTS = ("first_hit_cache_counts", "first_shadow_cache_counts", "first_shade_cache_counts")
SCENES = ("cat", "two_cats", "demo10", "smooth cat", "textured cat")


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


def _bits_equal(a, b, msg=""):
    np.testing.assert_array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32), err_msg=msg)


def _differ(a, b):
    return int((np.ascontiguousarray(a[..., :3], np.float32).view(np.uint32) != np.ascontiguousarray(b[..., :3], np.float32).view(np.uint32)).any(-1).sum())


def _params(b, spp=1, w=67, h=45, variant="auto", **kw):
    d = dict(rt.scenes.CPU_LAUNCHER)
    d.update(kw)
    return rt.make_params(w, h, spp, b, variant=variant, **d)


def _cat(g):
    return dict(vertices=g["vertices"], indices=g["tri_bvh_order"], bvh_arr10=g["bvh_arr10"], albedo=rt.scenes.CAT_ALBEDO, object_slot=SLOT)


def _vertex_normals(v, tv):
    vn = np.zeros_like(np.asarray(v, np.float64))
    fn = np.cross(v[tv[:, 1]] - v[tv[:, 0]], v[tv[:, 2]] - v[tv[:, 0]])
    for k in range(3):
        np.add.at(vn, tv[:, k], fn)
    return (vn / np.maximum(np.linalg.norm(vn, axis=1, keepdims=True), 1e-20)).astype(np.float32)


def _planar_uv(v):
    v = np.asarray(v, np.float32)
    lo, hi = v.min(0), v.max(0)
    return (((v[:, :2] - lo[:2]) / (hi[:2] - lo[:2])) * np.float32(2.6) - np.float32(0.8)).astype(np.float32)


def _texture():
    rng = np.random.default_rng(21)
    return rng.integers(0, 256, size=(23, 37, 3), dtype=np.uint8), rng.random(256).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _two_cats():
    g = np.load(rt.scenes.CAT_FIXTURE, allow_pickle=False)
    return ms.capi_scene("two_cats", g["vertices"], g["tri_obj_order"])     # (builds two trees: once)


def _upload(c, name, g):
    """one of the test scenes, with the one uploaded light rt.scenes.LIGHT"""
    if name == "two_cats":
        c.scene_upload(*_two_cats())
    elif name == "demo10":
        c.scene_upload(rt.scenes.spheres("demo10"), None)
    else:
        c.scene_upload(rt.scenes.spheres("cpu"), _cat(g))
        v, tv = g["vertices"], np.asarray(g["tri_bvh_order"])[:, :3]
        if name == "smooth cat":
            c.mesh_set_normals(_vertex_normals(v, tv), tv)
        if name == "textured cat":
            texels, decode = _texture()
            c.mesh_set_texture(_planar_uv(v), tv, texels, filter="bilinear", decode=decode)


def _light(c, lights, radii=None):
    """the list (one light: rt_scene_set_light), then its radii"""
    if len(lights) == 1:
        c.set_light(*lights[0])
    else:
        c.set_lights(lights)
    if radii is not None:
        c.set_light_radii(radii)


def _shot(c, mode, w=67, h=45):
    if mode == "plain":
        return c.render(_params(2, w=w, h=h))
    if mode == "posed":
        return c.render_pose(_params(2, w=w, h=h), rt.make_pose(**POSE))
    if mode == "spp4":
        return c.render(_params(2, spp=4, w=w, h=h))
    raise ValueError(mode)


def _moved(c, before):
    return [{k: getattr(c, n)()[k] - b[k] for k in b if k != "key_misses"} for n, b in zip(COUNTS, before)]


# ---- exact against what exists -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", SCENES)
def test_radii_zero_is_the_frame_without_the_call(ctx, ref, cat_golden, scene):
    """a list of one and a list of three; frames and all three still-view counters"""
    p = _params(2, w=96, h=64)
    for lights in (ONE, THREE):
        for c_ in (ctx, ref):
            _upload(c_, scene, cat_golden)
        _light(ctx, lights, [0.0] * len(lights))
        _light(ref, lights)
        assert ctx.light_radii() == [0.0] * len(lights) == ref.light_radii()
        before = [[getattr(c_, n)() for n in COUNTS] for c_ in (ctx, ref)]
        for _ in range(4):                                            # fill, use, store the records, resume
            _bits_equal(ctx.render(p), ref.render(p))
        a, b = _moved(ctx, before[0]), _moved(ref, before[1])
        assert a == b, (a, b)
        if scene == "cat" and len(lights) == 1:
            assert a[2]["resumed"] > 0                                # the shade level was reached: the comparison covers all three
        for mode in ("posed", "spp4"):
            _bits_equal(_shot(ctx, mode), _shot(ref, mode), mode)


@pytest.mark.parametrize("scene", SCENES)
def test_one_soft_light_is_three_co_located_ones(ctx, ref, cat_golden, scene):
    """I/4, I/2, I/4 at one position with one radius: the direction does not depend on k and the prefix sums are exact"""
    for c_ in (ctx, ref):
        _upload(c_, scene, cat_golden)
    _light(ref, [(P_B, I0)], [3.0])
    _light(ctx, [(P_B, I0 / 4), (P_B, I0 / 2), (P_B, I0 / 4)], [3.0, 3.0, 3.0])
    for mode in ("plain", "posed", "spp4"):
        exp = _shot(ref, mode)
        assert exp[..., 3].sum() > 0
        _bits_equal(_shot(ctx, mode), exp, mode)
    _bits_equal(_shot(ctx, "plain", 1, 1), _shot(ref, "plain", 1, 1))
    point = _shot(ref, "plain")
    ref.set_light_radius_at(0, 0.0)
    assert _differ(point, _shot(ref, "plain")) > 300                  # the radius does change the frame


# ---- against the model -------------------------------------------------------------------------------------------------------------------------------------------------------

_MODEL = {}


def _oracle_scene(oracle, oracle_cat, g, name):
    """-> (oracle scene, materials, surface hook or None)"""
    if name == "demo10":
        return oracle.Scene.preset("demo10"), lm.materials(rt.scenes.spheres("demo10")), None
    if name == "two_cats":
        spheres, meshes = _two_cats()
        return ms.oracle_scene(oracle, "two_cats", g["vertices"], g["tri_obj_order"]), lm.materials(spheres, meshes), None
    mats = lm.materials(rt.scenes.spheres("cpu"), [_cat(g)])
    if name == "cat":
        return oracle.Scene.preset("cpu", oracle_cat), mats, None
    mesh = oracle.Mesh.from_arrays(g["vertices"], g["tri_obj_order"]).build_bvh()      # (its own mesh: the session's stays flat)
    surface = None
    if name == "smooth cat":
        mesh.set_normals(_vertex_normals(g["vertices"], np.asarray(g["tri_bvh_order"])[:, :3]), mesh.triangles)
    else:
        texels, decode = _texture()
        verts, tris, uvs = mesh.vertices, mesh.triangles, _planar_uv(g["vertices"])

        def surface(oid, O, u, alb):
            if oid != SLOT:
                return alb
            found, _, _, tri = mesh.intersect_tri(O, u, 1e-4)
            assert found and tri >= 0
            return tm.surface(verts, tris, tris, uvs, texels, decode, tm.BILINEAR, tm.REPEAT, alb, [tri], np.asarray(O, np.float32)[None], np.asarray(u, np.float32)[None])[1][0]
    return oracle.Scene.preset("cpu", mesh), mats, surface


def _walker(oracle, oracle_cat, g, name, lights, radii, **kw):
    if ("scene", name) not in _MODEL:
        _MODEL[("scene", name)] = _oracle_scene(oracle, oracle_cat, g, name)
    osc, mats, surface = _MODEL[("scene", name)]
    w = sm.Walker(osc, mats, lights, radii, **kw)
    w.surface = surface
    return w


def _model(oracle, oracle_cat, g, name, which, b, spp=1, w=67, h=45, pose=None, rows=None):
    """the model's frame, computed once"""
    key = (name, which, b, spp, w, h, pose, None if rows is None else tuple(rows))
    if key not in _MODEL:
        kw = dict(fov=np.pi / 2) if pose is not None else {}
        _MODEL[key] = _walker(oracle, oracle_cat, g, name, *LISTS[which], **kw).render(w, h, spp, b, pose=pose, rows=rows)
    return _MODEL[key]


@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("b", [0, 2, 3])
@pytest.mark.parametrize("which", ["one", "three"])
@pytest.mark.parametrize("scene", ["cat", "demo10", "two_cats"])
def test_frames_equal_the_model(ctx, oracle, oracle_cat, cat_golden, scene, which, b, spp):
    _upload(ctx, scene, cat_golden)
    _light(ctx, *LISTS[which])
    exp = _model(oracle, oracle_cat, cat_golden, scene, which, b, spp)
    _bits_equal(ctx.render(_params(b, spp=spp)), exp)
    assert exp[..., 3].max() >= 2 and (exp[..., :3] > 0).any()


@pytest.mark.parametrize("which", ["one", "three"])
@pytest.mark.parametrize("scene", ["smooth cat", "textured cat"])
def test_smooth_and_textured_frames_equal_the_model(ctx, oracle, oracle_cat, cat_golden, scene, which):
    _upload(ctx, scene, cat_golden)
    _light(ctx, *LISTS[which])
    exp = _model(oracle, oracle_cat, cat_golden, scene, which, 2)
    _bits_equal(ctx.render(_params(2)), exp)
    assert _differ(exp, _model(oracle, oracle_cat, cat_golden, "cat", which, 2)) > 50      # the normals / the texture do reach the frame


def test_posed_camera_interleaved_rows_and_one_pixel_equal_the_model(ctx, oracle, oracle_cat, cat_golden):
    import torch
    _upload(ctx, "cat", cat_golden)
    _light(ctx, THREE, THREE_R)
    p = _params(2)
    _bits_equal(ctx.render_pose(p, rt.make_pose(**POSE)), _model(oracle, oracle_cat, cat_golden, "cat", "three", 2, pose=(POSE["yaw"], POSE["pitch"])))
    rows, image_rows = rt.interleaved_rows(45, 8, 1, 3)               # tiles 1 and 4 of six: rows 8 .. 15 and 32 .. 39
    buf = torch.zeros((rows.n_rows, 67, 4), dtype=torch.float32, device="cuda")
    ctx.render_device(p, rows, buf.data_ptr())
    ctx.synchronize()
    _bits_equal(buf.cpu().numpy(), _model(oracle, oracle_cat, cat_golden, "cat", "three", 2)[list(image_rows)])
    for which in LISTS:
        _light(ctx, *LISTS[which])
        _bits_equal(ctx.render(_params(2, w=1, h=1)), _model(oracle, oracle_cat, cat_golden, "cat", which, 2, w=1, h=1))


@pytest.mark.parametrize("knobs", [dict(RT_PARTS="1"), dict(RT_PARTS="2"), dict(RT_PARTS="3"), dict(RT_TRAVQ_ANYHIT="0"), dict(RT_DEAD_CHANNELS="0")])
def test_other_cuts_and_rules_render_the_same_words(oracle, oracle_cat, cat_golden, knobs):
    """RT_PARTS 1, 2 and 3; any-hit off; the dead-channel rule off: the model's frame, word for word"""
    c_ = sv.context(**knobs)
    try:
        _upload(c_, "cat", cat_golden)
        for which in LISTS:
            _light(c_, *LISTS[which])
            for spp in (1, 3):
                _bits_equal(c_.render(_params(2, spp=spp)), _model(oracle, oracle_cat, cat_golden, "cat", which, 2, spp), f"{knobs} {which} {spp}")
        if "RT_PARTS" in knobs:
            assert c_.stats()["parts"] == int(knobs["RT_PARTS"])
    finally:
        c_.close()


def test_a_batch_of_three_equals_the_lone_frames_and_async(ctx, ref, cat_golden):
    import torch
    W, H = 67, 45
    _upload(ctx, "cat", cat_golden)
    _light(ctx, THREE, THREE_R)
    rows = _capi.Rows(0, H, H, 1)
    cams = [((0.5 * k, 0.0, 55.0 - 3 * k), 40 + k) for k in range(3)]
    bufs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in cams]
    ctx.render_device_batch(_params(2), rows, [(bf.data_ptr(), cam, None, seed) for bf, (cam, seed) in zip(bufs, cams)])
    ctx.synchronize()
    for bf, (cam, seed) in zip(bufs, cams):
        ref.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden), camera=(cam, None))
        _light(ref, THREE, THREE_R)
        _bits_equal(bf.cpu().numpy(), ref.render(_params(2, seed=seed)), str(cam))
    out = rt.PinnedArray((H, W, 4), np.float32)                       # rt_render_async goes through the same entries
    try:
        ctx.render_async(_params(2), out.array, slot=0)
        ctx.wait(0)
        _bits_equal(out.array, ctx.render(_params(2)))
    finally:
        out.close()


def test_a_shell_larger_than_the_room_allows(ctx, oracle, oracle_cat, cat_golden):
    """the ten-sphere scene, the light at (-20, 25, 0) with radius 40: the ceiling is 35 away, the floor 35, and the shell passes through the spheres at the origin and at
    (20, 0, 0) -- some L' lie behind a wall, some inside a sphere (counted on the model's own points), and the frame is the model's"""
    lights, radii = [((-20.0, 25.0, 0.0), I0)], [40.0]
    _upload(ctx, "demo10", cat_golden)
    _light(ctx, lights, radii)
    for b, spp in ((0, 1), (2, 3)):
        w = _walker(oracle, oracle_cat, cat_golden, "demo10", lights, radii)
        exp = w.render(67, 45, spp, b)
        _bits_equal(ctx.render(_params(b, spp=spp)), exp, f"b {b} spp {spp}")
    inside = dict(wall=0, sphere=0, room=0, lit=0)
    for pixel, samp, d, _, lit in w.picks:
        Lp = w.light_point(pixel, samp, d)[1].astype(np.float64)
        hit = [np.linalg.norm(Lp - np.asarray(s[0], np.float64)) < s[1] for s in rt.scenes.spheres("demo10")]
        inside["sphere"] += any(hit[:4])
        inside["wall"] += any(hit[4:])
        inside["room"] += not any(hit)
        inside["lit"] += lit
    print(inside)
    assert min(inside.values()) >= 100, inside


# ---- the still view ----------------------------------------------------------------------------------------------------------------------------------------------------------

def test_soft_keeps_the_hit_level_only_and_a_point_again_fills_the_others(ctx, ref, cat_golden):
    for c_ in (ctx, ref):
        _upload(c_, "cat", cat_golden)
    _light(ctx, ONE, ONE_R)
    _light(ref, ONE)
    p = _params(2, w=96, h=64)
    before = [getattr(ctx, n)() for n in COUNTS]
    frames = [ctx.render(p) for _ in range(3)]
    hit, sh, rec = _moved(ctx, before)
    n = ctx.stats()["parts"]
    assert hit["filled"] == n and hit["skipped"] == 2 * n
    assert sh["skipped"] == 0 and sh["filled"] == 0 and rec["resumed"] == 0 and rec["filled"] == 0
    for f in frames[1:]:
        _bits_equal(f, frames[0])
    off = sv.context(RT_FIRST_HIT_CACHE="0")
    try:
        _upload(off, "cat", cat_golden)
        _light(off, ONE, ONE_R)
        _bits_equal(off.render(p), frames[0])
    finally:
        off.close()
    # the radius returns to 0: the shadow and shade levels fill again, and the frames are the point light's
    ctx.set_light_radius_at(0, 0.0)
    before = [getattr(ctx, n)() for n in COUNTS]
    exp = ref.render(p)
    for _ in range(4):
        _bits_equal(ctx.render(p), exp)
    hit, sh, rec = _moved(ctx, before)
    assert sh["filled"] == n and sh["skipped"] > 0 and rec["filled"] == n and rec["resumed"] > 0, (hit, sh, rec)
    # ... and a radius set while the point light's levels are full is a light change: nothing stale is used
    ctx.set_light_radii(ONE_R)
    _bits_equal(ctx.render(p), frames[0])
    ctx.set_light_radii([0.0])
    before = [getattr(ctx, n)() for n in COUNTS]
    _bits_equal(ctx.render(p), exp)
    assert _moved(ctx, before)[1]["filled"] == n                      # filled again, not used


# ---- edits -------------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_edits_of_radii_and_what_keeps_them(ctx, ref, cat_golden):
    for c_ in (ctx, ref):
        _upload(c_, "cat", cat_golden)
    p = _params(2)
    assert ctx.light_radii() == [0.0]                                 # an upload leaves a point
    _light(ctx, THREE, [0.0, 0.0, 0.0])
    for k, r in enumerate(THREE_R):
        ctx.set_light_radius_at(k, r)
    assert ctx.light_radii() == THREE_R
    _light(ref, THREE, THREE_R)
    assert ref.light_radii() == THREE_R
    _bits_equal(ctx.render(p), ref.render(p))
    # set_light_at and move_light_at keep the radius of the light they touch
    ctx.set_light_at(1, P_C, 7e10)
    ctx.move_light_at(2, 2.5, 0.04)
    want = [THREE[0], (P_C, 7e10), rt.light_orbit(THREE[2], 2.5, 0.04)]
    assert ctx.light_radii() == THREE_R
    _light(ref, want, THREE_R)
    _bits_equal(ctx.render(p), ref.render(p))
    # set_lights, set_light and an upload leave points
    ctx.set_lights(THREE)
    assert ctx.light_radii() == [0.0, 0.0, 0.0]
    ref.set_lights(THREE)
    _bits_equal(ctx.render(p), ref.render(p))
    ctx.set_light_radii(THREE_R)
    ctx.set_light(P_A, 2e10)
    assert ctx.light_radii() == [0.0]
    ref.set_light(P_A, 2e10)
    _bits_equal(ctx.render(p), ref.render(p))
    ctx.set_light_radii([4.0])
    _upload(ctx, "cat", cat_golden)
    _upload(ref, "cat", cat_golden)
    assert ctx.light_radii() == [0.0]
    _bits_equal(ctx.render(p), ref.render(p))
    # a list of one: set_light_at, move_light_at and move_light keep its radius
    ctx.set_light_radii([4.0])
    ctx.set_light_at(0, P_B, 1e10)
    assert ctx.light_radii() == [4.0]
    ctx.move_light_at(0, 3.0)
    assert ctx.light_radii() == [4.0]
    ctx.move_light(-1.5, 0.05)
    assert ctx.light_radii() == [4.0]
    moved = rt.light_orbit(rt.light_orbit((P_B, 1e10), 3.0, 2e-2), -1.5, 0.05)
    _light(ref, [moved], [4.0])
    assert ctx.lights() == ref.lights()
    soft = ctx.render(p)
    _bits_equal(soft, ref.render(p))
    ref.set_light_radii([0.0])
    assert _differ(soft, ref.render(p)) > 300
    # a soft list of one takes whatever intensity rt_scene_set_light takes
    for inten in (0.0, -2e10):
        _light(ctx, [(P_B, inten)], [4.0])
        _light(ref, [(P_B, inten)])
        a, b = ctx.render(p), ref.render(p)
        _bits_equal(a[..., 3], b[..., 3])
        if inten == 0.0:
            _bits_equal(a, b)                                          # no light: the shell's point does not matter


def test_bad_radii_are_refused_and_leave_everything(ctx, cat_golden):
    _upload(ctx, "cat", cat_golden)
    _light(ctx, THREE, THREE_R)
    have, radii = ctx.lights(), ctx.light_radii()
    p = _params(2)
    frame = ctx.render(p)
    lib, h = ctx._L, ctx._h
    arr = (C.c_float * 17)(*([1.0] * 17))
    out = (C.c_float * 17)(*([-7.0] * 17))
    n = C.c_int(-7)
    bad = [lambda: lib.rt_scene_set_light_radii(h, None, 3), lambda: lib.rt_scene_set_light_radii(h, arr, 2), lambda: lib.rt_scene_set_light_radii(h, arr, 4),
           lambda: lib.rt_scene_set_light_radii(h, arr, 0), lambda: lib.rt_scene_set_light_radii(h, arr, -1), lambda: lib.rt_scene_set_light_radii(h, arr, 17),
           lambda: lib.rt_scene_get_light_radii(h, None, 3, C.byref(n)), lambda: lib.rt_scene_get_light_radii(h, out, 3, None),
           lambda: lib.rt_scene_get_light_radii(h, out, 2, C.byref(n)), lambda: lib.rt_scene_get_light_radii(h, out, -1, C.byref(n)),
           lambda: lib.rt_scene_set_light_radius_at(h, 3, C.c_float(1.0)), lambda: lib.rt_scene_set_light_radius_at(h, -1, C.c_float(1.0))]
    bad += [lambda r=r: lib.rt_scene_set_light_radius_at(h, 1, C.c_float(r)) for r in (-1.0, -0.0, float("inf"), float("nan"))]
    for f in bad:
        assert f() == -1
        assert ctx.lights() == have and ctx.light_radii() == radii
    assert list(out) == [-7.0] * 17
    for r in (-1.0, -0.0, float("inf"), float("nan")):
        arr[1] = r
        assert lib.rt_scene_set_light_radii(h, arr, 3) == -1, r
        assert ctx.lights() == have and ctx.light_radii() == radii
    assert lib.rt_scene_get_light_radii(h, None, 0, C.byref(n)) == 0 and n.value == 3     # the count alone
    _bits_equal(ctx.render(p), frame)
    # sixteen soft lights render
    ctx.set_lights([((float(k) - 8.0, 20.0 + k, 30.0), float(k % 5)) for k in range(16)])
    ctx.set_light_radii([0.25 * k for k in range(16)])
    assert ctx.light_radii() == [0.25 * k for k in range(16)]
    f16 = ctx.render(p)
    assert f16[..., 3].sum() > 0 and (f16[..., :3] > 0).any()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_what_cannot_render_a_soft_light_refuses(ctx, cat_golden):
    """one soft light: RT_ERR_UNSUPPORTED (-5), outputs as they were (filled with -7), list, radii and a following frame unchanged"""
    import torch
    W, H = 67, 45
    _upload(ctx, "cat", cat_golden)
    _light(ctx, ONE, ONE_R)
    have, radii = ctx.lights(), ctx.light_radii()
    p = _params(2)
    frame = ctx.render(p)
    lib, h = ctx._L, ctx._h
    fp = C.POINTER(C.c_float)

    def after(what):
        assert ctx.lights() == have and ctx.light_radii() == radii, what
        _bits_equal(ctx.render(p), frame, what)

    for v in ("path", "lockstep", "global"):
        out = np.full((H, W, 4), -7.0, np.float32)
        pv = _params(2, variant=v)
        assert lib.rt_render(h, C.byref(pv), 0, H, out.ctypes.data_as(fp)) == -5, v
        assert (out == -7.0).all(), v
        after(v)
    for v in ("auto", "wavefront", "wavefront_lds", "wavefront_queue", "lds_verts", "lds_top", "lds_all"):
        _bits_equal(ctx.render(_params(2, variant=v)), frame, v)
    work = _capi.Work()
    C.memset(C.byref(work), 7, C.sizeof(work))
    assert lib.rt_count_work(h, C.byref(p), 0, H, C.byref(work)) == -5
    assert bytes(work) == b"\x07" * C.sizeof(work)
    after("rt_count_work")
    counts = np.full((H, W), 2, np.uint8)
    out = np.full((H, W, 4), -7.0, np.float32)
    assert lib.rt_render_counts(h, C.byref(p), None, counts.ctypes.data_as(C.POINTER(C.c_uint8)), None, out.ctypes.data_as(fp)) == -5
    assert (out == -7.0).all()
    dcounts = torch.full((H, W), 2, dtype=torch.uint8, device="cuda")
    dout = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
    assert lib.rt_render_counts_device(h, C.byref(p), None, C.c_void_p(dcounts.data_ptr()), None, C.c_void_p(dout.data_ptr()), None) == -5
    ctx.synchronize()
    assert bool((dout == -7.0).all())
    after("rt_render_counts")
    rows = _capi.Rows(0, H, H, 1)
    bufs = [torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda") for _ in range(2)]
    frames = [(bf.data_ptr(), (0.0, 0.0, 55.0), None, 123456) for bf in bufs]
    poses = [((s[0]), float(s[1])) for s in rt.scenes.spheres("cpu")]
    with pytest.raises(rt.RtError) as e:
        ctx.render_device_batch(p, rows, frames, scenes=[(THREE[0], poses), (THREE[1], poses)])
    assert e.value.code == -5
    ctx.synchronize()
    assert all(bool((bf == -7.0).all()) for bf in bufs)
    after("rt_render_device_batch_scenes")
    ctx.render_device_batch(p, rows, frames)
    ctx.synchronize()
    _bits_equal(bufs[0].cpu().numpy(), frame)
    _bits_equal(bufs[1].cpu().numpy(), frame)
    # a point again: everything renders
    ctx.set_light_radii([0.0])
    assert ctx.count_work(p)["rays"] > 0
    assert ctx.render(_params(2, variant="path"))[..., 3].sum() > 0


def test_a_sphere_only_scene_under_auto_renders_the_wavefronts_words(ctx, oracle, oracle_cat, cat_golden):
    _upload(ctx, "demo10", cat_golden)
    _light(ctx, ONE)
    p = _params(2)
    point = ctx.render(p)
    _light(ctx, ONE, ONE_R)
    soft = ctx.render(p)
    _bits_equal(soft, ctx.render(_params(2, variant="wavefront_queue")))
    _bits_equal(soft, _model(oracle, oracle_cat, cat_golden, "demo10", "one", 2))
    assert _differ(soft, point) > 300
