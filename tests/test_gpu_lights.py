"""Several point lights on the device (rt_scene_set_lights: one light picked per diffuse hit, by intensity).  -m gpu.

Every comparison is on uint32 views, .w (the ray count) included.  Three kinds of reference, none of them the code under test:
  what exists   a list that can only ever pick ONE light -- (0, I, 0), three co-located lights I/4, I/2, I/4, [1e10, 1] -- against rt_scene_set_light on a second context;
  the oracle    one segment, three lights 1 : 2 : 5: every pixel is the oracle's frame for the light the rule names, at the intensity of all;
  the model     tests/lights_model.py (held to the oracle by tests/test_lights_model.py): several segments, samples, a posed camera, row shares.
Frames are 96 x 64, 67 x 45 (partial tiles both ways, two sub-frames) and 1 x 1."""
import ctypes as C
import functools

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi
from . import lights_model as lm
from . import material_scenes as ms
from . import still_view as sv

pytestmark = pytest.mark.gpu

SLOT = 6
I0 = 3e10                                                             # rt.scenes.LIGHT's intensity: I0 / 4 and I0 / 2 are exact
P_A, P_B, P_C = (-10.0, 20.0, 40.0), (15.0, 25.0, 30.0), (0.0, 35.0, 5.0)
THREE = [(P_A, 1e10), (P_B, 2e10), (P_C, 5e10)]                      # 1 : 2 : 5
POSE = dict(yaw=0.2, pitch=0.1)


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


SCENES = ("cat", "two_cats", "demo10", "smooth cat", "textured cat")


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
            rng = np.random.default_rng(21)
            c.mesh_set_texture(_planar_uv(v), tv, rng.integers(0, 256, size=(23, 37, 3), dtype=np.uint8), filter="bilinear", decode=rng.random(256).astype(np.float32))


def _shot(c, mode, w=67, h=45):
    if mode == "plain":
        return c.render(_params(2, w=w, h=h))
    if mode == "posed":
        return c.render_pose(_params(2, w=w, h=h), rt.make_pose(**POSE))
    if mode == "spp4":
        return c.render(_params(2, spp=4, w=w, h=h))
    if mode == "sigma":
        return c.render(_params(2, spp=2, w=w, h=h, sigma=0.2, seed=9))
    raise ValueError(mode)


# ---- exact against what exists -------------------------------------------------------------------------------------------------------------------------------------------

def test_a_list_of_one_is_set_light(ctx, ref, cat_golden):
    """frames and all three still-view counters: a list of one light is rt_scene_set_light"""
    for c_ in (ctx, ref):
        _upload(c_, "cat", cat_golden)
    ctx.set_lights([(P_B, 2e10)])
    ref.set_light(P_B, 2e10)
    assert ctx.lights() == [(P_B, float(np.float32(2e10)))] == ref.lights() and ctx.light() == ref.light()
    names = ("first_hit_cache_counts", "first_shadow_cache_counts", "first_shade_cache_counts")
    before = [[getattr(c_, n)() for n in names] for c_ in (ctx, ref)]
    p = _params(2, w=96, h=64)
    for _ in range(4):                                                # fill, use, store the records, resume
        _bits_equal(ctx.render(p), ref.render(p))
    moved = [[{k: getattr(c_, n)()[k] - b[k] for k in b if k != "key_misses"} for n, b in zip(names, bc)] for c_, bc in zip((ctx, ref), before)]
    assert moved[0] == moved[1], moved
    assert moved[0][2]["resumed"] > 0                                 # the shade level was reached: the comparison covers all three


@pytest.mark.parametrize("mode", ["plain", "posed", "spp4"])
@pytest.mark.parametrize("scene", SCENES)
def test_lists_that_pick_one_light_equal_that_light(ctx, ref, cat_golden, scene, mode):
    """(0, I, 0) at three positions is the single light I at the middle position; I/4, I/2, I/4 at one position is the single light I there"""
    for c_ in (ctx, ref):
        _upload(c_, scene, cat_golden)
    ref.set_light(P_B, I0)
    exp = _shot(ref, mode)
    assert exp[..., 3].sum() > 0
    ctx.set_lights([(P_A, 0.0), (P_B, I0), (P_C, 0.0)])
    _bits_equal(_shot(ctx, mode), exp, "(0, I, 0)")
    ctx.set_lights([(P_B, I0 / 4), (P_B, I0 / 2), (P_B, I0 / 4)])
    _bits_equal(_shot(ctx, mode), exp, "co-located")
    assert _differ(exp, _light_frame(ref, P_A, I0, mode)) > 300       # the scene does tell the positions apart


def _differ(a, b):
    return int((np.ascontiguousarray(a[..., :3], np.float32).view(np.uint32) != np.ascontiguousarray(b[..., :3], np.float32).view(np.uint32)).any(-1).sum())


def _light_frame(c, pos, inten, mode):
    c.set_light(pos, inten)
    return _shot(c, mode)


def test_jittered_camera_absorbed_light_and_one_pixel(ctx, ref, cat_golden):
    """sigma = 0.2 (both sides on the device); [1e10, 1]: the running sum absorbs the second light; a 1 x 1 frame"""
    for c_ in (ctx, ref):
        _upload(c_, "cat", cat_golden)
    ref.set_light(P_B, I0)
    ctx.set_lights([(P_B, I0 / 4), (P_B, I0 / 2), (P_B, I0 / 4)])
    _bits_equal(_shot(ctx, "sigma"), _shot(ref, "sigma"))
    _bits_equal(_shot(ctx, "plain", 1, 1), _shot(ref, "plain", 1, 1))
    ctx.set_lights([(P_A, 0.0), (P_B, I0), (P_C, 0.0)])
    _bits_equal(_shot(ctx, "sigma"), _shot(ref, "sigma"))
    ref.set_light(P_B, 1e10)
    ctx.set_lights([(P_B, 1e10), (P_C, 1.0)])
    for mode in ("plain", "spp4"):
        _bits_equal(_shot(ctx, mode, 96, 64), _shot(ref, mode, 96, 64), mode)


def test_the_hit_level_fills_and_is_used_the_others_do_not_move(ctx, cat_golden):
    _upload(ctx, "cat", cat_golden)
    ctx.set_lights(THREE)
    p = _params(2, w=96, h=64)
    hit0, sh0, rec0 = ctx.first_hit_cache_counts(), ctx.first_shadow_cache_counts(), ctx.first_shade_cache_counts()
    frames = [ctx.render(p) for _ in range(3)]
    hit, sh, rec = ctx.first_hit_cache_counts(), ctx.first_shadow_cache_counts(), ctx.first_shade_cache_counts()
    n = ctx.stats()["parts"]
    assert hit["filled"] - hit0["filled"] == n and hit["skipped"] - hit0["skipped"] == 2 * n
    assert sh["skipped"] == sh0["skipped"] and sh["filled"] == sh0["filled"]
    assert rec["resumed"] == rec0["resumed"] and rec["filled"] == rec0["filled"]
    for f in frames[1:]:
        _bits_equal(f, frames[0])
    off = sv.context(RT_FIRST_HIT_CACHE="0")
    try:
        _upload(off, "cat", cat_golden)
        off.set_lights(THREE)
        _bits_equal(off.render(p), frames[0])
    finally:
        off.close()


# ---- direct lighting against the oracle ------------------------------------------------------------------------------------------------------------------------------------

def test_one_segment_is_the_oracles_frame_of_the_picked_light(ctx, oracle, oracle_cat, cat_golden):
    W, H = 96, 64
    _upload(ctx, "cat", cat_golden)
    ctx.set_lights(THREE)
    got = ctx.render(_params(0, w=W, h=H))
    pre = lm.prefix([i for _, i in THREE])
    osc = oracle.Scene.preset("cpu", oracle_cat)
    per_light = []
    for pos, _ in THREE:
        osc.set_light(pos, float(pre[-1]))                            # the position is the light's, the intensity is the total
        per_light.append(osc.render(W, H, 1, 0, want_rgb8=False)[0])
    r = np.array([[oracle.uniform(123456, y * W + x, 0, 1, 2) for x in range(W)] for y in range(H)], np.float32)
    k = lm.pick(pre, r)
    exp = np.choose(k[..., None], per_light)
    _bits_equal(got, exp)
    for n in range(3):
        others = [per_light[m] for m in range(3) if m != n]
        decided = (k == n) & (per_light[n][..., :3] > 0).any(-1) & np.logical_and.reduce([(per_light[n][..., :3] != o[..., :3]).any(-1) for o in others])
        print(f"light {n}: picked for {(k == n).sum()} pixels, decides {decided.sum()} lit ones")
        assert decided.sum() >= 200, (n, int(decided.sum()))


# ---- against the model -------------------------------------------------------------------------------------------------------------------------------------------------------

def _oracle_scene(oracle, oracle_cat, g, name):
    if name == "cat":
        return oracle.Scene.preset("cpu", oracle_cat), lm.materials(rt.scenes.spheres("cpu"), [_cat(g)])
    if name == "demo10":
        return oracle.Scene.preset("demo10"), lm.materials(rt.scenes.spheres("demo10"))
    spheres, meshes = _two_cats()
    return ms.oracle_scene(oracle, "two_cats", g["vertices"], g["tri_obj_order"]), lm.materials(spheres, meshes)


_MODEL = {}


def _model(oracle, oracle_cat, g, name, b, spp=1, w=67, h=45, pose=None, rows=None):
    """the model's frame, computed once"""
    key = (name, b, spp, w, h, pose, None if rows is None else tuple(rows))
    if key not in _MODEL:
        if ("scene", name) not in _MODEL:
            _MODEL[("scene", name)] = _oracle_scene(oracle, oracle_cat, g, name)
        osc, mats = _MODEL[("scene", name)]
        kw = dict(fov=np.pi / 2) if pose is not None else {}
        _MODEL[key] = lm.Walker(osc, mats, THREE, **kw).render(w, h, spp, b, pose=pose, rows=rows)
    return _MODEL[key]


@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("b", [2, 3])
@pytest.mark.parametrize("scene", ["cat", "demo10", "two_cats"])
def test_frames_equal_the_model(ctx, oracle, oracle_cat, cat_golden, scene, b, spp):
    _upload(ctx, scene, cat_golden)
    ctx.set_lights(THREE)
    exp = _model(oracle, oracle_cat, cat_golden, scene, b, spp)
    _bits_equal(ctx.render(_params(b, spp=spp)), exp)
    assert exp[..., 3].max() > b + 1


def test_posed_camera_and_interleaved_rows_equal_the_model(ctx, oracle, oracle_cat, cat_golden):
    import torch
    _upload(ctx, "cat", cat_golden)
    ctx.set_lights(THREE)
    p = _params(2)
    _bits_equal(ctx.render_pose(p, rt.make_pose(**POSE)), _model(oracle, oracle_cat, cat_golden, "cat", 2, pose=(POSE["yaw"], POSE["pitch"])))
    rows, image_rows = rt.interleaved_rows(45, 8, 1, 3)               # tiles 1 and 4 of six: rows 8 .. 15 and 32 .. 39
    buf = torch.zeros((rows.n_rows, 67, 4), dtype=torch.float32, device="cuda")
    ctx.render_device(p, rows, buf.data_ptr())
    ctx.synchronize()
    _bits_equal(buf.cpu().numpy(), _model(oracle, oracle_cat, cat_golden, "cat", 2)[list(image_rows)])
    _bits_equal(ctx.render(_params(2, w=1, h=1)), _model(oracle, oracle_cat, cat_golden, "cat", 2, w=1, h=1))


@pytest.mark.parametrize("knobs", [dict(RT_PARTS="1"), dict(RT_PARTS="2"), dict(RT_PARTS="3"), dict(RT_TRAVQ_ANYHIT="0"), dict(RT_DEAD_CHANNELS="0")])
def test_other_cuts_and_rules_render_the_same_words(oracle, oracle_cat, cat_golden, knobs):
    """RT_PARTS 1, 2 and 3; any-hit off; the dead-channel rule off: the model's frame, word for word (the cat's room has walls with zero channels)"""
    c_ = sv.context(**knobs)
    try:
        _upload(c_, "cat", cat_golden)
        c_.set_lights(THREE)
        for spp in (1, 3):
            _bits_equal(c_.render(_params(2, spp=spp)), _model(oracle, oracle_cat, cat_golden, "cat", 2, spp), str(knobs))
        if "RT_PARTS" in knobs:
            assert c_.stats()["parts"] == int(knobs["RT_PARTS"])
    finally:
        c_.close()


def test_a_batch_of_three_equals_the_lone_frames(ctx, ref, cat_golden):
    import torch
    W, H = 67, 45
    _upload(ctx, "cat", cat_golden)
    ctx.set_lights(THREE)
    rows = _capi.Rows(0, H, H, 1)
    cams = [((0.5 * k, 0.0, 55.0 - 3 * k), 40 + k) for k in range(3)]
    bufs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in cams]
    ctx.render_device_batch(_params(2), rows, [(bf.data_ptr(), cam, None, seed) for bf, (cam, seed) in zip(bufs, cams)])
    ctx.synchronize()
    for bf, (cam, seed) in zip(bufs, cams):
        ref.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden), camera=(cam, None))
        ref.set_lights(THREE)
        _bits_equal(bf.cpu().numpy(), ref.render(_params(2, seed=seed)), str(cam))
    # rt_render_async goes through the same entries
    out = rt.PinnedArray((H, W, 4), np.float32)
    try:
        ctx.render_async(_params(2), out.array, slot=0)
        ctx.wait(0)
        _bits_equal(out.array, ctx.render(_params(2)))
    finally:
        out.close()


# ---- edits -------------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_edits_equal_a_fresh_list(ctx, ref, cat_golden):
    for c_ in (ctx, ref):
        _upload(c_, "cat", cat_golden)
    f32 = lambda l: [(tuple(float(np.float32(x)) for x in p), float(np.float32(i))) for p, i in l]
    assert ctx.lights() == f32([rt.scenes.LIGHT])                     # an upload leaves the one uploaded light
    ctx.set_lights(THREE)
    assert ctx.lights() == f32(THREE) and ctx.light() == f32(THREE)[0]
    p = _params(2)
    # set_light_at
    ctx.set_light_at(1, P_C, 7e10)
    want = [THREE[0], (P_C, 7e10), THREE[2]]
    assert ctx.lights() == f32(want)
    ref.set_lights(want)
    _bits_equal(ctx.render(p), ref.render(p))
    # move_light_at: get, rt_light_orbit, set
    ctx.move_light_at(2, 2.5, 0.04)
    want[2] = rt.light_orbit(want[2], 2.5, 0.04)
    assert ctx.lights() == f32(want)
    ref.set_lights(want)
    moved = ctx.render(p)
    _bits_equal(moved, ref.render(p))
    ctx.move_light_at(0, -1.0)
    want[0] = rt.light_orbit(want[0], -1.0, 2e-2)
    assert ctx.lights() == f32(want) and ctx.light() == f32(want)[0]   # rt_scene_get_light answers light 0
    # rt_scene_set_light collapses the list
    ctx.set_light(P_A, 2e10)
    ref.set_light(P_A, 2e10)
    assert ctx.lights() == f32([(P_A, 2e10)])
    _bits_equal(ctx.render(p), ref.render(p))
    # an upload resets it
    ctx.set_lights(THREE)
    _upload(ctx, "cat", cat_golden)
    _upload(ref, "cat", cat_golden)
    assert ctx.lights() == f32([rt.scenes.LIGHT])
    _bits_equal(ctx.render(p), ref.render(p))
    # a single light through the _at entries
    ctx.set_light_at(0, P_B, 1e10)
    ctx.move_light_at(0, 3.0)
    ref.set_light(P_B, 1e10)
    ref.move_light(3.0)
    assert ctx.lights() == ref.lights() and len(ctx.lights()) == 1
    _bits_equal(ctx.render(p), ref.render(p))


def test_bad_lists_are_refused_and_leave_the_list(ctx, cat_golden):
    _upload(ctx, "cat", cat_golden)
    ctx.set_lights(THREE)
    have = ctx.lights()
    p = _params(2)
    frame = ctx.render(p)
    lib, h = ctx._L, ctx._h
    arr = (_capi.Light * 17)()
    for k in range(17):
        arr[k].position[:] = (float(k), 20.0, 30.0)
        arr[k].intensity = 1.0
    n = C.c_int(-7)
    bad = [lambda: lib.rt_scene_set_lights(h, None, 3), lambda: lib.rt_scene_set_lights(h, arr, 0), lambda: lib.rt_scene_set_lights(h, arr, 17),
           lambda: lib.rt_scene_set_lights(h, arr, -1), lambda: lib.rt_scene_get_lights(h, None, 3, C.byref(n)), lambda: lib.rt_scene_get_lights(h, arr, 3, None),
           lambda: lib.rt_scene_get_lights(h, arr, 2, C.byref(n)), lambda: lib.rt_scene_set_light_at(h, 3, C.byref(arr[0])), lambda: lib.rt_scene_set_light_at(h, -1, C.byref(arr[0])),
           lambda: lib.rt_scene_set_light_at(h, 0, None), lambda: lib.rt_scene_move_light_at(h, 3, C.c_float(1.0), C.c_float(0.02))]
    for f in bad:
        assert f() == -1
        assert ctx.lights() == have
    for inten in ([1.0, -1.0, 1.0], [1.0, -0.0, 1.0], [1.0, float("inf"), 1.0], [1.0, float("nan"), 1.0], [0.0, 0.0, 0.0], [3e38, 3e38, 1.0]):
        for k, i in enumerate(inten):
            arr[k].intensity = i
        assert lib.rt_scene_set_lights(h, arr, 3) == -1, inten
        assert ctx.lights() == have
    bad_light = _capi.Light()
    bad_light.intensity = -2.0
    assert lib.rt_scene_set_light_at(h, 1, C.byref(bad_light)) == -1 and ctx.lights() == have
    assert lib.rt_scene_get_lights(h, None, 0, C.byref(n)) == 0 and n.value == 3     # the count alone
    _bits_equal(ctx.render(p), frame)
    # sixteen lights are a list
    for k in range(16):
        arr[k].intensity = float(k % 5)
    assert lib.rt_scene_set_lights(h, arr, 16) == 0 and len(ctx.lights()) == 16
    assert ctx.render(p)[..., 3].sum() > 0


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_what_cannot_render_several_lights_refuses(ctx, cat_golden):
    """RT_ERR_UNSUPPORTED (-5), outputs as they were (filled with -7), the list and a following frame unchanged"""
    import torch
    W, H = 67, 45
    _upload(ctx, "cat", cat_golden)
    ctx.set_lights(THREE)
    have = ctx.lights()
    p = _params(2)
    frame = ctx.render(p)
    lib, h = ctx._L, ctx._h
    fp = C.POINTER(C.c_float)

    def after(what):
        assert ctx.lights() == have, what
        _bits_equal(ctx.render(p), frame, what)

    # the variants that do not run wf_advance; the wavefront ones render
    for v in ("path", "lockstep", "global"):
        out = np.full((H, W, 4), -7.0, np.float32)
        pv = _params(2, variant=v)
        assert lib.rt_render(h, C.byref(pv), 0, H, out.ctypes.data_as(fp)) == -5, v
        assert (out == -7.0).all(), v
        after(v)
    for v in ("auto", "wavefront", "wavefront_lds", "wavefront_queue", "lds_verts", "lds_top", "lds_all"):
        _bits_equal(ctx.render(_params(2, variant=v)), frame, v)
    # rt_count_work
    work = _capi.Work()
    C.memset(C.byref(work), 7, C.sizeof(work))
    assert lib.rt_count_work(h, C.byref(p), 0, H, C.byref(work)) == -5
    assert bytes(work) == b"\x07" * C.sizeof(work)
    after("rt_count_work")
    # rt_render_counts and its device form
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
    # an animated batch; the plain batch renders
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
    # one light again: everything renders
    ctx.set_light(*THREE[0])
    assert ctx.count_work(p)["rays"] > 0
    assert ctx.render(_params(2, variant="path"))[..., 3].sum() > 0
