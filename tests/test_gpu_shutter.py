"""The shutter on the device (rt_scene_set_shutter: every wf_advance launch of a chain is a kFormShutter form while some displacement is not +-0).  -m gpu.

Every comparison is on uint32 views, .w (the ray count) included.  References, none of them the code under test:
  what exists   a closed shutter -- zeros, or a motion followed by NULL -- against a context that never heard of the shutter: frames and all three still-view counters;
  the model     tests/shutter_model.py (held to lens_model.py and to the oracle by tests/test_shutter_model.py): segments, samples, a mirror and nested glass that move, a
                sphere whose shadow sweeps the cat, a light that moves alone, smooth normals, a texture, the lens, a posed camera, row shares, the streak of a small sphere.
sigma stays 0 in the model cases: the walkers the model rests on do not restate the jitter.  Frames are 67 x 45 (partial tiles both ways, two sub-frames), 96 x 64 and 1 x 1.
The C-API cases that need a context (get after set, an upload closes the shutter, what is refused leaves the state) live here too: a context needs a device."""
import ctypes as C

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi
from . import lights_model as lm
from . import shutter_model as shm
from . import still_view as sv
from .test_gpu_soft_lights import (COUNTS, POSE, SLOT, THREE, _bits_equal, _cat, _differ, _moved, _oracle_scene, _params, _upload)

pytestmark = pytest.mark.gpu

NEAR = (0.0, 0.0, 20.0)                                               # a pose position whose directions look along the view axis (tests/test_gpu_lens.py)
LENS = (1.5, 45.0)
WAVEFRONTS = ("auto", "wavefront", "wavefront_lds", "wavefront_queue", "lds_verts", "lds_top", "lds_all")
# ten spheres: the mirror (slot 1) and the hollow glass ball (slots 2 and 3, one inside the other, moving together) travel
SH_TEN = ((0.0, 0.0, 0.0), {1: (-3.0, 2.0, 4.0), 2: (4.0, 1.0, 0.0), 3: (4.0, 1.0, 0.0)})
# the cat's scenes: the light travels and the floor (slot 1) rises
SH_CAT = ((6.0, 0.0, -4.0), {1: (0.0, 0.75, 0.0)})
SH_LIGHT = ((10.0, 0.0, 0.0), {})                                     # a moving light only
# a ball between the light (-10, 20, 40) and the cat, at slot 7 behind the cat's slot 6: its shadow sweeps the cat
BALL = ((-5.0, 10.0, 20.0), 3.0, (0.5, 0.5, 0.5))
SH_BALL = ((0.0, 0.0, 0.0), {7: (8.0, 0.0, 0.0)})
SHUTTERS = {"demo10": SH_TEN, "cat": SH_CAT, "smooth cat": SH_CAT, "textured cat": SH_CAT, "cat+ball": SH_BALL}


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


def _up(c, name, g):
    if name == "cat+ball":
        c.scene_upload(rt.scenes.spheres("cpu") + [BALL], _cat(g))
    else:
        _upload(c, name, g)


def _open(c, sh):
    c.set_shutter(light=sh[0], objects=sh[1])


_MODEL = {}


def _scene(oracle, oracle_cat, g, name):
    """-> (objects, materials, surface hook or None), built once"""
    if ("scene", name) not in _MODEL:
        if name == "demo10":
            s = (shm.objects(rt.scenes.spheres("demo10")), lm.materials(rt.scenes.spheres("demo10")), None)
        elif name == "cat+ball":
            sph = rt.scenes.spheres("cpu") + [BALL]
            s = (shm.objects(sph, {SLOT: oracle_cat}), lm.materials(sph, [_cat(g)]), None)
        else:
            osc, mats, surface = _oracle_scene(oracle, oracle_cat, g, name)
            _MODEL[("keep", name)] = osc                               # (the hook may look at it)
            s = (shm.objects(rt.scenes.spheres("cpu"), {SLOT: osc._meshes[0]}), mats, surface)
        _MODEL[("scene", name)] = s
    return _MODEL[("scene", name)]


def _model(oracle, oracle_cat, g, name, b, spp=1, w=67, h=45, pose=None, rows=None, sh=None, lens=(0.0, 1.0), cam=(0, 0, 55), seed=123456):
    """the model's frame with the shutter of the scene (or sh), computed once"""
    sh = SHUTTERS[name] if sh is None else sh
    key = (name, b, spp, w, h, pose, None if rows is None else tuple(rows), repr(sh), lens, cam, seed)
    if key not in _MODEL:
        objs, mats, surface = _scene(oracle, oracle_cat, g, name)
        kw = dict(fov=np.pi / 2) if pose is not None else {}
        wk = shm.Walker(objs, mats, [rt.scenes.LIGHT], shutter=sh, lens=lens, cam=cam, seed=seed, **kw)
        wk.surface = surface
        _MODEL[key] = wk.render(w, h, spp, b, pose=pose, rows=rows)
    return _MODEL[key]


# ---- exact against what exists -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["zeros", "on then NULL"])
@pytest.mark.parametrize("scene", ["cat", "demo10", "textured cat"])
def test_a_closed_shutter_is_the_context_that_never_heard_of_it(cat_golden, scene, how):
    """frames and all three still-view counters, on new contexts (nothing cached before)"""
    a, b = rt.Context(0), rt.Context(0)
    try:
        p = _params(2, w=96, h=64)
        for c_ in (a, b):
            _upload(c_, scene, cat_golden)
        if how == "zeros":
            a.set_shutter(light=(0.0, -0.0, 0.0), objects={0: (0.0, 0.0, -0.0), 1: (0.0, 0.0, 0.0), 15: (-0.0, 0.0, 0.0)})
        else:
            _open(a, SHUTTERS[scene])
            a.set_shutter()
        assert not a.shutter()[0].any() and not a.shutter()[1].any()
        before = [[getattr(c_, n)() for n in COUNTS] for c_ in (a, b)]
        for _ in range(4):                                            # fill, use, store the records, resume
            _bits_equal(a.render(p), b.render(p))
        assert [getattr(a, n)() for n in COUNTS] == [getattr(b, n)() for n in COUNTS]
        assert _moved(a, before[0]) == _moved(b, before[1])
        if scene == "cat":
            assert a.first_shade_cache_counts()["resumed"] > 0        # the shade level was reached: the comparison covers all three
        _bits_equal(a.render_pose(_params(2), rt.make_pose(**POSE)), b.render_pose(_params(2), rt.make_pose(**POSE)))
        _bits_equal(a.render(_params(2, spp=4)), b.render(_params(2, spp=4)))
    finally:
        a.close()
        b.close()


# ---- against the model -------------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b,spp", [(0, 1), (1, 1), (2, 1), (3, 1), (0, 4), (2, 4)])      # (four samples at 0 and 2 bounces: the model walks every path in Python)
def test_ten_spheres_with_a_moving_mirror_and_moving_nested_glass_equal_the_model(ctx, oracle, oracle_cat, cat_golden, b, spp):
    _upload(ctx, "demo10", cat_golden)
    _open(ctx, SH_TEN)
    exp = _model(oracle, oracle_cat, cat_golden, "demo10", b, spp)
    _bits_equal(ctx.render(_params(b, spp=spp)), exp)
    assert exp[..., 3].max() >= 2 and (exp[..., :3] > 0).any()
    ctx.set_shutter()
    assert _differ(ctx.render(_params(b, spp=spp)), exp) > 100         # the motion does change the frame


@pytest.mark.parametrize("scene,sh", [("cat+ball", None), ("cat", SH_LIGHT), ("cat", None), ("smooth cat", None), ("textured cat", None)],
                         ids=["a shadow sweeps the cat", "a moving light only", "light and floor", "smooth cat", "textured cat"])
def test_the_cat_under_a_shutter_equals_the_model(ctx, oracle, oracle_cat, cat_golden, scene, sh):
    _up(ctx, scene, cat_golden)
    _open(ctx, SHUTTERS[scene] if sh is None else sh)
    exp = _model(oracle, oracle_cat, cat_golden, scene, 2, sh=sh)
    _bits_equal(ctx.render(_params(2)), exp)
    ctx.set_shutter()
    assert _differ(ctx.render(_params(2)), exp) > 100
    if scene in ("smooth cat", "textured cat"):
        assert _differ(exp, _model(oracle, oracle_cat, cat_golden, "cat", 2)) > 50       # the normals / the texture do reach the frame


def test_the_lens_and_the_shutter_together_equal_the_model(ctx, oracle, oracle_cat, cat_golden):
    _upload(ctx, "cat", cat_golden)
    _open(ctx, SH_CAT)
    ctx.set_lens(*LENS)
    for spp in (1, 4):
        both = _model(oracle, oracle_cat, cat_golden, "cat", 2, spp, lens=LENS)
        _bits_equal(ctx.render(_params(2, spp=spp)), both, f"spp {spp}")
    both = _model(oracle, oracle_cat, cat_golden, "cat", 2, lens=LENS)
    assert _differ(both, _model(oracle, oracle_cat, cat_golden, "cat", 2)) > 300
    ctx.set_shutter()                                                 # the lens alone again: its own opening launch
    assert _differ(ctx.render(_params(2)), both) > 100
    ctx.set_lens(0.0, 1.0)


def test_posed_camera_row_shares_one_pixel_and_every_wavefront_variant_equal_the_model(ctx, oracle, oracle_cat, cat_golden):
    import torch
    _upload(ctx, "cat", cat_golden)
    _open(ctx, SH_CAT)
    p = _params(2)
    near = ctx.render_pose(p, rt.make_pose(position=NEAR, **POSE))
    _bits_equal(near, _model(oracle, oracle_cat, cat_golden, "cat", 2, pose=(POSE["yaw"], POSE["pitch"]), cam=NEAR))
    rows = list(range(13, 31))                                        # starts and ends inside an 8-row tile
    _bits_equal(ctx.render(p, 13, 31), _model(oracle, oracle_cat, cat_golden, "cat", 2, rows=rows))
    share, image_rows = rt.interleaved_rows(45, 8, 1, 3)              # tiles 1 and 4 of six: rows 8 .. 15 and 32 .. 39
    buf = torch.zeros((share.n_rows, 67, 4), dtype=torch.float32, device="cuda")
    ctx.render_device(p, share, buf.data_ptr())
    ctx.synchronize()
    whole = _model(oracle, oracle_cat, cat_golden, "cat", 2)
    _bits_equal(buf.cpu().numpy(), whole[list(image_rows)])
    _bits_equal(ctx.render(_params(2, w=1, h=1)), _model(oracle, oracle_cat, cat_golden, "cat", 2, w=1, h=1))
    _bits_equal(np.concatenate([ctx.render(p, 0, 20), ctx.render(p, 20, 45)]), whole)      # two row shares against the whole frame
    for v in WAVEFRONTS:
        _bits_equal(ctx.render(_params(2, variant=v)), whole, v)
    ctx.set_shutter()
    assert _differ(near, ctx.render_pose(p, rt.make_pose(position=NEAR, **POSE))) > 100


@pytest.mark.parametrize("knobs", [dict(RT_PARTS="1"), dict(RT_PARTS="3"), dict(RT_FIRST_HIT_CACHE="0")])
def test_other_cuts_render_the_same_words(oracle, oracle_cat, cat_golden, knobs):
    c_ = sv.context(**knobs)
    try:
        _upload(c_, "cat", cat_golden)
        _open(c_, SH_CAT)
        _bits_equal(c_.render(_params(2)), _model(oracle, oracle_cat, cat_golden, "cat", 2), f"{knobs}")
        _upload(c_, "demo10", cat_golden)
        _open(c_, SH_TEN)
        _bits_equal(c_.render(_params(2, spp=4)), _model(oracle, oracle_cat, cat_golden, "demo10", 2, 4), f"{knobs} spp 4")
        if "RT_PARTS" in knobs:
            assert c_.stats()["parts"] == int(knobs["RT_PARTS"])
    finally:
        c_.close()


def test_a_batch_of_three_cameras_async_and_pipelined_frames(ctx, ref, oracle, oracle_cat, cat_golden):
    import torch
    W, H = 67, 45
    _upload(ctx, "cat", cat_golden)
    _open(ctx, SH_CAT)
    rows = _capi.Rows(0, H, H, 1)
    cams = [((0.5 * k, 0.0, 55.0 - 3 * k), 40 + k) for k in range(3)]
    bufs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in cams]
    ctx.render_device_batch(_params(2), rows, [(bf.data_ptr(), cam, None, seed) for bf, (cam, seed) in zip(bufs, cams)])
    ctx.synchronize()
    for bf, (cam, seed) in zip(bufs, cams):
        ref.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden), camera=(cam, None))
        _open(ref, SH_CAT)
        _bits_equal(bf.cpu().numpy(), ref.render(_params(2, seed=seed)), str(cam))
    cam, seed = cams[1]                                               # each frame's own seed keys its times: the model's frame from there
    _bits_equal(bufs[1].cpu().numpy(), _model(oracle, oracle_cat, cat_golden, "cat", 2, cam=cam, seed=seed))
    out = rt.PinnedArray((H, W, 4), np.float32)
    try:
        ctx.render_async(_params(2), out.array, slot=0)
        ctx.wait(0)
        _bits_equal(out.array, _model(oracle, oracle_cat, cat_golden, "cat", 2))
    finally:
        out.close()
    # pipelined frames into alternating buffers, the shutter switched between them: frame k is the lone frame of its shutter
    want = {}
    for on in (True, False):
        if on:
            _open(ctx, SH_CAT)
        else:
            ctx.set_shutter()
        want[on] = ctx.render(_params(2, seed=77))
    assert _differ(want[True], want[False]) > 100
    pair = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    got = []
    ctx.set_pipelining(True)
    try:
        for k in range(6):
            if k % 3:
                _open(ctx, SH_CAT)
            else:
                ctx.set_shutter()
            ctx.render_device(_params(2, seed=77), rows, pair[k % 2].data_ptr())
            if k % 2 == 1:                                            # both buffers hold a frame: read them before the next two overwrite them
                ctx.synchronize()
                got.extend(b.cpu().numpy() for b in pair)
    finally:
        ctx.set_pipelining(False)
    for k, g in enumerate(got):
        _bits_equal(g, want[bool(k % 3)], f"pipelined frame {k}")


def test_the_streak_on_the_device(ctx):
    ctx.scene_upload([shm.ST_SPHERE], None, light=shm.ST_LIGHT, camera=(shm.ST_CAM, None))
    _open(ctx, shm.ST_SHUTTER)
    frame = ctx.render(_params(0, spp=shm.ST_SPP, w=shm.ST_W, h=shm.ST_H))
    print(shm.st_check(frame))
    _bits_equal(frame, shm.st_frame())


# ---- the still view ----------------------------------------------------------------------------------------------------------------------------------------------------------

def test_shutter_frames_leave_the_still_view_alone_and_a_closed_frame_again_is_cold(cat_golden):
    c_, cold = rt.Context(0), sv.context(RT_FIRST_HIT_CACHE="0")
    try:
        for x in (c_, cold):
            _upload(x, "cat", cat_golden)
        p = _params(2, w=96, h=64)
        exp = cold.render(p)
        for _ in range(4):                                            # the closed shutter's levels are full
            _bits_equal(c_.render(p), exp)
        _open(c_, SH_CAT)
        before = [getattr(c_, n)() for n in COUNTS]
        assert sum(len(b) for b in before) == 12                      # three levels, four counters each
        frames = [c_.render(p) for _ in range(3)]
        assert [getattr(c_, n)() for n in COUNTS] == before           # the twelve counters of all three levels, the ineligible chains' too
        for f in frames[1:]:
            _bits_equal(f, frames[0])
        _open(cold, SH_CAT)
        _bits_equal(cold.render(p), frames[0])
        assert _differ(frames[0], exp) > 100
        # the shutter closed: the next frame is the cold frame, and its chains fill -- nothing stored before the shutter opened is used
        c_.set_shutter()
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
    light, objs = c.shutter()
    return light.tobytes() + objs.tobytes()


def test_get_after_set_moves_keep_it_uploads_close_it_and_what_is_refused(ctx, ref, cat_golden):
    _up(ctx, "cat+ball", cat_golden)
    assert not ctx.shutter()[0].any() and not ctx.shutter()[1].any()
    ctx.set_shutter(light=(0.25, -1.0, 0.0), objects={7: (8.0, 0.0, 0.5), 0: (0.0, 0.0, -2.0)})
    light, objs = ctx.shutter()
    assert light.tolist() == [0.25, -1.0, 0.0] and objs[7].tolist() == [8.0, 0.0, 0.5] and objs[0].tolist() == [0.0, 0.0, -2.0] and not objs[1:7].any() and not objs[8:].any()
    # the edits keep the motion: after rt_scene_move_sphere the frame is that of an upload of the moved scene with the same shutter
    _open(ctx, SH_BALL)
    was = _state(ctx)
    ctx.move_sphere(7, (0.0, 2.0, 0.0), 0.5)
    ctx.set_sphere(0, rt.scenes.spheres("cpu")[0])
    ctx.move_light(0.3, 0.5)
    ctx.set_light(*rt.scenes.LIGHT)
    assert _state(ctx) == was
    moved = ((BALL[0][0], BALL[0][1] + 1.0, BALL[0][2]),) + BALL[1:]
    ref.scene_upload(rt.scenes.spheres("cpu") + [moved], _cat(cat_golden))
    assert not ref.shutter()[1].any()
    _open(ref, SH_BALL)
    _bits_equal(ctx.render(_params(2)), ref.render(_params(2)))
    # rt_scene_move_sphere(v = dC, dt = 1) gives the tau = 1 pose exactly
    np.testing.assert_array_equal(np.asarray(ctx.sphere(7)[0], np.float32), np.asarray(moved[0], np.float32))
    ctx.move_sphere(7, SH_BALL[1][7], 1.0)
    np.testing.assert_array_equal(np.asarray(ctx.sphere(7)[0], np.float32), shm.pose(moved[0], SH_BALL[1][7], 1.0))
    _up(ctx, "cat+ball", cat_golden)
    assert not ctx.shutter()[0].any() and not ctx.shutter()[1].any()  # an upload closes the shutter
    _open(ctx, SH_BALL)
    was = _state(ctx)
    lib, h = ctx._L, ctx._h
    inf, nan = float("inf"), float("nan")

    def motion(light=(0.0, 0.0, 0.0), **objects):
        s = _capi.Shutter()
        s.light[:] = light
        for k, v in objects.items():
            s.object[int(k[1:])][:] = v
        return s

    bad = [motion(light=(x, 0.0, 0.0)) for x in (inf, -inf, nan)] + [motion(s7=(0.0, x, 0.0)) for x in (inf, nan)] + [motion(s15=(0.0, 0.0, nan))]
    bad += [motion(s6=(1.0, 0.0, 0.0)), motion(s6=(0.0, 0.0, -1e-30))]                 # the cat's slot: meshes do not move within an exposure
    bad += [motion(s8=(0.0, 1.0, 0.0)), motion(s15=(0.0, 0.0, 1.0))]                   # beyond the scene's eight objects
    for s in bad:
        assert lib.rt_scene_set_shutter(h, C.byref(s)) == -1
        assert b"shutter" in lib.rt_last_error(h)
        assert _state(ctx) == was
    assert lib.rt_scene_get_shutter(h, None) == -1 and _state(ctx) == was
    ok = motion(s6=(0.0, -0.0, 0.0), s8=(-0.0, 0.0, 0.0), s7=(1.0, 0.0, 0.0))           # +-0 for a mesh's slot and beyond the scene is no motion
    assert lib.rt_scene_set_shutter(h, C.byref(ok)) == 0 and ctx.shutter()[1][7].tolist() == [1.0, 0.0, 0.0]
    fresh = rt.Context(0)                                             # no upload: RT_ERR_NO_SCENE, and the get writes nothing
    try:
        s = _capi.Shutter()
        C.memset(C.byref(s), 7, C.sizeof(s))
        assert fresh._L.rt_scene_get_shutter(fresh._h, C.byref(s)) == -4 and bytes(s) == b"\x07" * C.sizeof(s)
        assert fresh._L.rt_scene_set_shutter(fresh._h, C.byref(ok)) == -4 and fresh._L.rt_scene_set_shutter(fresh._h, None) == -4
    finally:
        fresh.close()


def test_what_cannot_render_a_shutter_refuses(ctx, cat_golden):
    """RT_ERR_UNSUPPORTED (-5), outputs as they were (filled with -7), "shutter" in the error text, the state and a following frame unchanged; closed, each of them works"""
    import torch
    W, H = 67, 45
    _upload(ctx, "cat", cat_golden)
    _open(ctx, SH_CAT)
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
            out = np.full((H, W, 4), -7.0, np.float32)
            pv = _params(2, variant=v)
            yield v, lib.rt_render(h, C.byref(pv), 0, H, out.ctypes.data_as(fp)), bool((out == -7.0).all())
        work = _capi.Work()
        C.memset(C.byref(work), 7, C.sizeof(work))
        yield "rt_count_work", lib.rt_count_work(h, C.byref(p), 0, H, C.byref(work)), bytes(work) == b"\x07" * C.sizeof(work)
        out = np.full((H, W, 4), -7.0, np.float32)
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
        assert b"shutter" in lib.rt_last_error(h), what
        after(what)
        seen.append(what)
    assert len(seen) == 7
    # a light list of several, or a radius above 0, while the shutter is on: no form takes both
    for what, setup in (("several lights", lambda: ctx.set_lights(THREE)), ("a radius", lambda: ctx.set_light_radii([2.0]))):
        ctx.set_light(*rt.scenes.LIGHT)
        setup()
        for v in ("auto", "wavefront"):
            out = np.full((H, W, 4), -7.0, np.float32)
            pv = _params(2, variant=v)
            assert lib.rt_render(h, C.byref(pv), 0, H, out.ctypes.data_as(fp)) == -5 and (out == -7.0).all(), (what, v)
            assert b"shutter" in lib.rt_last_error(h), what
        assert _state(ctx) == was
        ctx.set_shutter()                                             # closed, the list renders
        assert _differ(ctx.render(p), frame) > 100
        _open(ctx, SH_CAT)
    ctx.set_light(*rt.scenes.LIGHT)
    after("one point light again")
    ctx.set_shutter()                                                 # closed: each of them works
    for what, rc, untouched in refused():
        assert rc == 0 and not untouched, (what, rc, untouched)
    assert ctx.count_work(p)["rays"] > 0


def test_auto_on_a_sphere_only_scene_and_a_progressive_frame(ctx, oracle, oracle_cat, cat_golden):
    _upload(ctx, "demo10", cat_golden)
    _open(ctx, SH_TEN)
    on = ctx.render(_params(2))                                       # auto: never lockstep while the shutter is on
    _bits_equal(on, ctx.render(_params(2, variant="wavefront_queue")))
    _bits_equal(on, _model(oracle, oracle_cat, cat_golden, "demo10", 2))
    pose = rt.make_pose(position=NEAR, **POSE)
    ctx.progressive_reset()
    disp, _ = ctx.progressive_frame(_params(2), pose)
    ctx.set_shutter()
    ctx.progressive_reset()
    still, _ = ctx.progressive_frame(_params(2), pose)
    assert np.isfinite(disp).all() and _differ(disp, still) > 100


def test_svgf_sequence_runs_with_the_shutter_on_and_is_itself_with_it_closed(ctx, cat_golden):
    W, H = 96, 64
    _upload(ctx, "cat", cat_golden)

    def run():
        outs = []
        with rt.SvgfSequence(ctx, W, H) as seq:
            for i in range(3):
                ptr = seq.frame(_params(2, w=W, h=H, seed=100 + i))
                ctx.synchronize()
                outs.append(ctx.device_to_host(ptr, (H, W, 4)))
        return outs

    plain = run()
    ctx.set_shutter(light=(0.0, 0.0, 0.0), objects={1: (0.0, -0.0, 0.0)})
    for a, b in zip(run(), plain):
        _bits_equal(a, b)
    _open(ctx, SH_CAT)
    on = run()
    assert all(np.isfinite(o).all() for o in on)
    assert _differ(on[2], plain[2]) > 100
