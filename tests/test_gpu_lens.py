"""The thin lens on the device (rt_camera_set_lens: wf_advance<kFormFirst | kFormLens> opens every chain while the aperture radius is above 0).  -m gpu.

Every comparison is on uint32 views, .w (the ray count) included.  References, none of them the code under test:
  what exists   a radius of 0, set at once or after a lens was on, against a context that never heard of the lens: frames and all three still-view counters;
  the model     tests/lens_model.py (held to lights_model.py and to the oracle by tests/test_lens_model.py): segments, samples, a posed camera, a row share that starts
                mid-tile, smooth normals, a texture, three lights with radii, the circle of confusion of a small sphere.
sigma stays 0 in the model cases: the walkers the model rests on do not restate the jitter.  Frames are 67 x 45 (partial tiles both ways, two sub-frames), 96 x 64 and 1 x 1.
The C-API cases that need a context (get after set, an upload leaves a pinhole, what is refused leaves the lens) live here too: a context needs a device."""
import ctypes as C

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi
from . import lens_model as lens
from . import still_view as sv
from .test_gpu_soft_lights import (COUNTS, POSE, THREE, THREE_R, _bits_equal, _cat, _differ, _moved, _oracle_scene, _params, _upload)

pytestmark = pytest.mark.gpu

NEAR = (0.0, 0.0, 20.0)                                               # a pose position whose directions look along the view axis: see the posed test
LENS = (1.5, 45.0)                                                    # the cat stands about 55 from the camera: in front of and behind the plane of focus
WAVEFRONTS = ("auto", "wavefront", "wavefront_lds", "wavefront_queue", "lds_verts", "lds_top", "lds_all")


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


_MODEL = {}


def _model(oracle, oracle_cat, g, name, b, spp=1, w=67, h=45, pose=None, rows=None, lights=None, radii=None, cam=(0, 0, 55), seed=123456):
    """the model's frame with the lens LENS, computed once"""
    key = (name, b, spp, w, h, pose, None if rows is None else tuple(rows), None if lights is None else "three", cam, seed)
    if key not in _MODEL:
        if ("scene", name) not in _MODEL:
            _MODEL[("scene", name)] = _oracle_scene(oracle, oracle_cat, g, name)
        osc, mats, surface = _MODEL[("scene", name)]
        kw = dict(fov=np.pi / 2) if pose is not None else {}
        wk = lens.Walker(osc, mats, [rt.scenes.LIGHT] if lights is None else lights, radii, lens=LENS, cam=cam, seed=seed, **kw)
        wk.surface = surface
        _MODEL[key] = wk.render(w, h, spp, b, pose=pose, rows=rows)
    return _MODEL[key]


# ---- exact against what exists -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["zero", "on then zero"])
@pytest.mark.parametrize("scene", ["cat", "demo10", "textured cat"])
def test_radius_zero_is_the_context_that_never_heard_of_the_lens(cat_golden, scene, how):
    """frames and all three still-view counters, on new contexts (nothing cached before)"""
    a, b = rt.Context(0), rt.Context(0)
    try:
        p = _params(2, w=96, h=64)
        for c_ in (a, b):
            _upload(c_, scene, cat_golden)
        if how != "zero":
            a.set_lens(*LENS)
        a.set_lens(0.0, LENS[1])
        assert a.lens() == (0.0, LENS[1]) and b.lens() == (0.0, 1.0)
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
@pytest.mark.parametrize("scene", ["cat", "demo10"])
def test_frames_equal_the_model(ctx, oracle, oracle_cat, cat_golden, scene, b, spp):
    _upload(ctx, scene, cat_golden)
    ctx.set_lens(*LENS)
    exp = _model(oracle, oracle_cat, cat_golden, scene, b, spp)
    _bits_equal(ctx.render(_params(b, spp=spp)), exp)
    assert exp[..., 3].max() >= 2 and (exp[..., :3] > 0).any()
    ctx.set_lens(0.0, 1.0)
    assert _differ(ctx.render(_params(b, spp=spp)), exp) > 300         # the lens does change the frame


@pytest.mark.parametrize("scene", ["smooth cat", "textured cat"])
def test_smooth_and_textured_frames_equal_the_model(ctx, oracle, oracle_cat, cat_golden, scene):
    _upload(ctx, scene, cat_golden)
    ctx.set_lens(*LENS)
    exp = _model(oracle, oracle_cat, cat_golden, scene, 2)
    _bits_equal(ctx.render(_params(2)), exp)
    assert _differ(exp, _model(oracle, oracle_cat, cat_golden, "cat", 2)) > 50       # the normals / the texture do reach the frame


def test_three_lights_with_radii_equal_the_model(ctx, oracle, oracle_cat, cat_golden):
    _upload(ctx, "cat", cat_golden)
    ctx.set_lights(THREE)
    ctx.set_light_radii(THREE_R)
    ctx.set_lens(*LENS)
    _bits_equal(ctx.render(_params(2)), _model(oracle, oracle_cat, cat_golden, "cat", 2, lights=THREE, radii=THREE_R))
    ctx.set_light_radii([0.0, 0.0, 0.0])                              # ... and as points: wf_advance<kFormLights> behind the same opening launch
    pts = ctx.render(_params(1))
    _upload(ctx, "cat", cat_golden)
    assert ctx.lens() == (0.0, 1.0)                                   # the upload left a pinhole
    ctx.set_lights(THREE)
    assert _differ(pts, ctx.render(_params(1))) > 300


def test_posed_camera_a_row_share_from_mid_tile_and_one_pixel_equal_the_model(ctx, oracle, oracle_cat, cat_golden):
    import torch
    _upload(ctx, "cat", cat_golden)
    ctx.set_lens(*LENS)
    p = _params(2)
    # The posed camera keeps its position inside the direction (posed_dir): u = normalize(C + bz z + ...).  From C = (0, 0, 55) with |z| = 33.5 every u looks away from the
    # view axis, c < 0, and the rule leaves the ray as it is: the pinhole's frame.  From C = (0, 0, 20) c > 0 and the lens is on.
    far = ctx.render_pose(p, rt.make_pose(**POSE))
    _bits_equal(far, _model(oracle, oracle_cat, cat_golden, "cat", 2, pose=(POSE["yaw"], POSE["pitch"])))
    near = ctx.render_pose(p, rt.make_pose(position=NEAR, **POSE))
    _bits_equal(near, _model(oracle, oracle_cat, cat_golden, "cat", 2, pose=(POSE["yaw"], POSE["pitch"]), cam=NEAR))
    ctx.set_lens(0.0, 1.0)
    _bits_equal(far, ctx.render_pose(p, rt.make_pose(**POSE)))
    assert _differ(near, ctx.render_pose(p, rt.make_pose(position=NEAR, **POSE))) > 300
    ctx.set_lens(*LENS)
    rows = list(range(13, 31))                                        # starts and ends inside an 8-row tile
    _bits_equal(ctx.render(p, 13, 31), _model(oracle, oracle_cat, cat_golden, "cat", 2, rows=rows))
    share, image_rows = rt.interleaved_rows(45, 8, 1, 3)              # tiles 1 and 4 of six: rows 8 .. 15 and 32 .. 39
    buf = torch.zeros((share.n_rows, 67, 4), dtype=torch.float32, device="cuda")
    ctx.render_device(p, share, buf.data_ptr())
    ctx.synchronize()
    whole = _model(oracle, oracle_cat, cat_golden, "cat", 2)
    _bits_equal(buf.cpu().numpy(), whole[list(image_rows)])
    _bits_equal(ctx.render(_params(2, w=1, h=1)), _model(oracle, oracle_cat, cat_golden, "cat", 2, w=1, h=1))
    # two row shares against the whole frame
    _bits_equal(np.concatenate([ctx.render(p, 0, 20), ctx.render(p, 20, 45)]), whole)
    for v in WAVEFRONTS:
        _bits_equal(ctx.render(_params(2, variant=v)), whole, v)


@pytest.mark.parametrize("knobs", [dict(RT_PARTS="1"), dict(RT_PARTS="3"), dict(RT_FIRST_HIT_CACHE="0")])
def test_other_cuts_render_the_same_words(oracle, oracle_cat, cat_golden, knobs):
    c_ = sv.context(**knobs)
    try:
        _upload(c_, "cat", cat_golden)
        c_.set_lens(*LENS)
        for spp in (1, 4):
            _bits_equal(c_.render(_params(2, spp=spp)), _model(oracle, oracle_cat, cat_golden, "cat", 2, spp), f"{knobs} {spp}")
        if "RT_PARTS" in knobs:
            assert c_.stats()["parts"] == int(knobs["RT_PARTS"])
    finally:
        c_.close()


def test_a_batch_of_three_cameras_equals_the_lone_frames_and_async(ctx, ref, oracle, oracle_cat, cat_golden):
    import torch
    W, H = 67, 45
    _upload(ctx, "cat", cat_golden)
    ctx.set_lens(*LENS)
    rows = _capi.Rows(0, H, H, 1)
    cams = [((0.5 * k, 0.0, 55.0 - 3 * k), 40 + k) for k in range(3)]
    bufs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in cams]
    ctx.render_device_batch(_params(2), rows, [(bf.data_ptr(), cam, None, seed) for bf, (cam, seed) in zip(bufs, cams)])
    ctx.synchronize()
    for bf, (cam, seed) in zip(bufs, cams):
        ref.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden), camera=(cam, None))
        ref.set_lens(*LENS)
        _bits_equal(bf.cpu().numpy(), ref.render(_params(2, seed=seed)), str(cam))
    cam, seed = cams[1]                                               # each frame's own camera carries the lens: the model's frame from there
    _bits_equal(bufs[1].cpu().numpy(), _model(oracle, oracle_cat, cat_golden, "cat", 2, cam=cam, seed=seed))
    out = rt.PinnedArray((H, W, 4), np.float32)
    try:
        ctx.render_async(_params(2), out.array, slot=0)
        ctx.wait(0)
        _bits_equal(out.array, ctx.render(_params(2)))
        _bits_equal(out.array, _model(oracle, oracle_cat, cat_golden, "cat", 2))
    finally:
        out.close()
    # pipelined frames into alternating buffers, the lens switched between them: frame k is the lone frame of its lens
    want = {}
    for on in (True, False):
        ctx.set_lens(*(LENS if on else (0.0, 1.0)))
        want[on] = ctx.render(_params(2, seed=77))
    assert _differ(want[True], want[False]) > 300
    pair = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    got = []
    ctx.set_pipelining(True)
    try:
        for k in range(6):
            ctx.set_lens(*(LENS if k % 3 else (0.0, 1.0)))
            ctx.render_device(_params(2, seed=77), rows, pair[k % 2].data_ptr())
            if k % 2 == 1:                                            # both buffers hold a frame: read them before the next two overwrite them
                ctx.synchronize()
                got.extend(b.cpu().numpy() for b in pair)
    finally:
        ctx.set_pipelining(False)
    for k, g in enumerate(got):
        _bits_equal(g, want[bool(k % 3)], f"pipelined frame {k}")


def test_the_circle_of_confusion_on_the_device(ctx, oracle):
    ctx.scene_upload([lens.COC_SPHERE], None, light=lens.COC_LIGHT, camera=(lens.COC_CAM, None))
    ctx.set_lens(lens.COC_R, lens.COC_F)
    frame = ctx.render(_params(0, spp=lens.COC_SPP, w=lens.COC_W, h=lens.COC_H))
    print(lens.coc_check(frame))
    _bits_equal(frame, lens.coc_frame(oracle))


# ---- the still view ----------------------------------------------------------------------------------------------------------------------------------------------------------

def test_lens_frames_leave_the_still_view_alone_and_a_pinhole_again_is_cold(cat_golden):
    c_, cold = rt.Context(0), sv.context(RT_FIRST_HIT_CACHE="0")
    try:
        for x in (c_, cold):
            _upload(x, "cat", cat_golden)
        p = _params(2, w=96, h=64)
        exp = cold.render(p)
        for _ in range(4):                                            # the pinhole's levels are full
            _bits_equal(c_.render(p), exp)
        c_.set_lens(*LENS)
        before = [getattr(c_, n)() for n in COUNTS]
        frames = [c_.render(p) for _ in range(3)]
        assert [getattr(c_, n)() for n in COUNTS] == before           # every counter of all three, the ineligible chains' too
        for f in frames[1:]:
            _bits_equal(f, frames[0])
        cold.set_lens(*LENS)
        _bits_equal(cold.render(p), frames[0])
        assert _differ(frames[0], exp) > 300
        # the lens off: the next frame is the cold pinhole frame, and its chains fill -- nothing stored before the lens came on is used
        c_.set_lens(0.0, LENS[1])
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

def test_get_after_set_uploads_and_what_is_refused(ctx, cat_golden):
    _upload(ctx, "cat", cat_golden)
    assert ctx.lens() == (0.0, 1.0)
    ctx.set_lens(0.25, 12.5)
    assert ctx.lens() == (0.25, 12.5)
    ctx.set_lens(0.0, -3.0)                                           # a pinhole: the focus distance is stored as given and never read
    assert ctx.lens() == (0.0, -3.0)
    ctx.set_lens(2.0, 30.0)
    _upload(ctx, "cat", cat_golden)
    assert ctx.lens() == (0.0, 1.0)                                   # the camera comes with the upload
    ctx.set_lens(2.0, 30.0)
    lib, h = ctx._L, ctx._h
    r, f = C.c_float(-7.0), C.c_float(-7.0)
    inf, nan = float("inf"), float("nan")
    bad = [lambda: lib.rt_camera_get_lens(h, None, C.byref(f)), lambda: lib.rt_camera_get_lens(h, C.byref(r), None)]
    bad += [lambda x=x: lib.rt_camera_set_lens(h, C.c_float(x), C.c_float(30.0)) for x in (-1.0, -0.0, inf, -inf, nan)]
    bad += [lambda x=x: lib.rt_camera_set_lens(h, C.c_float(1.0), C.c_float(x)) for x in (0.0, -0.0, -5.0, inf, -inf, nan)]
    for fn in bad:
        assert fn() == -1
        assert ctx.lens() == (2.0, 30.0)
    assert (r.value, f.value) == (-7.0, -7.0)                         # a refused get writes nothing
    assert lib.rt_camera_set_lens(None, C.c_float(1.0), C.c_float(30.0)) == -1
    ctx.set_lens(0.0, nan)                                            # lens off: any focus distance
    assert ctx.lens()[0] == 0.0


def test_what_cannot_render_a_lens_refuses(ctx, cat_golden):
    """RT_ERR_UNSUPPORTED (-5), outputs as they were (filled with -7), the lens and a following frame unchanged; with R == 0 each of them works"""
    import torch
    W, H = 67, 45
    _upload(ctx, "cat", cat_golden)
    ctx.set_lens(*LENS)
    p = _params(2)
    frame = ctx.render(p)
    lib, h = ctx._L, ctx._h
    fp = C.POINTER(C.c_float)
    rows = _capi.Rows(0, H, H, 1)
    poses = [((s[0]), float(s[1])) for s in rt.scenes.spheres("cpu")]
    counts = np.full((H, W), 2, np.uint8)
    dcounts = torch.full((H, W), 2, dtype=torch.uint8, device="cuda")

    def after(what):
        assert ctx.lens() == LENS, what
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
        assert b"lens" in lib.rt_last_error(h), what
        after(what)
        seen.append(what)
    assert len(seen) == 7
    for v in WAVEFRONTS:
        _bits_equal(ctx.render(_params(2, variant=v)), frame, v)
    ctx.set_lens(0.0, LENS[1])                                        # a pinhole again: each of them works
    for what, rc, untouched in refused():
        assert rc == 0 and not untouched, (what, rc, untouched)
    assert ctx.count_work(p)["rays"] > 0


def test_auto_on_a_sphere_only_scene_and_a_progressive_frame(ctx, oracle, oracle_cat, cat_golden):
    _upload(ctx, "demo10", cat_golden)
    ctx.set_lens(*LENS)
    on = ctx.render(_params(2))                                       # auto: never lockstep while the lens is on
    _bits_equal(on, ctx.render(_params(2, variant="wavefront_queue")))
    _bits_equal(on, _model(oracle, oracle_cat, cat_golden, "demo10", 2))
    pose = rt.make_pose(position=NEAR, **POSE)
    ctx.progressive_reset()
    disp, _ = ctx.progressive_frame(_params(2), pose)
    ctx.set_lens(0.0, 1.0)
    ctx.progressive_reset()
    pin, _ = ctx.progressive_frame(_params(2), pose)
    assert np.isfinite(disp).all() and _differ(disp, pin) > 300


def test_svgf_sequence_runs_with_the_lens_on_and_is_itself_with_it_off(ctx, cat_golden):
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
    ctx.set_lens(0.0, LENS[1])
    for a, b in zip(run(), plain):
        _bits_equal(a, b)
    ctx.set_lens(*LENS)
    on = run()
    assert all(np.isfinite(o).all() for o in on)
    assert _differ(on[2], plain[2]) > 300
