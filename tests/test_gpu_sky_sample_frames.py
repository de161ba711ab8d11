"""Frames under sky sampling (rt_scene_set_environment_sampling with a positive share over a lit map: every wf_advance launch after the opening one is a kFormSkySample
form, a diffuse segment's one shadow ray may go to the sky).  -m gpu.  Every case fails on a library without the entry.

Every comparison is on uint32 views, .w (the ray count) included.  References, none of them the code under test:
  what exists   .w of a sampled frame == .w of the frame at share 0 (the paths are the same); a scene of mirrors and glass only at any share == share 0;
  the model     tests/sky_sample_model.py Walker (held to sky_model.Walker and the mathematics by tests/test_sky_sample_model.py) on test_gpu_sky's five open scenes;
  a closed form the n = 1 map at share 1 over one convex diffuse sphere at b = 0;
  statistics    the frame-mean at share 0.5 against the frame-mean at share 0 over 8 seeds.
Frames are 67 x 45, 96 x 64 and 1 x 1; maps have n = 1, 2, 5 and 64."""
import ctypes as C

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi
from raytracinggpu_amd import environment as envm
from . import lens_model as lnm
from . import sky_sample_model as ssm
from . import still_view as sv
from .test_gpu_sky import BALLS, LENS, MAPS, NEAR, OPEN, RADII, WAVEFRONTS, _MODEL, _oracle_scene, _up
from .test_gpu_soft_lights import POSE, THREE, _bits_equal, _differ, _params

pytestmark = pytest.mark.gpu

f32 = np.float32
FP = C.POINTER(C.c_float)
SAMPLING = [(0, 1), (2, 1), (3, 1), (0, 4), (2, 4)]
SCENE_MAP = {"open cat": 64, "smooth open cat": 5, "textured open cat": 2, "balls": 5, "room": 5}
SCENE_SHARE = {"open cat": 0.5, "smooth open cat": 0.25, "textured open cat": 1.0, "balls": 0.5, "room": 0.25}


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


class _LensWalker(ssm.Walker, lnm.Walker):
    """the sampling walker's path behind the lens walker's camera rays"""


def _model(oracle, g, name, n, share, b, spp=1, w=67, h=45, pose=None, rows=None, lights=(rt.scenes.LIGHT,), radii=None, lens=None, cam=(0, 0, 55), seed=123456):
    """the model's frame under MAPS[n] at `share`, computed once"""
    key = ("sample", name, n, share, b, spp, w, h, pose, None if rows is None else tuple(rows), repr(lights), repr(radii), lens, cam, seed)
    if key not in _MODEL:
        osc, mats, surface = _oracle_scene(oracle, g, name)
        kw = dict(fov=np.pi / 2) if pose is not None else {}
        if lens is not None:
            kw["lens"] = lens
        wk = (_LensWalker if lens is not None else ssm.Walker)(osc, mats, list(lights), radii, env=MAPS[n], share=share, cam=cam, seed=seed, **kw)
        wk.surface = surface
        _MODEL[key] = wk.render(w, h, spp, b, pose=pose, rows=rows)
    return _MODEL[key]


def _sampled(c, name, g, n, share):
    _up(c, name, g)
    c.set_environment(MAPS[n])
    c.set_environment_sampling(share)


# ---- exact against what exists ----------------------------------------------------------------------------------------------------------------------------------------------

def test_w_of_a_sampled_frame_is_w_at_share_0_and_mirrors_and_glass_do_not_change(ctx, ref, cat_golden):
    for name in ("open cat", "room", "textured open cat"):
        for c_ in (ctx, ref):
            _up(c_, name, cat_golden)
            c_.set_environment(MAPS[5])
        ctx.set_environment_sampling(0.5)
        for p in (_params(3), _params(2, spp=4, w=96, h=64)):
            lit, plain = ctx.render(p), ref.render(p)
            _bits_equal(lit[..., 3], plain[..., 3], name)
            assert _differ(lit, plain) > 100
    specular = [rt.scenes.DEMO[1], rt.scenes.DEMO[2], rt.scenes.DEMO[3]]           # a mirror and a hollow glass ball: no diffuse segment, no shadow ray
    for c_ in (ctx, ref):
        c_.scene_upload(specular, None)
        c_.set_environment(MAPS[64])
    for share in (0.25, 1.0):
        ctx.set_environment_sampling(share)
        for p in (_params(3), _params(4, spp=4)):
            _bits_equal(ctx.render(p), ref.render(p), f"specular, share {share}")


# ---- against the model, word for word --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b,spp", SAMPLING)
@pytest.mark.parametrize("scene", OPEN)
def test_open_scenes_under_sampling_equal_the_model(ctx, oracle, cat_golden, scene, b, spp):
    n, share = SCENE_MAP[scene], SCENE_SHARE[scene]
    _sampled(ctx, scene, cat_golden, n, share)
    _bits_equal(ctx.render(_params(b, spp=spp)), _model(oracle, cat_golden, scene, n, share, b, spp), f"{scene} b={b} spp={spp}")


def test_shares_intensity_0_a_light_list_and_radii_equal_the_model(ctx, oracle, cat_golden):
    for scene, n in (("open cat", 64), ("room", 5)):
        _up(ctx, scene, cat_golden)
        ctx.set_environment(MAPS[n])
        for share in (0.25, 0.5, 1.0):
            ctx.set_environment_sampling(share)
            _bits_equal(ctx.render(_params(2)), _model(oracle, cat_golden, scene, n, share, 2), f"{scene} share {share}")
        dark = [(rt.scenes.LIGHT[0], 0.0)]
        ctx.set_light(*dark[0])                                       # intensity 0: the effective share is 1 whatever the share
        ctx.set_environment_sampling(0.25)
        exp = _model(oracle, cat_golden, scene, n, 0.25, 2, lights=dark)
        _bits_equal(ctx.render(_params(2)), exp, "intensity 0")
        _bits_equal(exp, _model(oracle, cat_golden, scene, n, 1.0, 2, lights=dark), "effective share 1")
        ctx.set_lights(THREE)
        _bits_equal(ctx.render(_params(2)), _model(oracle, cat_golden, scene, n, 0.25, 2, lights=THREE), "three lights")
        ctx.set_light_radii(RADII)
        _bits_equal(ctx.render(_params(2)), _model(oracle, cat_golden, scene, n, 0.25, 2, lights=THREE, radii=RADII), "radii")
    _up(ctx, "textured open cat", cat_golden)                         # tex | soft | sky | sample with radii
    ctx.set_environment(MAPS[2])
    ctx.set_environment_sampling(0.5)
    ctx.set_lights(THREE)
    ctx.set_light_radii(RADII)
    _bits_equal(ctx.render(_params(2)), _model(oracle, cat_golden, "textured open cat", 2, 0.5, 2, lights=THREE, radii=RADII), "textured, radii")


def test_lens_posed_camera_row_shares_one_pixel_and_every_wavefront_variant_equal_the_model(ctx, oracle, cat_golden):
    import torch
    _sampled(ctx, "open cat", cat_golden, 64, 0.5)
    p = _params(2)
    whole = _model(oracle, cat_golden, "open cat", 64, 0.5, 2)
    ctx.set_lens(*LENS)
    _bits_equal(ctx.render(p), _model(oracle, cat_golden, "open cat", 64, 0.5, 2, lens=LENS), "lens")
    ctx.set_lens(0.0, 1.0)
    near = ctx.render_pose(p, rt.make_pose(position=NEAR, **POSE))
    _bits_equal(near, _model(oracle, cat_golden, "open cat", 64, 0.5, 2, pose=(POSE["yaw"], POSE["pitch"]), cam=NEAR))
    share, image_rows = rt.interleaved_rows(45, 8, 1, 3)
    buf = torch.zeros((share.n_rows, 67, 4), dtype=torch.float32, device="cuda")
    ctx.render_device(p, share, buf.data_ptr())
    ctx.synchronize()
    _bits_equal(buf.cpu().numpy(), whole[list(image_rows)])
    _bits_equal(ctx.render(_params(2, w=1, h=1)), _model(oracle, cat_golden, "open cat", 64, 0.5, 2, w=1, h=1))
    for v in WAVEFRONTS:
        _bits_equal(ctx.render(_params(2, variant=v)), whole, v)


@pytest.mark.parametrize("knobs", [dict(RT_PARTS="1"), dict(RT_PARTS="3"), dict(RT_DEAD_CHANNELS="0"), dict(RT_TRAVQ_ANYHIT="0")])
def test_other_cuts_and_knobs_render_the_same_words(ctx, oracle, cat_golden, knobs):
    """the room with a wall removed: pure-colour walls kill channels of paths whose later shadow rays go to the sky"""
    c_ = sv.context(**knobs)
    try:
        for scene, n, share, b, spp in (("room", 5, 0.25, 3, 1), ("open cat", 2, 0.5, 2, 4)):
            _sampled(c_, scene, cat_golden, n, share)
            got = c_.render(_params(b, spp=spp))
            _bits_equal(got, _model(oracle, cat_golden, scene, n, share, b, spp), f"{knobs} {scene}")
            _sampled(ctx, scene, cat_golden, n, share)
            _bits_equal(got, ctx.render(_params(b, spp=spp)), f"{knobs} {scene} against the default")
    finally:
        c_.close()


def test_a_batch_of_three_async_and_map_and_share_replaced_between_pipelined_frames(ctx, ref, oracle, cat_golden):
    import torch
    W, H = 67, 45
    _sampled(ctx, "open cat", cat_golden, 5, 0.5)
    rows = _capi.Rows(0, H, H, 1)
    cams = [((0.5 * k, 0.0, 55.0 - 3 * k), 40 + k) for k in range(3)]
    bufs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in cams]
    ctx.render_device_batch(_params(2), rows, [(bf.data_ptr(), cam, None, seed) for bf, (cam, seed) in zip(bufs, cams)])
    ctx.synchronize()
    for bf, (cam, seed) in zip(bufs, cams):
        _up(ref, "open cat", cat_golden, camera=(cam, None))
        ref.set_environment(MAPS[5])
        ref.set_environment_sampling(0.5)
        _bits_equal(bf.cpu().numpy(), ref.render(_params(2, seed=seed)), str(cam))
    cam, seed = cams[1]
    _bits_equal(bufs[1].cpu().numpy(), _model(oracle, cat_golden, "open cat", 5, 0.5, 2, cam=cam, seed=seed))
    out = rt.PinnedArray((H, W, 4), np.float32)
    try:
        ctx.render_async(_params(2), out.array, slot=0)
        ctx.wait(0)
        _bits_equal(out.array, _model(oracle, cat_golden, "open cat", 5, 0.5, 2))
    finally:
        out.close()
    order = [(5, 0.5), (2, 0.5), (2, 1.0), (64, 0.25), (64, 0.0), (5, 0.5)]
    want = {}
    for n, share in set(order):
        ctx.set_environment(MAPS[n])
        ctx.set_environment_sampling(share)
        want[(n, share)] = ctx.render(_params(2, seed=77))
    assert _differ(want[(2, 0.5)], want[(2, 1.0)]) > 100 and _differ(want[(64, 0.25)], want[(64, 0.0)]) > 100
    pair = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    got = []
    ctx.set_pipelining(True)
    try:
        for k, (n, share) in enumerate(order):
            ctx.set_environment(MAPS[n])
            ctx.set_environment_sampling(share)
            ctx.render_device(_params(2, seed=77), rows, pair[k % 2].data_ptr())
            if k % 2 == 1:
                ctx.synchronize()
                got.extend(b.cpu().numpy() for b in pair)
    finally:
        ctx.set_pipelining(False)
    for k, g in enumerate(got):
        _bits_equal(g, want[order[k]], f"pipelined frame {k}")


# ---- a closed form -------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_one_convex_diffuse_sphere_under_the_constant_map_at_share_1(ctx, cat_golden):
    """b = 0: one segment.  A pixel that hits the sphere (nothing can block a ray that leaves a convex body) is fl(fl(l alb) / pi) + fl(alb (+0)) per channel with
    l = fl(w_sky fl(g E)), w_sky = 1, g from the model's draw and the sphere's own normal; a pixel that misses is E."""
    env = MAPS[1]
    alb = np.array([0.25, 0.5, 0.75], f32)
    centre, R = np.array([0.0, 0.0, 0.0], f32), f32(10.0)
    ctx.scene_upload([(tuple(centre), float(R), tuple(alb))], None)
    ctx.set_environment(env)
    ctx.set_environment_sampling(1.0)
    W, H, seed = 67, 45, 123456
    got = ctx.render(_params(0, seed=seed))
    tb = ssm.Table(env)
    E = env[0, 0]
    hit = got[..., 3] == 2                                               # the camera ray and the shadow ray
    assert 200 < hit.sum() < W * H and (got[..., 3][~hit] == 1).all()
    _bits_equal(got[~hit][:, :3], np.broadcast_to(E, ((~hit).sum(), 3)))
    checked = 0
    from . import soft_lights_model as slm
    from oracle import oracle_py as orc
    osc = orc.Scene()
    osc.add_sphere(tuple(centre), float(R), tuple(alb))
    for row, px in zip(*np.nonzero(hit)):
        if (row * W + px) % 7:
            continue
        pixel = int(row * W + px)
        u = slm.camera_dir(W, H, int(row), int(px))
        ok, _, P, N = osc.intersect_all(np.array([0, 0, 55], f32), u, 1e-4)
        assert ok
        t, w, m, r = tb.sample(ssm.sample_key(seed, pixel, 0), 0)
        dn = ssm._dot(N, w[0])
        g = tb.weight(t, m, r, f32(0) if dn < 0 else dn)[0]
        l3 = (f32(1) * (g * E)).astype(f32)
        exp = ((l3 * alb).astype(f32) / f32(np.pi)).astype(f32) + (alb * f32(0)).astype(f32)
        _bits_equal(got[row, px, :3], exp, f"pixel {row},{px}")
        checked += 1
    assert checked > 30


# ---- unbiased on the device, against the parent's own path ---------------------------------------------------------------------------------------------------------------------

def test_the_frame_mean_at_share_half_is_the_frame_mean_at_share_0(ctx, cat_golden):
    """balls at 24 x 16 under a smooth gradient sky alone, b = 2, 64 samples, 8 seeds: the two estimators have the same expectation"""
    ctx.scene_upload(BALLS, None)
    ctx.set_light(rt.scenes.LIGHT[0], 0.0)
    ctx.set_environment(envm.gradient_sky((0.2, 0.5, 2.0), (1.5, 1.5, 1.5), (0.3, 0.2, 0.1), 64))
    means = {}
    for share in (0.0, 0.5):
        ctx.set_environment_sampling(share)
        # (intensity 0 makes the effective share 1 at any positive share: the sampled frames take every shadow ray to the sky)
        means[share] = np.array([ctx.render(_params(2, spp=64, w=24, h=16, seed=1000 + k))[..., :3].astype(np.float64).mean() for k in range(8)])
    m0, m1 = means[0.0].mean(), means[0.5].mean()
    se = np.sqrt(means[0.0].var(ddof=1) / 8 + means[0.5].var(ddof=1) / 8)
    print(f"share 0: {m0:.6f}, share 0.5: {m1:.6f}, five combined standard errors {5 * se:.6f}")
    assert 5 * se < 0.01 * m0                                            # a wrong constant cannot pass
    assert abs(m1 - m0) <= 5 * se


# ---- what refuses ----------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_what_cannot_render_an_environment_refuses_and_names_sampling(ctx, cat_golden):
    """RT_ERR_UNSUPPORTED (-5), outputs as they were (filled with -7), "environment sampling" in the error text"""
    from .test_gpu_soft_lights import _upload
    W, H = 67, 45
    _upload(ctx, "cat", cat_golden)
    ctx.set_environment(MAPS[5])
    ctx.set_environment_sampling(0.5)
    p = _params(2)
    frame = ctx.render(p)
    lib, h = ctx._L, ctx._h
    counts = np.full((H, W), 2, np.uint8)

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

    seen = 0
    for what, rc, untouched in refused():
        assert rc == -5 and untouched, (what, rc, untouched)
        assert b"environment sampling" in lib.rt_last_error(h), what
        assert ctx.environment_sampling() == 0.5
        seen += 1
    assert seen == 5
    ctx.set_shutter(light=(6.0, 0.0, -4.0))
    out = np.full((H, W, 4), -7.0, f32)
    assert lib.rt_render(h, C.byref(p), 0, H, out.ctypes.data_as(FP)) == -5 and (out == -7.0).all()
    assert b"environment sampling" in lib.rt_last_error(h)
    ctx.set_shutter()
    _bits_equal(ctx.render(p), frame)
