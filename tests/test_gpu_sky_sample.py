"""Sky sampling on the device (rt_scene_set_environment_sampling: the table of the environment map, built by rt_skydist.hip.h, and the draw sky_draw / sky_weight of
rt_shade.hip.h).  -m gpu.  Every case fails on a library without the entries.

Every comparison is on integer views.  References, none of them the code under test:
  the model     tests/sky_sample_model.py (held to the mathematics by tests/test_sky_sample_model.py): the table for maps of n = 1, 2, 5 and 64, a map with dark regions
                and one of 1024 x 1024 (the only case whose scan crosses many workgroups with sums above 2^32); the draw on 2^16 keys per map
  what exists   share 0, and any share over an all-zero map, against a context that never heard of the call: frames of 67 x 45, 96 x 64 and 1 x 1 and all three
                still-view counters
The frames that draw from the table: tests/test_gpu_sky_sample_frames.py.  The C-API cases that need a context live here too."""
import ctypes as C

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi
from raytracinggpu_amd import environment as envm
from . import sky_sample_model as ssm
from . import still_view as sv
from .test_gpu_sky import MAPS, ROOM, _up  # noqa: F401
from .test_gpu_soft_lights import COUNTS, POSE, THREE, _bits_equal, _moved, _params, _upload

pytestmark = pytest.mark.gpu

f32 = np.float32
FP = C.POINTER(C.c_float)


def _dark_map():
    """a 64 x 64 map that is dark except for a sun and a few texels: c is 0 over most of it"""
    env = envm.add_sun(np.zeros((64, 64, 3), f32), (0.3, 0.8, -0.5), np.radians(4.0), (5000.0, 4500.0, 4000.0))
    env[0, 0] = (0.0, 0.0, 1e-3)
    env[63, 17] = (2.0, 0.0, 0.0)
    env[31, 63] = (0.0, 1e3, 0.0)
    return env


SAMPLE_MAPS = {**{str(n): m for n, m in MAPS.items()}, "dark": _dark_map()}


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


_TABLES = {}


def _table(name):
    if name not in _TABLES:
        _TABLES[name] = ssm.Table(SAMPLE_MAPS[name])
    return _TABLES[name]


def _same_table(ctx, tb):
    c, prefix, total = ctx.kat_environment_table()
    assert total == tb.total
    assert (c == tb.c).all()
    assert (prefix == tb.prefix).all()


# ---- the table and the draw ----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SAMPLE_MAPS))
def test_the_table_and_the_draw_equal_the_model(ctx, cat_golden, name):
    _up(ctx, "balls", cat_golden)
    ctx.set_environment(SAMPLE_MAPS[name])
    ctx.set_environment_sampling(0.5)
    tb = _table(name)
    assert tb.total > 0
    _same_table(ctx, tb)
    hs = ssm.mix32(np.arange(1 << 16, dtype=np.uint64) ^ np.uint64(0x2545F491)).astype(np.uint32)
    hs[:4] = (0, 1, 0xFFFFFFFF, 0x80000000)
    seg = (np.arange(1 << 16) % 7).astype(np.int32)
    texel, dirs, g = ctx.kat_environment_sample(hs, seg)
    t, w, m, r = tb.sample(hs, seg)
    assert (texel == t).all()
    _bits_equal(dirs, w)
    _bits_equal(g, tb.weight(t, m, r))
    assert (tb.c[texel] > 0).all()                                     # a draw never lands on a texel the lookup cannot light
    if name == "dark":
        assert (tb.c == 0).sum() > 3000 and len(np.unique(texel)) > 20
    ctx.set_environment_sampling(0.0)


def test_the_flat_search_draws_the_same_texels(cat_golden):
    """RT_SKY_SEARCH=0: one binary search over all prefixes instead of the block level first -- on the map whose long runs of equal prefixes are where the two could differ"""
    c_ = sv.context(RT_SKY_SEARCH="0")
    try:
        _up(c_, "balls", cat_golden)
        for name in ("dark", "5", "1"):
            c_.set_environment(SAMPLE_MAPS[name])
            c_.set_environment_sampling(1.0)
            tb = _table(name)
            hs = ssm.mix32(np.arange(1 << 14, dtype=np.uint64) ^ np.uint64(0x9E3779B1)).astype(np.uint32)
            texel, dirs, g = c_.kat_environment_sample(hs, 3)
            t, w, m, r = tb.sample(hs, 3)
            assert (texel == t).all()
            _bits_equal(dirs, w)
            _bits_equal(g, tb.weight(t, m, r))
    finally:
        c_.close()


def test_the_table_of_a_1024_map_equals_the_model(ctx, cat_golden):
    """4096 workgroups, a scan of four rounds, prefixes far above 2^32"""
    rng = np.random.default_rng(1024)
    env = envm.gradient_sky((0.2, 0.5, 2.0), (1.5, 1.5, 1.5), (0.3, 0.2, 0.1), 1024) * rng.uniform(0.5, 1.5, (1024, 1024, 3)).astype(f32)
    env = envm.add_sun(env, (-0.4, 0.6, 0.3), np.radians(0.5), 4.0)
    _up(ctx, "balls", cat_golden)
    ctx.set_environment_sampling(1.0)                                   # the share first: setting the map builds the table
    ctx.set_environment(env)
    tb = ssm.Table(env)
    assert tb.total > 2 ** 45
    _same_table(ctx, tb)
    ctx.set_environment()
    ctx.set_environment_sampling(0.0)


# ---- exact against what exists ----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", ["cat", "demo10"])
def test_share_0_is_the_context_that_never_heard_of_the_call(cat_golden, scene):
    """frames and all three still-view counters, on new contexts; then under a map, and under an all-zero map at share 0.5 (an empty table: the effective share is 0)"""
    a, b = rt.Context(0), rt.Context(0)
    try:
        for c_ in (a, b):
            _upload(c_, scene, cat_golden)
        a.set_environment_sampling(0.5)                                 # no map: nothing to build
        a.set_environment_sampling(0.0)
        p = _params(2, w=96, h=64)
        before = [[getattr(c_, n)() for n in COUNTS] for c_ in (a, b)]
        for _ in range(4):                                              # fill, use, store the records, resume
            _bits_equal(a.render(p), b.render(p))
        assert _moved(a, before[0]) == _moved(b, before[1])
        a.set_environment_sampling(0.75)                                # a share without a map: still the same frames
        _bits_equal(a.render(_params(2, spp=4)), b.render(_params(2, spp=4)))
        _bits_equal(a.render_pose(_params(2), rt.make_pose(**POSE)), b.render_pose(_params(2), rt.make_pose(**POSE)))
        for env, share in ((MAPS[5], 0.0), (np.zeros((5, 5, 3), f32), 0.5), (np.zeros((1, 1, 3), f32), 1.0)):
            a.set_environment(env)
            b.set_environment(env)
            a.set_environment_sampling(share)
            before = [[getattr(c_, n)() for n in COUNTS] for c_ in (a, b)]
            for q in (_params(2), _params(3, spp=4), _params(0, w=1, h=1)):
                _bits_equal(a.render(q), b.render(q))
            assert _moved(a, before[0]) == _moved(b, before[1])
            if share > 0:
                assert a.kat_environment_table()[2] == 0                # the table is empty
                with pytest.raises(rt.RtError):
                    a.kat_environment_sample([1], 0)
    finally:
        a.close()
        b.close()


# ---- the boundary, on a context ----------------------------------------------------------------------------------------------------------------------------------------------

def test_get_after_set_what_keeps_the_share_what_resets_it_and_what_is_refused(ctx, ref, cat_golden):
    _up(ctx, "room", cat_golden)
    assert ctx.environment_sampling() == 0.0
    lib, h = ctx._L, ctx._h
    ctx.set_environment(MAPS[5])
    ctx.set_environment_sampling(0.25)
    assert ctx.environment_sampling() == 0.25
    tb5 = ssm.Table(MAPS[5])
    _same_table(ctx, tb5)
    for bad in (np.nan, -0.25, 1.0000001, np.inf, -np.inf, 2.0):
        assert lib.rt_scene_set_environment_sampling(h, C.c_float(bad)) == -1, bad
        assert b"environment sampling" in lib.rt_last_error(h)
        assert ctx.environment_sampling() == 0.25
    _same_table(ctx, tb5)                                               # nothing that was refused touched the table
    assert lib.rt_scene_get_environment_sampling(h, None) == -1
    for share in (1.0, 0.5):                                            # another positive share: the table is the map's
        ctx.set_environment_sampling(share)
        assert ctx.environment_sampling() == share
        _same_table(ctx, tb5)
    # the sphere, light, lens and shutter edits keep the share and the table
    ctx.move_sphere(0, (0.0, 2.0, 0.0), 0.5)
    ctx.set_sphere(0, ROOM[0])
    ctx.move_light(0.3, 0.5)
    ctx.set_light(*rt.scenes.LIGHT)
    ctx.set_lights(THREE)
    ctx.set_light(*rt.scenes.LIGHT)
    ctx.set_lens(1.5, 45.0)
    ctx.set_lens(0.0, 1.0)
    ctx.set_shutter(light=(1.0, 0.0, 0.0))
    ctx.set_shutter()
    assert ctx.environment_sampling() == 0.5
    _same_table(ctx, tb5)
    # a replaced map keeps the share and rebuilds the table; a removed one drops it
    ctx.set_environment(MAPS[2])
    assert ctx.environment_sampling() == 0.5
    _same_table(ctx, ssm.Table(MAPS[2]))
    ctx.set_environment()
    assert ctx.environment_sampling() == 0.5
    with pytest.raises(rt.RtError):
        ctx.kat_environment_table()
    with pytest.raises(rt.RtError):
        ctx.kat_environment_sample([1, 2], 0)
    ctx.set_environment(MAPS[64])                                       # set again under the share that stayed
    _same_table(ctx, ssm.Table(MAPS[64]))
    ctx.set_environment_sampling(0.0)                                   # off: no table to read, and the frame is the one without the call
    with pytest.raises(rt.RtError):
        ctx.kat_environment_table()
    _up(ref, "room", cat_golden)
    ref.set_environment(MAPS[64])
    _bits_equal(ctx.render(_params(2)), ref.render(_params(2)))
    ctx.set_environment_sampling(0.5)
    _up(ctx, "room", cat_golden)                                        # an upload resets the share (and removes the map)
    assert ctx.environment_sampling() == 0.0 and ctx.environment() is None
    ctx.set_environment(MAPS[64])
    _bits_equal(ctx.render(_params(2)), ref.render(_params(2)))
    fresh = rt.Context(0)                                               # no upload: RT_ERR_NO_SCENE, and the get writes nothing
    try:
        s = C.c_float(-7.0)
        assert fresh._L.rt_scene_get_environment_sampling(fresh._h, C.byref(s)) == -4 and s.value == -7.0
        assert fresh._L.rt_scene_set_environment_sampling(fresh._h, C.c_float(0.5)) == -4
        total = C.c_uint64(7)
        assert fresh._L.rt_kat_environment_table(fresh._h, None, None, C.byref(total)) == -4 and total.value == 7
    finally:
        fresh.close()
