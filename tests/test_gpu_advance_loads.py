"""The load order of the plain chain's wf_advance launches on the device (csrc/rt_wavefront.hip.h wf_advance_path, PLAIN: the Y record in one access, the result words and
the dead-channel byte in one round behind the flag word, the shadow ray formed again from the Y record and the light instead of being read back, the closing kernel's fold
words asked for at once): frames against the CPU oracle, the colour word for word and the frame's ray count.  -m gpu.

The cat at 70 x 45: 9 x 6 tiles of 8 x 8 pixel slots, so pixel slots lie outside the frame, a sub-frame's path count is no multiple of 256 (its last wave ends in
padding) and the two sub-frames take an odd number of tile rows between them.  num_bounce b is a chain of b + 1 segments: 1, 2, 3 and 5 bounces, and 0 and 4 beside them.
num_bounce 0 (one segment) is the route on which the closing launch meets shadow rays of the chain's first shading launch; 2 fills the round of three segments the
closing kernel holds in registers; 3 is the headline's chain, three form-0 launches and one more segment through the fold's loop; 5 goes two past the round.
Every route of the shadow ray's close is named by a test: a traced ray that misses, one that hits the mesh (the light behind the cat: form 0 at the positions before
the last, the closing kernel at the last), a chain without the closing kernel (RT_CHAIN_ENDS=0: form 0 closes the last segment's rays from the origin the last shading
launch stored), the first-shadow cache's fill and read, the records' fill and resume, and segments that emit a continuation ray and no shadow ray (mirror, glass).

rt_count_work has no counter of shadow rays that HIT the mesh (trav_shadow counts the shadow rays handed to the traversal), so that such rays exist is shown from four
oracle frames of one segment, see _wall_pixels_the_cat_shadows."""
import numpy as np
import pytest

import raytracinggpu_amd as rt

from . import still_view as sv

pytestmark = pytest.mark.gpu

W, H = 70, 45
SEED = 123456                                          # (the oracle's default)
MIRROR = ((-25.0, 0.0, 0.0), 8.0, (0.0, 0.0, 0.0), 1, 1.0, 1.0)
GLASS = ((25.0, 0.0, 5.0), 8.0, (0.0, 0.0, 0.0), 0, 1.5, 1.0)
_bits_equal, _params, _cat = sv.bits_equal, sv.params, sv.cat
_refs = {}


def _behind(cat_golden):
    """a light close behind the cat, seen from the camera at z = 55"""
    v = np.asarray(cat_golden["vertices"], np.float32)
    lo, hi = v.min(0), v.max(0)
    return (float(0.5 * (lo[0] + hi[0])), float(0.5 * (lo[1] + hi[1])), float(lo[2] - 2.0))


def _ref(oracle, oracle_cat, w=W, h=H, spp=1, b=2, light=None, extra=(), cam=(0.0, 0.0, 55.0), seed=SEED, cat=True):
    """the oracle's frame, computed once per configuration and never written to"""
    key = (w, h, spp, b, light, extra, cam, seed, cat)
    if key not in _refs:
        s = oracle.Scene.preset("cpu", oracle_cat if cat else None)
        for c, r, a, m, ni, no in extra:
            s.add_sphere(c, r, a, m, ni, no)
        if light is not None:
            s.set_light(light, rt.scenes.LIGHT[1])
        exp, _, _ = s.render(w, h, spp, b, cam=cam, seed=seed, want_rgb8=False)
        exp.setflags(write=False)
        _refs[key] = exp
    return _refs[key]


def _wall_pixels_the_cat_shadows(oracle, oracle_cat, light):
    """Pixels of the one-segment frame whose shadow ray ends on the mesh, from the oracle alone.  A pixel whose colour under the default light is the same nonzero words
    with and without the cat has a wall as its first hit (the cat is grey, every wall has a zero channel) -- the same first hit under any light.  If under `light` it is
    lit without the cat (a direct term above +0: the ray is neither moot nor shaded by a sphere) and +0 in every channel with it, the cat's mesh hides the light: the
    shadow ray's word is a hit and light_hidden holds for it.  Segment 0's shadow ray does not depend on the depth: in a longer chain the same rays are closed by form 0."""
    bits = lambda a: np.ascontiguousarray(a[..., :3]).view(np.uint32)
    front_cat, front_none = _ref(oracle, oracle_cat, b=0), _ref(oracle, oracle_cat, b=0, cat=False)
    wall = (bits(front_cat) == bits(front_none)).all(-1) & (front_none[..., :3] > 0).any(-1)
    with_cat, without = _ref(oracle, oracle_cat, b=0, light=light), _ref(oracle, oracle_cat, b=0, light=light, cat=False)
    return wall & (without[..., :3] > 0).any(-1) & (bits(with_cat) == 0).all(-1)


def _same(got, exp):
    _bits_equal(got[..., :3], exp[..., :3])
    assert int(got[..., 3].sum()) == int(exp[..., 3].sum()) > 0


def _upload(c, cat_golden, extra=(), light=None):
    c.scene_upload(rt.scenes.spheres("cpu") + list(extra), _cat(cat_golden))
    if light is not None:
        c.set_light(light, rt.scenes.LIGHT[1])


@pytest.fixture(scope="module")
def ctx():
    c = sv.context()
    try:
        yield c
    finally:
        c.close()


def _knob_context(**kw):
    c = sv.context(**kw)
    try:
        yield c
    finally:
        c.close()


@pytest.mark.parametrize("b", [0, 1, 2, 3, 4, 5])
def test_every_depth(ctx, cat_golden, oracle, oracle_cat, b):
    _upload(ctx, cat_golden)
    _same(ctx.render(_params(W, H, b=b, seed=SEED)), _ref(oracle, oracle_cat, b=b))


def test_four_samples(ctx, cat_golden, oracle, oracle_cat):
    _upload(ctx, cat_golden)
    for b in (2, 3):
        _same(ctx.render(_params(W, H, b=b, spp=4, seed=SEED)), _ref(oracle, oracle_cat, spp=4, b=b))


def test_an_interleaved_row_share(ctx, cat_golden, oracle, oracle_cat):
    """tiles of 8 rows, every second one: a path's key is its pixel's, so the share's rows are the whole frame's"""
    _upload(ctx, cat_golden)
    p = _params(W, H, b=2, seed=SEED)
    exp = _ref(oracle, oracle_cat)
    for r in (0, 1):
        rows, idx = rt.interleaved_rows(H, 8, r, 2)
        _same(sv.render_rows(ctx, p, rows, len(idx)), exp[idx])


def test_a_batch_of_three_against_three_lone_frames(ctx, cat_golden, oracle, oracle_cat):
    _upload(ctx, cat_golden)
    got = sv.batch_of_three(ctx, _params(b=2, seed=0))             # (sv.W x sv.H, a camera and a seed per frame)
    for k in range(3):
        _same(got[k], _ref(oracle, oracle_cat, sv.W, sv.H, cam=(0.5 * k, 0.0, 55.0 - 3 * k), seed=40 + k))


@pytest.mark.parametrize("b", [0, 2, 3])
def test_a_still_view_then_a_light_that_moves_by_an_ulp(ctx, cat_golden, oracle, oracle_cat, b):
    """five frames of one view: the chains fill the levels, store the records, resume; then five under a light one ulp further each: no level above the hit is read"""
    _upload(ctx, cat_golden)
    p = _params(W, H, b=b, seed=SEED)
    before = ctx.first_shade_cache_counts()
    for _ in range(5):
        _same(ctx.render(p), _ref(oracle, oracle_cat, b=b))
    after = ctx.first_shade_cache_counts()
    assert after["filled"] > before["filled"] and after["resumed"] > before["resumed"]
    x = np.float32(rt.scenes.LIGHT[0][0])
    for _ in range(5 if b == 3 else 2):
        x = np.nextafter(x, np.float32(0.0))
        light = (float(x),) + tuple(rt.scenes.LIGHT[0][1:])
        ctx.set_light(light, rt.scenes.LIGHT[1])
        _same(ctx.render(p), _ref(oracle, oracle_cat, b=b, light=light))
    assert ctx.first_shade_cache_counts()["resumed"] == after["resumed"]


@pytest.mark.parametrize("knob", [dict(RT_PARTS="1"), dict(RT_PARTS="3"), dict(RT_CHAIN_ENDS="0"), dict(RT_TRAVQ_ANYHIT="0"), dict(RT_DEAD_CHANNELS="0")],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_contexts_that_take_other_launches(cat_golden, oracle, oracle_cat, knob):
    """the same frames where form 0 runs in the closing kernel's place or traces the rays the default elides; three frames of a still view each"""
    for c in _knob_context(**knob):
        _upload(c, cat_golden)
        for b in (0, 2, 3):
            for _ in range(3):
                _same(c.render(_params(W, H, b=b, seed=SEED)), _ref(oracle, oracle_cat, b=b))
        _same(c.render(_params(W, H, b=2, spp=4, seed=SEED)), _ref(oracle, oracle_cat, spp=4))


@pytest.mark.parametrize("shadow_cache", ["1", "0"])
@pytest.mark.parametrize("ends", ["1", "0"])
def test_the_light_behind_the_cat(cat_golden, oracle, oracle_cat, ends, shadow_cache):
    """many shadow rays end on the mesh: the close forms the ray again from the Y record at every position, at the last one in the closing kernel (or, without it, in
    form 0) from the origin the last shading launch stored.  Without the first-shadow cache the one-segment chain takes that route too; with it, the read-back."""
    light = _behind(cat_golden)
    hit = _wall_pixels_the_cat_shadows(oracle, oracle_cat, light)
    assert hit.sum() > 0                                             # the frame has shadow rays that end on the mesh (716 of its 3150 pixels)
    for c in _knob_context(RT_CHAIN_ENDS=ends, RT_FIRST_SHADOW_CACHE=shadow_cache, RT_TRAVQ_QW_COUNT="1"):
        _upload(c, cat_golden, light=light)
        for b in (0, 1, 2, 3, 4):
            p = _params(W, H, b=b, seed=SEED)
            exp = _ref(oracle, oracle_cat, b=b, light=light)
            for _ in range(3 if b in (0, 2, 3) else 1):              # (a still view: fill, records, resume)
                got = c.render(p)
                _same(got, exp)
                if b == 0:                                           # the device closed those rays as hits: +0 where the wall alone is lit
                    assert (np.ascontiguousarray(got[..., :3]).view(np.uint32)[hit] == 0).all()
        assert (_ref(oracle, oracle_cat, b=2, light=light)[..., :3] != _ref(oracle, oracle_cat, b=2)[..., :3]).any()
        wk = c.count_work(_params(W, H, b=2, seed=SEED), detail=True)
        assert wk["dead_channels"]["trav_shadow"] > 0, wk["dead_channels"]       # the frame has shadow rays that go through the mesh


def test_a_mirror_and_a_glass_sphere(ctx, cat_golden, oracle, oracle_cat):
    """segments that emit a continuation ray and no shadow ray"""
    extra = (MIRROR, GLASS)
    _upload(ctx, cat_golden, extra=extra)
    for b in (1, 2, 3, 4):
        exp = _ref(oracle, oracle_cat, b=b, extra=extra)
        for _ in range(2):
            _same(ctx.render(_params(W, H, b=b, seed=SEED)), exp)
    assert (_ref(oracle, oracle_cat, b=2, extra=extra)[..., :3] != _ref(oracle, oracle_cat, b=2)[..., :3]).any()


@pytest.mark.parametrize("b", [0, 3])
def test_count_work_is_that_of_a_chain_without_the_closing_kernel(ctx, cat_golden, b):
    _upload(ctx, cat_golden)
    p = _params(W, H, b=b, seed=1)
    on = ctx.count_work(p, detail=True)
    for off in _knob_context(RT_CHAIN_ENDS="0"):
        _upload(off, cat_golden)
        assert on == off.count_work(p, detail=True) and on["rays"] > 0
