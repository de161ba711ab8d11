"""The kernel of a plain chain's last position on the device (csrc/rt_wavefront.hip.h wf_advance<kFormClose>, csrc/rt_still.h kAdvClose, enqueue_chain): a default context against
one created under RT_CHAIN_ENDS=0, which runs the generic wf_advance at every position, word for word, colour and the ray count in .w.  -m gpu.

The reference of every comparison is the knob-off context; the cat and the two sphere presets are compared to the CPU oracle besides.  The shapes are the smallest that can
go wrong: 61 x 45 (no multiple of the 8 x 8 tile: pixel slots outside the frame, a path count that is no multiple of 256) and 64 x 48; num_bounce 0, 1, 2, 3 and 6 (one
segment: the closing launch is the one that closes segment 0's shadow rays from, or into, the first-shadow cache)."""
import numpy as np
import pytest

import raytracinggpu_amd as rt

from . import material_scenes as ms
from . import still_view as sv
from .still_view import H, W

pytestmark = pytest.mark.gpu

KNOB = "RT_CHAIN_ENDS"
_bits_equal, _params, _cat = sv.bits_equal, sv.params, sv.cat
SIZES = [(61, 45), (64, 48)]
BOUNCES = [0, 1, 2, 3, 6]


def _pair(**both):
    on, off = sv.context(**both), sv.context(**both, **{KNOB: "0"})
    try:
        yield on, off
    finally:
        on.close()
        off.close()


@pytest.fixture(scope="module")
def pair():
    yield from _pair()


def _upload(cs, cat_golden, **kw):
    sv.upload(cs, cat_golden, **kw)


def _both(cs, p, render=None):
    """one frame on both contexts, equal word for word"""
    render = render or (lambda c: c.render(p))
    got, exp = render(cs[0]), render(cs[1])
    _bits_equal(got, exp)
    assert np.asarray(got)[..., 3].sum() > 0
    return got


@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("w,h", SIZES)
def test_every_depth(pair, cat_golden, w, h, spp):
    """a new camera height per depth: every frame a miss of every still-view level, the chains open with wf_advance<kFormFirst>"""
    for k, b in enumerate(BOUNCES):
        for c in pair:
            c.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden), camera=((0.0, 0.25 * k, 55.0), None))
        _both(pair, _params(w, h, b=b, spp=spp, seed=3 + b))


@pytest.mark.parametrize("parts", ["1", "2", "3"])
def test_parts(cat_golden, parts):
    for cs in _pair(RT_PARTS=parts):
        _upload(cs, cat_golden)
        for b in (0, 1, 3):
            _both(cs, _params(61, 45, b=b, seed=b))
            assert cs[0].stats()["parts"] == int(parts)


@pytest.mark.parametrize("b", BOUNCES)
def test_a_still_view_of_four_frames(pair, cat_golden, b):
    """the chain that fills the levels, the one that reads them and stores the records, two that resume"""
    _upload(pair, cat_golden)
    on = pair[0]
    before = on.first_shade_cache_counts()
    frames = [_both(pair, _params(61, 45, b=b, seed=9)) for _ in range(4)]
    after = on.first_shade_cache_counts()
    assert after["filled"] - before["filled"] == 2 and after["resumed"] - before["resumed"] == 4
    for f in frames[1:]:
        _bits_equal(f, frames[0])
    _both(pair, _params(61, 45, b=b, spp=3, seed=10))   # three samples as items of one resumed chain


@pytest.mark.parametrize("b", [0, 1, 3])
def test_a_light_that_moves_every_frame(pair, cat_golden, b):
    """the first-shadow cache misses every frame: the hit level is read, the shadow level filled, no records"""
    _upload(pair, cat_golden)
    on = pair[0]
    before = on.first_shade_cache_counts()
    for k in range(4):
        for c in pair:
            c.set_light((5.0 + k, 25.0, 35.0), 2e10)
        _both(pair, _params(b=b, seed=4))
    after = on.first_shade_cache_counts()
    assert after["resumed"] == before["resumed"] and after["filled"] == before["filled"]


def test_no_first_hit_cache(cat_golden):
    for cs in _pair(RT_FIRST_HIT_CACHE="0"):
        _upload(cs, cat_golden)
        for b in (0, 1, 3):
            for _ in range(2):
                _both(cs, _params(61, 45, b=b, seed=2))


def _shadow_work(c, p):
    return c.count_work(p, detail=True)["dead_channels"]


@pytest.mark.parametrize("knob", [None, "RT_TRAVQ_ANYHIT", "RT_DEAD_CHANNELS"])
def test_elision_rules(cat_golden, knob):
    """default rules, a cat with dead channels: shadow rays of the last segment are elided -- the closing launch folds paths whose ray was never traced -- and others go to
    the traversal; a rule off: nothing is elided for dead channels, the rays are handed over"""
    # (RT_TRAVQ_QW_COUNT=1: rt_count_work counts the production kernels' work, any-hit and the dead-channel rule as the frames have them)
    for cs in _pair(RT_TRAVQ_QW_COUNT="1", **({knob: "0"} if knob else {})):
        _upload(cs, cat_golden, albedo=(0.0, 0.5, 1.0))
        for b in (1, 3):
            p = _params(61, 45, b=b, seed=5)
            _both(cs, p)
            _both(cs, _params(61, 45, b=b, spp=3, seed=6))
            d = _shadow_work(cs[0], p)
            assert d == _shadow_work(cs[1], p)
            assert d["trav_shadow"] > 0
            if knob is not None:
                assert d["elided"] == 0, d
            elif b == 3:                                 # every wall has two zero channels: after three diffuse walls a path's channels are dead
                assert d["elided"] > 0, d


@pytest.mark.parametrize("name", ["spheres", "demo10"])
def test_sphere_presets(pair, oracle, name):
    """no mesh: every shadow ray misses the root box; demo10's mirror and glass paths end without a shadow ray"""
    for c in pair:
        c.scene_upload(rt.scenes.spheres(name), None)
    for b in (0, 1, 3, 6):
        got = _both(pair, _params(61, 45, b=b, seed=123456, variant="wavefront_queue"))   # (the oracle's seed)
        if b == 3:
            exp, _, _ = oracle.Scene.preset(name).render(61, 45, 1, b, want_rgb8=False)
            _bits_equal(got[..., :3], exp[..., :3])
            assert int(got[..., 3].sum()) == int(exp[..., 3].sum())


@pytest.mark.parametrize("name", ["cpu_mirror", "cpu_glass", "two_cats"])
def test_material_scenes(pair, cat_golden, name):
    spheres, meshes = ms.capi_scene(name, cat_golden["vertices"], cat_golden["tri_obj_order"])
    for c in pair:
        c.scene_upload(spheres, meshes)
    for b in (1, 2, 6):
        for _ in range(3):
            _both(pair, _params(b=b, seed=6))


def test_the_cat_against_the_oracle(pair, cat_golden, oracle, oracle_cat):
    _upload(pair, cat_golden)
    for b in (0, 2):
        got = _both(pair, _params(b=b, seed=123456))
        exp, _, _ = oracle.Scene.preset("cpu", oracle_cat).render(W, H, 1, b, want_rgb8=False)
        _bits_equal(got[..., :3], exp[..., :3])
        assert int(got[..., 3].sum()) == int(exp[..., 3].sum())


def test_a_batch_of_three_cameras(pair, cat_golden):
    import torch
    _upload(pair, cat_golden)
    for b in (0, 1, 3):
        p = _params(b=b, seed=0)
        got = _both(pair, p, lambda c: sv.batch_of_three(c, p))
        rows = rt._capi.Rows(0, H, H, 1)
        for k in range(3):                               # ... against three lone frames of the knob-off context, through a batch of one
            buf = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
            pair[1].render_device_batch(p, rows, [(buf.data_ptr(), (0.5 * k, 0.0, 55.0 - 3 * k), None, 40 + k)])
            pair[1].synchronize()
            _bits_equal(got[k], buf.cpu().numpy())


@pytest.mark.parametrize("b", [0, 1, 3])
def test_count_work(pair, cat_golden, b):
    _upload(pair, cat_golden)
    p = _params(61, 45, b=b, seed=1)
    on, off = (c.count_work(p, detail=True) for c in pair)
    assert on == off and on["rays"] > 0


def test_a_textured_cat_and_two_lights_keep_the_generic_kernels(pair, cat_golden):
    """outside the scope: the frames of the parent's launches"""
    v, tv = np.asarray(cat_golden["vertices"], np.float32), np.asarray(cat_golden["tri_bvh_order"])[:, :3]
    lo, hi = v.min(0), v.max(0)
    uv = ((v[:, :2] - lo[:2]) / (hi[:2] - lo[:2])).astype(np.float32)
    px = np.random.default_rng(3).integers(0, 256, size=(23, 37, 3), dtype=np.uint8)
    _upload(pair, cat_golden, albedo=(1.0, 1.0, 1.0))
    for c in pair:
        c.mesh_set_texture(uv, tv, px, filter="bilinear", wrap="repeat")
    for b in (0, 2):
        _both(pair, _params(61, 45, b=b, seed=2))
    for c in pair:
        c.mesh_set_texture(None, None, None)
        c.set_lights([((-10.0, 20.0, 40.0), 2e10), ((15.0, 10.0, 30.0), 1e10)])
    for b in (0, 2):
        _both(pair, _params(61, 45, b=b, seed=2))
