"""The dead-channel rule on the device (rt_wavefront.hip.h: wf_dead_channels): a context with the rule on against one with RT_DEAD_CHANNELS=0, word for word, colour
and .w -- and the step counters that say the rule elided rays at all.  -m gpu.

Frames of 64 x 48 (12 tiles of 8 x 8: several workgroups of wf_advance, two sub-frames).  The arithmetic behind the rule is tests/test_dead_channels.py."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import raytracinggpu_amd as rt

pytestmark = pytest.mark.gpu

W, H = 64, 48
CASES = [(spp, b) for spp in (1, 4) for b in (0, 3, 5)]


@contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _context(**kw):
    with _env(**kw):                                   # the knobs are read once, when the context is created
        return rt.Context(0)


@pytest.fixture(scope="module")
def pair():
    on, off = _context(), _context(RT_DEAD_CHANNELS="0")
    yield on, off
    on.close()
    off.close()


@pytest.fixture(scope="module")
def counting_pair():
    """rt_count_work through the production kernels' counting instantiation (any-hit on, as in a frame)"""
    on, off = _context(RT_TRAVQ_QW_COUNT="1"), _context(RT_TRAVQ_QW_COUNT="1", RT_DEAD_CHANNELS="0")
    yield on, off
    on.close()
    off.close()


def _bits_equal(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _cat(cat_golden, slot, albedo=rt.scenes.CAT_ALBEDO):
    return dict(vertices=cat_golden["vertices"], indices=cat_golden["tri_bvh_order"], bvh_arr10=cat_golden["bvh_arr10"], albedo=albedo, object_slot=slot)


def _params(spp, b, **kw):
    d = dict(rt.scenes.CPU_LAUNCHER)
    d.update(kw)
    return rt.make_params(W, H, spp, b, **d)


def _same_frames(pair, cases=CASES, **kw):
    on, off = pair
    for spp, b in cases:
        p = _params(spp, b, **kw)
        _bits_equal(on.render(p), off.render(p))


@pytest.mark.parametrize("preset", ["cpu", "demo10"])
def test_wall_presets_with_the_cat(pair, cat_golden, preset):
    """the six pure-colour walls and the grey cat; demo10 puts mirror and glass spheres between the dead segments"""
    for c in pair:
        c.scene_upload(rt.scenes.spheres(preset), _cat(cat_golden, rt.scenes.mesh_slot(preset)))
    _same_frames(pair)
    _same_frames(pair, cases=[(2, 3)], sigma=0.2)


def test_the_cat_against_the_oracle(pair, oracle, oracle_cat, cat_golden):
    on, _ = pair
    on.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden, 6))
    osc = oracle.Scene.preset("cpu", oracle_cat)
    for spp, b in ((1, 3), (4, 5)):
        exp, _, _ = osc.render(W, H, spp, b, want_rgb8=False)
        _bits_equal(on.render(_params(spp, b)), exp)


def test_texture_with_zero_texels(pair, cat_golden):
    """a white cat whose texture decodes a third of its bytes to 0: the sampled albedo, not the material's, kills the channels (nearest) -- and a bilinear mix of zero
    and non-zero texels is only dead where all four are"""
    rng = np.random.default_rng(21)
    v, tv = np.asarray(cat_golden["vertices"], np.float32), np.asarray(cat_golden["tri_bvh_order"])[:, :3]
    lo, hi = v.min(0), v.max(0)
    uv = ((v[:, :2] - lo[:2]) / (hi[:2] - lo[:2])).astype(np.float32)
    px = rng.integers(0, 256, size=(23, 37, 3), dtype=np.uint8)
    dec = np.where(np.arange(256) % 3 == 0, 0.0, rng.random(256)).astype(np.float32)
    for filt in ("nearest", "bilinear"):
        for c in pair:
            c.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden, 6, albedo=(1.0, 1.0, 1.0)))
            c.mesh_set_texture(uv, tv, px, filter=filt, wrap="repeat", decode=dec)
        _same_frames(pair, cases=[(1, 3), (4, 5)])


def _random_scene(rng):
    pick = lambda: tuple(float(x) for x in rng.choice([0.0, 0.5, 1.0], 3))
    spheres = [(c, r, pick()) for c, r, _ in rt.scenes.WALLS]
    spheres.append(((float(rng.uniform(-25, -12)), float(rng.uniform(-5, 15)), float(rng.uniform(-10, 20))), 6.0, pick()))
    spheres.append(((float(rng.uniform(12, 25)), float(rng.uniform(-5, 15)), float(rng.uniform(-10, 20))), 6.0, (0, 0, 0), int(rng.integers(0, 2)), 1.0, 1.0))
    return spheres, pick()


def test_random_albedos_from_zero_half_one(pair, cat_golden):
    rng = np.random.default_rng(5)
    for _ in range(12):
        spheres, cat_albedo = _random_scene(rng)
        for c in pair:
            c.scene_upload(spheres, _cat(cat_golden, len(spheres), albedo=cat_albedo))
        _same_frames(pair, cases=[(1, 3), (4, 5)])


def test_a_batch_of_three_frames(pair, cat_golden):
    import torch
    rows = rt._capi.Rows(0, H, H, 1)
    out = []
    for c in pair:
        c.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden, 6))
        bufs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
        c.render_device_batch(_params(1, 3), rows, [(bf.data_ptr(), (0.0, 0.0, 55.0 - 3 * k), None, 40 + k) for k, bf in enumerate(bufs)])
        c.synchronize()
        out.append([bf.cpu().numpy() for bf in bufs])
    for g, w in zip(*out):
        _bits_equal(g, w)
    assert not np.array_equal(out[0][0], out[0][1])


@pytest.mark.parametrize("preset", ["cpu", "demo10"])
def test_the_rule_elides_rays_in_the_wall_scenes(counting_pair, cat_golden, preset):
    """so that the comparisons above are not vacuous: with the rule on shadow rays are elided and fewer reach the traversal; the reference's ray count (.w) is the same,
    the continuation rays are the same, and no path leaves the range the rule is argued for"""
    on, off = counting_pair
    for c in counting_pair:
        c.scene_upload(rt.scenes.spheres(preset), _cat(cat_golden, rt.scenes.mesh_slot(preset)))
    for spp, b in ((1, 3), (4, 5)):
        p = _params(spp, b)
        a, z = on.count_work(p, detail=True), off.count_work(p, detail=True)
        da, dz = a["dead_channels"], z["dead_channels"]
        assert a["rays"] == z["rays"]
        assert da["elided"] > 0 and dz["elided"] == 0
        assert da["trav_continuation"] == dz["trav_continuation"] > 0
        assert 0 < dz["trav_shadow"] - da["trav_shadow"] <= da["elided"]        # an elided ray is not even tested against the root box
        assert da["unsure"] == 0 and dz["unsure"] == 0
    p0 = _params(1, 0)                                                           # one segment: one wall kills two channels at most
    assert on.count_work(p0, detail=True)["dead_channels"]["elided"] == 0
