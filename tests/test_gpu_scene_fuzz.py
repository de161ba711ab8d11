"""The shading step on generated scenes (tests/scene_fuzz.py) against the CPU oracle, which tests/test_scene_fuzz_model.py holds to the reference on the same
generator.  -m gpu.

One test per family over seeds 0 to 23.  sigma is 0, so a frame is the oracle's word for word: colours are compared as uint32 (a signed-zero difference fails)
except where both are NaN, `.w` is the oracle's ray count.  Every render structure (`auto` and the six of test_gpu_parity.VARIANTS), the 8-bit image, the posed
camera and the animated batch see the same scenes: open scenes, exact ties, nested glass with unmatched indices, a light on a surface, odd radii, 16 segments,
and 61 x 43 frames (2623 pixels: the tail of tonemap_kernel, partial 8 x 8 tiles).

A failure names the family, seed and variant, the first differing pixel and both words; scene_fuzz.scene(family, seed) rebuilds the scene."""
import time

import numpy as np
import pytest

import raytracinggpu_amd as rt
from . import scene_fuzz as sf
from .test_gpu_parity import VARIANTS as STRUCTURES

pytestmark = pytest.mark.gpu
VARIANTS = ("auto",) + tuple(STRUCTURES)
POSED = ("room", "glass", "with_mesh")      # seeds 0 to 5 also through rt_render_pose
ANIMATED = ("room", "open", "ties")         # three-frame rt_render_device_batch_scenes
SHOWN = 10                                  # differences spelled out in a failure message


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    yield c
    c.close()


def _params(d, variant="auto", seed=123456):
    return rt.make_params(d["W"], d["H"], d["spp"], d["num_bounce"], depth_convention=0, sigma=float(d["sigma"]), eps=float(d["eps"]), tri_tmin=float(d["tri_tmin"]),
                          seed=seed, variant=variant)


def _differences(got, exp, what, found):
    """colour and ray-count words of two [H, W, 4] float frames; NaN equals NaN in a colour"""
    differ = got.view(np.uint32) != exp.view(np.uint32)
    differ[..., :3] &= ~(np.isnan(got[..., :3]) & np.isnan(exp[..., :3]))
    if differ.any():
        r, c, k = (int(x) for x in np.argwhere(differ)[0])
        found.append(f"{what}: {int(differ.sum())} words differ, first at pixel (row {r}, column {c}) word {k}: device {got.view(np.uint32)[r, c, k]:#010x} "
                     f"({got[r, c, k]!r}) oracle {exp.view(np.uint32)[r, c, k]:#010x} ({exp[r, c, k]!r})")


def _bytes_differ(got, exp, what, found):
    differ = got != exp
    if differ.any():
        r, c, k = (int(x) for x in np.argwhere(differ)[0])
        found.append(f"{what}: {int(differ.sum())} bytes differ, first at pixel (row {r}, column {c}) channel {k}: device {int(got[r, c, k])} oracle {int(exp[r, c, k])}")


def _animated_batch(ctx, oracle, family, seed, found):
    """three frames in one launch chain, each with its own light and sphere poses (one set of materials, num_rays 1): every frame is the oracle's frame of that
    draw -- the ANIM instantiation's sphere search on these scenes"""
    draws = [dict(sf.animated(family, seed, k), spp=1) for k in range(3)]
    d = draws[0]
    ctx.scene_upload(*sf.upload_args(d))
    rows, _ = rt.interleaved_rows(d["H"], 8, 0, 1)
    bufs = [ctx.device_alloc(d["H"] * d["W"] * 16) for _ in draws]
    try:
        frames = [(b, [float(x) for x in d["cam"]], None, 1000 + k) for k, b in enumerate(bufs)]
        scenes = [(([float(x) for x in q["light"][:3]], float(q["light"][3])), [([float(x) for x in s[:3]], float(s[3])) for s in q["spheres"]]) for q in draws]
        ctx.render_device_batch(_params(d), rows, frames, scenes=scenes)
        for k, (q, b) in enumerate(zip(draws, bufs)):
            got = ctx.device_to_host(b, (d["H"], d["W"], 4))
            exp, _ = sf.oracle_render(oracle, q, seed=1000 + k)
            _differences(got, exp, f"{family} seed {seed} animated batch frame {k}", found)
    finally:
        for b in bufs:
            ctx.device_free(b)


@pytest.mark.parametrize("family", sf.FAMILIES)
def test_generated_scenes_equal_the_oracle(ctx, oracle, family):
    found, t0 = [], time.perf_counter()
    for seed in sf.SEEDS:
        d = sf.scene(family, seed)
        osc = sf.oracle_scene(oracle, d)
        exp, _ = sf.oracle_render(oracle, d, scene=osc)
        ctx.scene_upload(*sf.upload_args(d))
        for variant in VARIANTS:
            try:
                _differences(ctx.render(_params(d, variant)), exp, f"{family} seed {seed} variant {variant}", found)
            except rt.RtError as e:                                     # a refused frame is a finding like any other: the remaining scenes still run
                found.append(f"{family} seed {seed} variant {variant}: {e}")
        _bytes_differ(ctx.render_rgb8(_params(d)), oracle.tonemap(exp), f"{family} seed {seed} 8-bit image", found)
        if family in POSED and seed < 6:
            pose = rt.make_pose([float(x) for x in d["cam"]], float(d["pose"][0]), float(d["pose"][1]))
            _differences(ctx.render_pose(_params(d), pose), sf.oracle_render(oracle, d, scene=osc, pose=d["pose"])[0], f"{family} seed {seed} posed camera", found)
        if family in ANIMATED:
            _animated_batch(ctx, oracle, family, seed, found)
    print(f"{family}: {len(sf.SEEDS)} scenes, {len(VARIANTS)} variants each: {time.perf_counter() - t0:.2f} s, {len(found)} comparisons differ")
    for line in found:
        print("  " + line)
    if found:
        pytest.fail(f"{len(found)} comparisons differ (scene_fuzz.scene(family, seed) rebuilds a scene):\n" + "\n".join(found[:SHOWN]))


def test_sixteen_segments_are_the_limit(ctx):
    """num_bounce = 15 in the reference's convention is RT_MAX_SEGMENTS segments and renders; 16 is refused with RT_ERR_INVALID"""
    d = sf.scene("glass", 0)
    ctx.scene_upload(*sf.upload_args(d))
    ctx.render(_params(dict(d, num_bounce=15)))
    for variant in VARIANTS:
        with pytest.raises(rt.RtError) as e:
            ctx.render(_params(dict(d, num_bounce=16), variant))
        assert e.value.code == -1, variant
