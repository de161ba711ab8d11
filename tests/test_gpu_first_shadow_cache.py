"""The first-shadow cache on the device (the shadow level of csrc/rt_still.h, enqueue_chain, the two wf_advance launches that emit and close segment 0's shadow rays): a default context
against one created under RT_FIRST_SHADOW_CACHE=0, word for word, colour and .w -- and rt_first_shadow_cache_counts, which says whether a chain read the cache, filled it
or was not eligible, so that every comparison below is known to have gone through the path it names.  -m gpu.

The cat at 64 x 48 with num_bounce 2 (two sub-frames of three 8-row tiles: two launch chains per frame and sample chunk), the shapes of test_gpu_first_hit_cache.py.  The
reference of every comparison is the knob-off context, never the cached one.  The scenes of tests/material_scenes.py hold no mirror or glass SPHERE: the three used here
show the camera a mirror mesh, a glass mesh and two meshes (one of them a mirror) -- first hits without a shadow ray next to first hits with one."""
from functools import partial

import numpy as np
import pytest

import raytracinggpu_amd as rt

from . import material_scenes as ms
from . import still_view as sv
from .still_view import B, H, W

pytestmark = pytest.mark.gpu

LEVEL = sv.SHADOW
ZERO = sv.zero(LEVEL)
_bits_equal, _params, _upload, _chunk, _render_rows = sv.bits_equal, sv.params, sv.upload, sv.chunk, sv.render_rows
_pair, _delta, _expect, _frame = partial(sv.pair, LEVEL), partial(sv.delta, LEVEL), partial(sv.expect, LEVEL), partial(sv.frame, LEVEL)


@pytest.fixture(scope="module")
def pair():
    yield from _pair()


@pytest.fixture(scope="module")
def pair_one_sample_per_chain():
    """RT_PATH_SAMP_MB=1: a chain's state may take 1 MB; a sample of 64 x 48 with 13 segments takes 0.73: one sample per chain"""
    yield from _pair(RT_PATH_SAMP_MB="1")


def _miss_then_skip(pair, p, render=None):
    got = _frame(pair, p, render, filled=1, key_misses=1)
    _bits_equal(_frame(pair, p, render, skipped=1), got)
    return got


def test_the_same_frame_three_times(pair, cat_golden):
    _upload(pair, cat_golden)
    p = _params()
    a = _frame(pair, p, cold=True, filled=1)
    b = _frame(pair, p, skipped=1)
    c = _frame(pair, p, skipped=1)
    _bits_equal(a, b)
    _bits_equal(a, c)
    assert pair[1].first_shadow_cache_counts()["skipped"] == 0


def test_a_new_seed_with_everything_else_still(pair, cat_golden):
    _upload(pair, cat_golden)
    a = _frame(pair, _params(seed=1), cold=True, filled=1)
    b = _frame(pair, _params(seed=2), skipped=1)
    assert not np.array_equal(a, b)                   # the bounce rays do read the seed


def test_light_and_sphere_edits_miss_and_refill(pair, cat_golden):
    _upload(pair, cat_golden)
    p = _params()
    on = pair[0]
    frames = [_frame(pair, p, cold=True, filled=1)]
    slot = 0
    s = on.sphere(slot)
    edits = [lambda c: c.set_light((5.0, 25.0, 35.0), 2e10),
             lambda c: c.move_light(1.0),
             lambda c: c.move_sphere(slot, (3.0, 1.0, -2.0)),
             lambda c: c.set_sphere(slot, (s[0], s[1] * 1.5, (0.9, 0.1, 0.2), 0, 1.0, 1.0)),   # new geometry (and albedo)
             lambda c: c.set_sphere(slot, (s[0], s[1], s[2], 1, 1.0, 1.0)),                     # a mirror: its first hits have no shadow ray
             lambda c: c.set_sphere(slot, s)]                                                   # and back

    def all_edits():
        for e in edits:
            for c in pair:
                e(c)
            frames.append(_miss_then_skip(pair, p))
            assert not np.array_equal(frames[-1], frames[-2])
    _, fh = _delta(on, all_edits, "first_hit_cache_counts")
    assert fh["key_misses"] == 0 and fh["filled"] == 0 and fh["skipped"] == 2 * 2 * len(edits), fh   # the first-hit cache was kept throughout


def _vertex_normals(v, t):
    n = np.zeros_like(v)
    fn = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    for k in range(3):
        np.add.at(n, t[:, k], fn)
    return (n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-20)).astype(np.float32)


def test_texture_and_smooth_normal_edits_miss(pair, cat_golden):
    rng = np.random.default_rng(3)
    v, tv = np.asarray(cat_golden["vertices"], np.float32), np.asarray(cat_golden["tri_bvh_order"])[:, :3]
    lo, hi = v.min(0), v.max(0)
    uv = ((v[:, :2] - lo[:2]) / (hi[:2] - lo[:2])).astype(np.float32)
    px0 = rng.integers(0, 256, size=(23, 37, 3), dtype=np.uint8)
    px0[::2, ::3] = 0                                  # texels of albedo +0: dead channels at segment 0
    _upload(pair, cat_golden, albedo=(1.0, 1.0, 1.0))
    p = _params()
    on = pair[0]
    a = _frame(pair, p, cold=True, filled=1)

    def edits():
        for c in pair:
            c.mesh_set_texture(uv, tv, px0, filter="bilinear", wrap="repeat")
        b = _miss_then_skip(pair, p)
        assert not np.array_equal(a, b)
        px = rng.integers(0, 256, size=(11, 5, 3), dtype=np.uint8)
        for c in pair:
            c.mesh_set_texture(uv, tv, px, filter="nearest", wrap="clamp")
        c2 = _miss_then_skip(pair, p)
        assert not np.array_equal(b, c2)
        for c in pair:
            c.mesh_set_texture(None, None, None)
        _bits_equal(_miss_then_skip(pair, p), a)
        vn = _vertex_normals(v, tv)
        for c in pair:
            c.mesh_set_normals(vn, cat_golden["tri_bvh_order"])
        d = _miss_then_skip(pair, p)
        assert not np.array_equal(a, d)
        for c in pair:
            c.mesh_set_normals(-vn, cat_golden["tri_bvh_order"])    # in place: the same pointer, other normals
        assert not np.array_equal(_miss_then_skip(pair, p), d)
        for c in pair:
            c.mesh_set_normals(None, None)
        _bits_equal(_miss_then_skip(pair, p), a)
    _, fh = _delta(on, edits, "first_hit_cache_counts")
    assert fh["key_misses"] == 0, fh


ROT = [0.96, 0.0, 0.28, 0.0, 1.0, 0.0, -0.28, 0.0, 0.96]


def test_frame_camera_and_mesh_edits_miss(pair, cat_golden):
    _upload(pair, cat_golden)
    p = _params()
    a = _frame(pair, p, cold=True, filled=1)
    _frame(pair, p, skipped=1)
    assert not np.array_equal(_miss_then_skip(pair, _params(eps=2e-3)), a)
    _miss_then_skip(pair, p)
    _miss_then_skip(pair, _params(tri_tmin=30.0))      # beyond the nearest triangles of many rays: other hits
    _miss_then_skip(pair, p)
    pose = rt.make_pose(position=(0.5, 0.0, 55.0), yaw=0.1, pitch=0.05)
    _miss_then_skip(pair, p, lambda c: c.render_pose(p, pose))
    _miss_then_skip(pair, p)
    for c in pair:
        c.mesh_transform(ROT, (1.5, -2.0, 0.5))
    _miss_then_skip(pair, p)
    for c in pair:
        c.mesh_rebuild(len(cat_golden["tri_bvh_order"]), mode="lbvh")
    _miss_then_skip(pair, p)
    _upload(pair, cat_golden, albedo=(0.0, 0.5, 1.0))  # a re-upload with another albedo (a channel of the cat dead)
    b = _miss_then_skip(pair, p)
    assert not np.array_equal(a, b)


@pytest.mark.parametrize("which", ["default_chunk", "one_sample_per_chain"])
def test_five_samples_per_pixel(pair, pair_one_sample_per_chain, cat_golden, which):
    cs = pair if which == "default_chunk" else pair_one_sample_per_chain
    b = B if which == "default_chunk" else 12          # 13 segments: 177 bytes per item, 0.73 MB per sample
    chunk = _chunk(5, (400 if which == "default_chunk" else 1) << 20, b)
    assert chunk == (5 if which == "default_chunk" else 1)
    chains = (5 + chunk - 1) // chunk
    _upload(cs, cat_golden)                            # a cold cache: whatever the context held is another mesh generation
    p = _params(b=b, spp=5)
    _frame(cs, p, cold=True, filled=1, skipped=chains - 1)   # one chain per part fills (its later samples' items read the first sample's rays), the rest read
    _frame(cs, p, skipped=chains)
    _frame(cs, _params(b=b, spp=5, seed=77), skipped=chains)
    # a counting run goes round the cache: the reference's work, the same on both contexts
    on, off = cs
    wk, d = _delta(on, lambda: on.count_work(p))
    assert d["ineligible"] > 0 and d["skipped"] == d["filled"] == d["key_misses"] == 0, d
    ref = off.count_work(p)
    for k in ("rays", "box_tests", "nodes", "tri_tests"):
        assert wk[k] == ref[k] > 0, k
    _frame(cs, p, skipped=chains)                      # ... and leaves it as it was


@pytest.mark.parametrize("b", [0, 1])
def test_short_paths(pair, cat_golden, b):
    """num_bounce 0: one segment -- a reading chain enqueues neither traversal launch; num_bounce 1: the launch that closes segment 0's shadow rays emits segment 1's"""
    _upload(pair, cat_golden)
    for spp in (1, 3):
        p = _params(b=b, spp=spp)
        a = _frame(pair, p, cold=spp == 1, filled=0 if spp == 3 else 1, skipped=1 if spp == 3 else 0)   # (the depth is not in the key: the three-sample frame reads)
        _bits_equal(_frame(pair, p, skipped=1), a)
        _frame(pair, _params(b=b, spp=spp, seed=5), skipped=1)


@pytest.mark.parametrize("knob", ["RT_TRAVQ_ANYHIT", "RT_DEAD_CHANNELS"])
def test_an_elision_rule_off_on_both_contexts(cat_golden, knob):
    for cs in _pair(**{knob: "0"}):
        _upload(cs, cat_golden, albedo=(0.0, 0.5, 1.0))
        for spp in (1, 3):
            p = _params(spp=spp)
            _frame(cs, p, cold=spp == 1, filled=1 if spp == 1 else 0, skipped=0 if spp == 1 else 1)
            _frame(cs, p, skipped=1)
            _frame(cs, _params(spp=spp, seed=9), skipped=1)


def test_without_the_first_hit_cache_it_is_off(cat_golden):
    for cs in _pair(on_kw=dict(RT_FIRST_HIT_CACHE="0")):
        _upload(cs, cat_golden)
        for k in range(3):
            _frame(cs, _params(spp=1 + k), ineligible=1)
        assert cs[0].first_shadow_cache_counts() == dict(ZERO, ineligible=6)


def test_row_shares_and_sizes_alternate(pair, cat_golden):
    _upload(pair, cat_golden)
    p = _params()
    shares = [rt.interleaved_rows(H, 8, r, 2) for r in (0, 1)]
    first = True
    for k in range(2):
        for rows, idx in shares:                       # each share is one sub-frame of three tiles cut in two
            _frame(pair, p, lambda c: _render_rows(c, p, rows, len(idx)), cold=first, filled=1, key_misses=0 if first else 1)
            first = False
    rows, idx = shares[1]
    _frame(pair, p, lambda c: _render_rows(c, p, rows, len(idx)), skipped=1)
    for k in range(2):
        _frame(pair, _params(72, 40), filled=1, key_misses=1)
        _frame(pair, p, filled=1, key_misses=1)
    _frame(pair, p, skipped=1)


def test_pipelined_frames_into_two_buffers(pair, cat_golden):
    sv.pipelined_frames(LEVEL, pair, cat_golden, filled=1, used=5)


def test_batches_stats_and_count_lists_go_round_the_cache(pair, cat_golden):
    _upload(pair, cat_golden)
    on, off = pair
    p = _params()
    base = _frame(pair, p, cold=True, filled=1)
    got, d = _delta(on, lambda: sv.batch_of_three(on, p))
    _bits_equal(got, sv.batch_of_three(off, p))
    assert d["ineligible"] > 0 and d["skipped"] == d["filled"] == d["key_misses"] == 0, d
    _frame(pair, p, skipped=1)
    on.stats_enable(True)
    try:
        _frame(pair, p, ineligible=1)
        assert on.stats()["trav_launches"] == (B + 1) + 1
    finally:
        on.stats_enable(False)
    _frame(pair, p, skipped=1)
    counts = np.random.default_rng(5).integers(0, 4, size=(H, W), dtype=np.uint8)
    got, d = _delta(on, lambda: on.render_counts(p, counts, base=base))
    _bits_equal(got, off.render_counts(p, counts, base=base))
    _expect(d)                                         # a list chain does not look at the cache: the counters stay where they are
    _bits_equal(_frame(pair, p, skipped=1), base)


@pytest.mark.parametrize("name", ["cpu_mirror", "cpu_glass", "two_cats"])
def test_material_scenes(pair, cat_golden, name):
    spheres, meshes = ms.capi_scene(name, cat_golden["vertices"], cat_golden["tri_obj_order"])
    for c in pair:
        c.scene_upload(spheres, meshes)
    a = _frame(pair, _params(seed=1), cold=True, filled=1)
    b = _frame(pair, _params(seed=2), skipped=1)
    assert not np.array_equal(a, b)
