"""The first-shadow cache on the device (rt_ctx::FirstShadow, enqueue_chain, the two wf_advance launches that emit and close segment 0's shadow rays): a default context
against one created under RT_FIRST_SHADOW_CACHE=0, word for word, colour and .w -- and rt_first_shadow_cache_counts, which says whether a chain read the cache, filled it
or was not eligible, so that every comparison below is known to have gone through the path it names.  -m gpu.

The cat at 64 x 48 with num_bounce 2 (two sub-frames of three 8-row tiles: two launch chains per frame and sample chunk), the shapes of test_gpu_first_hit_cache.py.  The
reference of every comparison is the knob-off context, never the cached one.  The scenes of tests/material_scenes.py hold no mirror or glass SPHERE: the three used here
show the camera a mirror mesh, a glass mesh and two meshes (one of them a mirror) -- first hits without a shadow ray next to first hits with one."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import raytracinggpu_amd as rt

from . import material_scenes as ms

pytestmark = pytest.mark.gpu

W, H, B = 64, 48, 2
OFF = dict(RT_FIRST_SHADOW_CACHE="0")
ZERO = dict(skipped=0, filled=0, ineligible=0, key_misses=0)


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


def _pair(on_kw=None, **both):
    on, off = _context(**both, **(on_kw or {})), _context(**both, **OFF)
    try:
        yield on, off
    finally:
        on.close()
        off.close()


@pytest.fixture(scope="module")
def pair():
    yield from _pair()


@pytest.fixture(scope="module")
def pair_one_sample_per_chain():
    """RT_PATH_SAMP_MB=1: a chain's state may take 1 MB; a sample of 64 x 48 with 13 segments takes 0.73: one sample per chain"""
    yield from _pair(RT_PATH_SAMP_MB="1")


def _bits_equal(a, b, msg=""):
    np.testing.assert_array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32), err_msg=msg)


def _cat(cat_golden, slot=6, albedo=rt.scenes.CAT_ALBEDO):
    return dict(vertices=np.asarray(cat_golden["vertices"], np.float32), indices=cat_golden["tri_bvh_order"], bvh_arr10=cat_golden["bvh_arr10"], albedo=albedo,
                object_slot=slot)


def _params(w=W, h=H, b=B, spp=1, **kw):
    d = dict(rt.scenes.CPU_LAUNCHER)
    d.update(kw)
    return rt.make_params(w, h, spp, b, **d)


def _upload(pair, cat_golden, albedo=rt.scenes.CAT_ALBEDO, **kw):
    for c in pair:
        c.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden, albedo=albedo), **kw)


def _delta(ctx, fn, counts="first_shadow_cache_counts"):
    """(what fn returns, how far each counter of ctx moved meanwhile)"""
    before = getattr(ctx, counts)()
    r = fn()
    after = getattr(ctx, counts)()
    return r, {k: after[k] - before[k] for k in after}


def _expect(d, **kw):
    want = dict(ZERO)
    want.update(kw)
    assert d == want, (d, want)


def _frame(pair, p, render=None, cold=False, **expect):
    """one frame on both contexts: equal word for word, the cached context's counters moved by `expect` (in chains per sub-frame), the reference context's chains all
    ineligible.  cold: the first frame after an upload -- a key miss if an earlier test left the context's cache filled, none on a new context: not compared"""
    on, off = pair
    render = render or (lambda c: c.render(p))
    got, d = _delta(on, lambda: render(on))
    exp, e = _delta(off, lambda: render(off))
    _bits_equal(got, exp)
    n = on.stats()["parts"]
    assert n == 2
    if cold:
        d["key_misses"] = 0
    _expect(d, **{k: v * n if k != "key_misses" else v for k, v in expect.items()})
    assert e["skipped"] == e["filled"] == e["key_misses"] == 0 and e["ineligible"] > 0
    assert got[..., 3].sum() > 0
    return got


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


def _chunk(spp, samp_bytes, b, w=W, h=H, parts=2):
    """cut_wavefront's samples per chain"""
    px_all = ((w + 7) // 8) * ((h + 7) // 8 + parts) * 64
    per_item = 16 + 16 + 64 + 16 + 5 * (b + 1)
    cmax = max(1, min(spp, samp_bytes // (px_all * per_item), ((1 << 29) - 1) // (px_all // parts + 64)))
    chains = (spp + cmax - 1) // cmax
    return (spp + chains - 1) // chains


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


def _render_rows(c, p, rows, n_rows):
    import torch
    buf = torch.zeros((n_rows, p.width, 4), dtype=torch.float32, device="cuda")
    c.render_device(p, rows, buf.data_ptr())
    c.synchronize()
    return buf.cpu().numpy()


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
    import torch
    _upload(pair, cat_golden)
    on, off = pair
    rows = rt._capi.Rows(0, H, H, 1)
    bufs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    seeds = [11, 12, 13, 14, 15, 16]
    exp = [off.render(_params(seed=s)) for s in seeds]
    on.set_pipelining(True)
    try:
        got = []

        def six():
            for k, s in enumerate(seeds):
                on.render_device(_params(seed=s), rows, bufs[k % 2].data_ptr())
                if k % 2 == 1:                         # both buffers hold a frame: read them before the next two overwrite them
                    on.synchronize()
                    got.extend(b.cpu().numpy() for b in bufs)
        _, d = _delta(on, six)
    finally:
        on.set_pipelining(False)
    n = on.stats()["parts"]
    assert d["filled"] == n and d["skipped"] == 5 * n and d["ineligible"] == 0, d
    for g, e in zip(got, exp):
        _bits_equal(g, e)


def test_batches_stats_and_count_lists_go_round_the_cache(pair, cat_golden):
    import torch
    _upload(pair, cat_golden)
    on, off = pair
    p = _params()
    rows = rt._capi.Rows(0, H, H, 1)
    base = _frame(pair, p, cold=True, filled=1)

    def batch(c):
        bufs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
        c.render_device_batch(p, rows, [(bf.data_ptr(), (0.5 * k, 0.0, 55.0 - 3 * k), None, 40 + k) for k, bf in enumerate(bufs)])
        c.synchronize()
        return np.stack([bf.cpu().numpy() for bf in bufs])
    got, d = _delta(on, lambda: batch(on))
    _bits_equal(got, batch(off))
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
