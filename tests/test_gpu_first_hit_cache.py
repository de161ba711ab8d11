"""The first-hit cache on the device (the hit level of csrc/rt_still.h, enqueue_chain, wf_advance's close of segment 0): a default context against one created under
RT_FIRST_HIT_CACHE=0, word for word, colour and .w -- and rt_first_hit_cache_counts, which says whether a chain skipped its first traversal launch, filled the cache or
was not eligible, so that every comparison below is known to have gone through the path it names.  -m gpu.  The helpers
all three files of this kind share are tests/still_view.py; the state machine alone is replayed without a device in tests/test_still_view_model.py.

The cat at 64 x 48 (two sub-frames of three 8-row tiles: two launch chains per frame and sample chunk).  The reference of every comparison is the second context, never
the cached one.  The library has no entry that edits vertices in place or refits on its own (a refit happens inside rt_mesh_transform); those two cases of the mesh-edit
list do not exist here."""
from functools import partial

import numpy as np
import pytest

import raytracinggpu_amd as rt

from . import material_scenes as ms
from . import still_view as sv
from .still_view import B, H

pytestmark = pytest.mark.gpu

LEVEL = sv.HIT
_bits_equal, _cat, _params, _upload, _chunk, _render_rows = sv.bits_equal, sv.cat, sv.params, sv.upload, sv.chunk, sv.render_rows
_pair, _delta, _frame = partial(sv.pair, LEVEL), partial(sv.delta, LEVEL), partial(sv.frame, LEVEL)


@pytest.fixture(scope="module")
def pair():
    yield from _pair()


@pytest.fixture(scope="module")
def pair_one_sample_per_chain():
    """RT_PATH_SAMP_MB=1: a chain's state may take 1 MB; a sample of 64 x 48 with 13 segments takes 0.73: one sample per chain"""
    yield from _pair(RT_PATH_SAMP_MB="1")


def test_the_same_frame_three_times(pair, cat_golden):
    _upload(pair, cat_golden)
    p = _params()
    a = _frame(pair, p, cold=True, filled=1)
    b = _frame(pair, p, skipped=1)
    c = _frame(pair, p, skipped=1)
    _bits_equal(a, b)
    _bits_equal(a, c)
    assert pair[1].first_hit_cache_counts()["skipped"] == 0


def test_a_new_seed_with_the_camera_still(pair, cat_golden):
    _upload(pair, cat_golden)
    a = _frame(pair, _params(seed=1), cold=True, filled=1)
    b = _frame(pair, _params(seed=2), skipped=1)
    assert not np.array_equal(a, b)                   # the bounce rays do read the seed
    _frame(pair, _params(b=0, seed=3), skipped=1)     # neither depth nor eps is in the key: the camera rays are the same
    _frame(pair, _params(b=4, seed=3, eps=2e-3), skipped=1)


def test_a_jittered_camera_always_traces(pair, cat_golden):
    _upload(pair, cat_golden)
    _frame(pair, _params(), cold=True, filled=1)
    _frame(pair, _params(sigma=0.2), ineligible=1)
    _frame(pair, _params(sigma=0.2, depth_convention=1, b=3), ineligible=1)
    _frame(pair, _params(), skipped=1)                # what a jittered frame traced went nowhere near the cache


def test_tri_tmin_is_in_the_key(pair, cat_golden):
    _upload(pair, cat_golden)
    _frame(pair, _params(), cold=True, filled=1)
    _frame(pair, _params(tri_tmin=30.0), filled=1, key_misses=1)   # beyond the nearest triangles of many pixels: other hits
    _frame(pair, _params(), filled=1, key_misses=1)


def test_a_moved_camera_is_a_miss(pair, cat_golden):
    _upload(pair, cat_golden)
    p = _params()
    x = np.float32(0.5)
    x1 = np.nextafter(x, np.float32(1.0))
    pose = lambda px, yaw=0.1: rt.make_pose(position=(float(px), 0.0, 55.0), yaw=yaw, pitch=0.05)
    posed = lambda ps: (lambda c: c.render_pose(p, ps))
    _frame(pair, p, posed(pose(x)), cold=True, filled=1)
    _frame(pair, p, posed(pose(x)), skipped=1)
    _frame(pair, p, posed(pose(x1)), filled=1, key_misses=1)        # one ulp in x
    _frame(pair, p, posed(pose(x)), filled=1, key_misses=1)         # and back: no stale hit
    _frame(pair, p, posed(pose(x, yaw=float(np.nextafter(np.float32(0.1), np.float32(1.0))))), filled=1, key_misses=1)   # a basis component
    _frame(pair, p, filled=1, key_misses=1)                          # the uploaded camera: cam_mode 0
    _frame(pair, p, skipped=1)
    # the uploaded camera moved by one ulp: an upload, which is a miss for two reasons
    _upload(pair, cat_golden, camera=((0.25, 0.0, 55.0), None))
    _frame(pair, p, filled=1, key_misses=1)
    _upload(pair, cat_golden, camera=((float(np.nextafter(np.float32(0.25), np.float32(1.0))), 0.0, 55.0), None))
    _frame(pair, p, filled=1, key_misses=1)
    _upload(pair, cat_golden, camera=((0.0, 0.0, 55.0), float(np.float32(np.pi / 3) * np.float32(1.01))))   # the field of view: z
    _frame(pair, p, filled=1, key_misses=1)


ROT = [0.96, 0.0, 0.28, 0.0, 1.0, 0.0, -0.28, 0.0, 0.96]


@pytest.mark.parametrize("edit", ["transform", "rebuild_reference", "rebuild_lbvh", "upload_another_mesh"])
def test_a_mesh_edit_is_a_miss(pair, cat_golden, edit):
    _upload(pair, cat_golden)
    p = _params()
    before = _frame(pair, p, cold=True, filled=1)
    _frame(pair, p, skipped=1)
    nt = len(cat_golden["tri_bvh_order"])
    for c in pair:
        if edit == "transform":
            c.mesh_transform(ROT, (1.5, -2.0, 0.5))
        elif edit == "upload_another_mesh":
            c.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden, scale=0.5))
        else:
            c.mesh_rebuild(nt, mode=edit.split("_")[1])
    after = _frame(pair, p, filled=1, key_misses=1)
    _frame(pair, p, skipped=1)
    if edit in ("transform", "upload_another_mesh"):
        assert not np.array_equal(before, after)


@pytest.mark.parametrize("edit", ["transform_of", "rebuild_of_reference", "rebuild_of_lbvh"])
def test_an_edit_of_one_mesh_of_two_is_a_miss(pair, cat_golden, edit):
    spheres, meshes = ms.capi_scene("two_cats", cat_golden["vertices"], cat_golden["tri_obj_order"])
    for c in pair:
        c.scene_upload(spheres, meshes)
    slot, nt = meshes[1]["object_slot"], len(cat_golden["tri_obj_order"])
    p = _params()
    before = _frame(pair, p, cold=True, filled=1)
    _frame(pair, p, skipped=1)
    for c in pair:
        if edit == "transform_of":
            c.mesh_transform(ROT, (1.5, -2.0, 0.5), object_slot=slot)
        else:
            c.mesh_rebuild(nt, mode=edit.split("_")[2], object_slot=slot)
    after = _frame(pair, p, filled=1, key_misses=1)
    _frame(pair, p, skipped=1)
    if edit == "transform_of":
        assert not np.array_equal(before, after)


def test_light_sphere_and_material_edits_keep_the_cache(pair, cat_golden):
    _upload(pair, cat_golden)
    p = _params()
    frames = [_frame(pair, p, cold=True, filled=1)]
    on = pair[0]
    sphere_slot = 0
    s = on.sphere(sphere_slot)
    edits = [lambda c: c.set_light((5.0, 25.0, 35.0), 2e10),
             lambda c: c.move_light(1.0),
             lambda c: c.move_sphere(sphere_slot, (3.0, 1.0, -2.0)),
             lambda c: c.set_sphere(sphere_slot, (s[0], s[1] * 1.5, (0.9, 0.1, 0.2), 0, 1.0, 1.0)),   # geometry and material
             lambda c: c.set_sphere(sphere_slot, (s[0], s[1], s[2], 1, 1.0, 1.0))]                     # a mirror
    for e in edits:
        for c in pair:
            e(c)
        frames.append(_frame(pair, p, skipped=1))
        assert not np.array_equal(frames[-1], frames[-2])


def test_a_texture_change_keeps_the_cache(pair, cat_golden):
    rng = np.random.default_rng(3)
    v, tv = np.asarray(cat_golden["vertices"], np.float32), np.asarray(cat_golden["tri_bvh_order"])[:, :3]
    lo, hi = v.min(0), v.max(0)
    uv = ((v[:, :2] - lo[:2]) / (hi[:2] - lo[:2])).astype(np.float32)
    px0 = rng.integers(0, 256, size=(23, 37, 3), dtype=np.uint8)
    for c in pair:
        c.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden, albedo=(1.0, 1.0, 1.0)))
        c.mesh_set_texture(uv, tv, px0, filter="bilinear", wrap="repeat")
    p = _params()
    a = _frame(pair, p, cold=True, filled=1)
    px = rng.integers(0, 256, size=(11, 5, 3), dtype=np.uint8)
    for c in pair:
        c.mesh_set_texture(uv, tv, px, filter="nearest", wrap="clamp")
    b = _frame(pair, p, skipped=1)
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
    _frame(cs, p, cold=True, filled=1, skipped=chains - 1)
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


def test_a_batch_with_a_camera_per_frame_is_ineligible(pair, cat_golden):
    _upload(pair, cat_golden)
    p = _params()
    got, d = _delta(pair[0], lambda: sv.batch_of_three(pair[0], p))
    _bits_equal(got, sv.batch_of_three(pair[1], p))
    assert d["ineligible"] > 0 and d["skipped"] == d["filled"] == 0, d
    assert not np.array_equal(got[0], got[1])


def test_a_frame_under_stats_is_traced_in_full(pair, cat_golden):
    _upload(pair, cat_golden)
    on = pair[0]
    p = _params()
    _frame(pair, p, cold=True, filled=1)
    on.stats_enable(True)
    try:
        _frame(pair, p, ineligible=1)
        st = on.stats()                                # raises if an event was never recorded
        assert st["trav_launches"] == (B + 1) + 1
        assert st["trav_ms"] > 0
    finally:
        on.stats_enable(False)
    _frame(pair, p, skipped=1)
