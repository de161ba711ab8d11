"""Row windows of the traversal queue on the device (rt_qrows.h, wf_travq's fetch, enqueue_chain): a default context against one with RT_TRAVQ_ROWS=0, word for word,
colour and .w -- and the step counters that say the windowed launches fetched less and traversed the same.  -m gpu.

The first traversal launch of a chain enumerates the rows that hold continuation rays only, the last the rows that hold shadow rays only; with num_bounce 0 the two are
adjacent.  Sizes: one tile, several workgroups, ragged tiles with a mixed row, 256 x 256 (two oversubscribed sub-frames), and a rank's interleaved share of the rows.
The index arithmetic itself is tests/test_queue_rows.py."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import raytracinggpu_amd as rt

from . import material_scenes as ms

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (64, 48), (71, 29), (256, 256)]
DEPTHS = [0, 1, 3]
OFF = dict(RT_TRAVQ_ROWS="0")


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
    on, off = _context(), _context(**OFF)
    yield on, off
    on.close()
    off.close()


@pytest.fixture(scope="module")
def counting_pairs():
    """rt_count_work through both counting instantiations: the binary32 pairs (the reference's work) and the production kernel's own.  The second with any-hit off: a
    shadow ray that may stop at its first certain hit does as many box tests as its wave's schedule lets it before that hit (the headline frame counts 182 883 129,
    182 883 293 and 182 891 265 box tests in three runs, two of them of one build) -- traced to the end, every ray's tests are a set and the sums are exact"""
    cs = [(_context(**kw), _context(**kw, **OFF)) for kw in (dict(), dict(RT_TRAVQ_QW_COUNT="1", RT_TRAVQ_ANYHIT="0"))]
    yield cs
    for on, off in cs:
        on.close()
        off.close()


def _bits_equal(a, b, msg=""):
    np.testing.assert_array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32), err_msg=msg)


def _cat(cat_golden, slot, albedo=rt.scenes.CAT_ALBEDO):
    return dict(vertices=cat_golden["vertices"], indices=cat_golden["tri_bvh_order"], bvh_arr10=cat_golden["bvh_arr10"], albedo=albedo, object_slot=slot)


def _params(w, h, b, spp=1, **kw):
    d = dict(rt.scenes.CPU_LAUNCHER)
    d.update(kw)
    return rt.make_params(w, h, spp, b, **d)


def _same_frames(pair, sizes=SIZES, depths=DEPTHS, spp=1, **kw):
    on, off = pair
    for w, h in sizes:
        for b in depths:
            p = _params(w, h, b, spp, **kw)
            _bits_equal(on.render(p), off.render(p), f"{w}x{h} b={b} spp={spp}")


def test_the_cat_at_every_size_and_depth(pair, cat_golden):
    for c in pair:
        c.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden, 6))
    _same_frames(pair)


def test_the_cat_against_the_oracle(pair, oracle, oracle_cat, cat_golden):
    """so that the two contexts do not merely agree with each other"""
    on, _ = pair
    on.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden, 6))
    osc = oracle.Scene.preset("cpu", oracle_cat)
    for (w, h), b in (((71, 29), 0), ((64, 48), 3)):
        exp, _, _ = osc.render(w, h, 1, b, want_rgb8=False)
        _bits_equal(on.render(_params(w, h, b)), exp)


def test_a_rank_share_of_the_rows(pair, cat_golden):
    """rank 1 of 3, tiles of 8 rows"""
    import torch
    w, h = 71, 61
    rows, idx = rt.interleaved_rows(h, 8, 1, 3)
    for b in DEPTHS:
        out = []
        for c in pair:
            c.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden, 6))
            buf = torch.zeros((len(idx), w, 4), dtype=torch.float32, device="cuda")
            c.render_device(_params(w, h, b), rows, buf.data_ptr())
            c.synchronize()
            out.append(buf.cpu().numpy())
        _bits_equal(*out)
        assert out[0][..., 3].sum() > 0


def test_spheres_only(pair):
    """no mesh: no traversal launch at all"""
    for c in pair:
        c.scene_upload(rt.scenes.spheres("demo10"))
    _same_frames(pair, sizes=[(64, 48), (71, 29)], variant="wavefront_queue")


def test_mirror_and_glass_with_the_cat(pair, cat_golden):
    """paths of unequal length: continuation rays at every depth, shadow rays only behind a diffuse hit"""
    for c in pair:
        c.scene_upload(rt.scenes.spheres("demo10"), _cat(cat_golden, rt.scenes.mesh_slot("demo10")))
    _same_frames(pair, sizes=[(64, 48), (71, 29)], depths=[0, 1, 3, 5])


def test_two_meshes(pair, cat_golden):
    spheres, meshes = ms.capi_scene("two_cats", cat_golden["vertices"], cat_golden["tri_obj_order"])
    for c in pair:
        c.scene_upload(spheres, meshes)
    _same_frames(pair, sizes=[(64, 48), (71, 29)])


def test_a_textured_cat(pair, cat_golden):
    rng = np.random.default_rng(3)
    v, tv = np.asarray(cat_golden["vertices"], np.float32), np.asarray(cat_golden["tri_bvh_order"])[:, :3]
    lo, hi = v.min(0), v.max(0)
    uv = ((v[:, :2] - lo[:2]) / (hi[:2] - lo[:2])).astype(np.float32)
    px = rng.integers(0, 256, size=(23, 37, 3), dtype=np.uint8)
    for c in pair:
        c.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden, 6, albedo=(1.0, 1.0, 1.0)))
        c.mesh_set_texture(uv, tv, px, filter="bilinear", wrap="repeat")
    _same_frames(pair, sizes=[(64, 48), (71, 29)])


def test_four_samples_per_pixel(pair, cat_golden):
    """sample chunks and path_reduce"""
    for c in pair:
        c.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden, 6))
    _same_frames(pair, sizes=[(64, 48), (71, 29)], spp=4)
    _same_frames(pair, sizes=[(64, 48)], depths=[3], spp=4, sigma=0.2)


def _batch(c, p, w, h, n, scenes=None):
    import torch
    rows = rt._capi.Rows(0, h, h, 1)
    bufs = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(n)]
    c.render_device_batch(p, rows, [(bf.data_ptr(), (0.0, 0.0, 55.0 - 3 * k), None, 40 + k) for k, bf in enumerate(bufs)], scenes=scenes)
    c.synchronize()
    return [bf.cpu().numpy() for bf in bufs]


def test_a_batch_of_four_frames(pair, cat_golden):
    for w, h in ((64, 48), (71, 29)):
        for b in DEPTHS:
            out = []
            for c in pair:
                c.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden, 6))
                out.append(_batch(c, _params(w, h, b), w, h, 4))
            for g, e in zip(*out):
                _bits_equal(g, e)
            assert not np.array_equal(out[0][0], out[0][1])


def test_an_animated_batch_of_two_frames(pair, cat_golden):
    base = rt.scenes.spheres("demo10")
    scenes = [(((-10.0 + 6 * k, 20.0, 40.0), 3e10), [((c[0] + 2.0 * k, c[1], c[2]), r) for c, r, *_ in base]) for k in range(2)]
    for w, h in ((64, 48), (71, 29)):
        for b in DEPTHS:
            out = []
            for c in pair:
                c.scene_upload(base, _cat(cat_golden, rt.scenes.mesh_slot("demo10")))
                out.append(_batch(c, _params(w, h, b), w, h, 2, scenes=scenes))
            for g, e in zip(*out):
                _bits_equal(g, e)
            assert not np.array_equal(out[0][0], out[0][1])


@pytest.mark.parametrize("size", [(64, 48), (256, 256)])
def test_the_windows_fetch_less_and_traverse_the_same(counting_pairs, cat_golden, size):
    """rt_count_work returns only if the kernels' index invariants held (the word fr.work[4] is 0: RT_ERR_INTERNAL otherwise)"""
    w, h = size
    for on, off in counting_pairs:
        for c in (on, off):
            c.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden, 6))
        for b in DEPTHS:
            p = _params(w, h, b)
            a, z = on.count_work(p, detail=True), off.count_work(p, detail=True)
            for k in ("rays", "box_tests", "nodes", "tri_tests"):
                assert a[k] == z[k] > 0, (k, b)
            assert a["dead_channels"] == z["dead_channels"]
            for k in ("tri_steps", "box_steps"):
                assert a["steps"][k] > 0
            assert a["steps"]["fetches"] < z["steps"]["fetches"], b

