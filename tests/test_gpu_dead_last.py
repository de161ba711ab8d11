"""The dead-last rule on the device (rt_wavefront.hip.h kPolDeadLast, the permission of rt_deadlast.h): a context with the rule on against one with RT_DEAD_LAST=0, word
for word, colour and .w; the counter that says the rule skipped rays at all (rt_dead_last_count, from the counting form, which traces every ray and counts the ones the
rule would skip); the scenes whose permission must be refused or whose paths give the rule nothing; the oracle's frames, since on-against-off cannot see an error both
share; and a sequence of edits with a frame after each, since the permission is decided from the scene at every call.  -m gpu.

Frames of 64 x 48 and 96 x 64 (several workgroups of wf_advance, two sub-frames).  The arithmetic behind the permission is tests/test_dead_last_guard.py."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import raytracinggpu_amd as rt

pytestmark = pytest.mark.gpu

SIZES = [(64, 48), (96, 64)]


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
    """rule on / off; rt_count_work through the production kernels' counting forms (any-hit on, as in a frame) in both"""
    on, off = _context(RT_TRAVQ_QW_COUNT="1"), _context(RT_TRAVQ_QW_COUNT="1", RT_DEAD_LAST="0")
    yield on, off
    on.close()
    off.close()


def _bits_equal(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _cat(cat_golden, slot, albedo=rt.scenes.CAT_ALBEDO):
    return dict(vertices=cat_golden["vertices"], indices=cat_golden["tri_bvh_order"], bvh_arr10=cat_golden["bvh_arr10"], albedo=albedo, object_slot=slot)


def _params(W, H, spp, b, **kw):
    d = dict(rt.scenes.CPU_LAUNCHER)
    d.update(kw)
    return rt.make_params(W, H, spp, b, **d)


def _upload(pair, cat_golden, spheres=None, light=(rt.scenes.LIGHT[0], rt.scenes.LIGHT[1]), albedo=rt.scenes.CAT_ALBEDO):
    spheres = rt.scenes.spheres("cpu") if spheres is None else spheres
    for c in pair:
        c.scene_upload(spheres, _cat(cat_golden, len(spheres), albedo), light=light)


def _skipped(c, p):
    return c.count_work(p, detail=True)["dead_last"]


def _same(pair, p):
    on, off = pair
    a = on.render(p)
    _bits_equal(a, off.render(p))
    return a


def _oracle_scene(oracle, oracle_cat, spheres, light):
    s = oracle.Scene()
    for q in spheres:
        s.add_sphere(*q)
    s.add_mesh(oracle_cat)
    s.set_light(*light)
    return s


@pytest.mark.parametrize("W,H", SIZES)
def test_the_cat_scene_on_against_off_and_the_oracle(pair, oracle, oracle_cat, cat_golden, W, H):
    """3 bounces and 2 and 5, one sample and four; the counter is non-zero from three segments on and zero with the knob off; a chain of two segments is left alone"""
    on, off = pair
    _upload(pair, cat_golden)
    osc = oracle.Scene.preset("cpu", oracle_cat)
    for spp, b in ((1, 3), (1, 2), (1, 5), (4, 3)):
        p = _params(W, H, spp, b)
        got = _same(pair, p)
        if (W, H) == SIZES[0] or (spp, b) == (1, 3):
            exp, _, _ = osc.render(W, H, spp, b, want_rgb8=False)
            _bits_equal(got, exp)
        n = _skipped(on, p)
        print(f"{W}x{H} spp={spp} b={b}: {n} last continuation rays skipped")
        assert n > 0
        assert _skipped(off, p) == 0
    assert _skipped(on, _params(W, H, 1, 1)) == 0                      # two segments
    assert _skipped(on, _params(W, H, 1, 0)) == 0


def test_a_batch_of_two_frames_and_a_row_share(pair, cat_golden):
    import torch
    W, H = SIZES[0]
    _upload(pair, cat_golden)
    out = []
    for c in pair:
        bufs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
        c.render_device_batch(_params(W, H, 1, 3), rt._capi.Rows(0, H, H, 1), [(bf.data_ptr(), (0.0, 0.0, 55.0 - 3 * k), None, 40 + k) for k, bf in enumerate(bufs)])
        share = torch.zeros((16, W, 4), dtype=torch.float32, device="cuda")
        c.render_device(_params(W, H, 1, 3), rt._capi.Rows(8, 16, 8, 2), share.data_ptr())      # every other tile of 8 rows from row 8: image rows 8..15 and 24..31
        c.synchronize()
        out.append([bf.cpu().numpy() for bf in bufs] + [share.cpu().numpy(), c.render(_params(W, H, 1, 3), 13, 37)])
    for g, w in zip(*out):
        _bits_equal(g, w)
    assert not np.array_equal(out[0][0], out[0][1])
    whole = pair[0].render(_params(W, H, 1, 3))
    _bits_equal(out[0][2], np.concatenate([whole[8:16], whole[24:32]]))
    _bits_equal(out[0][3], whole[13:37])


@pytest.mark.parametrize("b", [3, 2, 5])
def test_a_still_view_across_three_frames(pair, oracle, oracle_cat, cat_golden, b):
    """the third frame of a still view resumes from the first-shade records: the resumed chain's plain launches carry the rule too"""
    on, off = pair
    W, H = SIZES[1]
    _upload(pair, cat_golden)
    p = _params(W, H, 1, b)
    exp, _, _ = oracle.Scene.preset("cpu", oracle_cat).render(W, H, 1, b, want_rgb8=False)
    before = on.first_shade_cache_counts()["resumed"]
    for _ in range(3):
        _bits_equal(_same(pair, p), exp)
    assert on.first_shade_cache_counts()["resumed"] > before                  # a chain did resume


def _refusals(cat_golden):
    lo, hi = np.asarray(cat_golden["vertices"], np.float32).min(0), np.asarray(cat_golden["vertices"], np.float32).max(0)
    walls = rt.scenes.spheres("cpu")
    grey = [(c, r, (0.5, 0.75, 0.25)) for c, r, _ in walls]
    hot = [walls[0][:2] + ((0.0, 1.5, 0.0),)] + walls[1:]
    light = (rt.scenes.LIGHT[0], rt.scenes.LIGHT[1])
    return {"demo10": (rt.scenes.spheres("demo10"), light, rt.scenes.CAT_ALBEDO),                       # mirror and glass spheres
            "no_zero_albedo": (grey, light, rt.scenes.CAT_ALBEDO),                                      # permitted, but no path dies
            "light_in_the_root_box": (walls, (tuple(float(x) for x in (lo + hi) / 2), 3e10), rt.scenes.CAT_ALBEDO),
            "wall_albedo_above_one": (hot, light, rt.scenes.CAT_ALBEDO)}


@pytest.mark.parametrize("name", ["demo10", "no_zero_albedo", "light_in_the_root_box", "wall_albedo_above_one"])
def test_scenes_that_give_the_rule_nothing(pair, oracle, oracle_cat, cat_golden, name):
    on, _ = pair
    W, H = SIZES[0]
    spheres, light, albedo = _refusals(cat_golden)[name]
    _upload(pair, cat_golden, spheres, light, albedo)
    osc = _oracle_scene(oracle, oracle_cat, spheres, light)
    for spp, b in ((1, 3), (4, 5)):
        p = _params(W, H, spp, b)
        assert _skipped(on, p) == 0
        exp, _, _ = osc.render(W, H, spp, b, want_rgb8=False)
        _bits_equal(_same(pair, p), exp)


def test_a_wall_removed(pair, oracle, oracle_cat, cat_golden):
    """without the back wall some last continuation rays of dead paths miss every sphere: those are traced (they may still hit the cat), the others are skipped"""
    on, _ = pair
    W, H = SIZES[0]
    spheres = rt.scenes.spheres("cpu")[1:]
    light = (rt.scenes.LIGHT[0], rt.scenes.LIGHT[1])
    _upload(pair, cat_golden, spheres, light)
    osc = _oracle_scene(oracle, oracle_cat, spheres, light)
    for spp, b in ((1, 3), (4, 5)):
        p = _params(W, H, spp, b)
        exp, _, _ = osc.render(W, H, spp, b, want_rgb8=False)
        _bits_equal(_same(pair, p), exp)
        assert _skipped(on, p) > 0


def test_the_permission_follows_the_scene(pair, oracle, oracle_cat, cat_golden):
    """edits between frames, a frame and a count after each: light into the root box and back, a wall to mirror and back, the mesh moved onto the light and back"""
    on, _ = pair
    W, H = SIZES[0]
    p = _params(W, H, 1, 3)
    _upload(pair, cat_golden)
    lo, hi = np.asarray(cat_golden["vertices"], np.float32).min(0), np.asarray(cat_golden["vertices"], np.float32).max(0)
    mid = tuple(float(x) for x in (lo + hi) / 2)
    L, inten = rt.scenes.LIGHT
    wall = on.sphere(3)
    eye, zero = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    shift = (np.asarray(L, np.float32) - np.asarray(mid, np.float32)).astype(np.float32)
    first = _same(pair, p)
    n0 = _skipped(on, p)
    assert n0 > 0
    steps = [(lambda c: c.set_light(mid, inten), False), (lambda c: c.set_light(L, inten), True),
             (lambda c: c.set_sphere(3, wall[:3] + (1,) + wall[4:]), False), (lambda c: c.set_sphere(3, wall), True),
             (lambda c: c.mesh_transform(eye, shift), False), (lambda c: c.mesh_transform(eye, -shift), None),
             (lambda c: c.mesh_transform(eye, zero), None)]
    for k, (edit, fires) in enumerate(steps):
        for c in pair:
            edit(c)
        frame = _same(pair, p)
        n = _skipped(on, p)
        print("edit", k, "skipped", n)
        if fires is not None:
            assert (n > 0) == fires, (k, n)
        if k in (1, 3):                                               # the scene is the first one again
            _bits_equal(frame, first)
            assert n == n0
    # the light edit against the oracle (the mesh as uploaded again): the frame with the light inside the box is the reference's
    _upload(pair, cat_golden)
    for c in pair:
        c.set_light(mid, inten)
    s = _oracle_scene(oracle, oracle_cat, rt.scenes.spheres("cpu"), (mid, inten))
    exp, _, _ = s.render(W, H, 1, 3, want_rgb8=False)
    _bits_equal(_same(pair, p), exp)


def _vertex_normals(v, t, zero_from=None):
    """area-weighted vertex normals of the cat; zero_from: the vertices from that index on get (0, 0, 0) -- what faces that cancel leave, and a triangle of three such
    corners shades with N = normalize(0) = NaN"""
    v, t = np.asarray(v, np.float64), np.asarray(t)[:, :3]
    fn = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    vn = np.zeros_like(v)
    for k in range(3):
        np.add.at(vn, t[:, k], fn)
    vn /= np.maximum(np.linalg.norm(vn, axis=1), 1e-30)[:, None]
    if zero_from is not None:
        vn[zero_from:] = 0.0
    return vn.astype(np.float32)


@pytest.mark.parametrize("zero_from", [None, 0, 1200])
def test_a_smooth_mesh_refuses(pair, oracle, cat_golden, zero_from):
    """nobody validates vertex normals, and a hit on a triangle whose corner normals are zero is NaN in the reference: with a smooth mesh in the scene the permission is
    refused (the counter stays 0), the frames are the knob-off context's word for word and the oracle's, NaN where it has NaN; flat again, the rule is back"""
    on, _ = pair
    W, H = SIZES[0]
    _upload(pair, cat_golden)
    p = _params(W, H, 1, 3)
    assert _skipped(on, p) > 0
    tb = np.asarray(cat_golden["tri_bvh_order"])[:, :3]
    vn = _vertex_normals(cat_golden["vertices"], tb, zero_from)
    for c in pair:
        c.mesh_set_normals(vn, tb)
    om = oracle.Mesh.from_arrays(cat_golden["vertices"], cat_golden["tri_obj_order"]).build_bvh()      # (its own mesh: the session's stays flat)
    om.set_normals(vn, om.triangles)
    osc = oracle.Scene.preset("cpu", om)
    nans = 0
    for spp, b in ((1, 3), (4, 5)):
        q = _params(W, H, spp, b)
        assert _skipped(on, q) == 0
        got = _same(pair, q)
        exp, _, _ = osc.render(W, H, spp, b, want_rgb8=False)
        np.testing.assert_array_equal(got, exp)                      # (NaN equals NaN here; the payload of a NaN is the processor's)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(exp))
        nans += int(np.isnan(exp).sum())
    print("zero normals from vertex", zero_from, ": NaN words in the oracle's frames:", nans)
    assert (nans > 0) == (zero_from is not None)
    for c in pair:
        c.mesh_set_normals(None, None)
    assert _skipped(on, p) > 0
