"""rt_render_counts[_device] on the device: a frame whose pixel (x, y) gets counts[y, x] samples, traced as a compacted list (rt_adaptive.hip.h: the plan, the LIST
form of wf_advance, the fold).  -m gpu.

The contract is bit for bit: every pixel of the result, .w included, is the pixel of the frame rt_render_device / rt_render_pose_device writes with num_rays = its
count -- code this feature does not touch, itself pinned to the oracle.  Those frames, at num_rays = 1 .. 4 from the same context, are the reference of every
comparison below (one test also goes to the oracle directly).  The cat at 64 x 48, b = 2, unless a test says otherwise."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import raytracinggpu_amd as rt

from . import material_scenes as ms

pytestmark = pytest.mark.gpu

W, H, B = 64, 48, 2


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
def ctx():
    c = rt.Context(0)
    yield c
    c.close()


def _cat(cat_golden, **kw):
    d = dict(vertices=cat_golden["vertices"], indices=cat_golden["tri_bvh_order"], bvh_arr10=cat_golden["bvh_arr10"], albedo=rt.scenes.CAT_ALBEDO, object_slot=6)
    d.update(kw)
    return d


def _params(w=W, h=H, b=B, spp=1, **kw):
    d = dict(rt.scenes.CPU_LAUNCHER)
    d.update(kw)
    return rt.make_params(w, h, spp, b, **d)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _frames(ctx, n_max=4, pose=None, **kw):
    """the reference: {c: the frame with num_rays = c} for c = 1 .. n_max"""
    if pose is None:
        return {c: ctx.render(_params(spp=c, **kw)) for c in range(1, n_max + 1)}
    return {c: ctx.render_pose(_params(spp=c, **kw), pose) for c in range(1, n_max + 1)}


def _expected(frames, counts, limit=rt.MAX_SAMPLE_COUNT):
    exp = np.zeros(counts.shape + (4,), np.float32)
    for c in np.unique(counts):
        if c > 0:
            m = counts == c
            exp[m] = frames[min(int(c), limit)][m]
    return exp


def _check(ctx, frames, counts, pose=None, with_base=True, msg="", **kw):
    """render_counts equals the frames pixel by pixel: without base, with base into another array, with base in place"""
    p = _params(w=counts.shape[1], h=counts.shape[0], spp=99, **kw)   # num_rays is not read
    exp = _expected(frames, counts)
    got = ctx.render_counts(p, counts, pose=pose)
    np.testing.assert_array_equal(_bits(got), _bits(exp), err_msg=msg + " (no base)")
    info = ctx.render_counts_info()
    assert info["items"] == int(np.minimum(counts, 64).sum())
    if with_base:
        exp = np.where((counts <= 1)[..., None], frames[1], exp)      # pixels with c <= 1 are copied from base: c == 0 too
        base = frames[1].copy()
        got = ctx.render_counts(p, counts, pose=pose, base=base)
        np.testing.assert_array_equal(_bits(got), _bits(exp), err_msg=msg + " (base)")
        np.testing.assert_array_equal(_bits(base), _bits(frames[1]))
        assert ctx.render_counts_info()["items"] == int(np.maximum(np.minimum(counts, 64).astype(int) - 1, 0).sum())
        assert ctx.render_counts(p, counts, pose=pose, base=base, out=base) is base
        np.testing.assert_array_equal(_bits(base), _bits(exp), err_msg=msg + " (base, in place)")
    return info


def _random_counts(seed, w=W, h=H, hi=5):
    return np.random.default_rng(seed).integers(0, hi, (h, w)).astype(np.uint8)


@pytest.fixture(scope="module")
def cat_frames(ctx, cat_golden):
    """the cat's frames at num_rays = 1 .. 4, default settings: computed once, left unchanged"""
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    f = _frames(ctx)
    assert not np.array_equal(f[1], f[2]) and f[1][..., 3].sum() > 0
    return f


def _upload_cat(ctx, cat_golden):
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))


def test_all_ones_is_the_one_sample_frame(ctx, cat_golden, cat_frames):
    _upload_cat(ctx, cat_golden)
    got = ctx.render_counts(_params(), np.ones((H, W), np.uint8))
    np.testing.assert_array_equal(_bits(got), _bits(cat_frames[1]))
    assert ctx.render_counts_info() == dict(items=W * H, chains=1, slots=W * H, chain_paths=W * H)


def test_random_counts_with_and_without_base(ctx, cat_golden, cat_frames):
    _upload_cat(ctx, cat_golden)
    for seed in (1, 2):
        counts = _random_counts(seed)
        assert set(np.unique(counts)) == {0, 1, 2, 3, 4}
        _check(ctx, cat_frames, counts, msg=f"seed {seed}")
    got = ctx.render_counts(_params(), _random_counts(1))
    assert (got[_random_counts(1) == 0] == 0).all()                    # c == 0 without base: (0, 0, 0, 0)


def test_the_device_form_in_place_on_a_second_stream(ctx, cat_golden, cat_frames):
    import torch
    _upload_cat(ctx, cat_golden)
    counts = _random_counts(3)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        frame = torch.from_numpy(cat_frames[1]).to("cuda:0", non_blocking=False)
        dc = torch.from_numpy(counts).to("cuda:0")
    st.synchronize()
    ctx.render_counts_device(_params(), dc.data_ptr(), frame.data_ptr(), base_ptr=frame.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    exp = np.where((counts <= 1)[..., None], cat_frames[1], _expected(cat_frames, counts))
    np.testing.assert_array_equal(_bits(frame.cpu().numpy()), _bits(exp))
    np.testing.assert_array_equal(dc.cpu().numpy(), counts)


def test_odd_sizes(ctx, cat_golden):
    _upload_cat(ctx, cat_golden)
    w, h = 61, 45
    frames = _frames(ctx, w=w, h=h)
    _check(ctx, frames, _random_counts(4, w, h), msg="61 x 45")
    _check(ctx, frames, np.full((h, w), 2, np.uint8), msg="61 x 45, two everywhere")


def test_edge_patterns(ctx, cat_golden, cat_frames):
    _upload_cat(ctx, cat_golden)
    last, first = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    last[-1, -1], first[0, 0] = 3, 4
    tiles = np.zeros((H, W), np.uint8)
    tiles.reshape(H // 8, 8, W // 8, 8)[::2, :, 1::3] = _random_counts(5).reshape(H // 8, 8, W // 8, 8)[::2, :, 1::3]   # whole tiles of zeros between the others
    tiles[8:16] = 0
    assert tiles.max() == 4 and (tiles.reshape(H // 8, 8, W // 8, 8).max(axis=(1, 3)) == 0).sum() > 20
    for name, counts in (("only the last pixel", last), ("only pixel 0", first), ("tiles of zeros", tiles)):
        info = _check(ctx, cat_frames, counts, msg=name)
        assert info["chains"] == 1
    zeros = np.zeros((H, W), np.uint8)
    info = _check(ctx, cat_frames, zeros, msg="all zeros")
    assert info["chains"] == 0 and info["items"] == 0                  # no chain; the fold still wrote the frame
    got = ctx.render_counts(_params(), zeros, out=np.full((H, W, 4), 5, np.float32))
    assert (got == 0).all()


def test_counts_above_the_limit_are_read_as_the_limit(ctx, cat_golden):
    _upload_cat(ctx, cat_golden)
    w, h = 16, 8
    f64 = ctx.render(_params(w, h, spp=64))
    f1 = ctx.render(_params(w, h, spp=1))
    counts = np.zeros((h, w), np.uint8)
    counts[3, 5], counts[6, 12] = 64, 200
    got = ctx.render_counts(_params(w, h), counts)
    assert ctx.render_counts_info()["items"] == 128
    m = counts > 0
    np.testing.assert_array_equal(_bits(got[m]), _bits(f64[m]))
    assert (got[~m] == 0).all()
    got = ctx.render_counts(_params(w, h), counts, base=f1)
    assert ctx.render_counts_info()["items"] == 126
    np.testing.assert_array_equal(_bits(got), _bits(np.where(m[..., None], f64, f1)))


@pytest.mark.parametrize("setting", ["sigma", "optimized_depth_no_bounce", "optimized_depth", "pose", "pose_sigma", "eps_tmin_seed"])
def test_render_settings(ctx, cat_golden, setting):
    _upload_cat(ctx, cat_golden)
    kw = dict(sigma=dict(sigma=0.2), optimized_depth_no_bounce=dict(depth_convention=1, b=0), optimized_depth=dict(depth_convention=1, b=2), pose={},
              pose_sigma=dict(sigma=0.2), eps_tmin_seed=dict(eps=2e-3, tri_tmin=30.0, seed=77))[setting]
    pose = rt.make_pose(position=(0.5, 1.0, 55.0), yaw=0.1, pitch=0.05) if setting.startswith("pose") else None
    frames = _frames(ctx, pose=pose, **kw)
    _check(ctx, frames, _random_counts(6), pose=pose, msg=setting, **kw)
    if setting == "optimized_depth_no_bounce":
        assert (frames[3] == 0).all()                                   # no segment: black, no ray


@pytest.fixture(scope="module")
def small_chains():
    """RT_PATH_SAMP_MB=1: a chain's state may take 1 MB; with 13 segments an item takes 177 bytes: 5 888 items per chain at the most"""
    c = _context(RT_PATH_SAMP_MB="1")
    yield c
    c.close()


def test_several_chains(small_chains, cat_golden):
    c = small_chains
    c.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    frames = _frames(c, n_max=8, b=12)
    counts = _random_counts(7, hi=9)
    items = int(counts.sum())
    per_chain = (1 << 20) // (16 + 16 + 64 + 16 + 5 * 13) // 64 * 64
    assert items > 2 * per_chain
    info = _check(c, frames, counts, b=12, msg="several chains")
    assert info["chains"] == -(-items // per_chain) >= 3 and info["chain_paths"] <= per_chain
    counts[:] = 8                                                       # every slot's items straddle chains somewhere
    info = _check(c, frames, counts, b=12, msg="several chains, eight everywhere")
    assert info["chains"] >= 4


def _vertex_normals(v, t):
    v = np.asarray(v, np.float64)
    fn = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    vn = np.zeros_like(v)
    for k in range(3):
        np.add.at(vn, t[:, k], fn)
    return (vn / np.maximum(np.linalg.norm(vn, axis=1, keepdims=True), 1e-20)).astype(np.float32)


@pytest.mark.parametrize("scene", ["cpu_mirror", "cpu_glass", "two_cats", "two_cats_smooth", "textured"])
def test_scenes(ctx, cat_golden, scene):
    v, t = cat_golden["vertices"], cat_golden["tri_obj_order"]
    if scene == "textured":
        rng = np.random.default_rng(3)
        vv, tv = np.asarray(v, np.float32), np.asarray(cat_golden["tri_bvh_order"])[:, :3]
        lo, hi = vv.min(0), vv.max(0)
        uv = ((vv[:, :2] - lo[:2]) / (hi[:2] - lo[:2])).astype(np.float32)
        ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden, albedo=(1.0, 1.0, 1.0)))
        ctx.mesh_set_texture(uv, tv, rng.integers(0, 256, size=(23, 37, 3), dtype=np.uint8), filter="bilinear", wrap="repeat")
    else:
        spheres, meshes = ms.capi_scene("two_cats" if scene == "two_cats_smooth" else scene, v, t)
        ctx.scene_upload(spheres, meshes)
        if scene == "two_cats_smooth":
            d = meshes[0]
            ctx.mesh_set_normals(_vertex_normals(d["vertices"], np.asarray(t)), d["indices"][:, :3], object_slot=d["object_slot"])
    b = 4 if scene in ("cpu_mirror", "cpu_glass") else B
    frames = _frames(ctx, b=b)
    assert not np.array_equal(frames[1], frames[3])
    _check(ctx, frames, _random_counts(8), b=b, msg=scene)


def test_device_transformed_and_rebuilt_meshes(ctx, cat_golden):
    _upload_cat(ctx, cat_golden)
    ctx.mesh_transform([0.96, 0.0, 0.28, 0.0, 1.0, 0.0, -0.28, 0.0, 0.96], (1.5, -2.0, 0.5))
    _check(ctx, _frames(ctx), _random_counts(9), msg="transformed")
    ctx.mesh_rebuild(len(cat_golden["tri_bvh_order"]), mode="lbvh")
    _check(ctx, _frames(ctx), _random_counts(10), msg="rebuilt (LBVH)")


def test_other_variants_are_refused(ctx, cat_golden):
    _upload_cat(ctx, cat_golden)
    counts = np.ones((H, W), np.uint8)
    for variant in ("lockstep", "global", "wavefront", "wavefront_lds", "path", "lds_all"):
        out = np.full((H, W, 4), -7, np.float32)
        with pytest.raises(rt.RtError) as e:
            ctx.render_counts(_params(variant=variant), counts, out=out)
        assert e.value.code == -5, variant
        assert (out == -7).all()
    got = ctx.render_counts(_params(variant="wavefront_queue"), counts)
    np.testing.assert_array_equal(_bits(got), _bits(ctx.render(_params())))


def test_refusals_leave_the_output_untouched(ctx, cat_golden):
    import torch
    _upload_cat(ctx, cat_golden)
    out = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda:0")
    dc = torch.ones((H, W), dtype=torch.uint8, device="cuda:0")
    p = _params()
    for args, kw in (((p, 0, out.data_ptr()), {}), ((p, dc.data_ptr(), 0), {}), ((p, out.data_ptr() + 64, out.data_ptr()), {}),
                     ((_params(w=0), dc.data_ptr(), out.data_ptr()), {}), ((_params(h=-3), dc.data_ptr(), out.data_ptr()), {}),
                     ((p, dc.data_ptr(), out.data_ptr()), dict(base_ptr=out.data_ptr() + 16))):
        with pytest.raises(rt.RtError) as e:
            ctx.render_counts_device(*args, **kw)
        assert e.value.code == -1
    ctx.synchronize()
    assert (out.cpu().numpy() == -7).all()


def test_the_first_hit_cache_is_left_alone(cat_golden, cat_frames):
    on, off = _context(), _context(RT_FIRST_HIT_CACHE="0")
    try:
        for c in (on, off):
            c.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
        p = _params(seed=5)
        a = on.render(p)                                               # a still camera: the cache is filled
        before = on.first_hit_cache_counts()
        assert before["filled"] > 0
        counts = _random_counts(11)
        got = on.render_counts(_params(), counts)
        assert on.first_hit_cache_counts() == before
        np.testing.assert_array_equal(_bits(got), _bits(_expected(cat_frames, counts)))
        b = on.render(_params(seed=6))
        after = on.first_hit_cache_counts()
        assert after["skipped"] > before["skipped"] and after["filled"] == before["filled"] and after["key_misses"] == before["key_misses"]
        np.testing.assert_array_equal(_bits(b), _bits(off.render(_params(seed=6))))
        np.testing.assert_array_equal(_bits(a), _bits(off.render(p)))
    finally:
        on.close()
        off.close()


def test_against_the_oracle(ctx, oracle, oracle_cat, cat_golden):
    _upload_cat(ctx, cat_golden)
    counts = _random_counts(12, hi=4)
    scene = oracle.Scene.preset("cpu", oracle_cat)
    frames = {c: scene.render(W, H, c, B, want_rgb8=False)[0] for c in (1, 2, 3)}
    exp = _expected(frames, counts)
    got = ctx.render_counts(_params(), counts)
    np.testing.assert_array_equal(_bits(got[..., :3]), _bits(exp[..., :3]))      # sigma == 0: every channel bit-identical to the oracle
    assert int(got[..., 3].sum()) == int(exp[..., 3].sum())
