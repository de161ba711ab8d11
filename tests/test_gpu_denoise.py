"""rt_denoise on the device against the numpy model of tests/denoise_model.py: every channel of every pixel, bit for bit as uint32 views.  -m gpu.

The inputs are real: one-sample b = 3 frames of the cat scene (and of two_cats with a textured cat, and of a room without its back wall, so that misses exist) with the
planes rt_render_aov gives for them, at a size no tile divides."""
import numpy as np
import pytest

import raytracinggpu_amd as rt
from . import denoise_model as dm
from . import material_scenes as ms

pytestmark = pytest.mark.gpu

W, H = 517, 389
K = dict(k_normal=2.0, k_position=0.25, k_albedo=16.0, k_color=5e-12)
NAMES = ("k_normal", "k_position", "k_albedo", "k_color")


@pytest.fixture(scope="module")
def ctx():
    c_ = rt.Context(0)
    yield c_
    c_.close()


def _bits_equal(a, b, msg=""):
    np.testing.assert_array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32), err_msg=msg)


def _cat(cat_golden, slot=6):
    return dict(vertices=cat_golden["vertices"], indices=cat_golden["tri_bvh_order"], bvh_arr10=cat_golden["bvh_arr10"], albedo=rt.scenes.CAT_ALBEDO, object_slot=slot)


def _frame(ctx, w=W, h=H):
    p = rt.make_params(w, h, 1, 3, **rt.scenes.CPU_LAUNCHER)
    color, aov = ctx.render(p), ctx.render_aov(p)
    assert np.isfinite(color).all() and np.isfinite(aov).all()
    return color, aov


def _check(ctx, color, aov, n, **k):
    f32 = {name: float(np.float32(v)) for name, v in k.items()}       # the library sees binary32 parameters; so does the model
    got = ctx.denoise(color, aov, n_passes=n, **k)
    exp = dm.denoise(color, aov, n, *[f32[name] for name in NAMES])
    assert got.shape == exp.shape == color.shape                     # no pixel is left out of the comparison
    _bits_equal(got, exp, f"n_passes {n}, {k}")
    return got


@pytest.fixture(scope="module")
def cat_frame(ctx, cat_golden):
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    return _frame(ctx)


@pytest.mark.parametrize("n", [1, 3, 5])
def test_cat_frame_equals_the_model(ctx, cat_frame, n):
    color, aov = cat_frame
    out = _check(ctx, color, aov, n, **K)
    assert (out[..., :3] != color[..., :3]).any(-1).mean() > 0.5     # it filters
    _check(ctx, color, aov, n, **{name: 0.0 for name in NAMES})


@pytest.mark.parametrize("zero", NAMES)
def test_each_term_switched_off_and_alone(ctx, cat_frame, zero):
    color, aov = cat_frame
    a = _check(ctx, color, aov, 3, **dict(K, **{zero: 0.0}))
    b = _check(ctx, color, aov, 3, **{name: (K[name] if name == zero else 0.0) for name in NAMES})
    c = ctx.denoise(color, aov, n_passes=3, **K)
    if zero != "k_albedo":                                           # (an untextured object has one albedo, and taps never cross objects: that term shows on the textured frame)
        assert (a != c).any() and (b != c).any()                     # the term does something on this frame


def test_textured_two_mesh_frame_equals_the_model(ctx, cat_golden):
    rng = np.random.default_rng(9)
    v, t_obj = cat_golden["vertices"], cat_golden["tri_obj_order"]
    spheres, meshes = ms.capi_scene("two_cats", v, t_obj)
    ctx.scene_upload(spheres, meshes)
    m3 = next(d for d in meshes if d["object_slot"] == 3)
    t3 = np.asarray(m3["indices"])[:, :3]
    vv = np.asarray(m3["vertices"], np.float32)
    lo, hi = vv.min(0), vv.max(0)
    uvs = ((vv[:, :2] - lo[:2]) / (hi[:2] - lo[:2])).astype(np.float32)
    ctx.mesh_set_texture(uvs, t3, rng.integers(0, 256, size=(23, 37, 3), dtype=np.uint8), filter="bilinear", object_slot=3)
    color, aov = _frame(ctx)
    assert {3.0, 7.0} <= set(np.unique(aov[0, ..., 3]))
    assert len(np.unique(aov[2][aov[0, ..., 3] == 3][:, 0])) > 50    # the textured cat's albedo varies
    _check(ctx, color, aov, 3, **K)
    _check(ctx, color, aov, 5, **dict(K, k_color=0.0))
    a = _check(ctx, color, aov, 1, **dict(K, k_albedo=400.0))
    assert (a != ctx.denoise(color, aov, n_passes=1, **dict(K, k_albedo=0.0))).any()   # the albedo term sees the texture
    ctx.mesh_set_texture(None, None, None, object_slot=3)


def test_frame_with_misses_and_small_frames(ctx, cat_golden):
    walls = [s for s in rt.scenes.spheres("cpu") if tuple(s[0]) != (0, 0, -1000)]
    ctx.scene_upload(walls, _cat(cat_golden, slot=len(walls)))
    color, aov = _frame(ctx)
    miss = aov[0, ..., 3] == -1
    assert 1000 < miss.sum() < W * H - 1000
    out = _check(ctx, color, aov, 4, **K)
    _bits_equal(out[miss], color[miss])
    for w, h in ((20, 9), (5, 3), (1, 1), (33, 64)):                  # narrower than a tile, than the stencil, than anything
        color, aov = _frame(ctx, w, h)
        for n in (1, 3, 8):
            _check(ctx, color, aov, n, **K)


def test_device_form_equals_the_host_form(ctx, cat_frame):
    import torch
    color, aov = cat_frame
    exp = ctx.denoise(color, aov, n_passes=4, **K)
    st = torch.cuda.Stream()
    dc, da = torch.from_numpy(color).to("cuda:0"), torch.from_numpy(aov).to("cuda:0")
    out = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.denoise_device(dc.data_ptr(), da.data_ptr(), W, H, out.data_ptr(), n_passes=4, stream=st.cuda_stream, **K)
    torch.cuda.synchronize()
    _bits_equal(out.cpu().numpy(), exp)
    _bits_equal(dc.cpu().numpy(), color)                              # the inputs are inputs
    _bits_equal(da.cpu().numpy(), aov)
    # refusals leave the output as it was: aliasing (the colour frame, the middle of the planes), n_passes outside 1 .. 8
    out.fill_(-7.0)
    torch.cuda.synchronize()
    for kw in (dict(out_ptr=dc.data_ptr()), dict(out_ptr=da.data_ptr() + W * H * 16 + 64), dict(out_ptr=out.data_ptr(), n_passes=0), dict(out_ptr=out.data_ptr(), n_passes=9)):
        args = dict(dict(n_passes=2), **kw)
        with pytest.raises(rt.RtError) as e:
            ctx.denoise_device(dc.data_ptr(), da.data_ptr(), W, H, args.pop("out_ptr"), **args)
        assert e.value.code == -1
    with pytest.raises(rt.RtError) as e:                              # an output that begins inside the colour frame
        ctx.denoise_device(dc.data_ptr(), da.data_ptr(), W, H // 2, dc.data_ptr() + 16 * W, n_passes=1)
    assert e.value.code == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all()
    _bits_equal(dc.cpu().numpy(), color)
    _bits_equal(da.cpu().numpy(), aov)


def test_host_form_refusals_leave_the_output_untouched(ctx, cat_frame):
    color, aov = cat_frame
    out = np.full_like(color, -7.0)
    for n in (0, 9, -1):
        with pytest.raises(rt.RtError) as e:
            ctx.denoise(color, aov, n_passes=n, out=out)
        assert e.value.code == -1
    with pytest.raises(rt.RtError) as e:                              # planes of another frame size
        ctx.denoise(color, aov[:, :-1], out=out)
    assert e.value.code == -1
    with pytest.raises(rt.RtError) as e:
        ctx.denoise(color[:, :-1], aov, out=out)
    assert e.value.code == -1
    assert (out == -7.0).all()
    keep = color.copy()
    with pytest.raises(rt.RtError) as e:                              # the output is the colour frame
        ctx.denoise(color, aov, out=color)
    assert e.value.code == -1
    planes = aov.copy()
    with pytest.raises(rt.RtError) as e:                              # ... or one of the planes
        ctx.denoise(color, planes, out=planes[1])
    assert e.value.code == -1
    _bits_equal(color, keep)
    _bits_equal(planes, aov)
    _bits_equal(ctx.denoise(color, aov, out=out), ctx.denoise(color, aov))   # and the context still works
