"""rt_temporal_accumulate and rt_denoise_var on the device against the numpy model of tests/temporal_model.py: every channel of every pixel of both history planes, and
of the filtered frame for n_passes 1, 3 and 5, bit for bit as uint32 views.  -m gpu.

The inputs are real: one-sample b = 3 frames with the planes rt_render_aov gives for them, at a size no tile divides -- a static sequence, a posed camera that yaws and
translates, a sphere moved by rt_scene_move_sphere, one of two cats moved by rt_mesh_transform_of, a room without its back wall (misses), the mirror and glass spheres of
demo10 behind the mask, frames narrower than anything."""
import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi
from . import denoise_model as dm
from . import material_scenes as ms
from . import temporal_model as tm

pytestmark = pytest.mark.gpu

W, H = 517, 389
VAR = {k: float(np.float32(v)) for k, v in _capi.DENOISE_VAR_DEFAULTS.items() if k != "n_passes"}
VAR_NAMES = ("k_normal", "k_position", "k_albedo", "k_sigma", "var_floor")


@pytest.fixture(scope="module")
def ctx():
    c_ = rt.Context(0)
    yield c_
    c_.close()


def _bits_equal(a, b, msg=""):
    np.testing.assert_array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32), err_msg=msg)


def _cat(cat_golden, slot=6):
    return dict(vertices=cat_golden["vertices"], indices=cat_golden["tri_bvh_order"], bvh_arr10=cat_golden["bvh_arr10"], albedo=rt.scenes.CAT_ALBEDO, object_slot=slot)


def _frame(ctx, seed, w=W, h=H, pose=None):
    p = rt.make_params(w, h, 1, 3, **dict(rt.scenes.CPU_LAUNCHER, seed=seed))
    color = ctx.render(p) if pose is None else ctx.render_pose(p, pose)
    aov = ctx.render_aov(p, pose=pose)
    assert np.isfinite(color).all() and np.isfinite(aov).all()
    return color, aov


def _step(ctx, color, aov, prev=None, camera=None, pose=None, motion=None, mask=0, taps=None, **tp):
    """one accumulation on the device and in the model, compared; prev = (planes, history) of the previous frame -> the history"""
    prev_aov, prev_hist = prev if prev is not None else (None, None)
    rp = rt.make_reproject(camera=camera, pose=pose, motion=motion, no_history_mask=mask) if prev is not None else None
    got = ctx.temporal_accumulate(color, aov, prev_aov, prev_hist, reproject=rp, params=rt.make_temporal_params(**tp))
    f32 = {k: (v if k == "max_history" else float(np.float32(v))) for k, v in tp.items()}
    exp = tm.accumulate(color, aov, prev_aov, prev_hist, camera=camera, pose=pose, motion=motion, mask=mask, taps=taps, **f32)
    assert got.shape == exp.shape == (2,) + color.shape                # no pixel is left out of the comparison
    assert np.isfinite(exp).all()
    _bits_equal(got, exp, f"history, {tp}")
    return got


def _check_var(ctx, hist, aov, passes=(1, 3, 5), **k):
    kk = dict(VAR, **{name: float(np.float32(v)) for name, v in k.items()})
    out = None
    for n in passes:
        got = ctx.denoise_var(hist, aov, n_passes=n, **k)
        exp = tm.denoise_var(hist, aov, n, *[kk[name] for name in VAR_NAMES])
        assert got.shape == exp.shape == hist[0].shape and np.isfinite(exp).all()
        _bits_equal(got, exp, f"denoise_var, n_passes {n}, {k}")
        out = got
    return out


def test_static_cat_sequence_of_four_frames(ctx, cat_golden):
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    prev, hist = None, None
    frames = []
    for i in range(4):
        color, aov = _frame(ctx, seed=100 + i)
        frames.append(color)
        hist = _step(ctx, color, aov, prev)
        assert (hist[1, ..., 2] == i + 1).all()                        # nothing moved: every pixel (no misses in the room) found itself
        if i == 0:
            _bits_equal(hist[0], color)                                # the first frame (NULL previous) is the frame
            assert (hist[1, ..., 3] > 0).mean() > 0.5                  # ... with the spatial variance
        prev = (aov, hist)
    _bits_equal(_step(ctx, frames[1], prev[0], (prev[0], _step(ctx, frames[0], prev[0])))[0, ..., :3],
                frames[0][..., :3] + (frames[1][..., :3] - frames[0][..., :3]) * np.float32(0.5))
    out = _check_var(ctx, hist, prev[0])
    assert (out[..., :3] != hist[0, ..., :3]).any(-1).mean() > 0.5     # it filters
    _check_var(ctx, hist, prev[0], passes=(2, 4), k_sigma=1.0, var_floor=1e6)
    _check_var(ctx, hist, prev[0], passes=(3,), k_normal=0.0, k_position=0.0, k_albedo=0.0, k_sigma=0.0, var_floor=0.0)   # only equal luminances pass
    # a shorter memory and a floor under the blend weight
    _step(ctx, frames[3], prev[0], prev, max_history=2)
    _step(ctx, frames[3], prev[0], prev, alpha_min=0.4)
    # rt_denoise on the same inputs gives the bits it gave before this context ran the variance-guided passes
    d = _capi.DENOISE_DEFAULTS
    _bits_equal(ctx.denoise(frames[3], prev[0]), dm.denoise(frames[3], prev[0], d["n_passes"], *[float(np.float32(d[k])) for k in ("k_normal", "k_position", "k_albedo", "k_color")]))


def test_posed_camera_that_yaws_and_translates(ctx, cat_golden):
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    poses = [rt.make_pose(), rt.make_pose(position=(1.5, 0.5, 54.0), yaw=0.04), rt.make_pose(position=(3.0, 1.0, 53.0), yaw=0.08, pitch=0.28)]
    prev = None
    for i, pose in enumerate(poses):
        color, aov = _frame(ctx, seed=7 + i, pose=pose)
        taps = {}
        hist = _step(ctx, color, aov, prev, pose=poses[i - 1] if i else None, taps=taps)
        if i:
            n = hist[1, ..., 2]
            assert (n == i + 1).mean() > 0.5 and (n == 1).sum() > 100  # most of the frame is reused, what came into view is not
            ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
            q = taps["q"]
            assert ((q[..., 0] != xs) | (q[..., 1] != ys))[q[..., 0] >= 0].mean() > 0.9   # ... from other pixels than its own
        prev = (aov, hist)
    _check_var(ctx, hist, prev[0])


def test_sphere_moved_by_scene_move_sphere(ctx, cat_golden):
    spheres = rt.scenes.spheres("cpu") + [((-14.0, -2.0, 18.0), 6.0, (0.8, 0.8, 0.8))]
    slot = len(spheres) - 1
    ctx.scene_upload(spheres, _cat(cat_golden, slot=len(spheres)))
    color0, aov0 = _frame(ctx, seed=1)
    h0 = _step(ctx, color0, aov0)
    before = [ctx.sphere(i) for i in range(len(spheres))]
    ctx.move_sphere(slot, (20.0, 10.0, -8.0), dt=0.2)
    after = [ctx.sphere(i) for i in range(len(spheres))]
    motion = rt.motion_from_spheres(before, after)
    assert np.abs(motion[slot, 9:]).max() > 1 and not motion[:slot, 9:].any()
    color1, aov1 = _frame(ctx, seed=2)
    on = aov1[0, ..., 3] == slot
    assert on.sum() > 1000
    taps = {}
    h1 = _step(ctx, color1, aov1, (aov0, h0), motion=motion, taps=taps)
    assert (h1[1, ..., 2][on] == 2).mean() > 0.8                        # the sphere's pixels follow it
    q = taps["q"][on & (h1[1, ..., 2] == 2)]
    assert (aov0[0, q[:, 1], q[:, 0], 3] == slot).all()                 # ... to the sphere's old image
    h1s = _step(ctx, color1, aov1, (aov0, h0))                          # without the record most of them find nothing
    assert (h1s[1, ..., 2][on] == 1).mean() > 0.5
    _check_var(ctx, h1, aov1)


def test_one_of_two_cats_moved_by_mesh_transform_of(ctx, cat_golden):
    spheres, meshes = ms.capi_scene("two_cats", cat_golden["vertices"], cat_golden["tri_obj_order"])
    ctx.scene_upload(spheres, meshes)
    color0, aov0 = _frame(ctx, seed=11)
    h0 = _step(ctx, color0, aov0)
    a = 0.12
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    T = np.array([-2.0, 1.0, 1.5], np.float32)
    ctx.mesh_transform(R, T, object_slot=3)
    color1, aov1 = _frame(ctx, seed=12)
    assert {3.0, 7.0} <= set(np.unique(aov1[0, ..., 3]))
    motion = rt.motion_from_mesh_transform(R, T, 3)
    h1 = _step(ctx, color1, aov1, (aov0, h0), motion=motion)
    moved, other = aov1[0, ..., 3] == 3, aov1[0, ..., 3] == 7
    assert (h1[1, ..., 2][moved] == 2).mean() > 0.3                     # (flat-shaded triangles a pixel apart need not agree within the tolerances)
    assert (h1[1, ..., 2][other] == 2).mean() > 0.9                     # the other cat stood still
    h1s = _step(ctx, color1, aov1, (aov0, h0))
    assert (h1s[1, ..., 2][moved] == 2).mean() < (h1[1, ..., 2][moved] == 2).mean()
    _check_var(ctx, h1, aov1)


def test_misses_first_frame_and_small_frames(ctx, cat_golden):
    walls = [s for s in rt.scenes.spheres("cpu") if tuple(s[0]) != (0, 0, -1000)]
    ctx.scene_upload(walls, _cat(cat_golden, slot=len(walls)))
    color0, aov0 = _frame(ctx, seed=3)
    miss = aov0[0, ..., 3] == -1
    assert 1000 < miss.sum() < W * H - 1000
    h0 = _step(ctx, color0, aov0)                                      # the first frame: NULL previous
    color1, aov1 = _frame(ctx, seed=4)
    h1 = _step(ctx, color1, aov1, (aov0, h0))
    _bits_equal(h1[0][miss], color1[miss])                             # a miss is a copy, without history or variance
    assert not h1[1][miss].any() and (h1[1, ..., 2][~miss] == 2).all()
    out = _check_var(ctx, h1, aov1)
    _bits_equal(out[miss], color1[miss])
    for w, h in ((20, 9), (5, 3), (1, 1)):                             # narrower than a tile, than the stencil, than anything
        prev = None
        for i in range(3):
            color, aov = _frame(ctx, seed=20 + i, w=w, h=h)
            hist = _step(ctx, color, aov, prev)
            prev = (aov, hist)
        _check_var(ctx, hist, prev[0])


def test_mask_for_the_mirror_and_glass_spheres_of_demo10(ctx):
    ctx.scene_upload(rt.scenes.spheres("demo10"))
    color0, aov0 = _frame(ctx, seed=5)
    h0 = _step(ctx, color0, aov0)
    color1, aov1 = _frame(ctx, seed=6)
    h1 = _step(ctx, color1, aov1, (aov0, h0), mask=0b1111)
    ids = aov1[0, ..., 3]
    masked = (ids >= 0) & (ids < 4)
    assert masked.sum() > 1000
    assert (h1[1, ..., 2][masked] == 1).all() and (h1[1, ..., 2][ids >= 4] == 2).all()
    _bits_equal(h1[0][masked], color1[masked])
    h1u = _step(ctx, color1, aov1, (aov0, h0))
    assert (h1u[1, ..., 2][masked] == 2).all()
    _check_var(ctx, h1, aov1)


def test_device_form_equals_the_host_form_and_refusals_touch_nothing(ctx, cat_golden):
    import torch
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    color0, aov0 = _frame(ctx, seed=31)
    color1, aov1 = _frame(ctx, seed=32)
    h0 = ctx.temporal_accumulate(color0, aov0)
    rp = rt.make_reproject(motion=rt.static_motion())
    exp = ctx.temporal_accumulate(color1, aov1, aov0, h0, reproject=rp)
    exp_var = ctx.denoise_var(exp, aov1, n_passes=4)
    st = torch.cuda.Stream()
    dev = lambda a: torch.from_numpy(a).to("cuda:0")
    dc, da, dpa, dph = dev(color1), dev(aov1), dev(aov0), dev(h0)
    out = torch.full((2, H, W, 4), -7.0, dtype=torch.float32, device="cuda:0")
    outc = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.temporal_accumulate_device(dc.data_ptr(), da.data_ptr(), dpa.data_ptr(), dph.data_ptr(), W, H, out.data_ptr(), reproject=rp, stream=st.cuda_stream)
    ctx.denoise_var_device(out.data_ptr(), da.data_ptr(), W, H, outc.data_ptr(), n_passes=4, stream=st.cuda_stream)
    torch.cuda.synchronize()
    _bits_equal(out.cpu().numpy(), exp)
    _bits_equal(outc.cpu().numpy(), exp_var)
    for t, a in ((dc, color1), (da, aov1), (dpa, aov0), (dph, h0)):    # the inputs are inputs
        _bits_equal(t.cpu().numpy(), a)
    hist_dev = out.clone()
    out.fill_(-7.0)
    outc.fill_(-7.0)
    torch.cuda.synchronize()
    ok = dict(color_ptr=dc.data_ptr(), aov_ptr=da.data_ptr(), prev_aov_ptr=dpa.data_ptr(), prev_history_ptr=dph.data_ptr(), width=W, height=H, out_ptr=out.data_ptr(), reproject=rp)
    plane = W * H * 16
    refused = [dict(color_ptr=0), dict(aov_ptr=0), dict(out_ptr=0),                                   # NULL where an input is required
               dict(out_ptr=dc.data_ptr()), dict(out_ptr=da.data_ptr() + plane), dict(out_ptr=dpa.data_ptr() + 64), dict(out_ptr=dph.data_ptr() + plane + 16),   # aliasing
               dict(color_ptr=out.data_ptr() + plane), dict(prev_history_ptr=out.data_ptr() + 2 * plane - 16),
               dict(width=0), dict(height=-1), dict(params=rt.make_temporal_params(max_history=0)),
               dict(prev_history_ptr=0), dict(prev_aov_ptr=0), dict(reproject=None)]                  # half a previous frame; a previous frame without its record
    for kw in refused:
        with pytest.raises(rt.RtError) as e:
            ctx.temporal_accumulate_device(**dict(ok, **kw))
        assert e.value.code == -1, kw
    ok = dict(history_ptr=hist_dev.data_ptr(), aov_ptr=da.data_ptr(), width=W, height=H, out_ptr=outc.data_ptr())
    for kw in (dict(n_passes=0), dict(n_passes=9), dict(out_ptr=hist_dev.data_ptr() + plane), dict(out_ptr=da.data_ptr() + 2 * plane + 32), dict(width=0), dict(height=0)):
        with pytest.raises(rt.RtError) as e:
            ctx.denoise_var_device(**dict(ok, **kw))
        assert e.value.code == -1, kw
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and (outc.cpu().numpy() == -7.0).all()
    _bits_equal(hist_dev.cpu().numpy(), exp)
    for t, a in ((dc, color1), (da, aov1), (dpa, aov0), (dph, h0)):
        _bits_equal(t.cpu().numpy(), a)
    # the host form: refusals leave the output as it was, and the context still works
    host_out = np.full_like(exp, -7.0)
    for kw in (dict(params=rt.make_temporal_params(max_history=0)), dict(prev_history=None), dict(prev_aov=None), dict(reproject=None), dict(prev_history=host_out)):
        args = dict(dict(prev_aov=aov0, prev_history=h0, reproject=rp), **kw)
        with pytest.raises(rt.RtError) as e:
            ctx.temporal_accumulate(color1, aov1, out=host_out, **args)
        assert e.value.code == -1, kw
    assert (host_out == -7.0).all()
    keep = exp.copy()
    with pytest.raises(rt.RtError) as e:                               # the output is the history it filters
        ctx.denoise_var(exp, aov1, out=exp[0])
    assert e.value.code == -1
    _bits_equal(exp, keep)
    _bits_equal(ctx.temporal_accumulate(color1, aov1, aov0, h0, reproject=rp, out=host_out), exp)
