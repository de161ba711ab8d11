"""rt_temporal_accumulate_fast[_device], rt_history_rectify[_device] and SvgfSequence(rectify=...) on the device against the numpy models of tests/rectify_model.py: every
plane, every channel of every pixel, as uint32.  -m gpu.

tests/test_rectify_model.py proves on the CPU that the synthetic inputs used here take every branch of the clamp and that the listed faults would change their bits.
Here: the two sizes with every radius and k_clamp 0 and 4, with and without planted NaN and Inf; frames in which every window is clipped; the fast accumulation on
every case of section 5.8 (its history word for word rt_temporal_accumulate's); a rendered two-frame sequence with the light moved in between; device form against host
form; in place against out of place; every refusal; SvgfSequence with and without the option.

Planted non-finite values follow _same of test_gpu_svgf.py: NaN exactly where the model has NaN (sign and payload not compared), bit-equal elsewhere."""
import numpy as np
import pytest

import raytracinggpu_amd as rt
from . import rectify_fixtures as rf
from . import rectify_model as rm
from . import svgf_model as sm
from . import synthetic_planes as sp
from . import temporal_model as tm
from .test_svgf_model import K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c_ = rt.Context(0)
    yield c_
    c_.close()


def _same(got, exp, finite, msg):
    got, exp = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(exp, np.float32)
    assert got.shape == exp.shape                                      # no pixel is left out of the comparison
    if finite:
        assert np.isfinite(exp).all(), msg
        np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32), err_msg=msg)
        return
    nan = np.isnan(exp)
    assert 0 < nan.sum() < sp.NAN_CHANNEL_CAP * exp.size, msg
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=msg + ": NaN in other places than the model's")
    np.testing.assert_array_equal(np.where(nan, 0, got.view(np.uint32)), np.where(nan, 0, exp.view(np.uint32)), err_msg=msg)


CASES = {(w, h, nf): rf.rectify_case(w, h, nonfinite=nf) for w, h in rf.SIZES for nf in (False, True)}      # built once, left unchanged


# ---------------------------------------------------------------- the clamp ----------------------------------------------------------------
@pytest.mark.parametrize("nonfinite", [False, True])
@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("w,h", rf.SIZES)
def test_rectify_on_the_synthetic_cases(ctx, w, h, radius, nonfinite):
    p = CASES[(w, h, nonfinite)]
    for k in (0.0, 4.0):
        got = ctx.history_rectify(p["history"], p["fast"], p["aov"], params=rt.make_rectify_params(radius=radius, k_clamp=k))
        exp = rm.rectify(p["history"], p["fast"], p["aov"], radius, k)
        _same(got, exp, not nonfinite, f"{w} x {h}, radius {radius}, k_clamp {k}")
        assert (got.view(np.uint32) != p["history"].view(np.uint32)).any()


@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (65, 1)])
def test_frames_in_which_every_window_is_clipped(ctx, w, h):
    p = rf.rectify_case(w, h)
    for radius in (1, 2, 3):
        got = ctx.history_rectify(p["history"], p["fast"], p["aov"][:1], params=rt.make_rectify_params(radius=radius, k_clamp=1.0))
        _same(got, rm.rectify(p["history"], p["fast"], p["aov"], radius, 1.0), True, f"{w} x {h}, radius {radius}")


def test_device_form_equals_host_form_and_in_place_equals_out_of_place(ctx):
    import torch
    w, h = rf.SIZES[1]
    p = CASES[(w, h, False)]
    exp = rm.rectify(p["history"], p["fast"], p["aov"], 2, 4.0)
    dh, df, da = (torch.from_numpy(p[k]).to("cuda:0") for k in ("history", "fast", "aov"))
    out = torch.full((2, h, w, 4), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rp = rt.make_rectify_params(radius=2, k_clamp=4.0)
    ctx.history_rectify_device(dh.data_ptr(), df.data_ptr(), da.data_ptr(), w, h, out.data_ptr(), params=rp)
    ctx.synchronize()
    _same(out.cpu().numpy(), exp, True, "the device form")
    _same(dh.cpu().numpy(), p["history"], True, "an input")
    ctx.history_rectify_device(dh.data_ptr(), df.data_ptr(), da.data_ptr(), w, h, dh.data_ptr(), params=rp)     # out == history
    ctx.synchronize()
    _same(dh.cpu().numpy(), exp, True, "in place")
    _same(df.cpu().numpy(), p["fast"], True, "an input")
    hist = p["history"].copy()
    assert ctx.history_rectify(hist, p["fast"], p["aov"], params=rp, out=hist) is hist                        # the host form in place
    _same(hist, exp, True, "the host form in place")


# ---------------------------------------------------------------- the fast accumulation ----------------------------------------------------------------
TEMPORAL = sp.temporal_gpu_cases(rt.make_pose)


def _reproject(c, kw):
    pose = kw.get("pose")
    return rt.make_reproject(camera=kw.get("camera"), pose=pose, motion=kw.get("motion"), no_history_mask=kw.get("mask", 0))


@pytest.mark.parametrize("name", sorted(TEMPORAL))
def test_fast_accumulation_on_the_cases_of_the_accumulation(ctx, name):
    build, keywords, finite = TEMPORAL[name]
    c = build()
    kw = keywords(c)
    pf = rf.previous_fast(c)
    tpk = {k: kw[k] for k in ("max_history", "alpha_min") if k in kw}
    params = rt.make_temporal_params(**tpk)
    rp = _reproject(c, kw)
    plain = ctx.temporal_accumulate(c["color"], c["aov"], c["prev_aov"], c["prev_history"], reproject=rp, params=params)
    for fh in (1, 4):
        got_h, got_f = ctx.temporal_accumulate_fast(c["color"], c["aov"], c["prev_aov"], c["prev_history"], pf, reproject=rp, params=params, fast_history=fh)
        exp_h, exp_f = rm.accumulate_fast(c["color"], c["aov"], c["prev_aov"], c["prev_history"], pf, fast_history=fh, **kw)
        _same(got_h, exp_h, finite, f"{name}: the history, fast_history {fh}")
        _same(got_f, exp_f, finite, f"{name}: the fast plane, fast_history {fh}")        # (previous_fast is made from the previous history, its NaNs too)
        np.testing.assert_array_equal(got_h.view(np.uint32), plain.view(np.uint32), err_msg=f"{name}: rt_temporal_accumulate's history word for word")
    got_h, got_f = ctx.temporal_accumulate_fast(c["color"], c["aov"], params=params)                        # a first frame
    exp_h, exp_f = rm.accumulate_fast(c["color"], c["aov"], **tpk)
    _same(got_h, exp_h, True, name + ": a first frame's history")
    _same(got_f, exp_f, True, name + ": a first frame's fast plane")


def test_fast_accumulation_takes_nan_in_the_previous_fast_plane(ctx):
    build, keywords, _ = TEMPORAL["96x64:movers"]
    c = build()
    kw = keywords(c)
    pf = rf.previous_fast(c)
    for t, (y, x) in enumerate((y, x) for y in range(5, 60, 9) for x in range(5, 90, 11)):
        pf[y, x, t % 4] = (sp.NAN, sp.INF, -sp.INF)[t % 3]
    got_h, got_f = ctx.temporal_accumulate_fast(c["color"], c["aov"], c["prev_aov"], c["prev_history"], pf, reproject=_reproject(c, kw))
    exp_h, exp_f = rm.accumulate_fast(c["color"], c["aov"], c["prev_aov"], c["prev_history"], pf, **kw)
    _same(got_h, exp_h, True, "the history does not see the fast plane")
    _same(got_f, exp_f, False, "the fast plane")


# ---------------------------------------------------------------- rendered ----------------------------------------------------------------
RW, RH = 203, 149


def _cat(cat_golden):
    return dict(vertices=cat_golden["vertices"], indices=cat_golden["tri_bvh_order"], bvh_arr10=cat_golden["bvh_arr10"], albedo=rt.scenes.CAT_ALBEDO, object_slot=6)


def _params(i, w=RW, h=RH):
    return rt.make_params(w, h, 1, 3, **dict(rt.scenes.CPU_LAUNCHER, seed=700 + i))


def test_rendered_sequence_with_the_light_moved_between_the_frames(ctx, cat_golden):
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    light = ctx.light()
    try:
        c0, a0 = ctx.render(_params(0)), ctx.render_aov(_params(0))
        ctx.set_light(*rt.light_orbit(light, 2.5, 0.2))                # half a radian: every shadow edge moves by many pixels
        c1, a1 = ctx.render(_params(1)), ctx.render_aov(_params(1))
    finally:
        ctx.set_light(*light)
    np.testing.assert_array_equal(a0, a1)                              # the light moves no plane: the reprojection accepts what it accepted
    rp, rc = rt.make_reproject(), rt.make_rectify_params(radius=1, k_clamp=0.5)
    h0, f0 = ctx.temporal_accumulate_fast(c0, a0, fast_history=2)
    h0 = ctx.history_rectify(h0, f0, a0, params=rc)
    e0 = rm.accumulate_fast(c0, a0, fast_history=2)
    _same(h0, rm.rectify(*e0, a0, 1, 0.5), True, "frame 0: the history")
    _same(h0, e0[0], True, "frame 0: n = n_f = 1 everywhere, a copy")
    _same(f0, e0[1], True, "frame 0: the fast plane")
    # a long history behind frame 0 (as if the light had stood still for 20 frames): the clamp has something to do
    h0[1, ..., 2][a0[0, ..., 3] != -1] = 20
    h1, f1 = ctx.temporal_accumulate_fast(c1, a1, a0, h0, f0, reproject=rp, fast_history=2)
    e1 = rm.accumulate_fast(c1, a1, a0, h0, f0, fast_history=2)
    _same(h1, e1[0], True, "frame 1: the accumulated history")
    _same(f1, e1[1], True, "frame 1: the fast plane")
    st = {}
    exp = rm.rectify(*e1, a1, 1, 0.5, stats=st)
    _same(ctx.history_rectify(h1, f1, a1, params=rc), exp, True, "frame 1: the rectified history")
    assert min(st["clamped_low"], st["clamped_high"], st["unmoved"], st["lost_to_id"]) >= 200, st


SW = SH = 128
POSES = [dict(), dict(position=(1.5, 0.5, 54.0), yaw=0.04), dict(position=(3.0, 1.0, 53.0), yaw=0.08, pitch=0.28), dict(position=(4.5, 1.0, 52.5), yaw=0.12, pitch=0.28)]


def _frames(ctx, seq, n=4, cut_at=None, order=None):
    outs = []
    for i in (range(n) if order is None else order):
        ptr = seq.frame(_params(i, SW, SH), pose=rt.make_pose(**POSES[i]), cut=(i == cut_at))
        ctx.synchronize()
        outs.append(ctx.device_to_host(ptr, (SH, SW, 4)))
    return outs


def test_svgf_sequence_with_rectification_equals_the_models_chain(ctx, cat_golden):
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    rc, fh, d = rt.make_rectify_params(radius=2, k_clamp=0.5), 2, rt.make_svgf_params()
    assert d.feedback_pass == -1
    exp, prev, moved = [], None, 0
    for i, kw in enumerate(POSES):
        pose = rt.make_pose(**kw)
        color, aov = ctx.render_pose(_params(i, SW, SH), pose), ctx.render_aov(_params(i, SW, SH), pose=pose)
        if prev is None:
            h, f = rm.accumulate_fast(color, aov, fast_history=fh)
        else:
            h, f = rm.accumulate_fast(color, aov, prev[0], prev[1], prev[2], fast_history=fh, pose=rt.make_pose(**POSES[i - 1]))
        r = rm.rectify(h, f, aov, 2, 0.5)
        moved += int((r.view(np.uint32) != h.view(np.uint32)).any(axis=(0, 3)).sum())
        exp.append(dict(out=sm.svgf_filter(r, aov, d.n_passes, -1, d.prefilter, *K)[0], hist=r, fast=f))
        prev = (aov, r, f)
    assert moved >= 200                                                # the clamp did something on the way
    with rt.SvgfSequence(ctx, SW, SH, rectify=rc, fast_history=fh) as seq:
        for i, out in enumerate(_frames(ctx, seq)):
            _same(out, exp[i]["out"], True, f"SvgfSequence(rectify=...).frame {i}")
        _same(ctx.device_to_host(seq.history, (2, SH, SW, 4)), exp[3]["hist"], True, "the history it hands on")
        _same(ctx.device_to_host(seq.previous_fast, (SH, SW, 4)), exp[3]["fast"], True, "the fast plane it hands on")
        _same(_frames(ctx, seq, cut_at=0, order=[0])[0], exp[0]["out"], True, "cut=True passes no previous fast plane")
        assert len(seq._ptrs) == 8
    assert seq._ptrs == []


def test_svgf_sequence_without_the_option_is_what_it_was(ctx, cat_golden):
    """rectify=None: the calls made by hand -- render, planes, temporal_accumulate_device, svgf_filter_device -- give the sequence's bits, and it owns six buffers."""
    import torch
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    with rt.SvgfSequence(ctx, SW, SH) as seq:
        got = _frames(ctx, seq)
        assert len(seq._ptrs) == 6 and not hasattr(seq, "fast")
    buf = lambda n: torch.zeros((n, SH, SW, 4), dtype=torch.float32, device="cuda:0")
    color, out, hists, planes = buf(1), buf(1), [buf(2), buf(2)], [buf(3), buf(3)]
    torch.cuda.synchronize()
    for i, kw in enumerate(POSES):
        p, pose = _params(i, SW, SH), rt.make_pose(**kw)
        ctx.render_pose_device(p, pose, color.data_ptr())
        ctx.render_aov_device(p, planes[i % 2].data_ptr(), pose=pose)
        if i == 0:
            ctx.temporal_accumulate_device(color.data_ptr(), planes[0].data_ptr(), None, None, SW, SH, hists[0].data_ptr())
        else:
            ctx.temporal_accumulate_device(color.data_ptr(), planes[i % 2].data_ptr(), planes[(i - 1) % 2].data_ptr(), hists[(i - 1) % 2].data_ptr(), SW, SH, hists[i % 2].data_ptr(),
                                           reproject=rt.make_reproject(pose=rt.make_pose(**POSES[i - 1])))
        ctx.svgf_filter_device(hists[i % 2].data_ptr(), planes[i % 2].data_ptr(), SW, SH, out.data_ptr(), None)
        ctx.synchronize()
        _same(got[i], out.cpu().numpy()[0], True, f"SvgfSequence().frame {i} against the calls made by hand")


# ---------------------------------------------------------------- refusals ----------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(ctx):
    import torch
    build, keywords, _ = TEMPORAL["96x64:movers"]
    c = build()
    kw = keywords(c)
    W, H = 96, 64
    plane = W * H * 16
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda:0")
    dc, da, dpa, dph, dpf = dev(c["color"]), dev(c["aov"]), dev(c["prev_aov"]), dev(c["prev_history"]), dev(rf.previous_fast(c))
    out = torch.full((4, H, W, 4), -7.0, dtype=torch.float32, device="cuda:0")      # (room to slide overlapping outputs along)
    outf = torch.full((2, H, W, 4), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rp = _reproject(c, kw)
    ok = dict(color_ptr=dc.data_ptr(), aov_ptr=da.data_ptr(), prev_aov_ptr=dpa.data_ptr(), prev_history_ptr=dph.data_ptr(), prev_fast_ptr=dpf.data_ptr(), width=W, height=H,
              out_ptr=out.data_ptr(), out_fast_ptr=outf.data_ptr(), reproject=rp, fast_history=4)
    ctx.temporal_accumulate_fast_device(**ok)                          # the call these are variations of is accepted
    ctx.synchronize()
    assert not (out.cpu().numpy()[:2] == -7.0).any() and not (outf.cpu().numpy()[0] == -7.0).any()
    out.fill_(-7.0)
    outf.fill_(-7.0)
    torch.cuda.synchronize()
    refused = [dict(fast_history=0), dict(fast_history=-3), dict(prev_fast_ptr=0), dict(prev_history_ptr=0, prev_aov_ptr=0), dict(prev_history_ptr=0), dict(prev_aov_ptr=0),
               dict(out_fast_ptr=0), dict(out_ptr=0), dict(color_ptr=0), dict(aov_ptr=0), dict(reproject=None), dict(width=0), dict(height=-1),
               dict(params=rt.make_temporal_params(max_history=0)),
               dict(out_fast_ptr=out.data_ptr() + 2 * plane - 16), dict(out_fast_ptr=out.data_ptr()), dict(out_ptr=outf.data_ptr() - plane - plane + 16),   # the two outputs over each other
               dict(out_fast_ptr=dpf.data_ptr() + plane - 16), dict(out_fast_ptr=dc.data_ptr()), dict(out_fast_ptr=da.data_ptr() + 2 * plane - 16),
               dict(out_fast_ptr=dpa.data_ptr() + plane), dict(out_fast_ptr=dph.data_ptr() + 2 * plane - 16),
               dict(out_ptr=dpf.data_ptr() - 2 * plane + 16), dict(out_ptr=dpf.data_ptr()), dict(out_ptr=dph.data_ptr() + plane), dict(out_ptr=dc.data_ptr())]
    for bad in refused:
        with pytest.raises(rt.RtError) as e:
            ctx.temporal_accumulate_fast_device(**dict(ok, **bad))
        assert e.value.code == -1, bad
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and (outf.cpu().numpy() == -7.0).all()
    # the rectifier
    p = CASES[(96, 64, False)]
    dh, df, dg = dev(p["history"]), dev(p["fast"]), dev(p["aov"])
    R = lambda **k: rt.make_rectify_params(**dict(dict(radius=2, k_clamp=1.0), **k))
    ok = dict(history_ptr=dh.data_ptr(), fast_ptr=df.data_ptr(), aov_ptr=dg.data_ptr(), width=W, height=H, out_ptr=out.data_ptr(), params=R())
    ctx.history_rectify_device(**ok)
    ctx.synchronize()
    assert not (out.cpu().numpy()[:2] == -7.0).any()
    out.fill_(-7.0)
    torch.cuda.synchronize()
    refused = [dict(params=R(radius=0)), dict(params=R(radius=4)), dict(params=R(radius=-1)), dict(params=R(k_clamp=-0.5)), dict(params=R(k_clamp=float("nan"))),
               dict(history_ptr=0), dict(fast_ptr=0), dict(aov_ptr=0), dict(out_ptr=0), dict(width=0), dict(height=0), dict(width=2 ** 14, height=2 ** 14),
               dict(out_ptr=dh.data_ptr() + 16), dict(out_ptr=dh.data_ptr() + plane), dict(out_ptr=dh.data_ptr() - plane),        # a partial overlap with the history
               dict(out_ptr=df.data_ptr()), dict(out_ptr=df.data_ptr() - 2 * plane + 16), dict(out_ptr=dg.data_ptr() + plane - 16), dict(out_ptr=dg.data_ptr() - plane)]
    before = dh.cpu().numpy().copy()
    for bad in refused:
        with pytest.raises(rt.RtError) as e:
            ctx.history_rectify_device(**dict(ok, **bad))
        assert e.value.code == -1, bad
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all()
    for t, a in ((dh, before), (df, p["fast"]), (dg, p["aov"])):
        _same(t.cpu().numpy(), a, True, "an input")
    # the host forms
    ho, hf = np.full((2, H, W, 4), -7, np.float32), np.full((H, W, 4), -7, np.float32)
    for bad in (dict(fast_history=0), dict(prev_fast=None), dict(prev_aov=None, prev_history=None)):
        args = dict(dict(prev_aov=c["prev_aov"], prev_history=c["prev_history"], prev_fast=rf.previous_fast(c), reproject=rp), **bad)
        with pytest.raises(rt.RtError) as e:
            ctx.temporal_accumulate_fast(c["color"], c["aov"], out=ho, out_fast=hf, **args)
        assert e.value.code == -1, bad
    for bad in (R(radius=0), R(radius=4), R(k_clamp=-1.0)):
        with pytest.raises(rt.RtError) as e:
            ctx.history_rectify(p["history"], p["fast"], p["aov"], params=bad, out=ho)
        assert e.value.code == -1
    assert (ho == -7).all() and (hf == -7).all()
    _same(ctx.history_rectify(p["history"], p["fast"], p["aov"], params=R()), rm.rectify(p["history"], p["fast"], p["aov"], 2, 1.0), True, "and the context still works")
