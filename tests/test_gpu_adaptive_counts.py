"""rt_sample_counts* against tests/adaptive_model.py byte for byte, and SvgfSequence(adaptive=...): off, the chain as it was; on, the same steps issued by hand
through the entry points, and after a cut every hit pixel gets new_surface_samples.  -m gpu."""
import ctypes as C

import numpy as np
import pytest

import raytracinggpu_amd as rt

from . import adaptive_model as am
from . import synthetic_planes as sp
from .test_adaptive_model import PARAMS, ROWS

pytestmark = pytest.mark.gpu

W, H, B = 64, 48, 2


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    yield c
    c.close()


def _cp(t):
    return rt.make_sample_count_params(*t)


def _histories():
    case = sp.reprojection_case(96, 64, 5)
    yield "reprojection", case["prev_history"]
    yield "nonfinite", sp.nonfinite_history(case)
    for name in sp.ARITHMETIC_CASES:
        yield "arithmetic:" + name, sp.arithmetic_case(name)[0]["history"]


@pytest.mark.parametrize("cp", PARAMS)
def test_counts_equal_the_model_on_synthetic_histories(ctx, cp):
    for name, h in _histories():
        h = np.ascontiguousarray(h, np.float32)
        np.testing.assert_array_equal(ctx.sample_counts(h, _cp(cp)), am.sample_counts(h, *cp), err_msg=name)


@pytest.mark.parametrize("cp", PARAMS)
def test_nan_inf_miss_and_denormal_rows(ctx, cp):
    rows = ROWS + [(1e-39, 4.0, 1e-41), (1e-20, 4.0, 1e-39), (0.0, 4.0, 1e-45), (1e-39, 1e-45, 1.0), (0.5, 3.0, 0.0625)]
    h = np.zeros((2, 3, len(rows), 4), np.float32)
    for i, (m1, n, V) in enumerate(rows):
        h[1, :, i] = (m1, 7.0, n, V)
    h[0] = np.nan                                       # plane 0 is not read
    got = ctx.sample_counts(h, _cp(cp))
    np.testing.assert_array_equal(got, am.sample_counts(h, *cp))
    assert got.min() >= 1 and got.max() <= cp[0]


def test_device_form_and_refusals(ctx):
    import torch
    h = np.ascontiguousarray(sp.reprojection_case(96, 64, 5)["prev_history"], np.float32)
    d = torch.from_numpy(h).to("cuda:0")
    out = torch.full((64, 96), 77, dtype=torch.uint8, device="cuda:0")
    cp = _cp(PARAMS[2])
    ctx.sample_counts_device(d.data_ptr(), 96, 64, out.data_ptr(), params=cp)
    ctx.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), am.sample_counts(h, *PARAMS[2]))
    out.fill_(77)
    for bad in (dict(max_samples=0), dict(max_samples=65), dict(max_samples=4, new_surface_samples=5), dict(new_surface_samples=0), dict(short_history=-1)):
        with pytest.raises(rt.RtError) as e:
            ctx.sample_counts_device(d.data_ptr(), 96, 64, out.data_ptr(), params=rt.make_sample_count_params(**bad))
        assert e.value.code == -1, bad
    for args in ((0, 96, 64, out.data_ptr()), (d.data_ptr(), 96, 64, 0), (d.data_ptr(), 0, 64, out.data_ptr()), (d.data_ptr(), 96, -1, out.data_ptr()),
                 (d.data_ptr(), 96, 64, d.data_ptr() + 64)):
        with pytest.raises(rt.RtError) as e:
            ctx.sample_counts_device(*args)
        assert e.value.code == -1, args
    ctx.synchronize()
    assert (out.cpu().numpy() == 77).all()


# ---------------------------------------------------------------- the sequence ----------------------------------------------------------------
POSES = [dict(position=(0.0, 2.0, 55.0), yaw=0.00, pitch=0.05), dict(position=(0.5, 2.0, 55.0), yaw=0.03, pitch=0.05), dict(position=(9.0, 4.0, 50.0), yaw=0.35, pitch=0.1)]
CUT = 2
ADAPTIVE = dict(max_samples=4, short_history=2, new_surface_samples=3, k_rel=0.0, lum_floor=1e-4)


def _cat(cat_golden):
    return dict(vertices=cat_golden["vertices"], indices=cat_golden["tri_bvh_order"], bvh_arr10=cat_golden["bvh_arr10"], albedo=rt.scenes.CAT_ALBEDO, object_slot=6)


def _params(i):
    return rt.make_params(W, H, 1, B, **dict(rt.scenes.CPU_LAUNCHER, seed=900 + i))


def _by_hand(ctx, adaptive):
    """the three frames through the entry points, one call after the other -> per frame (filtered frame, counts or None, planes)"""
    import torch
    buf = lambda n: torch.zeros((n, H, W, 4), dtype=torch.float32, device="cuda:0")
    color, acc, out = buf(1), [buf(2), buf(2)], buf(1)
    planes = [buf(3), buf(3)]
    counts = torch.zeros((H, W), dtype=torch.uint8, device="cuda:0")
    res = []
    for i, kw in enumerate(POSES):
        p, pose = _params(i), rt.make_pose(**kw)
        first = i == 0 or i == CUT
        cur, prev = planes[i % 2], planes[1 - i % 2]
        a, h = acc[i % 2], acc[1 - i % 2]              # nothing is fed back: the accumulated history is the one handed on
        ctx.render_pose_device(p, pose, color.data_ptr())
        ctx.render_aov_device(p, cur.data_ptr(), pose=pose)

        def accumulate():
            if first:
                ctx.temporal_accumulate_device(color.data_ptr(), cur.data_ptr(), None, None, W, H, a.data_ptr())
            else:
                ctx.temporal_accumulate_device(color.data_ptr(), cur.data_ptr(), prev.data_ptr(), h.data_ptr(), W, H, a.data_ptr(),
                                               reproject=rt.make_reproject(pose=rt.make_pose(**POSES[i - 1])))
        accumulate()
        if adaptive is not None:
            ctx.sample_counts_device(a.data_ptr(), W, H, counts.data_ptr(), params=adaptive)
            ctx.render_counts_device(p, counts.data_ptr(), color.data_ptr(), pose=pose, base_ptr=color.data_ptr())
            accumulate()
        ctx.svgf_filter_device(a.data_ptr(), cur.data_ptr(), W, H, out.data_ptr(), None)
        ctx.synchronize()
        res.append((out.cpu().numpy()[0], counts.cpu().numpy() if adaptive is not None else None, cur.cpu().numpy()))
    return res


def _sequence(ctx, adaptive):
    outs = []
    with rt.SvgfSequence(ctx, W, H, adaptive=adaptive) as seq:
        for i, kw in enumerate(POSES):
            ptr = seq.frame(_params(i), pose=rt.make_pose(**kw), cut=(i == CUT))
            ctx.synchronize()
            counts = None
            if adaptive is not None:
                counts = np.empty((H, W), np.uint8)
                ctx._check(ctx._L.rt_device_to_host(ctx._h, counts.ctypes.data_as(C.c_void_p), C.c_void_p(seq.counts), counts.nbytes))
            outs.append((ctx.device_to_host(ptr, (H, W, 4)), counts))
    return outs


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_sequence_off_is_the_chain_as_it_was(ctx, cat_golden):
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    hand = _by_hand(ctx, None)
    for i, ((out, _), (exp, _, _)) in enumerate(zip(_sequence(ctx, None), hand)):
        np.testing.assert_array_equal(_bits(out), _bits(exp), err_msg=f"frame {i}")


def test_adaptive_sequence_equals_the_steps_by_hand(ctx, cat_golden):
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    ad = rt.make_sample_count_params(**ADAPTIVE)
    hand, plain = _by_hand(ctx, ad), _by_hand(ctx, None)
    seq = _sequence(ctx, ad)
    for i, ((out, counts), (exp, ecounts, planes)) in enumerate(zip(seq, hand)):
        np.testing.assert_array_equal(_bits(out), _bits(exp), err_msg=f"frame {i}")
        np.testing.assert_array_equal(counts, ecounts, err_msg=f"counts of frame {i}")
        hit = planes[0, ..., 3] != -1
        assert hit.sum() > 100
        if i in (0, CUT):                              # no previous frame: every hit pixel is newly revealed, and k_rel = 0 asks for nothing else
            assert (counts[hit] == ADAPTIVE["new_surface_samples"]).all()
            assert (counts[~hit] == 1).all()
        assert not np.array_equal(_bits(out), _bits(plain[i][0]))       # the extra samples did reach the frame
    assert (seq[1][1] == 1).mean() > 0.3                                # a frame with a history: most of it is not short any more
