"""rt_svgf_filter[_device] and SvgfSequence on the device against the numpy model of tests/svgf_model.py: both outputs, every channel of every pixel, as uint32.  -m gpu.

tests/test_svgf_model.py proves on the CPU that the synthetic inputs used here reach the pre-filter (D changed, Gaussian taps skipped for each reason) and that the
listed faults would change their bits.  Here: the four switch combinations at 1, 3 and 5 passes with the first and the last pass fed back; frames around the 32 x 8
tile and with partly empty sub-images; every pass count from 1 to 6 with every feedback pass (and the two other filters, which share the pass plan); a rendered four-frame chain through the device entries on a second stream, with the fed-back history as the next frame's
previous one; SvgfSequence against those explicit calls; every refusal; NaN and Inf planted in the variance; the pipelining note of both outputs.

Planted non-finite values follow _same of test_gpu_synthetic_filters.py: NaN exactly where the model has NaN (sign and payload not compared), bit-equal elsewhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi
from . import denoise_model as dm
from . import svgf_model as sm
from . import synthetic_planes as sp
from . import temporal_model as tm
from .test_svgf_model import K, synthetic

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


def _check(ctx, hist, aov, n, f, pre, finite=True, msg=""):
    """the host form against the model -> (colour, history or None)"""
    got, got_h = ctx.svgf_filter(hist, aov, params=rt.make_svgf_params(n_passes=n, feedback_pass=f, prefilter=pre))
    exp, exp_h = sm.svgf_filter(hist, aov, n, f, pre, *K)
    msg = f"{msg} n_passes {n}, feedback_pass {f}, prefilter {pre}"
    _same(got, exp, finite, "colour," + msg)
    assert (got_h is None) == (exp_h is None) == (f == -1)
    if f != -1:
        _same(got_h, exp_h, finite, "history," + msg)
    return got, got_h


SYNTHETIC = synthetic()
KD = [_capi.DENOISE_DEFAULTS[name] for name in ("k_normal", "k_position", "k_albedo", "k_color")]   # rt_denoise's, as K is rt_denoise_var's


@pytest.mark.parametrize("n", [1, 3, 5])
def test_synthetic_planes_every_switch_combination(ctx, n):
    hist, aov = SYNTHETIC["history"], SYNTHETIC["aov"]
    plain = ctx.denoise_var(hist, aov, n_passes=n)
    for pre in (0, 1):
        for f in sorted({-1, 0, n - 1}):
            got, _ = _check(ctx, hist, aov, n, f, pre)
            if pre == 0:                                               # feedback or not: the frame is rt_denoise_var's
                _same(got, plain, True, f"rt_denoise_var on the same inputs, n_passes {n}, feedback_pass {f}")
            else:
                assert (got.view(np.uint32) != plain.view(np.uint32)).any()


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (33, 9), (70, 20)])
def test_sizes_where_tiles_and_sub_images_go_wrong(ctx, w, h):
    """33 x 9: one pixel over the 32 x 8 tile each way.  70 x 20 with four passes: at step 8 the sub-images are 9 x 3 and 8 x 2, some of the 64 partly empty."""
    p = sp.planes(w, h, 300 + w)
    for f in (-1, 0, 2, 3):
        _check(ctx, p["history"], p["aov"], 4, f, 1, msg=f" {w} x {h},")
    _check(ctx, p["history"], p["aov"], 4, 1, 0, msg=f" {w} x {h},")
    _check(ctx, p["history"], p["aov"], 1, 0, 1, msg=f" {w} x {h},")


def test_every_pass_count_and_feedback_pass(ctx):
    """The pass plan of rt_denoise.hip.h, which all three filters run through: every n_passes in 1 .. 6 with every feedback_pass, on one context, so that its frame and
    its variance planes are reused from call to call.  33 x 9 is one pixel over a tile each way, and at step 32 most sub-images are a single pixel.  A pass that read
    the frame it writes, or wrote into the second history after the feedback pass, would change the bits; the 27 expected results differ from each other, so taking the
    wrong pass's frame would too."""
    p = sp.planes(33, 9, 333)
    hist, aov = p["history"], p["aov"]
    expected = set()
    for n in range(1, 7):
        for f in range(-1, n):
            _check(ctx, hist, aov, n, f, 1, msg=" 33 x 9,")
            exp, exp_h = sm.svgf_filter(hist, aov, n, f, 1, *K)
            expected.add(exp.tobytes() + (b"" if exp_h is None else exp_h.tobytes()))
        _same(ctx.denoise_var(hist, aov, n_passes=n), tm.denoise_var(hist, aov, n, *K), True, f"rt_denoise_var, n_passes {n}")
        _same(ctx.denoise(p["color"], aov, n_passes=n), dm.denoise(p["color"], aov, n, *KD), True, f"rt_denoise, n_passes {n}")
    assert len(expected) == 27


def test_nan_and_inf_in_the_variance_spread_to_d_and_no_further(ctx):
    p = synthetic()
    hist, aov, ids = p["history"].copy(), p["aov"], p["ids"]
    spots = {(30, 10): np.nan, (70, 50): np.inf, (12, 40): np.nan, (80, 20): np.inf}
    for (x, y), v in spots.items():
        assert ids[y, x] != -1
        hist[1, y, x, 3] = v
    clean_out, _ = sm.svgf_filter(p["history"], aov, 1, 0, 1, *K)
    for n, f in ((1, 0), (3, 1)):
        got, got_h = ctx.svgf_filter(hist, aov, params=rt.make_svgf_params(n_passes=n, feedback_pass=f, prefilter=1))
        exp, exp_h = sm.svgf_filter(hist, aov, n, f, 1, *K)
        assert np.isfinite(exp).all()                                  # a non-finite D weighs taps 0 or 1: it never reaches the colour
        _same(got, exp, True, f"colour with planted variances, n_passes {n}")
        _same(got_h[0], exp_h[0], True, "history plane 0")
        _same(got_h[1], exp_h[1], False, "history plane 1")            # the planted values themselves, copied
        if n == 1:                                                     # one pass: only the pixels within one step of a planted variance, on its object, differ
            changed = (got.view(np.uint32) != clean_out.view(np.uint32)).any(-1)
            near = np.zeros_like(changed)
            for (x, y) in spots:
                near[y - 1:y + 2, x - 1:x + 2] = ids[y - 1:y + 2, x - 1:x + 2] == ids[y, x]
            assert changed.sum() >= len(spots) and not (changed & ~near).any()


# ---------------------------------------------------------------- a rendered chain ----------------------------------------------------------------
RW = RH = 128
POSES = [dict(), dict(position=(1.5, 0.5, 54.0), yaw=0.04), dict(position=(3.0, 1.0, 53.0), yaw=0.08, pitch=0.28), dict(position=(4.5, 1.0, 52.5), yaw=0.12, pitch=0.28)]
CHAIN = dict(n_passes=3, feedback_pass=0, prefilter=1)


def _cat(cat_golden):
    return dict(vertices=cat_golden["vertices"], indices=cat_golden["tri_bvh_order"], bvh_arr10=cat_golden["bvh_arr10"], albedo=rt.scenes.CAT_ALBEDO, object_slot=6)


def _params(i):
    return rt.make_params(RW, RH, 1, 3, **dict(rt.scenes.CPU_LAUNCHER, seed=500 + i))


@pytest.fixture(scope="module")
def chain(ctx, cat_golden):
    """Four frames with a yawing posed camera, the cat at 128 x 128, b = 3: per frame the colour and planes the device rendered and, from the chained MODELS (the
    fed-back history as the next frame's previous one), the accumulated history, the filtered frame and the fed-back history.  Computed once, left unchanged."""
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    frames, prev = [], None
    for i, kw in enumerate(POSES):
        pose = rt.make_pose(**kw)
        color, aov = ctx.render_pose(_params(i), pose), ctx.render_aov(_params(i), pose=pose)
        acc = tm.accumulate(color, aov, None if prev is None else prev[0], None if prev is None else prev[1], pose=None if prev is None else rt.make_pose(**POSES[i - 1]))
        out, fed = sm.svgf_filter(acc, aov, CHAIN["n_passes"], CHAIN["feedback_pass"], CHAIN["prefilter"], *K)
        assert np.isfinite(out).all() and np.isfinite(fed).all()
        frames.append(dict(color=color, aov=aov, acc=acc, out=out, fed=fed))
        prev = (aov, fed)
    return frames


def test_rendered_chain_on_a_second_stream(ctx, cat_golden, chain):
    import torch
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    st = torch.cuda.Stream()
    s = st.cuda_stream
    sp_ = rt.make_svgf_params(**CHAIN)
    buf = lambda n: torch.full((n, RH, RW, 4), -7.0, dtype=torch.float32, device="cuda:0")
    prev = None
    keep = []
    for i, fr in enumerate(chain):
        dc, da = torch.from_numpy(fr["color"]).to("cuda:0"), torch.from_numpy(fr["aov"]).to("cuda:0")
        acc, out, fed = buf(2), buf(1), buf(2)
        torch.cuda.synchronize()
        if prev is None:
            ctx.temporal_accumulate_device(dc.data_ptr(), da.data_ptr(), None, None, RW, RH, acc.data_ptr(), stream=s)
        else:
            rp = rt.make_reproject(pose=rt.make_pose(**POSES[i - 1]))
            ctx.temporal_accumulate_device(dc.data_ptr(), da.data_ptr(), prev[0].data_ptr(), prev[1].data_ptr(), RW, RH, acc.data_ptr(), reproject=rp, stream=s)
        ctx.svgf_filter_device(acc.data_ptr(), da.data_ptr(), RW, RH, out.data_ptr(), fed.data_ptr(), params=sp_, stream=s)
        torch.cuda.synchronize()
        _same(acc.cpu().numpy(), fr["acc"], True, f"accumulated history, frame {i}")
        _same(out.cpu().numpy()[0], fr["out"], True, f"filtered frame {i}")
        _same(fed.cpu().numpy(), fr["fed"], True, f"fed-back history, frame {i}")
        _same(da.cpu().numpy(), fr["aov"], True, "an input")
        got, got_h = ctx.svgf_filter(fr["acc"], fr["aov"], params=sp_)   # the host form on the same history
        _same(got, fr["out"], True, f"host form, frame {i}")
        _same(got_h, fr["fed"], True, f"host form's history, frame {i}")
        prev = (da, fed)
        keep.append((dc, acc, out))
    n = chain[-1]["acc"][1, ..., 2]
    assert (n == 4).mean() > 0.5 and (n == 1).sum() > 20               # most of the frame was reused through the fed-back histories


def _sequence_frames(ctx, seq, order, cut_at=None):
    outs = []
    for i in order:
        ptr = seq.frame(_params(i), pose=rt.make_pose(**POSES[i]), cut=(i == cut_at))
        ctx.synchronize()
        outs.append(ctx.device_to_host(ptr, (RH, RW, 4)))
    return outs


def test_svgf_sequence_equals_the_explicit_calls(ctx, cat_golden, chain):
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    with rt.SvgfSequence(ctx, RW, RH, svgf=rt.make_svgf_params(**CHAIN)) as seq:
        for i, out in enumerate(_sequence_frames(ctx, seq, range(4))):
            _same(out, chain[i]["out"], True, f"SvgfSequence.frame {i}")
        _same(ctx.device_to_host(seq.history, (2, RH, RW, 4)), chain[3]["fed"], True, "the history it hands on")
        # a cut is a first frame: frame 0 again, after three frames of history
        _same(_sequence_frames(ctx, seq, [0], cut_at=0)[0], chain[0]["out"], True, "cut=True")
        assert len(seq._ptrs) == 6
    assert seq._ptrs == []
    # nothing fed back (the defaults): the accumulated history itself is handed on
    d = rt.make_svgf_params()
    assert d.feedback_pass == -1
    with rt.SvgfSequence(ctx, RW, RH) as seq:
        outs = _sequence_frames(ctx, seq, range(2))
    h0 = tm.accumulate(chain[0]["color"], chain[0]["aov"])
    h1 = tm.accumulate(chain[1]["color"], chain[1]["aov"], chain[0]["aov"], h0, pose=rt.make_pose(**POSES[0]))
    for out, h, fr in zip(outs, (h0, h1), chain):
        _same(out, sm.svgf_filter(h, fr["aov"], d.n_passes, -1, d.prefilter, *K)[0], True, "SvgfSequence with the defaults")


# ---------------------------------------------------------------- refusals ----------------------------------------------------------------
def test_refusals_leave_both_outputs_untouched(ctx):
    import torch
    p = SYNTHETIC
    W, H = p["ids"].shape[1], p["ids"].shape[0]
    plane = W * H * 16
    dh, da = torch.from_numpy(p["history"]).to("cuda:0"), torch.from_numpy(p["aov"]).to("cuda:0")
    out = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda:0")
    outh = torch.full((3, H, W, 4), -7.0, dtype=torch.float32, device="cuda:0")   # (a third plane: room to slide an overlapping pair along)
    torch.cuda.synchronize()
    P = lambda **kw: rt.make_svgf_params(**dict(dict(n_passes=3, feedback_pass=1, prefilter=1), **kw))
    ok = dict(history_ptr=dh.data_ptr(), aov_ptr=da.data_ptr(), width=W, height=H, out_ptr=out.data_ptr(), out_history_ptr=outh.data_ptr(), params=P())
    ctx.svgf_filter_device(**ok)                                       # the call these are variations of is accepted
    ctx.synchronize()
    torch.cuda.synchronize()
    assert not (out.cpu().numpy() == -7.0).any()
    out.fill_(-7.0)
    outh.fill_(-7.0)
    torch.cuda.synchronize()
    refused = [dict(out_history_ptr=0), dict(params=P(feedback_pass=-1)),                             # the history and the switch go together
               dict(params=P(prefilter=2)), dict(params=P(prefilter=-1)),
               dict(params=P(feedback_pass=3)), dict(params=P(feedback_pass=-2)), dict(params=P(n_passes=1, feedback_pass=1)),
               dict(params=P(n_passes=0, feedback_pass=-1), out_history_ptr=0), dict(params=P(n_passes=9)), dict(width=0), dict(height=-1),      # what rt_denoise_var refuses
               dict(history_ptr=0), dict(aov_ptr=0), dict(out_ptr=0),
               dict(out_ptr=dh.data_ptr() + plane), dict(out_ptr=da.data_ptr() + 2 * plane + 32),
               dict(out_history_ptr=dh.data_ptr() + 2 * plane - 16), dict(out_history_ptr=da.data_ptr() + 3 * plane - 16),   # the second output over an input's last bytes
               dict(out_history_ptr=dh.data_ptr()),
               dict(out_ptr=outh.data_ptr() + 2 * plane - 16), dict(out_ptr=outh.data_ptr()), dict(out_history_ptr=out.data_ptr())]   # the two outputs over each other
    for kw in refused:
        with pytest.raises(rt.RtError) as e:
            ctx.svgf_filter_device(**dict(ok, **kw))
        assert e.value.code == -1, kw
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and (outh.cpu().numpy() == -7.0).all()
    _same(dh.cpu().numpy(), p["history"], True, "an input")
    _same(da.cpu().numpy(), p["aov"], True, "an input")
    # a 1 x (2^27 + 1) frame with eight passes: refused as rt_denoise_var refuses it
    with pytest.raises(rt.RtError) as e:
        ctx.svgf_filter_device(dh.data_ptr(), da.data_ptr(), 1, 2 ** 27 + 1, out.data_ptr(), outh.data_ptr(), params=P(n_passes=8))
    assert e.value.code == -1 and "workgroups" in str(e.value)
    # the host form
    ho, hh = np.full((H, W, 4), -7, np.float32), np.full((2, H, W, 4), -7, np.float32)
    for kw in (dict(params=P(prefilter=3)), dict(params=P(feedback_pass=5)), dict(params=P(feedback_pass=-1))):
        with pytest.raises(rt.RtError) as e:
            ctx.svgf_filter(p["history"], p["aov"], out=ho, out_history=hh, **kw)
        assert e.value.code == -1, kw
    with pytest.raises(rt.RtError):
        ctx.svgf_filter(hh, p["aov"], params=P(), out=ho, out_history=hh)                              # the history it filters as the history it writes
    assert (ho == -7).all() and (hh == -7).all()
    _check(ctx, p["history"], p["aov"], 3, 1, 1)                       # and the context still works


# ---------------------------------------------------------------- pipelining ----------------------------------------------------------------
CHILD = """
import sys
sys.path.insert(0, {root!r})
import numpy as np, torch
import raytracinggpu_amd as rt
g = np.load(rt.scenes.CAT_FIXTURE, allow_pickle=False)
ctx = rt.Context(0)
ctx.scene_upload(rt.scenes.spheres("cpu"), dict(vertices=g["vertices"], indices=g["tri_bvh_order"], bvh_arr10=g["bvh_arr10"], albedo=rt.scenes.CAT_ALBEDO, object_slot=6))
W, H = 64, 48
st = torch.cuda.Stream()
s = st.cuda_stream
rows, _ = rt.interleaved_rows(H, 8, 0, 1)
p = rt.make_params(W, H, 1, 3, **rt.scenes.CPU_LAUNCHER)
buf = lambda *shape: torch.zeros(shape + (H, W, 4), dtype=torch.float32, device="cuda:0")
big, other, planes, hist, out, B = buf(2), buf(2), buf(3), buf(2), buf(), buf()
A = big[1].data_ptr()                # frame A is plane 1 of `big`: a history laid over `big` covers it with the plane the feedback pass's lanes copy into
ctx.set_pipelining(True)
sp = rt.make_svgf_params(n_passes=2, feedback_pass=0, prefilter=1)

def case(name, between):
    ctx.render_device(p, rows, A, s)
    ctx.render_device(p, rows, B.data_ptr(), s)
    between()
    try:
        ctx.render_device(p, rows, A, s)
        print(name, "ACCEPTED", flush=True)
    except rt.RtError as e:
        print(name, "REFUSED", e.code, e, flush=True)

case("history written over A:", lambda: ctx.svgf_filter_device(hist.data_ptr(), planes.data_ptr(), W, H, out.data_ptr(), big.data_ptr(), params=sp, stream=s))
case("frame written into A:", lambda: ctx.svgf_filter_device(hist.data_ptr(), planes.data_ptr(), W, H, A, other.data_ptr(), params=sp, stream=s))
case("history read from A:", lambda: ctx.svgf_filter_device(big.data_ptr(), planes.data_ptr(), W, H, out.data_ptr(), other.data_ptr(), params=sp, stream=s))
case("elsewhere:", lambda: ctx.svgf_filter_device(hist.data_ptr(), planes.data_ptr(), W, H, out.data_ptr(), other.data_ptr(), params=sp, stream=s))
torch.cuda.synchronize()
print("END", flush=True)
"""


def test_a_pipelined_frame_does_not_overtake_the_history_write(tmp_path):
    """As test_gpu_post_between.py: the -DRT_DEBUG library refuses, instead of racing, a pipelined frame into a buffer that a call since the previous frame touches."""
    dbg = os.path.join(os.path.dirname(rt.__file__), "libraytrace_hip_debug.so")
    assert os.path.exists(dbg), "build() compiles the -DRT_DEBUG library"
    script = tmp_path / "svgf_between.py"
    script.write_text(CHILD.format(root=os.path.dirname(os.path.dirname(rt.__file__))))
    r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, RT_LIB=dbg), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "END", r.stdout[-2000:]
    verdict = {ln.split(":")[0]: ln for ln in lines if ":" in ln}
    for name in ("history written over A", "frame written into A", "history read from A"):
        assert "REFUSED -1" in verdict[name] and "pipelining rule broken" in verdict[name], verdict[name]
    assert "ACCEPTED" in verdict["elsewhere"], verdict["elsewhere"]
