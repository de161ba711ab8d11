"""The stream policy of wf_advance on the device (csrc/rt_wavefront.hip.h kPol*, WfState::policy; the knob RT_STREAM_POLICY of csrc/rt_host_ctx.hip.h): a default context
against one created under RT_STREAM_POLICY=0, which issues every access as the plain instruction -- word for word, colour and .w.  A non-temporal access moves the same
bytes to and from the same addresses, so nothing may differ: not a frame, not a counter of the three still-view levels, not the work a counting run reports.  -m gpu.

The cat at 61 x 45 (pixel slots outside the frame) and 64 x 48, two sub-frames of three 8-row tiles.  The two groups: the first-shade records a resumed chain loads
(every frame of a still view from the third on, chains of one sample per pixel slot) and the pixel store of the fold (every frame of one sample; with more samples
the fold stores samp_out, plainly, and path_reduce writes the frame)."""
import numpy as np
import pytest

import raytracinggpu_amd as rt

from . import still_view as sv

pytestmark = pytest.mark.gpu

KNOB = "RT_STREAM_POLICY"
LEVELS = ("first_hit_cache_counts", "first_shadow_cache_counts", "first_shade_cache_counts")


def _pair(on=None, **both):
    """(a context of the default policy, or of policy `on`; the reference: policy 0)"""
    a = sv.context(**both, **({} if on is None else {KNOB: str(on)}))
    b = sv.context(**both, **{KNOB: "0"})
    try:
        yield a, b
    finally:
        a.close()
        b.close()


@pytest.fixture(scope="module")
def pair():
    yield from _pair()


def _counters(c):
    return {m: getattr(c, m)() for m in LEVELS}


def _still_view(cs, seeds, **kw):
    """frames of one still view after an upload on both contexts: the first fills the hit and shadow levels, the second stores the records, every later one resumes.  Every
    frame equal word for word, the three levels' counters equal after every frame"""
    on, off = cs
    out = []
    for s in seeds:
        p = sv.params(seed=s, **kw)
        got, exp = on.render(p), off.render(p)
        sv.bits_equal(got, exp, f"seed {s} {kw}")
        assert got[..., 3].sum() > 0
        assert _counters(on) == _counters(off)
        out.append(got)
    return out


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("wh", [(61, 45), (64, 48)])
def test_three_frames_of_a_still_view(pair, cat_golden, wh, b):
    """fill, store, resume -- and one more resumed frame with another seed"""
    sv.upload(pair, cat_golden)
    on = pair[0]
    before = on.first_shade_cache_counts()
    frames = _still_view(pair, [5, 5, 5, 6], w=wh[0], h=wh[1], b=b)
    sv.bits_equal(frames[2], frames[0])
    assert not np.array_equal(frames[3], frames[2]) or b == 0
    after = on.first_shade_cache_counts()
    assert after["filled"] - before["filled"] == 2 and after["resumed"] - before["resumed"] == 4    # per sub-frame: the second frame stored, the third and fourth resumed


@pytest.mark.parametrize("spp", [1, 3])
def test_samples(pair, cat_golden, spp):
    """three samples: the fold stores samp_out and path_reduce adds them; the items of a resumed chain read a slot's record three times, with the plain load"""
    sv.upload(pair, cat_golden)
    _still_view(pair, [2, 2, 2, 3], w=61, h=45, b=3, spp=spp)


@pytest.mark.parametrize("parts", ["1", "2"])
def test_parts(cat_golden, parts):
    for cs in _pair(RT_PARTS=parts):
        sv.upload(cs, cat_golden)
        _still_view(cs, [8, 8, 8, 9], w=61, h=45, b=3)
        assert cs[0].stats()["parts"] == int(parts)


def test_pipelined_frames_into_two_buffers(pair, cat_golden):
    """six frames of a still view into two alternating buffers on the default context, against the reference's frames one by one"""
    import torch
    sv.upload(pair, cat_golden)
    on, off = pair
    w, h = 61, 45
    rows = rt._capi.Rows(0, h, h, 1)
    bufs = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    seeds = [11, 12, 13, 14, 15, 16]
    exp = [off.render(sv.params(w, h, 3, seed=s)) for s in seeds]
    got = []
    on.set_pipelining(True)
    try:
        for k, s in enumerate(seeds):
            on.render_device(sv.params(w, h, 3, seed=s), rows, bufs[k % 2].data_ptr())
            if k % 2 == 1:
                on.synchronize()
                got.extend(bf.cpu().numpy() for bf in bufs)
    finally:
        on.set_pipelining(False)
    for g, e in zip(got, exp):
        sv.bits_equal(g, e)
    assert _counters(on) == _counters(off)


def test_count_work(pair, cat_golden):
    sv.upload(pair, cat_golden)
    on, off = pair
    p = sv.params(61, 45, 3, seed=4)
    a, b = on.count_work(p), off.count_work(p)
    assert a == b and a["rays"] > 0 and a["tri_tests"] > 0


@pytest.mark.parametrize("bit", [1, 2])
def test_one_group_alone(cat_golden, bit):
    """a single group's bit: the records' loads, the pixel store"""
    for cs in _pair(on=bit):
        sv.upload(cs, cat_golden)
        _still_view(cs, [1, 1, 1, 2], w=61, h=45, b=3)
        _still_view(cs, [3], w=61, h=45, b=3, spp=3)
