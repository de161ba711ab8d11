"""What the three test_gpu_first_*_cache.py files share (a helper module, like material_scenes.py): a pair of contexts -- a default one and one created with a level's knob
off, the reference of every comparison --, the cat at 64 x 48 with num_bounce 2 (two sub-frames of three 8-row tiles: two launch chains per frame and sample chunk), and
frames compared word for word while the level's counters say which path the cached context took (csrc/rt_still.h).  Every function takes the level it is about first."""
import os
from collections import namedtuple
from contextlib import contextmanager

import numpy as np

import raytracinggpu_amd as rt

W, H, B = 64, 48, 2
Level = namedtuple("Level", "knob counts used")          # the knob that turns the level off, the Context method that reads its counters, the name of its first counter
HIT = Level("RT_FIRST_HIT_CACHE", "first_hit_cache_counts", "skipped")
SHADOW = Level("RT_FIRST_SHADOW_CACHE", "first_shadow_cache_counts", "skipped")
SHADE = Level("RT_FIRST_SHADE_CACHE", "first_shade_cache_counts", "resumed")


def zero(level):
    return {level.used: 0, "filled": 0, "ineligible": 0, "key_misses": 0}


@contextmanager
def env(**kw):
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


def context(**kw):
    with env(**kw):                                    # the knobs are read once, when the context is created
        return rt.Context(0)


def pair(level, on_kw=None, **both):
    on, off = context(**both, **(on_kw or {})), context(**both, **{level.knob: "0"})
    try:
        yield on, off
    finally:
        on.close()
        off.close()


def bits_equal(a, b, msg=""):
    np.testing.assert_array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32), err_msg=msg)


def cat(cat_golden, slot=6, albedo=rt.scenes.CAT_ALBEDO, scale=1.0):
    v = np.asarray(cat_golden["vertices"], np.float32)
    bv = np.array(cat_golden["bvh_arr10"], np.float32)
    if scale != 1.0:                                   # another mesh: the same topology, every coordinate (and every box) scaled by a power of two
        v = v * np.float32(scale)
        bv[:, 2:8] *= np.float32(scale)
    return dict(vertices=v, indices=cat_golden["tri_bvh_order"], bvh_arr10=bv, albedo=albedo, object_slot=slot)


def params(w=W, h=H, b=B, spp=1, **kw):
    d = dict(rt.scenes.CPU_LAUNCHER)
    d.update(kw)
    return rt.make_params(w, h, spp, b, **d)


def upload(cs, cat_golden, albedo=rt.scenes.CAT_ALBEDO, **kw):
    for c in cs:
        c.scene_upload(rt.scenes.spheres("cpu"), cat(cat_golden, albedo=albedo), **kw)


def delta(level, ctx, fn, counts=None):
    """(what fn returns, how far each counter of ctx moved meanwhile); counts: another level's method"""
    read = getattr(ctx, counts or level.counts)
    before = read()
    r = fn()
    after = read()
    return r, {k: after[k] - before[k] for k in after}


def expect(level, d, **kw):
    want = zero(level)
    want.update(kw)
    assert d == want, (d, want)


def frame(level, cs, p, render=None, cold=False, parts=2, **want):
    """one frame on both contexts: equal word for word, the cached context's counters moved by `want` (in chains per sub-frame, `parts` of them), the reference context's
    chains all ineligible.  cold: the first frame after an upload -- a key miss if an earlier test left the context's level filled, none on a new context: not compared"""
    on, off = cs
    render = render or (lambda c: c.render(p))
    got, d = delta(level, on, lambda: render(on))
    exp, e = delta(level, off, lambda: render(off))
    bits_equal(got, exp)
    n = on.stats()["parts"]
    assert n == parts
    if cold:
        d["key_misses"] = 0
    expect(level, d, **{k: v * n if k != "key_misses" else v for k, v in want.items()})
    assert e[level.used] == e["filled"] == e["key_misses"] == 0 and e["ineligible"] > 0
    assert got[..., 3].sum() > 0
    return got


def chunk(spp, samp_bytes, b, w=W, h=H, parts=2):
    """cut_wavefront's samples per chain"""
    px_all = ((w + 7) // 8) * ((h + 7) // 8 + parts) * 64
    per_item = 16 + 16 + 64 + 16 + 5 * (b + 1)
    cmax = max(1, min(spp, samp_bytes // (px_all * per_item), ((1 << 29) - 1) // (px_all // parts + 64)))
    chains = (spp + cmax - 1) // cmax
    return (spp + chains - 1) // chains


def render_rows(c, p, rows, n_rows):
    import torch
    buf = torch.zeros((n_rows, p.width, 4), dtype=torch.float32, device="cuda")
    c.render_device(p, rows, buf.data_ptr())
    c.synchronize()
    return buf.cpu().numpy()


def batch_of_three(c, p):
    """three frames of a batch with a camera each"""
    import torch
    rows = rt._capi.Rows(0, H, H, 1)
    bufs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
    c.render_device_batch(p, rows, [(bf.data_ptr(), (0.5 * k, 0.0, 55.0 - 3 * k), None, 40 + k) for k, bf in enumerate(bufs)])
    c.synchronize()
    return np.stack([bf.cpu().numpy() for bf in bufs])


def pipelined_frames(level, cs, cat_golden, filled, used, parts=2, w=W, h=H):
    """six frames of a still view, pipelined into two buffers: equal to the reference context's, and in chains per sub-frame (`parts` of them) `filled` of them filled the
    level and `used` used it (stream order alone keeps a chain behind the one that stored its part's words).  Returns (seeds, frames)."""
    import torch
    upload(cs, cat_golden)
    on, off = cs
    rows = rt._capi.Rows(0, h, h, 1)
    bufs = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    seeds = [11, 12, 13, 14, 15, 16]
    exp = [off.render(params(w, h, seed=s)) for s in seeds]
    on.set_pipelining(True)
    try:
        got = []

        def six():
            for k, s in enumerate(seeds):
                on.render_device(params(w, h, seed=s), rows, bufs[k % 2].data_ptr())
                if k % 2 == 1:                         # both buffers hold a frame: read them before the next two overwrite them
                    on.synchronize()
                    got.extend(b.cpu().numpy() for b in bufs)
        _, d = delta(level, on, six)
    finally:
        on.set_pipelining(False)
    n = on.stats()["parts"]
    assert n == parts
    assert d["filled"] == filled * n and d[level.used] == used * n and d["ineligible"] == 0, d
    for g, e in zip(got, exp):
        bits_equal(g, e)
    return seeds, got
