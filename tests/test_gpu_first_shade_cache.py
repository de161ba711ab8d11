"""The first-shade cache on the device (the records level of csrc/rt_still.h, enqueue_chain, wf_advance<kFormFill> and wf_advance<kFormResume>): a default context against one created under
RT_FIRST_SHADE_CACHE=0, word for word, colour and .w -- and rt_first_shade_cache_counts, which says whether a chain resumed its paths at the shaded first hit, stored the
records or was not eligible, so that every comparison below is known to have gone through the path it names.  -m gpu.

The cat at 64 x 48 with num_bounce 2 (two sub-frames of three 8-row tiles: two launch chains per frame and sample chunk), the shapes of test_gpu_first_shadow_cache.py.
The reference of every comparison is the knob-off context, never the cached one.  A still view walks through three states: the first frame fills the first-shadow cache
(this cache's counters do not move), the second reads it and stores the records (filled), every later one resumes."""
from functools import partial

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import hostlib

from . import material_scenes as ms
from . import still_view as sv
from .still_view import B, H, W

pytestmark = pytest.mark.gpu

LEVEL = sv.SHADE
ZERO = sv.zero(LEVEL)
_context, _bits_equal, _cat, _params, _upload, _chunk, _render_rows = sv.context, sv.bits_equal, sv.cat, sv.params, sv.upload, sv.chunk, sv.render_rows
_pair, _delta, _expect, _frame = partial(sv.pair, LEVEL), partial(sv.delta, LEVEL), partial(sv.expect, LEVEL), partial(sv.frame, LEVEL)


@pytest.fixture(scope="module")
def pair():
    yield from _pair()


@pytest.fixture(scope="module")
def pair_one_sample_per_chain():
    """RT_PATH_SAMP_MB=1: a chain's state may take 1 MB; a sample of 64 x 48 with 13 segments takes 0.73: one sample per chain"""
    yield from _pair(RT_PATH_SAMP_MB="1")


def _still_view(pair, seeds, render=None, **kw):
    """frames of one still view after an upload: the first-shadow cache fills, the records are stored, every later frame resumes"""
    out = []
    for k, s in enumerate(seeds):
        p = _params(seed=s, **kw)
        r = (lambda c, p=p: render(c, p)) if render else None
        out.append(_frame(pair, p, r, cold=k == 0, **({} if k == 0 else dict(filled=1) if k == 1 else dict(resumed=1))))
    return out


def test_the_same_frame_five_times(pair, cat_golden):
    _upload(pair, cat_golden)
    frames = _still_view(pair, [7] * 5)
    for f in frames[1:]:
        _bits_equal(f, frames[0])
    ref = _context(RT_FIRST_HIT_CACHE="0")             # no cache at all
    try:
        ref.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
        _bits_equal(ref.render(_params(seed=7)), frames[0])
        assert ref.first_shade_cache_counts() == dict(ZERO, ineligible=2)
    finally:
        ref.close()
    on, off = pair
    assert off.first_shade_cache_counts()["resumed"] == 0
    # a resumed chain skipped its first traversal launch and handed no segment-0 shadow ray to the traversal: the older counters say so
    _, fh = _delta(on, lambda: on.render(_params(seed=7)), "first_hit_cache_counts")
    _, fs = _delta(on, lambda: on.render(_params(seed=7)), "first_shadow_cache_counts")
    assert fh == dict(skipped=2, filled=0, ineligible=0, key_misses=0) and fs == fh


def test_new_seeds_with_everything_else_still(pair, cat_golden):
    _upload(pair, cat_golden)
    frames = _still_view(pair, [1, 2, 3, 4, 5])
    for a in range(2, 5):
        for b in range(a + 1, 5):
            assert not np.array_equal(frames[a], frames[b])     # the bounce rays do read the seed


def test_edits_miss_refill_and_resume(pair, cat_golden):
    _upload(pair, cat_golden)
    p = _params()
    on = pair[0]
    _still_view(pair, [0, 0, 0])
    slot = 0
    s = on.sphere(slot)
    edits = [lambda c, k: c.set_light((5.0 + k, 25.0, 35.0), 2e10),
             lambda c, k: c.move_sphere(slot, (0.25, 0.0, -0.125)),
             lambda c, k: c.set_sphere(slot, (s[0], s[1], (0.9, 0.1 + 0.1 * k, 0.2), 0, 1.0, 1.0))]    # a material edit
    for e in edits:
        for c in pair:
            e(c, 0)
        _, fs = _delta(on, lambda: _frame(pair, p, key_misses=1), "first_shadow_cache_counts")   # the edit gives a miss: this chain fills the first-shadow cache only
        assert fs == dict(skipped=0, filled=2, ineligible=0, key_misses=1), fs
        a = _frame(pair, p, filled=1)
        _bits_equal(_frame(pair, p, resumed=1), a)
        # edited before every one of six frames: the key never holds for two chains, no chain pays for a fill

        def six():
            for k in range(1, 7):
                for c in pair:
                    e(c, k)
                on.render(p)
        _, d = _delta(on, six)
        assert d["filled"] == d["resumed"] == d["ineligible"] == 0 and d["key_misses"] == 1, d
        _frame(pair, p, filled=1)                      # (the reference context was edited as often: the frames are compared again)
        _frame(pair, p, resumed=1)


@pytest.mark.parametrize("which", ["default_chunk", "one_sample_per_chain"])
def test_five_samples_per_pixel(pair, pair_one_sample_per_chain, cat_golden, which):
    """one chain of five samples per part: the later samples' items read the first sample's records; five chains of one: a frame's first chain stores them and its other four
    resume"""
    cs = pair if which == "default_chunk" else pair_one_sample_per_chain
    b = B if which == "default_chunk" else 12          # 13 segments: 177 bytes per item, 0.73 MB per sample
    chunk = _chunk(5, (400 if which == "default_chunk" else 1) << 20, b)
    assert chunk == (5 if which == "default_chunk" else 1)
    chains = (5 + chunk - 1) // chunk
    _upload(cs, cat_golden)
    p = _params(b=b, spp=5)
    _frame(cs, p, cold=True)                           # (the chains behind the one that fills the first-shadow cache read it; the records' buffer is not allocated yet)
    _frame(cs, p, filled=1, resumed=chains - 1)
    _frame(cs, p, resumed=chains)
    _frame(cs, _params(b=b, spp=5, seed=77), resumed=chains)


@pytest.mark.parametrize("b", [0, 1])
def test_short_paths(pair, cat_golden, b):
    """num_bounce 0: one segment -- the resume kernel only folds and the chain enqueues no traversal launch; num_bounce 1: one traversal launch"""
    _upload(pair, cat_golden)
    frames = _still_view(pair, [3, 3, 3, 5], b=b)
    _bits_equal(frames[2], frames[0])
    _frame(pair, _params(b=b, spp=3, seed=5), resumed=1)   # three samples as items of one chain (the sample count is not in the key)


def test_the_depth_is_not_in_the_key(pair, cat_golden):
    """records stored by a chain of one segment serve a chain of three"""
    _upload(pair, cat_golden)
    _still_view(pair, [1, 2, 3], b=0)
    _frame(pair, _params(seed=4, b=2), resumed=1)
    _frame(pair, _params(seed=5, b=2, spp=3), resumed=1)


@pytest.mark.parametrize("name", ["cpu_mirror", "cpu_glass", "two_cats"])
def test_material_scenes(pair, cat_golden, name):
    """a specular first hit, refr_code, a second mesh"""
    spheres, meshes = ms.capi_scene(name, cat_golden["vertices"], cat_golden["tri_obj_order"])
    for c in pair:
        c.scene_upload(spheres, meshes)
    frames = _still_view(pair, [1, 2, 3, 4])
    assert not np.array_equal(frames[2], frames[3])
    for b in (0, 1):                                   # the continuation ray of a specular first hit in a path of one and of two segments
        _frame(pair, _params(seed=6, b=b), resumed=1)


def test_pixel_slots_outside_the_frame(pair, cat_golden):
    _upload(pair, cat_golden)
    _still_view(pair, [1, 2, 3, 4], w=61, h=45)
    _frame(pair, _params(w=61, h=45, spp=2, seed=2), resumed=1)


def _window(ctx, n_paths):
    """the Y window of a part of n_paths paths, from the grid the context reports (share_geometry's log2S and Q for it)"""
    st = ctx.stats()
    tblocks, n_groups = st["grid_blocks"], 2 * n_paths // 4
    gpb = (n_groups + tblocks - 1) // tblocks
    log2S = gpb.bit_length() - 1
    Q = (n_groups + (1 << log2S) - 1) >> log2S
    return hostlib.qrows_enumerate(n_paths, log2S, Q, tblocks, 1)[0]


@pytest.mark.parametrize("rows", ["0", "1"])
def test_nine_resumed_frames(cat_golden, rows):
    """more than two turns of the chain number's two bits.  RT_TRAVQ_ROWS=1 (the default): traversal launch 1 of a resumed chain enumerates the Y window -- asserted from the
    grid the context reports: a part of 1536 paths has rows of shadow rays, so the window is not every row; RT_TRAVQ_ROWS=0: there is no window, the launch scans every row
    and the resume kernel clears its items' shadow slots instead"""
    for cs in _pair(RT_TRAVQ_ROWS=rows):
        _upload(cs, cat_golden)
        frames = _still_view(cs, list(range(20, 31)))  # 2 + 9
        assert not np.array_equal(frames[-1], frames[-5])
        w = _window(cs[0], 3 * 8 * 64)
        assert w["rows"] > 0                           # this queue has a Y window that is not every row: RT_TRAVQ_ROWS alone decides whether launch 1 took it


@pytest.mark.parametrize("knob", ["RT_TRAVQ_ANYHIT", "RT_DEAD_CHANNELS"])
def test_an_elision_rule_off_on_both_contexts(cat_golden, knob):
    for cs in _pair(**{knob: "0"}):
        _upload(cs, cat_golden, albedo=(0.0, 0.5, 1.0))
        _still_view(cs, [1, 2, 3, 9])
        _frame(cs, _params(spp=3, seed=9), resumed=1)


def test_dead_channels_at_the_first_hit(pair, cat_golden):
    """an albedo with a +0 channel on the cat: the DCH byte of the record is not zero"""
    _upload(pair, cat_golden, albedo=(0.0, 0.0, 0.0))
    _still_view(pair, [1, 2, 3, 4])
    _upload(pair, cat_golden, albedo=(0.0, 0.5, 1.0))
    _still_view(pair, [1, 2, 3, 4])


def test_a_textured_cat_is_not_eligible(pair, cat_golden):
    rng = np.random.default_rng(3)
    v, tv = np.asarray(cat_golden["vertices"], np.float32), np.asarray(cat_golden["tri_bvh_order"])[:, :3]
    lo, hi = v.min(0), v.max(0)
    uv = ((v[:, :2] - lo[:2]) / (hi[:2] - lo[:2])).astype(np.float32)
    px = rng.integers(0, 256, size=(23, 37, 3), dtype=np.uint8)
    _upload(pair, cat_golden, albedo=(1.0, 1.0, 1.0))
    for c in pair:
        c.mesh_set_texture(uv, tv, px, filter="bilinear", wrap="repeat")
    on = pair[0]
    frames = []

    def three():
        for k in range(3):
            frames.append(_frame(pair, _params(), cold=k == 0, ineligible=1))
    _, fs = _delta(on, three, "first_shadow_cache_counts")
    assert fs["filled"] == 2 and fs["skipped"] == 4 and fs["ineligible"] == 0, fs    # the first-shadow cache works as it did
    _bits_equal(frames[0], frames[2])
    for c in pair:
        c.mesh_set_texture(None, None, None)
    _still_view(pair, [1, 2, 3])


def test_row_shares_and_sizes_alternate(pair, cat_golden):
    _upload(pair, cat_golden)
    p = _params()
    on = pair[0]
    shares = [rt.interleaved_rows(H, 8, r, 2) for r in (0, 1)]

    def alternate():
        for k in range(3):
            for rows, idx in shares:                   # each share is one sub-frame of three tiles cut in two: a key miss every time
                _frame(pair, p, lambda c: _render_rows(c, p, rows, len(idx)), cold=True)
        for k in range(2):
            _frame(pair, _params(72, 40), cold=True)
            _frame(pair, p, cold=True)
    _, d = _delta(on, alternate)
    assert d["filled"] == d["resumed"] == d["ineligible"] == 0, d
    rows, idx = shares[1]
    render = lambda c, q: _render_rows(c, q, rows, len(idx))
    _still_view(pair, [1, 2, 3, 4], render)


def test_pipelined_frames_into_two_buffers(pair, cat_golden):
    sv.pipelined_frames(LEVEL, pair, cat_golden, filled=1, used=4)


def test_batches_stats_and_count_lists_go_round_the_cache(pair, cat_golden):
    _upload(pair, cat_golden)
    on, off = pair
    p = _params(seed=0)
    base = _still_view(pair, [0, 0, 0])[2]
    got, d = _delta(on, lambda: sv.batch_of_three(on, p))
    _bits_equal(got, sv.batch_of_three(off, p))
    assert d["ineligible"] > 0 and d["resumed"] == d["filled"] == d["key_misses"] == 0, d
    _bits_equal(_frame(pair, p, resumed=1), base)
    on.stats_enable(True)
    try:
        _frame(pair, p, ineligible=1)
        assert on.stats()["trav_launches"] == (B + 1) + 1
    finally:
        on.stats_enable(False)
    _bits_equal(_frame(pair, p, resumed=1), base)
    wk, d = _delta(on, lambda: on.count_work(p))       # a counting run: the reference's work, the same on both contexts
    assert d["ineligible"] > 0 and d["resumed"] == d["filled"] == d["key_misses"] == 0, d
    ref = off.count_work(p)
    for k in ("rays", "box_tests", "nodes", "tri_tests"):
        assert wk[k] == ref[k] > 0, k
    _bits_equal(_frame(pair, p, resumed=1), base)
    counts = np.random.default_rng(5).integers(0, 4, size=(H, W), dtype=np.uint8)
    got, d = _delta(on, lambda: on.render_counts(p, counts, base=base))
    _bits_equal(got, off.render_counts(p, counts, base=base))
    _expect(d)                                         # a list chain does not look at the cache: the counters stay where they are
    _bits_equal(_frame(pair, p, resumed=1), base)
