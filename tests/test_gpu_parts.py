"""Every cut of a frame into sub-frames: contexts created under RT_PARTS 1, 3, 4, 5 and 8 (the suite's other files all render with the default two), and under the other
knobs of INTEGRATION.md section 4 that no test named -- RT_PART_PRIO, RT_ASYNC_PIPELINE, RT_AUTO_LOCKSTEP -- against the CPU oracle.  -m gpu.

The cat in the `cpu` room, num_bounce 2.  With sigma == 0 a frame is the oracle's word for word: colours compared as uint32, `.w` the oracle's ray count; where the oracle
has no such operation (jittered samples bit for bit, per-pixel sample counts) the reference is a default context, which the rest of the suite pins to the oracle.  The
frames are the smallest that still exercise the cut (csrc/rt_rowcut.h, cut_wavefront, start_chains / end_chains, enqueue_chain):
    61 x 43   6 row tiles, the last of 3 rows, a partial column tile          61 x 67   9 tiles: under RT_PARTS=8 one sub-frame has two tiles and owns the partial one
    64 x 5    one tile: every cut clamps to one sub-frame                     61 x 131  17 tiles, for row shares, ranges and chunks
A failure names RT_PARTS, the case and the first differing pixel.  tests/test_rowcut_model.py holds the row arithmetic itself to a model without a device."""
import numpy as np
import pytest

import raytracinggpu_amd as rt

from . import still_view as sv
from .test_gpu_parity import TOL, linf, upload
from .test_gpu_scene_fuzz import SHOWN, _bytes_differ, _differences

pytestmark = pytest.mark.gpu

PARTS = (1, 3, 4, 5, 8)
B = 2
LEVELS = (sv.HIT, sv.SHADOW, sv.SHADE)
LIGHT = rt.scenes.LIGHT


def _tiles(n_rows, tile_rows=8):
    return -(-n_rows // tile_rows)


def _report(found):
    for line in found:
        print("  " + line)
    if found:
        pytest.fail(f"{len(found)} comparisons differ:\n" + "\n".join(found[:SHOWN]))


def _parts_are(c, want, what, found):
    n = c.stats()["parts"]
    if n != want:
        found.append(f"{what}: {n} sub-frames, expected {want}")


@pytest.fixture(scope="module")
def contexts(cat_golden):
    """contexts(parts, scene, **knobs): one context per set of knobs for the whole module (knobs are read once, at creation), the scene uploaded; parts None: the default"""
    made = {}

    def get(parts=None, scene="cpu", **knobs):
        key = (parts, scene, tuple(sorted(knobs.items())))
        if key not in made:
            kw = dict(knobs, RT_PARTS=str(parts)) if parts is not None else knobs
            made[key] = sv.context(**kw)
            upload(made[key], scene, cat_golden)
        return made[key]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def expected(oracle, oracle_cat):
    """the oracle's frame, computed once per set of arguments and read-only.  spheres: [(centre, radius)] in place of the room's own"""
    frames = {}

    def get(w, h, spp=1, b=B, seed=123456, cam=(0.0, 0.0, 55.0), light=LIGHT, sigma=0.0, scene="cpu", spheres=None, counters=False):
        key = (w, h, spp, b, seed, cam, light, sigma, scene, spheres)
        if key not in frames:
            sc = oracle.Scene()
            for k, s in enumerate(rt.scenes.spheres(scene)):
                centre, radius = spheres[k] if spheres else s[:2]
                sc.add_sphere(centre, radius, *s[2:])
            if scene == "cpu":
                sc.add_mesh(oracle_cat)
            sc.set_light(*light)
            f, _, cnt = sc.render(w, h, spp, b, sigma=sigma, cam=cam, seed=seed, want_rgb8=False)
            f.setflags(write=False)
            frames[key] = f, cnt
        return frames[key] if counters else frames[key][0]
    return get


def _device_frames(n, w, h):
    import torch
    return [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0") for _ in range(n)]


# 1 ---- one frame, every cut

@pytest.mark.parametrize("P", PARTS)
def test_one_frame_every_cut(contexts, expected, P):
    c, found = contexts(P), []
    for w, h, bounces in ((61, 43, (B,)), (61, 67, (B, 0, 1)), (64, 5, (B,))):
        for b in bounces:                                      # (still_plan has special cases for one segment)
            exp = expected(w, h, b=b)
            for variant in ("auto", "wavefront", "lds_all"):
                for again in range(3 if variant == "auto" else 1):   # a still view under this cut: its levels fill, store the records and resume (test 4 counts them)
                    what = f"RT_PARTS={P} {w} x {h} num_bounce {b} variant {variant} frame {again}"
                    _differences(c.render(sv.params(w, h, b, variant=variant)), exp, what, found)
                    _parts_are(c, min(P, _tiles(h)), what, found)
    _report(found)


# 2 ---- row shares and ranges

@pytest.mark.parametrize("P", PARTS)
def test_row_shares_and_ranges(contexts, expected, P):
    c, found = contexts(P), []
    w, h = 61, 131
    p, exp = sv.params(w, h), expected(w, h)
    for tile_rows, world, tiles in ((8, 3, (6, 6, 5)), (16, 2, (5, 4)), (12, 2, (6, 5))):
        for rank in range(world):
            rows, idx = rt.interleaved_rows(h, tile_rows, rank, world)
            assert _tiles(rows.n_rows, tile_rows) == tiles[rank]
            what = f"RT_PARTS={P} {w} x {h} tiles of {tile_rows} rows, rank {rank} of {world}"
            _differences(sv.render_rows(c, p, rows, rows.n_rows), exp[idx], what, found)
            _parts_are(c, 1 if tile_rows % 8 else min(P, tiles[rank]), what, found)
    _differences(c.render(p, 13, 118), exp[13:118], f"RT_PARTS={P} {w} x {h} rows 13 to 118", found)
    _parts_are(c, min(P, 14), f"RT_PARTS={P} rows 13 to 118", found)
    _report(found)


# 3 ---- samples

@pytest.mark.parametrize("P", PARTS)
def test_samples(contexts, expected, oracle, P):
    found = []
    w, h, spp = 61, 67, 5
    jitter = sv.params(w, h, spp=spp, sigma=0.2)
    ref = contexts().render(jitter)
    for knobs in ({}, {"RT_PATH_SAMP_MB": "1"}):               # all five samples in one chain / one sample per chain (1.1 MB of state per sample at eight sub-frames, 0.65 at one)
        c = contexts(P, **knobs)
        for again in range(3):
            _differences(c.render(sv.params(w, h, spp=spp)), expected(w, h, spp), f"RT_PARTS={P} {knobs} {spp} samples frame {again}", found)
        got = c.render(jitter)                                  # jittered camera rays: not a still view
        _differences(got, ref, f"RT_PARTS={P} {knobs} {spp} samples sigma 0.2 against the default context", found)
        exp = expected(w, h, spp, sigma=0.2)
        err = linf(oracle, got, exp)
        print(f"RT_PARTS={P} {knobs} sigma 0.2: Linf(gamma) {err:.3g}")
        assert err <= TOL
        np.testing.assert_array_equal(got[..., 3], exp[..., 3])
    _report(found)


# 4 ---- the still-view levels

def _level_counts(c):
    return {lv: getattr(c, lv.counts)() for lv in LEVELS}


def _level_step(state, n):
    """how far the counters of the three levels move in one frame of n chains (tests/test_gpu_first_shade_cache.py documents the order for two)"""
    hit, shadow, shade = (sv.zero(lv) for lv in LEVELS)
    if state == "cold":                                         # the first frame of a view: camera rays and first shadow rays traced and kept
        hit["filled"] = shadow["filled"] = n
    elif state == "edit":                                       # the light moved: the camera rays' hits hold, the shadow level refills, the records are dropped
        hit["skipped"] = shadow["filled"] = n
        shadow["key_misses"] = shade["key_misses"] = 1
    else:                                                       # both older levels read; the records stored by the first such frame, resumed by the later ones
        hit["skipped"] = shadow["skipped"] = n
        shade["filled" if state == "store" else "resumed"] = n
    return dict(zip(LEVELS, (hit, shadow, shade)))


@pytest.mark.parametrize("P", (1, 3, 8))
def test_still_view_levels(contexts, expected, cat_golden, P):
    c, found = contexts(P), []
    w, h = 61, 67
    n = min(P, _tiles(h))
    moved = ((5.0, 25.0, 35.0), 2e10)
    steps = [("cold", 7, None), ("store", 7, None), ("resume", 7, None), ("resume", 7, None), ("resume", 7, None),
             ("resume", 8, None), ("edit", 8, moved), ("store", 8, None), ("resume", 8, None)]
    upload(c, "cpu", cat_golden)                               # a new scene: every level starts empty
    light = LIGHT
    try:
        for k, (state, seed, new_light) in enumerate(steps):
            if new_light:
                light = new_light
                c.set_light(*light)
            before = _level_counts(c)
            got = c.render(sv.params(w, h, seed=seed))
            after = _level_counts(c)
            what = f"RT_PARTS={P} frame {k} ({state}, seed {seed})"
            _differences(got, expected(w, h, seed=seed, light=light), what, found)
            _parts_are(c, n, what, found)
            for lv, want in _level_step(state, n).items():
                d = {key: after[lv][key] - before[lv][key] for key in want}
                if state == "cold":
                    d["key_misses"] = 0                         # (an earlier test's view may have been dropped by the upload)
                if d != want:
                    found.append(f"{what}: {lv.counts} moved by {d}, expected {want}")
    finally:
        upload(c, "cpu", cat_golden)
    _report(found)


# 5 ---- pipelined frames

@pytest.mark.parametrize("P", (3, 8))
def test_pipelined_frames(contexts, expected, oracle, cat_golden, P, knobs=None):
    import torch
    c, found = contexts(P, **(knobs or {})), []
    w, h = 61, 67
    n = min(P, _tiles(h))
    tag = f"RT_PARTS={P} {knobs or ''}"
    # six frames of a still view into two buffers: the records stored by the second frame, resumed by the other four
    seeds, frames = sv.pipelined_frames(sv.SHADE, (c, contexts()), cat_golden, filled=1, used=4, parts=n, w=w, h=h)
    for s, f in zip(seeds, frames):
        _differences(f, expected(w, h, seed=s), f"{tag} pipelined still view, seed {s}", found)
    if knobs:                                                   # (test 9: the run above is the one it asks for)
        return _report(found)
    # seven frames into two and three buffers on a stream of the caller's, a consumer of every frame in between, the parameters changing on the way
    st = torch.cuda.Stream()
    rows, _ = rt.interleaved_rows(h, 8, 0, 1)
    ps = [sv.params(w, h), sv.params(w, h, 1, spp=2)]
    exps = [expected(w, h), expected(w, h, 2, 1)]
    exps8 = [oracle.tonemap(e) for e in exps]
    try:
        c.set_pipelining(True)
        for n_buf in (2, 3):
            bufs = _device_frames(n_buf, w, h)
            img = [torch.zeros((h * w * 3 + 16,), dtype=torch.uint8, device="cuda:0") for _ in range(7)]
            torch.cuda.synchronize()
            which = [1 if k in (3, 4) else 0 for k in range(7)]
            for k in range(7):
                c.render_device(ps[which[k]], rows, bufs[k % n_buf].data_ptr(), st.cuda_stream)
                c.tonemap_device(bufs[k % n_buf].data_ptr(), h * w, img[k].data_ptr(), st.cuda_stream)
            torch.cuda.synchronize()
            for k in range(7):
                _bytes_differ(img[k][:h * w * 3].cpu().numpy().reshape(h, w, 3), exps8[which[k]], f"{tag} {n_buf} buffers, image {k}", found)
            for k in range(7 - n_buf, 7):
                _differences(bufs[k % n_buf].cpu().numpy(), exps[which[k]], f"{tag} {n_buf} buffers, frame {k}", found)
    finally:
        c.set_pipelining(False)
    c.selfcheck()
    _report(found)


# 6 ---- batches

def _camera(k):
    return (0.5 * k, 0.25 * k, 55.0 - k)


def _batch(c, w, h, n, scenes=None):
    rows = rt._capi.Rows(0, h, h, 1)
    bufs = _device_frames(n, w, h)
    c.render_device_batch(sv.params(w, h), rows, [(bf.data_ptr(), _camera(k), None, 40 + k) for k, bf in enumerate(bufs)], scenes=scenes)
    c.synchronize()
    return [bf.cpu().numpy() for bf in bufs]


# (sub-frames wanted, frames, height).  At 61 x 43 eight sub-frames clamp to the six tiles; 61 x 67 has the tiles for eight, so that 8 and 16 frames are cut by frames
BATCHES = [(3, 3, 43), (3, 6, 43), (3, 8, 43), (4, 6, 43), (8, 8, 43), (8, 16, 43), (5, 16, 43), (8, 8, 67), (8, 16, 67)]


@pytest.mark.parametrize("P,n,h", BATCHES)
def test_batches(contexts, expected, P, n, h):
    c, found = contexts(P), []
    w = 61
    for k, got in enumerate(_batch(c, w, h, n)):
        _differences(got, expected(w, h, seed=40 + k, cam=_camera(k)), f"RT_PARTS={P} batch of {n} at {w} x {h}, frame {k}", found)
    _parts_are(c, min(P, _tiles(h)), f"RT_PARTS={P} batch of {n} at {w} x {h}", found)
    _report(found)


@pytest.mark.parametrize("P,n", [(3, 10), (8, 16)])
def test_animated_batches(contexts, expected, P, n):
    """every frame with its own light and sphere poses; ten frames per sub-frame are two launches of the store kernel"""
    c, found = contexts(P), []
    w, h = 61, 43
    walls = rt.scenes.spheres("cpu")

    def poses(k):
        return tuple(((s[0][0] + (0.5 * k if j == 3 else 0.0), s[0][1], s[0][2] - (0.25 * k if j == 0 else 0.0)), float(s[1] + (0.125 * k if j == 1 else 0.0)))
                     for j, s in enumerate(walls))
    lights = [((LIGHT[0][0] + k, LIGHT[0][1], LIGHT[0][2] - 0.5 * k), LIGHT[1] * (1.0 + 0.0625 * k)) for k in range(n)]
    scenes = [(lights[k], [(list(ce), r) for ce, r in poses(k)]) for k in range(n)]
    for k, got in enumerate(_batch(c, w, h, n, scenes=scenes)):
        exp = expected(w, h, seed=40 + k, cam=_camera(k), light=lights[k], spheres=poses(k))
        _differences(got, exp, f"RT_PARTS={P} animated batch of {n}, frame {k}", found)
    _report(found)


# 7 ---- chunks x parts

@pytest.mark.parametrize("P", (4, 8))
def test_chunks_of_every_cut(contexts, expected, P):
    """RT_CHUNK_MPX=0.002: 61 x 131 in chunks of 48, 48 and 35 rows -- 6, 6 and 5 tiles, so under RT_PARTS=8 the last chunk's layout differs and the chains re-join"""
    c, found = contexts(P, RT_CHUNK_MPX="0.002"), []
    w, h = 61, 131
    p, exp = sv.params(w, h), expected(w, h)
    for again in range(2):                                     # the second call starts from what the first one left open
        what = f"RT_PARTS={P} RT_CHUNK_MPX=0.002 call {again}"
        _differences(c.render(p), exp, what + " whole frame", found)
        _parts_are(c, min(P, 5), what + " whole frame, last chunk", found)
        _differences(c.render(p, 13, 118), exp[13:118], what + " rows 13 to 118", found)
        for rank in range(3):
            rows, idx = rt.interleaved_rows(h, 8, rank, 3)
            _differences(sv.render_rows(c, p, rows, rows.n_rows), exp[idx], what + f" rank {rank} of 3", found)
    c.selfcheck()
    _report(found)


# 8 ---- render_async / wait

@pytest.mark.parametrize("pipeline", ("0", "1"))
def test_async_frames(contexts, expected, oracle, pipeline):
    c, found = contexts(3, RT_ASYNC_PIPELINE=pipeline), []
    w, h = 61, 67
    seeds = (21, 22, 23, 24)
    for rgb8 in (False, True):
        pins = [rt.PinnedArray((h, w, 3), dtype=np.uint8) if rgb8 else rt.PinnedArray((h, w, 4)) for _ in range(2)]
        got = []
        try:
            for k, s in enumerate(seeds):                      # frame k is submitted before frame k - 1 has been collected
                c.render_async(sv.params(w, h, seed=s), pins[k & 1].array, slot=k & 1, rgb8=rgb8)
                if k > 0:
                    c.wait((k - 1) & 1)
                    got.append(pins[(k - 1) & 1].array.copy())
            c.wait((len(seeds) - 1) & 1)
            got.append(pins[(len(seeds) - 1) & 1].array.copy())
        finally:
            for pn in pins:
                pn.close()
        for s, g in zip(seeds, got):
            what = f"RT_PARTS=3 RT_ASYNC_PIPELINE={pipeline} seed {s}"
            if rgb8:
                _bytes_differ(g, oracle.tonemap(expected(w, h, seed=s)), what + " 8-bit image", found)
            else:
                _differences(g, expected(w, h, seed=s), what, found)
    _parts_are(c, 3, f"RT_ASYNC_PIPELINE={pipeline}", found)
    _report(found)


# 9 ---- the other knobs no test named

@pytest.mark.parametrize("P", (2, 3))
def test_part_priority(contexts, expected, oracle, cat_golden, P):
    c, found = contexts(P, RT_PART_PRIO="1"), []
    w, h = 61, 67
    for variant in ("auto", "wavefront", "lds_all"):
        what = f"RT_PART_PRIO=1 RT_PARTS={P} {w} x {h} variant {variant}"
        _differences(c.render(sv.params(w, h, variant=variant)), expected(w, h), what, found)
        _parts_are(c, P, what, found)
    _report(found)
    test_pipelined_frames(contexts, expected, oracle, cat_golden, P, knobs={"RT_PART_PRIO": "1"})


def test_auto_without_the_lockstep_kernel(contexts, expected):
    """a scene without a mesh: RT_VARIANT_AUTO is the lock-step kernel, under RT_AUTO_LOCKSTEP=0 the work-stack pipeline -- the same words"""
    found = []
    w, h = 61, 67
    p, exp = sv.params(w, h), expected(w, h, scene="demo10")
    wf, default = contexts(scene="demo10", RT_AUTO_LOCKSTEP="0"), contexts(scene="demo10")
    got = wf.render(p)
    assert wf.stats()["variant"] == rt._capi.VARIANTS["wavefront_queue"]
    _differences(got, exp, "RT_AUTO_LOCKSTEP=0 demo10", found)
    ref = default.render(p)
    assert default.stats()["variant"] == rt._capi.VARIANTS["lockstep"]
    _differences(ref, exp, "demo10 on a default context", found)
    _differences(got, ref, "RT_AUTO_LOCKSTEP=0 demo10 against the default context", found)
    _report(found)


# 10 ---- what must not move

def test_counting_runs_and_count_lists_do_not_take_the_knob(contexts, expected):
    c, found = contexts(5), []
    w, h = 61, 67
    _, cnt = expected(w, h, counters=True)
    assert c.count_work(sv.params(w, h)) == {k: cnt[k] for k in ("rays", "box_tests", "nodes", "tri_tests")}
    assert c.stats()["parts"] == 1                             # a counting run is one sub-frame
    # the list chains share the queue buffers with the dense chains: a dense frame of five sub-frames before and after
    yy, xx = np.mgrid[0:h, 0:w]
    counts = ((xx + 2 * yy) % 5).astype(np.uint8)
    p = sv.params(w, h)
    _differences(c.render(p), expected(w, h), "RT_PARTS=5 frame before the count list", found)
    _differences(c.render_counts(p, counts), contexts().render_counts(p, counts), "RT_PARTS=5 render_counts against the default context", found)
    _differences(c.render(p), expected(w, h), "RT_PARTS=5 frame after the count list", found)
    _report(found)
