"""The reference models of rt_temporal_accumulate_fast and rt_history_rectify (tests/rectify_model.py) without a GPU:

  * the vectorised model equals a scalar, pixel-by-pixel reading of the header on every synthetic case;
  * reach: from stats=, the cases tests/test_gpu_rectify.py sends to the device take every branch of the clamp at no fewer than 200 pixels, and windows are clipped on
    all four sides and in the corners;
  * the history planes of the fast accumulation are temporal_model.accumulate's bits on section 5.8's synthetic cases;
  * mutants: every listed wrong reading of the header changes the bits of the 96 x 64 case;
  * quality: the rows of DESIGN.md section 5.12 that chose RECTIFY_DEFAULTS, at test size, and the strict orderings that were found."""
import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi
from . import denoise_model as dm
from . import rectify_fixtures as rf
from . import rectify_model as rm
from . import svgf_model as sm
from . import synthetic_planes as sp
from . import temporal_model as tm
from .test_svgf_model import K, _albedos, _rmse, differ, moving_sequence, same_bits, static_sequence

F = np.float32
SMALL = (96, 64)


# ---------------------------------------------------------------- the header, read pixel by pixel ----------------------------------------------------------------
@pytest.mark.parametrize("radius,k_clamp,nonfinite", [(1, 4.0, False), (2, 0.0, False), (3, 4.0, False), (2, 4.0, True), (1, 0.0, True)])
def test_rectify_model_equals_a_scalar_reading_of_the_header(radius, k_clamp, nonfinite):
    p = rf.rectify_case(*SMALL, nonfinite=nonfinite)
    same_bits(rm.rectify(p["history"], p["fast"], p["aov"], radius, k_clamp), rm.scalar_rectify(p["history"], p["fast"], p["aov"], radius, k_clamp), f"radius {radius}")


@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (65, 1)])
def test_rectify_model_equals_the_scalar_reading_where_every_window_is_clipped(w, h):
    p = rf.rectify_case(w, h)
    for radius in (1, 2, 3):
        same_bits(rm.rectify(p["history"], p["fast"], p["aov"], radius, 4.0), rm.scalar_rectify(p["history"], p["fast"], p["aov"], radius, 4.0), f"{w} x {h}")


def _pixels_of_the_large_case(ids, W, H, n=260):
    rng = np.random.default_rng(8)
    edge = [(x, y) for x in (0, 1, 2, W - 3, W - 2, W - 1) for y in (0, 1, 2, H // 2, H - 3, H - 2, H - 1)] + [(W // 2 + d, y) for d in (-2, -1, 0, 1) for y in range(3, H, 37)]
    return sorted(set(edge + [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(n)]))


def test_rectify_model_equals_the_scalar_reading_at_pixels_of_the_large_case():
    W, H = rf.SIZES[1]
    p = rf.rectify_case(W, H, nonfinite=True)
    px = _pixels_of_the_large_case(p["ids"], W, H)
    for radius, k in ((1, 0.0), (3, 4.0)):
        v, s = rm.rectify(p["history"], p["fast"], p["aov"], radius, k), rm.scalar_rectify(p["history"], p["fast"], p["aov"], radius, k, pixels=px)
        ys, xs = [y for _, y in px], [x for x, _ in px]
        same_bits(v[:, ys, xs], s[:, ys, xs], f"radius {radius}")


def _fast_case(name):
    build, kw, finite = sp.temporal_gpu_cases(rt.make_pose)[name]
    c = build()
    return c, kw(c), finite


@pytest.mark.parametrize("name", ["96x64:movers", "96x64:masked", "96x64:alpha_min=0.4", "96x64:max_history=2", "96x64:nonfinite_history"])
def test_fast_model_equals_a_scalar_reading_of_the_header(name):
    c, kw, _ = _fast_case(name)
    pf = rf.previous_fast(c)
    for fh in (1, 4):
        h, f = rm.accumulate_fast(c["color"], c["aov"], c["prev_aov"], c["prev_history"], pf, fast_history=fh, **kw)
        hs, fs = rm.scalar_accumulate_fast(c["color"], c["aov"], c["prev_aov"], c["prev_history"], pf, fast_history=fh, **kw)
        same_bits(h, hs, name)
        same_bits(f, fs, name + ": the fast plane")
    h, f = rm.accumulate_fast(c["color"], c["aov"], **{k: v for k, v in kw.items() if k in ("max_history", "alpha_min")})       # a first frame
    hs, fs = rm.scalar_accumulate_fast(c["color"], c["aov"], **{k: v for k, v in kw.items() if k in ("max_history", "alpha_min")})
    same_bits(f, fs)
    assert (f[..., 3] == (c["aov"][0, ..., 3] != -1)).all() and (f[..., :3] == c["color"][..., :3]).all()


# ---------------------------------------------------------------- reach ----------------------------------------------------------------
@pytest.mark.parametrize("w,h", rf.SIZES)
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_the_gpu_inputs_reach_every_branch_of_the_clamp(w, h, radius):
    p = rf.rectify_case(w, h)
    st = {}
    out = rm.rectify(p["history"], p["fast"], p["aov"], radius, 4.0, stats=st)
    print(st)
    assert np.isfinite(out).all()
    for name in rf.MINIMUMS:
        assert st[name] >= rf.REACH_MINIMUM, (name, st)
    for name in rf.EDGES:
        assert st[name] >= (1 if name.startswith("corner") else 20), (name, st)
    n, nf = p["history"][1, ..., 2], p["fast"][..., 3]
    hit = p["ids"] != -1
    for length in (rf.N_F, rf.N_F + 1, 32.0):                          # n equal to, one more than and far above n_f
        assert ((n == length) & (nf == rf.N_F) & hit).sum() >= rf.REACH_MINIMUM
    assert sorted(np.unique(p["ids"])) == [-1] + list(range(16))
    st0 = {}
    rm.rectify(p["history"], p["fast"], p["aov"], radius, 0.0, stats=st0)     # the band is a point: every window that runs moves its pixel
    assert st0["unmoved"] <= 2 and st0["moved_3"] >= rf.REACH_MINIMUM


def test_the_nonfinite_case_stays_under_the_cap_and_spreads_as_the_header_says():
    for w, h in rf.SIZES:
        p, clean = rf.rectify_case(w, h, nonfinite=True), rf.rectify_case(w, h)
        planted = sum(int((~np.isfinite(p[k])).sum()) for k in ("history", "fast"))
        assert 20 <= planted < sp.NAN_CHANNEL_CAP * p["fast"].size
        out, ref = rm.rectify(p["history"], p["fast"], p["aov"], 2, 4.0), rm.rectify(clean["history"], clean["fast"], clean["aov"], 2, 4.0)
        assert 0 < np.isnan(out).sum() < sp.NAN_CHANNEL_CAP * out.size
        changed = ((out.view(np.uint32) != ref.view(np.uint32))).any(axis=(0, 3))
        near = np.zeros_like(changed)
        for y, x in zip(*np.nonzero((~np.isfinite(p["history"])).any(axis=(0, 3)) | (~np.isfinite(p["fast"])).any(-1))):
            near[max(y - 2, 0):y + 3, max(x - 2, 0):x + 3] = True
        assert changed.any() and not (changed & ~near).any()            # nothing beyond the windows that hold a planted value
        # a NaN colour in the long history is replaced by lo; an Inf in the fast plane is clamped to by the pixels whose window holds it
        nan_h = np.isnan(p["history"][0, ..., :3]) & (p["history"][1, ..., 2] > p["fast"][..., 3])[..., None] & (p["ids"] != -1)[..., None]
        assert nan_h.any() and not np.isnan(out[0, ..., :3][nan_h]).any()
        assert np.isinf(out[0, ..., :3]).sum() > np.isinf(p["history"][0, ..., :3]).sum()


# ---------------------------------------------------------------- the long history is untouched ----------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sp.temporal_gpu_cases(rt.make_pose)))
def test_fast_accumulation_writes_the_history_of_accumulate(name):
    c, kw, _ = _fast_case(name)
    if "prev_aov" not in c:
        pytest.fail("every case of section 5.8 has a previous frame")
    pf = rf.previous_fast(c)
    st = {}
    h, f = rm.accumulate_fast(c["color"], c["aov"], c["prev_aov"], c["prev_history"], pf, fast_history=4, stats=st, **kw)
    same_bits(h, tm.accumulate(c["color"], c["aov"], c["prev_aov"], c["prev_history"], **kw), name)
    hit = c["aov"][0, ..., 3] != -1
    assert (f[..., 3][~hit] == 0).all() and (f[..., 3][hit] >= 1).all() and (f[..., 3] <= 4).all()
    if name.endswith("movers"):                                        # taps accepted with a short and with a long fast history, and no tap at all
        assert ((f[..., 3] == 4) & hit).sum() >= rf.REACH_MINIMUM and ((f[..., 3] > 1) & (f[..., 3] < 4)).sum() >= rf.REACH_MINIMUM and (f[..., 3] == 1)[hit].sum() >= rf.REACH_MINIMUM


# ---------------------------------------------------------------- mutants ----------------------------------------------------------------
@pytest.mark.parametrize("mutant", rm.RECTIFY_MUTANTS)
def test_each_rectify_mutant_changes_the_synthetic_case(mutant):
    p = rf.rectify_case(*SMALL)
    ok, bad = (rm.scalar_rectify(p["history"], p["fast"], p["aov"], 2, 4.0, mutant=m) for m in (None, mutant))
    assert differ(ok, bad), mutant
    if mutant in ("n_kept", "moments_kept"):                            # faults of plane 1 alone
        assert not differ(ok[0], bad[0])


@pytest.mark.parametrize("mutant", rm.FAST_MUTANTS)
def test_each_fast_mutant_changes_the_synthetic_case(mutant):
    c, kw, _ = _fast_case("96x64:movers")
    pf = rf.previous_fast(c)
    (h, f), (hm, fm) = (rm.scalar_accumulate_fast(c["color"], c["aov"], c["prev_aov"], c["prev_history"], pf, fast_history=4, mutant=m, **kw) for m in (None, mutant))
    assert differ(f, fm) and not differ(h, hm), mutant


# ---------------------------------------------------------------- quality ----------------------------------------------------------------
W = H = 128
LIGHT_STEP = (2.5, 0.04)                                               # rt_light_orbit's angular speed and dt: 0.1 rad a frame
BASE_ROWS = {"nothing": dict(), "alpha_min 0.2": dict(alpha_min=0.2), "alpha_min 0.5": dict(alpha_min=0.5)}
SCAN_FAST, SCAN_RADIUS, SCAN_K = (2, 4, 8), (1, 2, 3), (1.0, 2.0, 4.0)


def moving_light_sequence(oracle, oracle_cat, scene, n=16, still=8):
    """The scene with its light still for frames 0 .. still - 1 and then stepped once a frame by rt_light_orbit's rule (oracle.Scene.set_light); one-sample frames with a
    new seed each and a 256-sample reference of every frame's own light.  Nothing moves but the light: one set of planes, no motion table."""
    sc = oracle.Scene.preset(scene, oracle_cat if scene == "cpu" else None)
    aov = dm.oracle_aov(sc, _albedos(scene), W, H)
    light = rt.scenes.LIGHT
    frames, refs = [], []
    for i in range(n):
        if i >= still:
            light = rt.light_orbit(light, *LIGHT_STEP)
            sc.set_light(*light)
        frames.append(sc.render(W, H, 1, 3, want_rgb8=False, seed=3000 + i)[0])
        refs.append(sc.render(W, H, 256, 3, want_rgb8=False, seed=99)[0] if i >= still or i == 0 else refs[0])
    return frames, [aov] * n, [None] * n, refs


def sequence(oracle, oracle_cat, name):
    """"light:cpu", "light:demo10", "moving", "static:cpu", "static:demo10" -> (frames, planes, motions, one reference per frame)"""
    kind, _, scene = name.partition(":")
    if kind == "light":
        return moving_light_sequence(oracle, oracle_cat, scene)
    frames, planes, motions, ref = moving_sequence(oracle) if kind == "moving" else static_sequence(oracle, oracle_cat, scene)
    return frames, planes, motions, [ref] * len(frames)


def errors(oracle, seq, alpha_min=0.0, fast_history=None, radius=None, k_clamp=None):
    """The chain accumulate -> (rectify) -> svgf_filter with SVGF_DEFAULTS over a sequence -> every frame's RMSE against its reference.  fast_history None: no
    rectification."""
    frames, planes, motions, refs = seq
    d = _capi.SVGF_DEFAULTS
    out, prev, prev_fast = [], None, None
    for i, f in enumerate(frames):
        kw = dict(alpha_min=alpha_min, motion=motions[i] if prev is not None else None)
        pa = None if prev is None else planes[i - 1]
        if fast_history is None:
            hist = tm.accumulate(f, planes[i], pa, prev, **kw)
        else:
            hist, prev_fast = rm.accumulate_fast(f, planes[i], pa, prev, prev_fast, fast_history=fast_history, **kw)
            hist = rm.rectify(hist, prev_fast, planes[i], radius, k_clamp)
        prev = hist
        out.append(_rmse(oracle, sm.svgf_filter(hist, planes[i], d["n_passes"], -1, d["prefilter"], *K)[0], refs[i]))
    return out


DEFAULT_ROW = dict(fast_history=_capi.FAST_HISTORY_DEFAULT, **_capi.RECTIFY_DEFAULTS)
TEST_ROWS = dict(BASE_ROWS, **{"default": DEFAULT_ROW, "h2 r1 k1": dict(fast_history=2, radius=1, k_clamp=1.0)})
NEIGHBOURS = {"h4 r1 k2": dict(fast_history=4, radius=1, k_clamp=2.0), "h4 r2 k1": dict(fast_history=4, radius=2, k_clamp=1.0)}
# What the scan of DESIGN.md section 5.12 showed, strictly, best first (RMSE; light: the mean over frames 8 - 15, the others: after frame 8; "default" = h4 r1 k1):
#   light, cat scene     alpha_min 0.5 0.03271 < h2 r1 k1 0.04363 < alpha_min 0.2 0.04629 < default 0.05019 < h4 r2 k1 0.05292 < h4 r1 k2 0.05547 < nothing 0.05880
#   light, sphere scene  alpha_min 0.5 0.05993 < alpha_min 0.2 0.06745 < default 0.06896 < h2 r1 k1 0.06934 < h4 r2 k1 0.07007, h4 r1 k2 0.07010 < nothing 0.07113
#   moving sphere        alpha_min 0.5 0.02277 < h2 r1 k1 0.02598 < alpha_min 0.2 0.02667 < default 0.02719 < nothing 0.02837
#   static, cat scene    nothing 0.02360 < alpha_min 0.2 0.02380 < default 0.02509 < alpha_min 0.5 0.02621 < h2 r1 k1 0.02750
#   static, sphere scene alpha_min 0.5 0.05605 < default 0.05898 < nothing 0.05941 < h2 r1 k1 0.06054
# No row of the scan beats alpha_min = 0.5 where the light moves: at one sample per pixel the fast history's own noise makes the band wider than the lag (section 5.12).
# So SvgfSequence keeps rectification off and nothing recommends it; RECTIFY_DEFAULTS is the best (radius, k_clamp) on both light sequences at fast_history 4 and at 2.
ORDER = {"light:cpu": ("alpha_min 0.5", "h2 r1 k1", "alpha_min 0.2", "default", "h4 r2 k1", "h4 r1 k2", "nothing"),
         "light:demo10": ("alpha_min 0.5", "alpha_min 0.2", "default", "h2 r1 k1", "h4 r2 k1", "nothing"),
         "moving": ("alpha_min 0.5", "h2 r1 k1", "alpha_min 0.2", "default", "nothing"),
         "static:cpu": ("nothing", "alpha_min 0.2", "default", "alpha_min 0.5", "h2 r1 k1"),
         "static:demo10": ("alpha_min 0.5", "default", "nothing", "h2 r1 k1")}
EXTRA = {"light:demo10": [("default", "h4 r1 k2"), ("h4 r1 k2", "nothing")]}


def _figure(name, e):
    return sum(e[8:]) / len(e[8:]) if name.startswith("light") else e[-1]


@pytest.mark.parametrize("name", list(ORDER))
def test_quality_orderings(oracle, oracle_cat, name):
    """DESIGN.md section 5.12 at test size, by section 5.8's protocol: 128 x 128, b = 3, one-sample frames with a new seed each through accumulate -> (rectify) ->
    svgf_filter with the defaults, RMSE in the tonemap's [0, 1] scale against a 256-sample frame of the frame's own scene.  The orderings asserted are exactly the ones
    measured (see ORDER); the figures are printed."""
    seq = sequence(oracle, oracle_cat, name)
    rows = dict(TEST_ROWS, **(NEIGHBOURS if name.startswith("light") else {}))
    res = {row: errors(oracle, seq, **kw) for row, kw in rows.items()}
    for row, e in res.items():
        print(f"{name}: {row:14s} {_figure(name, e):.5f}   per frame " + " ".join(f"{v:.5f}" for v in e))
    fig = {row: _figure(name, e) for row, e in res.items()}
    o = ORDER[name]
    for better, worse in list(zip(o[:-1], o[1:])) + EXTRA.get(name, []):
        assert fig[better] < fig[worse], (name, better, worse, fig)
    if name.startswith("light"):                                       # before the light moves every row is within a few percent of the chain as it is
        for row, e in res.items():
            if row.startswith(("default", "h4")):
                assert e[7] < 1.1 * res["nothing"][7], (row, e[7], res["nothing"][7])


def test_the_defaults_are_the_chosen_row_and_the_sequence_keeps_it_off():
    import inspect
    assert _capi.RECTIFY_DEFAULTS == dict(radius=1, k_clamp=1.0) and _capi.FAST_HISTORY_DEFAULT == 4
    for name in ("light:cpu", "light:demo10"):                         # the best (radius, k_clamp) at the default fast history where the light moves ...
        o = ORDER[name]
        assert all(o.index("default") < o.index(n) for n in NEIGHBOURS if n in o)
        assert o[0] == "alpha_min 0.5" and o[-1] == "nothing"          # ... which gains on the chain as it is and loses to a raised alpha_min
    assert inspect.signature(rt.SvgfSequence.__init__).parameters["rectify"].default is None
