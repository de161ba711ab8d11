"""The reference model of rt_upsample (tests/upsample_model.py) without a GPU:

  * a scalar, pixel-by-pixel reading of the header text gives the vectorised model's bits at a few hundred pixels (borders, seams, misses, fallback pixels), for
    f = 2, 3, 4 and one and two planes;
  * reach: the main case of tests/upsample_fixtures.py has pixels with exactly 1, 2, 3 and 4 counted taps, taps dropped for each single reason, fallback pixels --
    and not mostly fallback pixels;
  * mutants: every listed wrong reading of the header changes the bits of the main case;
  * quality: the table of DESIGN.md section 5.11 at test size, the two conditions the feature stands on (guided beats plain bilinear in every pair, full resolution
    beats every upsampled row) and the orderings that were found in it."""
import numpy as np
import pytest

from raytracinggpu_amd import _capi
from . import denoise_model as dm
from . import svgf_model as sm
from . import temporal_model as tm
from . import upsample_fixtures as uf
from . import upsample_model as um
from .test_svgf_model import H, K, W, _albedos, _rmse, differ, same_bits, static_sequence

F = np.float32
KN, KP = (float(np.float32(_capi.UPSAMPLE_DEFAULTS[n])) for n in ("k_normal", "k_position"))


def test_the_defaults_are_the_filters_own():
    assert (_capi.UPSAMPLE_DEFAULTS["k_normal"], _capi.UPSAMPLE_DEFAULTS["k_position"]) == (2.0, 0.25)
    assert all(_capi.UPSAMPLE_DEFAULTS[k] == _capi.DENOISE_VAR_DEFAULTS[k] for k in _capi.UPSAMPLE_DEFAULTS)


# ---------------------------------------------------------------- the header, read pixel by pixel ----------------------------------------------------------------
def scalar_upsample(low, low_aov, aov, f, k_normal, k_position, pixels):
    """include/raytrace_hip.h read literally for the full-resolution pixels (x, y) given: python loops, one numpy.float32 operation at a time
    -> {(x, y): [n_planes, 4]}.  low: [n_planes, h, w, 4]."""
    n_planes, h, w = low.shape[:3]
    _f = np.float32
    kn, kp = _f(k_normal), _f(k_position)
    out = {}
    with np.errstate(all="ignore"):
        for x, y in pixels:
            gx = (_f(x) + _f(0.5)) / _f(f) - _f(0.5)
            gy = (_f(y) + _f(0.5)) / _f(f) - _f(0.5)
            ix, iy = int(np.floor(gx)), int(np.floor(gy))
            fx, fy = gx - np.floor(gx), gy - np.floor(gy)
            Np, idp, Pp = aov[0, y, x, :3], aov[0, y, x, 3], aov[1, y, x, :3]
            taps = []
            for qx, qy in ((ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1)):
                bx = fx if qx == ix + 1 else _f(1) - fx
                by = fy if qy == iy + 1 else _f(1) - fy
                taps.append((qx, qy, bx * by))
            S, Wt, w0 = np.zeros((n_planes, 4), np.float32), _f(0), None

            def count(qx, qy, wt):
                nonlocal Wt, w0
                for i in range(n_planes):
                    for c in range(4):
                        S[i, c] = S[i, c] + wt * low[i, qy, qx, c]
                Wt = Wt + wt
                if w0 is None:
                    w0 = low[0, qy, qx, 3]

            for qx, qy, b in taps:
                if qx < 0 or qx >= w or qy < 0 or qy >= h or not (low_aov[0, qy, qx, 3] == idp):
                    continue
                Nq, Pq = low_aov[0, qy, qx, :3], low_aov[1, qy, qx, :3]
                dn = ((Np[0] - Nq[0]) * (Np[0] - Nq[0]) + (Np[1] - Nq[1]) * (Np[1] - Nq[1])) + (Np[2] - Nq[2]) * (Np[2] - Nq[2])
                e = (Np[0] * (Pq[0] - Pp[0]) + Np[1] * (Pq[1] - Pp[1])) + Np[2] * (Pq[2] - Pp[2])
                wn = _f(1) if kn == 0 else np.fmax(_f(0), _f(1) - dn * kn)
                wp = _f(1) if kp == 0 else np.fmax(_f(0), _f(1) - (e * e) * kp)
                wt = b * wn * wp
                if wt > 0:
                    count(qx, qy, wt)
            if Wt == 0:
                for qx, qy, b in taps:
                    if 0 <= qx < w and 0 <= qy < h:
                        count(qx, qy, b)
            o = S / Wt
            o[0, 3] = w0
            out[(x, y)] = o
    return out


@pytest.mark.parametrize("n_planes", [1, 2])
@pytest.mark.parametrize("name", ["140x40", "99x27", "140x40/4", "6x2"])
def test_model_equals_a_scalar_reading_of_the_header(name, n_planes):
    p = uf.case(name)
    Wf, Hf, f = uf.CASES[name]
    low = p["low"][:n_planes]
    st = {}
    out = um.upsample(low, p["low_aov"], p["aov"], f, KN, KP, stats=st)
    ids = p["ids"]
    rng = np.random.default_rng(11)
    edge = [(x, y) for x in (0, 1, Wf - 2, Wf - 1) for y in range(0, Hf, 3)] + [(x, y) for y in (0, 1, Hf - 2, Hf - 1) for x in range(0, Wf, 5)]
    seam = [(x, y) for y in range(Hf) for x in range(1, Wf) if ids[y, x] != ids[y, x - 1]][::5]
    fb = [(int(x), int(y)) for y, x in zip(*np.nonzero(st["fallback"]))][::2]
    miss = [(int(x), int(y)) for y, x in zip(*np.nonzero(ids == -1))][::7]
    pixels = sorted(set(edge + seam + fb + miss + [(int(rng.integers(Wf)), int(rng.integers(Hf))) for _ in range(120)]))
    if Wf >= 99:
        assert len(pixels) >= 300 and len(fb) >= 10 and len(miss) >= 5
    got = scalar_upsample(low, p["low_aov"], p["aov"], f, KN, KP, pixels)
    for (x, y), v in got.items():
        same_bits(v, out[:, y, x], f"{name}, pixel {(x, y)}")
    if n_planes == 1:                                                  # a colour frame handed over as [h, w, 4] is the same call
        same_bits(um.upsample(low[0], p["low_aov"], p["aov"], f, KN, KP), out[0])


# ---------------------------------------------------------------- reach ----------------------------------------------------------------
def test_the_main_case_reaches_every_branch():
    p = uf.case(uf.MAIN)
    st = {}
    out = um.upsample(p["low"], p["low_aov"], p["aov"], p["factor"], KN, KP, stats=st)
    counted, fallback = st["counted"], st["fallback"]
    n = {c: int((counted == c).sum()) for c in range(5)}
    print("counted taps -> pixels:", n, "fallback:", int(fallback.sum()), "of", fallback.size, "dropped alone:", st["alone"])
    for c in (1, 2, 3, 4):
        assert n[c] >= uf.COUNTED_MINIMUM, n
    for why, v in st["alone"].items():
        assert v >= uf.DROPPED_MINIMUM, st["alone"]
    assert fallback.sum() >= uf.FALLBACK_MINIMUM
    assert fallback.mean() <= uf.FALLBACK_CAP
    assert (fallback == (counted == 0)).all()
    # both sides of rt_div.h's range: sums that are zero or denormal, and sums inside [2^-60, 2^60]
    slow = ~dm.div_in_range(out).reshape(2, -1, 4).all(axis=(0, 2))
    assert slow.sum() >= 100 and (~slow).sum() >= 100
    assert np.isfinite(out).all()


@pytest.mark.parametrize("name", sorted(uf.CASES))
def test_every_case_has_its_features_printed(name):
    p = uf.case(name)
    st = {}
    um.upsample(p["low"], p["low_aov"], p["aov"], p["factor"], KN, KP, stats=st)
    print(name, {c: int((st["counted"] == c).sum()) for c in range(5)}, "fallback", int(st["fallback"].sum()), st["alone"])
    assert st["counted"].shape == p["ids"].shape


# ---------------------------------------------------------------- mutants ----------------------------------------------------------------
@pytest.mark.parametrize("mutant", um.MUTANTS)
def test_each_mutant_changes_the_main_case(mutant):
    p = uf.case(uf.MAIN)
    out = um.upsample(p["low"], p["low_aov"], p["aov"], p["factor"], KN, KP)
    out_m = um.upsample(p["low"], p["low_aov"], p["aov"], p["factor"], KN, KP, mutant=mutant)
    assert differ(out, out_m), mutant
    if mutant == "w_averaged":                                         # a fault of plane 0's .w alone
        assert not differ(out[0, ..., :3], out_m[0, ..., :3]) and not differ(out[1], out_m[1])


def test_the_order_of_bx_and_by_is_not_a_mutant():
    """b = by bx cannot be told from b = bx by: binary32 multiplication commutes.  The association of the whole product can (b_not_formed_first, above)."""
    p = uf.case(uf.MAIN)
    out = um.upsample(p["low"], p["low_aov"], p["aov"], p["factor"], KN, KP)
    assert not differ(out, um.upsample(p["low"], p["low_aov"], p["aov"], p["factor"], KN, KP, mutant="b_is_by_bx"))


def test_plain_bilinear_is_the_model_without_guides():
    """both k = 0 and the id test off: every tap inside the image counts with w = b, which is what the fallback computes"""
    p = uf.case(uf.MAIN)
    st = {}
    guided = um.upsample(p["low"], p["low_aov"], p["aov"], p["factor"], KN, KP, stats=st)
    plain = um.bilinear(p["low"], p["low_aov"], p["aov"], p["factor"])
    fb = st["fallback"]
    same_bits(guided[:, fb], plain[:, fb])
    assert differ(guided[:, ~fb], plain[:, ~fb])


# ---------------------------------------------------------------- quality ----------------------------------------------------------------
FALLBACK_CAP_RENDERED = 0.02


def low_sequence(oracle, oracle_cat, scene, f):
    """static_sequence's frames and planes at 1 / f of its size: the same seeds, the same camera"""
    sc = oracle.Scene.preset(scene, oracle_cat if scene == "cpu" else None)
    w, h = W // f, H // f
    frames = [sc.render(w, h, 1, 3, want_rgb8=False, seed=1000 + i)[0] for i in range(8)]
    return frames, dm.oracle_aov(sc, _albedos(scene), w, h)


def chain(frames, aov):
    """eight static frames through accumulate -> svgf_filter with SVGF_DEFAULTS -> (the last frame's accumulated history, its filtered frame)"""
    d = _capi.SVGF_DEFAULTS
    hist = None
    for fr in frames:
        hist = tm.accumulate(fr, aov, None if hist is None else aov, hist)
    out, _ = sm.svgf_filter(hist, aov, d["n_passes"], -1, d["prefilter"], *K)
    return hist, out


def _table(oracle, oracle_cat, scene):
    frames, planes, _, ref = static_sequence(oracle, oracle_cat, scene)
    aov = planes[0]
    d = _capi.SVGF_DEFAULTS
    res, fallback = {"full": _rmse(oracle, chain(frames, aov)[1], ref)}, {}
    for f in (2, 4):
        lf, laov = low_sequence(oracle, oracle_cat, scene, f)
        hist, out = chain(lf, laov)
        st = {}
        res[f"A{f}"] = _rmse(oracle, um.upsample(out, laov, aov, f, KN, KP, stats=st), ref)
        res[f"A{f} bilinear"] = _rmse(oracle, um.bilinear(out, laov, aov, f), ref)
        fallback[f] = float(st["fallback"].mean())
        if f == 2:
            for row, up in (("B2", um.upsample(hist, laov, aov, f, KN, KP)), ("B2 bilinear", um.bilinear(hist, laov, aov, f))):
                res[row] = _rmse(oracle, sm.svgf_filter(up, aov, d["n_passes"], -1, d["prefilter"], *K)[0], ref)
    return res, fallback


# What the table showed after frame 8, strictly, best first (RMSE; DESIGN.md section 5.11 has all of it):
#   cat scene      full 0.02360 < B2 0.03459 < A2 0.03811 < A4 0.05565 < B2 bilinear 0.07635 < A2 bilinear 0.08630 < A4 bilinear 0.11294
#   sphere scene   full 0.05941 < B2 0.08081 < B2 bilinear 0.08954 < A2 0.09139 < A2 bilinear 0.10084 < A4 0.11879 < A4 bilinear 0.13105
# On both, filtering at full resolution (B) beats upsampling the filtered frame (A), and a quarter of the rays beats a sixteenth.  On the sphere scene, whose error is in
# reflections the planes do not see (section 5.8), the guides gain least: B with plain bilinear comes in before guided A.
ORDER = {"cpu": ("full", "B2", "A2", "A4", "B2 bilinear", "A2 bilinear", "A4 bilinear"), "demo10": ("full", "B2", "B2 bilinear", "A2", "A2 bilinear", "A4", "A4 bilinear")}
ORDERINGS = {scene: list(zip(o[:-1], o[1:])) for scene, o in ORDER.items()}
PAIRS = [("A2", "A2 bilinear"), ("B2", "B2 bilinear"), ("A4", "A4 bilinear")]


@pytest.mark.parametrize("scene", ["cpu", "demo10"])
def test_quality_orderings(oracle, oracle_cat, scene):
    """DESIGN.md section 5.11 at test size, by section 5.8's protocol: 128 x 128, b = 3, eight one-sample frames, SVGF_DEFAULTS, RMSE in the tonemap's [0, 1] scale
    against the 256-sample full-resolution frame, after frame 8.  The low-resolution chains trace 64 x 64 and 32 x 32 with the same seeds."""
    res, fallback = _table(oracle, oracle_cat, scene)
    for name, e in res.items():
        print(f"{scene}: {name:12s} rmse after frame 8: {e:.5f}")
    print(f"{scene}: fallback pixels: " + ", ".join(f"f = {f}: {100 * v:.2f} %" for f, v in fallback.items()))
    for guided, plain in PAIRS:
        assert res[guided] < res[plain], (scene, guided, plain, res)
    for row, e in res.items():
        if row != "full":
            assert res["full"] < e, (scene, row, res)
    for better, worse in ORDERINGS[scene]:
        assert res[better] < res[worse], (scene, better, worse, res)
    for f, v in fallback.items():
        assert v <= FALLBACK_CAP_RENDERED, (scene, f, v)
