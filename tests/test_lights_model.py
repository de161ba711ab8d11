"""The model of several point lights (tests/lights_model.py) held to the oracle, and the pick rule over every value the RNG can return.

One light: the walker is Scene.render bit for bit -- the cat with num_bounce 3 and the ten-sphere scene (mirror, glass, a hollow sphere) with num_bounce 5, 64 x 48, ray
counts included -- before any kernel is held to the walker.

The pick: r = m * 2^-24, m = 1 .. 2^24, are ALL values of uniform01.  x = fl(r * total) is one rounding of an exact product and does not decrease with m, so the picks are
monotone in r and light k gets the r between two boundaries: B_k = #{m : fl(m 2^-24 total) <= prefix[k]}.  fl(y) <= p (p a binary32 number) holds iff y lies at or below
the midpoint above p (ties to even), so with q_k = 2^24 prefix[k] / total:  q_k - 1 < B_k <= q_k + ulp(prefix[k]) / 2 * 2^24 / total.  For normal numbers ulp(prefix[k]) <=
ulp(total) <= 2^-23 total: a boundary moves by at most ONE value of r, and a light's count lies within 2 of 2^24 (prefix[k] - prefix[k - 1]) / total.  Denormal sums have
the fixed ulp 2^-149, and the same expression gives their (much wider) bound."""
from fractions import Fraction

import numpy as np
import pytest

import raytracinggpu_amd as rt
from . import lights_model as lm

ALL_R = 1 << 24
TABLES = {
    "equal": [1.0, 1.0, 1.0, 1.0],
    "1:2:5": [1e10, 2e10, 5e10],
    "zero in front": [0.0, 3.0, 1.0],
    "zero in the middle": [3.0, 0.0, 1.0],
    "zero at the end": [3.0, 1.0, 0.0],
    "absorbed": [1e10, 1.0],
    "denormals": [2.0 ** -149, 2.0 ** -148, 5 * 2.0 ** -149],
    "sixteen": [float(k % 5) for k in range(1, 17)],
}


def test_prefix_is_the_running_binary32_sum():
    pre = lm.prefix([1e10, 1.0, 3.0])
    assert pre.dtype == np.float32 and pre.tolist() == [1e10, 1e10, 1e10]                # 1 and 3 are below half an ulp of 1e10 (1024)
    pre = lm.prefix([0.1, 0.2, 0.3])
    assert pre[1] == np.float32(np.float32(0.1) + np.float32(0.2)) and pre[2] == np.float32(pre[1] + np.float32(0.3))


@pytest.mark.parametrize("name", list(TABLES))
def test_pick_over_every_r(name):
    inten = TABLES[name]
    pre = lm.prefix(inten)
    total = Fraction(float(pre[-1]))
    counts = np.zeros(len(inten), np.int64)
    last = 0
    for c0 in range(0, ALL_R, 1 << 20):
        r = (np.arange(c0 + 1, c0 + (1 << 20) + 1, dtype=np.float64) * 2.0 ** -24).astype(np.float32)   # exact: m <= 2^24
        k = lm.pick(pre, r)
        assert (np.diff(k) >= 0).all() and k[0] >= last, "the picks are monotone in r"
        last = int(k[-1])
        counts += np.bincount(k, minlength=len(inten))
    assert counts.sum() == ALL_R
    live = [k for k in range(len(inten)) if pre[k] > 0 and (k == 0 or pre[k] != pre[k - 1])]
    for k in range(len(inten)):
        if k not in live:
            assert counts[k] == 0, f"light {k} of {name} (zero or absorbed) was picked {counts[k]} times"
    # boundaries: B_k = lights 0 .. k together
    B = np.cumsum(counts)
    normal = float(pre[-1]) >= 2.0 ** -126
    slack_prev = Fraction(0)
    for k in live:
        q = Fraction(float(pre[k])) * ALL_R / total
        up = Fraction(float(np.spacing(pre[k]))) / 2 * ALL_R / total                      # how far rounding can move the boundary up, in values of r
        assert q - 1 < int(B[k]) <= q + up, (name, k, int(B[k]), float(q), float(up))
        if normal:
            assert up <= 1 and abs(int(B[k]) - q) <= 1, "a boundary moves by at most one value of r"
        lo = Fraction(float(pre[k - 1])) if k > 0 else Fraction(0)
        want = (Fraction(float(pre[k])) - lo) * ALL_R / total
        bound = 1 + max(up, slack_prev)                                                    # B_k - q_k in (-1, up], B_(k-1) - q_(k-1) in (-1, slack_prev]
        print(f"{name}: light {k}: {int(counts[k])} picks, expected {float(want):.3f}, bound {float(bound):.3f}")
        assert abs(int(counts[k]) - want) <= bound, (name, k, int(counts[k]), float(want), float(bound))
        slack_prev = up
    assert int(B[live[-1]]) == ALL_R                                                       # x <= total: every r picks a light


def test_r_one_picks_the_last_live_light():
    for inten in TABLES.values():
        pre = lm.prefix(inten)
        k = int(lm.pick(pre, np.float32(1.0)))
        assert pre[k] == pre[-1] and (k == 0 or pre[k - 1] < pre[k])


def _cat_scene(oracle, oracle_cat):
    return oracle.Scene.preset("cpu", oracle_cat), lm.materials(rt.scenes.spheres("cpu"), [dict(albedo=rt.scenes.CAT_ALBEDO, object_slot=6)])


@pytest.mark.parametrize("scene,b", [("cat", 3), ("demo10", 5)])
def test_one_light_is_the_oracle(oracle, oracle_cat, scene, b):
    W, H = 64, 48
    if scene == "cat":
        sc, mats = _cat_scene(oracle, oracle_cat)
    else:
        sc, mats = oracle.Scene.preset("demo10"), lm.materials(rt.scenes.spheres("demo10"))
    exp, _, _ = sc.render(W, H, 1, b, want_rgb8=False)
    got = lm.Walker(sc, mats, [rt.scenes.LIGHT]).render(W, H, 1, b)
    np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32))
    assert exp[..., 3].max() > b + 1                                                       # shadow rays were counted
