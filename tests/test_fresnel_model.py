"""The model of the Fresnel dielectrics (tests/fresnel_model.py) held to the mathematics, without a GPU: R against a binary64 evaluation of the same equations, its range,
its closed forms at normal and grazing incidence, the share of the draws that reflect, and the walker against the walker underneath."""
import numpy as np
import pytest

import raytracinggpu_amd as rt
from . import fresnel_model as fz
from . import lights_model as lm
from . import soft_lights_model as slm
from .sky_sample_model import sample_key

f32 = np.float32
PAIRS = [(1.0, 1.5), (1.5, 1.0), (1.0, 1.3), (1.3, 1.0), (1.5, 1.3), (1.0, 2.4), (2.4, 1.0)]


def _cosines(n=20001):
    """a grid of cosines in (0, 1], dense towards grazing incidence, both signs of un"""
    c = np.concatenate([np.linspace(1e-4, 1.0, n), np.geomspace(1e-6, 1e-2, 2001)]).astype(f32)
    return np.concatenate([c, -c])


def _exact(n1, n2, un):
    n1, n2 = float(f32(n1)), float(f32(n2))
    ci = np.abs(np.asarray(un, np.float64))
    k = (n1 / n2) ** 2 * (1 - ci * ci)
    ct = np.sqrt(np.where(k <= 1, 1 - k, np.nan))
    rs = (n1 * ci - n2 * ct) / (n1 * ci + n2 * ct)
    rp = (n1 * ct - n2 * ci) / (n1 * ct + n2 * ci)
    return 0.5 * (rs * rs + rp * rp), k


@pytest.mark.parametrize("n1,n2", PAIRS)
def test_r_agrees_with_binary64_and_lies_in_the_unit_interval(n1, n2):
    un = _cosines()
    R = fz.reflectance(f32(n1), f32(n2), un)
    exact, k = _exact(n1, n2, un)
    # The grid keeps off the critical angle of the dense-to-thin pairs, where 1 - k cancels: k carries four roundings (2.4e-7), so ct = sqrt(1 - k) is off by
    # 1.2e-7 / sqrt(1 - k) and R, whose rs and rp each move by 2 (n2 / (n1 ci)) dct there, by about 1e-6 (n2 / (n1 ci)) / sqrt(1 - k) relative: 1e-5 needs
    # sqrt(1 - k) >= 0.2 at n2 / (n1 ci) = 1.7 (1.5 -> 1.3 at its critical angle, the worst of the pairs), so the grid holds the cosines with 1 - k >= 0.05.
    # From the thin side k <= (n1 / n2)^2 and every cosine stays
    safe = k <= 1 - 0.05
    assert safe.sum() > 3000 and (n1 > n2 or safe.all())
    assert np.all(np.abs(R[safe].astype(np.float64) - exact[safe]) <= 1e-5 * exact[safe])
    k32 = ((f32(n1) / f32(n2)) * (f32(n1) / f32(n2))).astype(f32) * (f32(1) - (un * un).astype(f32)).astype(f32)
    inside = k32 <= 1                                                   # outside total reflection, as binary32 sees it
    assert not np.isnan(R[inside]).any()
    assert R[inside].min() >= 0 and R[inside].max() <= 1
    assert R.dtype == f32


@pytest.mark.parametrize("n1,n2", PAIRS)
def test_normal_incidence_is_the_closed_form(n1, n2):
    want = ((n1 - n2) / (n1 + n2)) ** 2
    for un in (1.0, -1.0):
        assert abs(float(fz.reflectance(f32(n1), f32(n2), f32(un))) - want) <= 1e-6


def test_the_values_the_header_names():
    assert fz.reflectance(f32(1), f32(1.5), f32(-1)).view(np.uint32) == 0x3D23D70B
    assert fz.reflectance(f32(1.5), f32(1), f32(1)).view(np.uint32) == 0x3D23D70B
    assert abs(float(fz.reflectance(f32(1), f32(2.4), f32(1))) - 0.16955018) < 1e-7


@pytest.mark.parametrize("n1,n2", [p for p in PAIRS if p[0] < p[1]])
def test_r_is_one_at_grazing_incidence_from_the_thin_side(n1, n2):
    assert fz.reflectance(f32(n1), f32(n2), f32(0)) == f32(1)
    assert fz.reflectance(f32(n1), f32(n2), f32(-0.0)) == f32(1)


def test_a_nan_r_refracts_and_total_reflection_forms_none():
    P, N = np.zeros((3, 3), f32), np.tile(np.array([0, 0, 1], f32), (3, 1))
    u = np.array([[0.8, 0, -0.6], [0.8, 0, 0.6], [0.8, 0, 0.6]], f32)
    # item 0: from outside, ordinary; item 1: from inside glass 1.5 at 53 degrees: total reflection; item 2: the quirk -- a ray of index 1.3 inside an object whose
    # indices are (1.5, 1): not out2in, refr > n_out, so total reflection as well; with refr 0.9 the index test fails and the radicand is negative: NaN, refracted
    R, code, O, un, after = fz.step(f32(1.5), f32(1), np.array([1, 1.5, 0.9], f32), f32(1e-3), P, N, u, np.array([1, 2, 3], np.uint32), 0)
    assert code[1] == fz.TOTAL and R[1] == 0 and after[1] == f32(1.5) and O[1, 2] < 0
    assert np.isnan(R[2]) and code[2] == fz.REFRACTED and after[2] == f32(1)
    assert 0 < R[0] < 1 and code[0] in (fz.REFRACTED, fz.REFLECTED)


@pytest.mark.parametrize("n_in,n_out,refr,cos", [(1.5, 1.0, 1.0, 1.0), (1.5, 1.0, 1.0, 0.2), (1.5, 1.0, 1.5, 0.9)])
def test_the_share_that_reflects_is_r_over_2_to_the_20_keys(n_in, n_out, refr, cos):
    n = 1 << 20
    s = np.sqrt(1 - cos * cos)
    out2in = refr == n_out
    u = np.array([s, 0, -cos], f32) if out2in else np.array([s, 0, cos], f32)     # from outside against the normal, from inside along it
    hs = np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(12345)
    ones = np.ones((n, 1), f32)
    R, code, *_ = fz.step(f32(n_in), f32(n_out), f32(refr), f32(1e-3), ones * np.zeros(3, f32), ones * np.array([0, 0, 1], f32), ones * u, hs, 3)
    assert (R == R[0]).all() and 0 < R[0] < 1 and not (code == fz.TOTAL).any()
    r = float(R[0])
    share = float((code == fz.REFLECTED).mean())
    assert abs(share - r) <= 5 * np.sqrt(r * (1 - r) / n), (share, r)


def _scene(oracle, spheres):
    osc = oracle.Scene()
    for s in spheres:
        osc.add_sphere(s[0], s[1], s[2], *(s[3:] if len(s) > 3 else ()))
    return osc


BALLS = [((0, -1000, 0), 990, (0.5, 0.5, 0.5)), rt.scenes.DEMO[1], rt.scenes.DEMO[2], rt.scenes.DEMO[3]]   # a diffuse floor, a mirror, a hollow glass ball


def test_without_a_flag_and_with_ineffective_flags_the_walker_is_the_walker_underneath(oracle):
    mats = lm.materials(BALLS)
    assert mats[1][1] and mats[2][2] != mats[2][3] and mats[0][2] == mats[0][3]
    base = slm.Walker(_scene(oracle, BALLS), mats, [rt.scenes.LIGHT], [0.0]).render(24, 16, 2, 3)
    for flags in ((), (0, 1)):                                          # none; the diffuse floor and the mirror
        w = fz.Walker(_scene(oracle, BALLS), mats, [rt.scenes.LIGHT], fresnel=flags)
        assert not w.flagged
        got = w.render(24, 16, 2, 3)
        np.testing.assert_array_equal(got.view(np.uint32), base.view(np.uint32))
    w = fz.Walker(_scene(oracle, BALLS), mats, [rt.scenes.LIGHT], fresnel=(0, 1, 2, 3))
    assert w.flagged == {2, 3}
    got = w.render(24, 16, 2, 3)
    assert w.reflected > 0 and (got.view(np.uint32) != base.view(np.uint32)).any()


def test_the_walkers_draw_is_the_vectorised_draw(oracle):
    from oracle import oracle_py as orc
    from .sky_sample_model import uniform01
    for pixel, samp, d in ((0, 0, 0), (1234, 3, 5), (67 * 45 - 1, 63, 15)):
        a = f32(orc.uniform(123456, pixel, samp, np.uint32(fz.D + d), 0))
        b = uniform01(np.uint32(sample_key(123456, pixel, samp)), np.uint64(fz.D + d), 0)
        assert a == b
