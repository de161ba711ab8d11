"""The model of the rough mirrors (tests/gloss_model.py) held to the mathematics, without a GPU: the walker against the walker underneath, the facets against the GGX
distribution they are meant to sample, the range argument of the header at its extremes, and the tangent frame's two branches."""
import numpy as np
import pytest

import raytracinggpu_amd as rt
from . import gloss_model as gm
from . import lights_model as lm
from . import soft_lights_model as slm
from .sky_sample_model import uniform24

f32 = np.float32
EPS = f32(1e-3)
# The sample keys whose first draw at segment 0 (depth 2^25, key 2^27) is the least and the greatest a draw can be, found by _search below over [0, 2^21) and committed:
HS_R1_LEAST = 0x12829D                               # r1 = 2^-24
HS_R1_ONE = 0x0DAE00                                 # r1 = 1


def _search(seg, lo, hi):
    """-> (the keys in [lo, hi) whose r1 at segment seg is 2^-24, those whose r1 is 1): vectorised"""
    hs = np.arange(lo, hi, dtype=np.uint64)
    k = uniform24(hs, np.uint64(gm.D + seg), 0)
    return hs[k == 0].tolist(), hs[k == (1 << 24) - 1].tolist()


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v)).astype(f32)


def _scene(oracle, spheres):
    osc = oracle.Scene()
    for s in spheres:
        osc.add_sphere(s[0], s[1], s[2], *(s[3:] if len(s) > 3 else ()))
    return osc


BALLS = [((0, -1000, 0), 990, (0.5, 0.5, 0.5)), rt.scenes.DEMO[1], rt.scenes.DEMO[2], rt.scenes.DEMO[3]]   # a diffuse floor, a mirror, a hollow glass ball


def test_without_an_effective_roughness_the_walker_is_the_walker_underneath(oracle):
    mats = lm.materials(BALLS)
    assert mats[1][1] and mats[2][2] != mats[2][3] and not mats[2][1] and mats[0][2] == mats[0][3] and not mats[0][1]
    base = slm.Walker(_scene(oracle, BALLS), mats, [rt.scenes.LIGHT], [0.0]).render(24, 16, 2, 3)
    for rough in ({}, {0: 0.5}, {2: 0.25, 3: 1.0}, {0: 0.5, 2: 0.25}, {1: 0.0}):   # none; the diffuse floor; the glass; both; a mirror at alpha 0
        w = gm.Walker(_scene(oracle, BALLS), mats, [rt.scenes.LIGHT], rough=rough)
        assert not w.rough
        got = w.render(24, 16, 2, 3)
        np.testing.assert_array_equal(got.view(np.uint32), base.view(np.uint32))
        assert w.facets == 0
    w = gm.Walker(_scene(oracle, BALLS), mats, [rt.scenes.LIGHT], rough={0: 0.5, 1: 0.25, 2: 0.25})
    assert set(w.rough) == {1}
    got = w.render(24, 16, 2, 3)
    assert w.facets > 0 and (got.view(np.uint32) != base.view(np.uint32)).any()


def test_the_walkers_draws_are_the_vectorised_draws():
    from oracle import oracle_py as orc
    from .sky_sample_model import sample_key, uniform01
    for pixel, samp, d in ((0, 0, 0), (1234, 3, 5), (67 * 45 - 1, 63, 15)):
        for dim in (0, 1):
            a = f32(orc.uniform(123456, pixel, samp, np.uint32(gm.D + d), dim))
            b = uniform01(np.uint32(sample_key(123456, pixel, samp)), np.uint64(gm.D + d), dim)
            assert a == b
    assert (gm.D + 15) * 4 + 1 < (1 << 28) and gm.D * 4 == 1 << 27      # below Fresnel's keys, above the bounce's


NORMALS = [_unit((0.3, 0.5, 0.8)), _unit((-0.7, 0.1, 0.5)), np.array([0, 0, 1], f32), np.array([1, 0, 0], f32), _unit((0, 0.6, 0.8)), _unit((0.6, 0, -0.8))]
INCOMING = [_unit((0.2, -0.4, -0.9)), _unit((0.9, 0.1, -0.1)), _unit((-0.3, 0.2, 0.7))]   # towards the surface, grazing, from behind


@pytest.mark.parametrize("alpha", [1 / 16, 1 / 4, 1.0])
def test_facets_are_unit_keep_the_length_stay_above_and_follow_ggx(alpha):
    n = 1 << 20
    hs = np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(977)
    ones = np.ones((n, 1), f32)
    k = int(round(np.log2(1 / alpha)))
    N = NORMALS[k % len(NORMALS)]
    folded = 0
    for j, u0 in enumerate(INCOMING):
        u = (u0 * f32(1 + j)).astype(f32)                               # (the ray is not renormalised: lengths 1, 2, 3)
        h, code, O, v = gm.step(f32(alpha), EPS, ones * np.zeros(3, f32), ones * N, ones * u, hs, 3 + j)
        h64, v64, N64, u64 = h.astype(np.float64), v.astype(np.float64), N.astype(np.float64), u.astype(np.float64)
        assert np.abs(np.linalg.norm(h64, axis=1) - 1).max() <= 1e-5
        assert np.abs(np.linalg.norm(v64, axis=1) / np.linalg.norm(u64) - 1).max() <= 1e-5
        # dot(u', N) never has un's sign.  The rule tests the binary32 vn; the binary64 dot product of the same words differs from it by the roundings of three
        # products and two sums of terms below |u|, and a folded ray's component is -vn within three roundings more: 5e-7 |u| covers both
        un = float(u64 @ N64)
        assert abs(un) > 1e-3                                           # (grazing, not tangent)
        assert ((v64 @ N64) * np.sign(un)).max() <= 5e-7 * np.linalg.norm(u64)
        folded += int(code.sum())
        assert set(np.unique(code)) <= {gm.PLAIN, gm.FOLDED}
        assert (O == (np.zeros(3, f32) + (EPS * N).astype(f32)).astype(f32)).all()
        if j == 0:
            # the share of facets with tan^2 theta_h <= T is T / (alpha^2 + T): in binary64 from h and N, not from the model's c2
            cos = (h64 @ N64) / (np.linalg.norm(h64, axis=1) * np.linalg.norm(N64))
            tan2 = (1 - cos * cos) / (cos * cos)
            for T in (alpha * alpha / 3, alpha * alpha, 3 * alpha * alpha):
                want = T / (alpha * alpha + T)
                share = float((tan2 <= T).mean())
                assert abs(share - want) <= 5 * np.sqrt(want * (1 - want) / n), (alpha, T, share, want)
    assert folded > 0 or alpha < 0.1                                    # (a wide lobe at grazing incidence does fold rays back)


def test_the_committed_keys_are_what_the_search_finds():
    least, one = _search(0, 0, 1 << 21)
    assert HS_R1_LEAST in least and HS_R1_ONE in one
    r1, _ = gm.draws([HS_R1_LEAST, HS_R1_ONE], 0)
    assert r1[0] == f32(2.0 ** -24) and r1[1] == f32(1)


@pytest.mark.parametrize("alpha", [2.0 ** -12, 1.0])
def test_the_extremes_keep_c2_in_the_unit_interval_and_nothing_is_nan(alpha):
    hs = np.array([HS_R1_LEAST, HS_R1_ONE], np.uint32)
    r1, r2 = gm.draws(hs, 0)
    c2, c, s = gm.polar(f32(alpha), r1)
    assert not np.isnan(c2).any() and (c2 >= 0).all() and (c2 <= 1).all()
    assert not np.isnan(c).any() and not np.isnan(s).any()
    a2 = f32(alpha) * f32(alpha)
    den = (f32(1) + ((a2 - f32(1)).astype(f32) * r1).astype(f32)).astype(f32)
    assert (den >= (f32(1) - r1).astype(f32)).all() and (den > 0).all()  # the header's range argument
    if alpha < 1:
        assert den[1] == f32(2.0 ** -24) and c2[1] == 0                   # r1 = 1 at alpha = 2^-12: the least denominator there is
    else:
        assert (den == 1).all()                                          # alpha = 1: m = 0, c2 = 1 - r1, the cosine-weighted hemisphere
    for N in NORMALS:
        for u in INCOMING:
            h, code, O, v = gm.step(f32(alpha), EPS, np.zeros((2, 3), f32), np.tile(N, (2, 1)), np.tile(u, (2, 1)), hs, 0)
            assert not np.isnan(h).any() and not np.isnan(v).any() and not np.isnan(O).any()


def test_at_the_least_alpha_the_ray_stays_by_the_mirror_ray():
    """alpha = 2^-12: a facet is theta_h off the normal with cos^2 theta_h = c2, and the ray reflected about it is at most 2 theta_h off the mirror's.  Over the keys with
    r1 <= 1/2, c2 = (1 - r1) / (1 - r1 + a2 r1) >= 1 / (1 + a2) up to its roundings, so tan^2 theta_h <= a2 = 2^-24 and the angle is about 2^-11; the bound is taken
    from the c2 the model formed (its range over these keys), plus 1e-5 for the binary32 vectors.  (At r1 = 1 the facet is at 90 degrees whatever alpha is: c2 = 0.)"""
    n = 1 << 16
    hs = np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(31)
    hs[0] = HS_R1_LEAST
    r1, r2 = gm.draws(hs, 0)
    keep = r1 <= 0.5
    keep[0] = True
    assert keep.sum() > n // 3
    alpha = f32(2.0 ** -12)
    c2 = gm.polar(alpha, r1)[0][keep].astype(np.float64)
    assert c2.min() >= 1 / (1 + 2.0 ** -24) - 2.0 ** -23 and c2.max() <= 1
    bound = 2 * np.arctan(np.sqrt((1 - c2.min()) / c2.min())) + 1e-5
    assert bound <= 1e-3                                                # (1 - c2 <= 2^-24 + 2^-23: theta_h <= 4.3e-4, twice that and the slack)
    for N in NORMALS[:3]:
        for u in INCOMING:
            m = keep.sum()
            h, code, O, v = gm.step(alpha, EPS, np.zeros((m, 3), f32), np.tile(N, (m, 1)), np.tile(u, (m, 1)), hs[keep], 0)
            N64, u64, v64 = N.astype(np.float64), u.astype(np.float64), v.astype(np.float64)
            mirror = u64 - 2 * (u64 @ N64) * N64
            ang = np.arctan2(np.linalg.norm(np.cross(v64, mirror), axis=1), v64 @ mirror)
            plain = code == gm.PLAIN
            assert plain.mean() > 0.99                                   # (a ray within 2^-11 of grazing may fold; none of these is)
            assert ang[plain].max() <= bound, (ang[plain].max(), bound)


def test_normals_with_a_zero_component_take_the_other_tangent_branch():
    """the vectorised frame against the walker's scalar expressions, bit for bit, on both branches"""
    Ns = [_unit((0.3, 0.5, 0.8)), _unit((0, 0.6, 0.8)), _unit((0.6, 0, -0.8)), np.array([0, 0, 1], f32), np.array([1, 0, 0], f32), np.array([0, 0, -1], f32),
          np.array([-1, 0, 0], f32)]
    T1, T2 = gm.frame(np.stack(Ns))
    for k, N in enumerate(Ns):
        first = N[1] != 0 and N[0] != 0
        assert first == (k == 0)
        t1 = lm._normalize(lm._v(-N[1], N[0], 0) if first else lm._v(-N[2], 0, N[0]))
        t2 = lm._cross(N, t1)
        np.testing.assert_array_equal(T1[k], t1)
        np.testing.assert_array_equal(T2[k], t2)
        assert abs(float(T1[k].astype(np.float64) @ N.astype(np.float64))) <= 1e-6 and abs(float(np.linalg.norm(T1[k].astype(np.float64))) - 1) <= 1e-6
        if not first:
            assert T1[k][1] == 0                                        # (-Nz, 0, Nx) / n
    h = gm.facet(f32(0.25), np.stack(Ns), np.arange(len(Ns), dtype=np.uint32) + np.uint32(5), 2)
    assert not np.isnan(h).any()
    # N = (0, 1, 0) has Nx = Nz = 0: the second branch's vector is zero and its quotient 0 / 0, in cosine_bounce as here
    assert np.isnan(gm.facet(f32(0.25), np.array([[0, 1, 0]], f32), [5], 2)).any()
