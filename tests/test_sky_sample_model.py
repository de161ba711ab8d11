"""Sky sampling without a GPU: the model of tests/sky_sample_model.py held to the mathematics it restates, before any kernel is held to it.
  the table     c(t) > 0 exactly where some tap of the texel's square can be positive; the lookup never exceeds B9; strictly increasing prefixes over the positive
                texels; the total's bound; the pick of a lattice of K against the exact quotient 2^48 prefix / total
  the weight    g c(t) / total against mx (4 / n^2) / (m r), inside a bound derived from the roundings
  unbiased      the mean of g E over 2^22 keys against a quadrature of sky_radiance cos over the sphere
  add_sun       the map it makes"""
import math

import numpy as np
import pytest

from raytracinggpu_amd import environment as envm
from . import sky_model as sky
from . import sky_sample_model as ssm

f32 = np.float32


def _sun_map(n=16):
    base = envm.gradient_sky((0.2, 0.5, 2.0), (1.5, 1.5, 1.5), (0.3, 0.2, 0.1), n)
    return envm.add_sun(base, (0.3, 0.8, -0.5), math.radians(8.0), (400.0, 380.0, 300.0))


def _sparse_map(n, seed):
    rng = np.random.default_rng(seed)
    env = np.zeros((n, n, 3), f32)
    ys, xs = rng.integers(0, n, 6), rng.integers(0, n, 6)
    env[ys, xs, rng.integers(0, 3, 6)] = rng.uniform(0.5, 4.0, 6).astype(f32)
    return env


def _dirs_of(n, k, rng):
    """random directions, as (w, texel the lookup's (a, b) land in)"""
    u = rng.normal(size=(k, 3)).astype(f32)
    u = (u / np.linalg.norm(u, axis=-1, keepdims=True)).astype(f32)
    a, b, ok = sky.oct_coords(u)
    assert ok.all()
    x = np.clip(np.floor(a.astype(np.float64) * n), 0, n - 1).astype(int)
    y = np.clip(np.floor(b.astype(np.float64) * n), 0, n - 1).astype(int)
    return u, y * n + x


@pytest.mark.parametrize("n", [1, 2, 5, 16])
def test_counts_are_positive_exactly_where_a_tap_can_be(n):
    for seed in range(3):
        env = _sparse_map(n, seed) if n > 1 else np.full((1, 1, 3), 0.25 * seed, f32)
        tb = ssm.Table(env)
        Y = env.sum(axis=-1) > 0
        pad = np.pad(Y, 1, mode="edge")
        near = np.zeros_like(Y)
        for dy in range(3):
            for dx in range(3):
                near |= pad[dy:dy + n, dx:dx + n]
        assert ((tb.c > 0) == near.ravel()).all()
        if tb.total == 0:
            assert not near.any()
            continue
        # the lookup of a direction is 0 where c is 0, and never exceeds B9 of the texel it lands in
        u, t = _dirs_of(n, 4096, np.random.default_rng(seed))
        E = sky.sky_radiance(env, u).astype(np.float64).sum(axis=-1)
        assert (E[tb.c[t] == 0] == 0).all()
        assert (E <= tb.B9.ravel()[t].astype(np.float64) * (1 + 2.0 ** -20)).all()


def test_an_all_zero_map_has_an_empty_table():
    tb = ssm.Table(np.zeros((5, 5, 3), f32))
    assert tb.total == 0 and not tb.c.any() and not tb.prefix.any()


def test_prefixes_rise_strictly_over_the_positive_texels():
    tb = ssm.Table(_sun_map())
    pos = tb.c > 0
    assert pos.all()                                                    # a gradient sky: no texel is dark
    assert (np.diff(tb.prefix.astype(object)) > 0).all() and int(tb.prefix[0]) == int(tb.c[0]) > 0
    assert tb.c.max() == 2 ** 31 and tb.c.min() >= 1                     # the brightest texel is the scale
    sp = ssm.Table(_sparse_map(16, 7))
    p = sp.prefix.astype(object)
    assert all((p[t] > (p[t - 1] if t else 0)) == bool(sp.c[t] > 0) for t in range(256))


def test_the_total_of_the_largest_map_fits():
    top = np.array([0x6f7fffff], np.uint32).view(f32)[0]                 # the largest texel rt_scene_set_environment accepts
    tb = ssm.Table(np.full((1024, 1024, 3), top, f32))
    assert np.isfinite(tb.W).all() and tb.c.min() >= 1
    assert 0 < tb.total <= 2 ** 51


def test_the_pick_inverts_the_prefix_to_one_k():
    tb = ssm.Table(_sun_map())
    rng = np.random.default_rng(5)
    ka = np.concatenate([[0, 0, 2 ** 24 - 1, 2 ** 24 - 1], rng.integers(0, 2 ** 24, 20000)]).astype(np.uint64)
    kb = np.concatenate([[0, 2 ** 24 - 1, 0, 2 ** 24 - 1], rng.integers(0, 2 ** 24, 20000)]).astype(np.uint64)
    t, X = tb.pick(ka, kb)                                               # (the vectorised route)
    ts, Xs = tb.pick(ka[:2000], kb[:2000])                               # (the Python integers)
    assert (t[:2000] == ts).all() and (X[:2000] == Xs).all()
    P = [0] + [int(v) for v in tb.prefix]
    for a, b, tt, xx in zip(ka.tolist(), kb.tolist(), t.tolist(), X.tolist()):
        K = (a << 24) | b
        assert 1 <= xx <= tb.total and xx == ((K * tb.total) >> 48) + 1
        assert P[tt] * 2 ** 48 <= K * tb.total < P[tt + 1] * 2 ** 48    # K lies in [2^48 prefix[t - 1] / total, 2^48 prefix[t] / total)
    # ... so the share of a lattice of K that lands on a texel is c(t) / total to within one K at either end
    assert int(t[2]) == 255 or tb.c[255] == 0 or int(t[3]) == 255


def test_the_weight_does_not_depend_on_the_table():
    """g c(t) / total == mx (4 / n^2) / (m r).  g is the binary32 rounding (2^-24 relative, all values are far from the subnormals) of a binary64 expression with six
    operations (2^-53 each); the left side adds two binary64 operations, the right side four: (1 + 2^-24)(1 + 2^-53)^12 - 1 < 2^-24 + 2^-48."""
    tb = ssm.Table(_sun_map())
    hs = ssm.mix32(np.arange(1 << 14, dtype=np.uint64))
    t, w, m, r = tb.sample(hs, 1)
    mx = np.maximum(w @ np.array([0.0, 1.0, 0.0], f32), f32(0)).astype(f32)
    g = tb.weight(t, m, r, mx)
    lhs = g.astype(np.float64) * tb.c[t].astype(np.float64) / float(tb.total)
    rhs = mx.astype(np.float64) * (4.0 / (tb.n * tb.n)) / (m.astype(np.float64) * r.astype(np.float64))
    assert (mx > 0).any() and (mx == 0).any()
    assert (np.abs(lhs - rhs) <= rhs * (2.0 ** -24 + 2.0 ** -48)).all()
    assert (g[mx == 0] == 0).all()
    # the direction is a unit vector and m r^-2 is 1 up to roundings
    assert np.abs(np.linalg.norm(w.astype(np.float64), axis=-1) - 1).max() < 4 * 2.0 ** -24


def test_scalar_and_array_draws_agree():
    tb = ssm.Table(_sun_map())
    hs = ssm.mix32(np.arange(64, dtype=np.uint64) + np.uint64(99))
    d = np.arange(64) % 5
    t, w, m, r = tb.sample(hs, d)
    for k in range(64):
        t1, w1, m1, r1 = tb.sample(int(hs[k]), int(d[k]))
        assert t1[0] == t[k] and (w1[0].view(np.uint32) == w[k].view(np.uint32)).all() and m1[0] == m[k] and r1[0] == r[k]


def _quadrature(env, normals, sub):
    """the integral of sky_radiance(w) max(N w, 0) over the sphere: the midpoint rule on sub x sub points per texel of the q-square, d omega = dq / |p|^3"""
    n = env.shape[0]
    c = (np.arange(n * sub, dtype=np.float64) + 0.5) / (n * sub) * 2.0 - 1.0
    qx, qz = np.meshgrid(c, c, indexing="xy")
    py = 1.0 - np.abs(qx) - np.abs(qz)
    low = py < 0
    px = np.where(low, (1.0 - np.abs(qz)) * np.where(qx < 0, -1.0, 1.0), qx)
    pz = np.where(low, (1.0 - np.abs(qx)) * np.where(qz < 0, -1.0, 1.0), qz)
    m = px * px + py * py + pz * pz
    w = np.stack([px, py, pz], axis=-1) / np.sqrt(m)[..., None]
    E = sky.sky_radiance(env, w.astype(f32)).astype(np.float64)
    dom = (2.0 / (n * sub)) ** 2 / m ** 1.5
    return np.array([(E * (np.maximum(w @ N, 0.0) * dom)[..., None]).sum(axis=(0, 1)) for N in normals])


def test_the_estimate_is_unbiased():
    env = _sun_map()
    tb = ssm.Table(env)
    normals = np.array([[0.0, 1.0, 0.0], [0.6, 0.0, -0.8], [-0.48, -0.6, 0.64]])
    I8, I16 = _quadrature(env, normals, 8), _quadrature(env, normals, 16)
    qerr = np.abs(I8 - I16)
    count = 1 << 22
    hs = ssm.mix32(np.arange(count, dtype=np.uint64) ^ np.uint64(0x5bd1e995))
    t, w, m, r = tb.sample(hs, np.arange(count) & 3)
    E = sky.sky_radiance(env, w).astype(np.float64)
    for k, N in enumerate(normals):
        mx = np.maximum((w * N.astype(f32)).astype(f32).sum(axis=-1, dtype=f32), f32(0)).astype(f32)
        f = tb.weight(t, m, r, mx).astype(np.float64)[:, None] * E
        mean, se = f.mean(axis=0), f.std(axis=0, ddof=1) / math.sqrt(count)
        thr = 5 * se
        print(f"normal {k}: mean {mean}, quadrature {I8[k]}, five standard errors {thr}, quadrature error {qerr[k]}")
        assert (qerr[k] < se).all()                                      # the quadrature's own error is small beside one standard error
        assert (thr < 0.01 * I8[k]).all()                                # a wrong constant cannot pass
        assert (np.abs(mean - I8[k]) <= thr).all()


def test_the_solid_angles_cover_the_sphere():
    sa = envm.texel_solid_angles(1024)
    # the midpoint rule on a lattice of spacing h = 2 / 1024: second order, the integrand's second derivatives are O(10) -> well inside 1e-4 relative
    assert abs(sa.sum() - 4 * math.pi) < 1e-4 * 4 * math.pi
    ratio = sa / (4.0 / 1024 ** 2)                                       # |p|^-3: 1 at the axes, 3^1.5 where |px| = |py| = |pz|
    assert ratio.min() >= 1.0 and ratio.max() <= 3 ** 1.5 + 1e-9
    tb = ssm.Table(np.ones((64, 64, 3), f32))
    assert np.allclose(tb.m_centre.astype(np.float64) ** -1.5 * (4.0 / 64 ** 2), envm.texel_solid_angles(64), rtol=1e-5)


def test_add_sun_stamps_a_disc():
    base = envm.gradient_sky((0.2, 0.5, 2.0), (1.5, 1.5, 1.5), (0.3, 0.2, 0.1), 64)
    d = np.array([0.3, 0.8, -0.5])
    half = math.radians(6.0)
    sun = envm.add_sun(base, d, half, (100.0, 90.0, 80.0))
    assert sun.dtype == np.float32 and sun.shape == base.shape and sky.valid_map(sun)
    inside = envm.texel_directions(64).astype(np.float64) @ (d / np.linalg.norm(d)) >= math.cos(half)
    assert 4 < inside.sum() < 64 * 64 // 8
    assert (sun[~inside] == base[~inside]).all()
    assert np.allclose(sun[inside] - base[inside], (100.0, 90.0, 80.0), rtol=1e-6)
    assert (base == envm.gradient_sky((0.2, 0.5, 2.0), (1.5, 1.5, 1.5), (0.3, 0.2, 0.1), 64)).all()   # a copy: the argument stays
    # the disc's solid angle is what its texels subtend, to the lattice's resolution
    assert abs(envm.texel_solid_angles(64)[inside].sum() / (2 * math.pi * (1 - math.cos(half))) - 1) < 0.25
    # a disc smaller than a texel: the nearest texel, with the disc's energy
    tiny = math.radians(0.25)
    one = envm.add_sun(np.zeros((16, 16, 3), f32), (0.0, 1.0, 0.01), tiny, 1000.0)
    ys, xs = np.nonzero(one[..., 0])
    assert len(ys) == 1 and (one[ys[0], xs[0]] == one[ys[0], xs[0], 0]).all()
    energy = one[ys[0], xs[0], 0] * envm.texel_solid_angles(16)[ys[0], xs[0]]
    assert abs(energy / (1000.0 * 2 * math.pi * (1 - math.cos(tiny))) - 1) < 1e-5
    assert envm.texel_directions(16)[ys[0], xs[0], 1] > 0.95             # next to the zenith
    for bad in (lambda: envm.add_sun(base, (0, 0, 0), half, 1.0), lambda: envm.add_sun(base, d, 0.0, 1.0), lambda: envm.add_sun(base[:, :32], d, half, 1.0),
                lambda: envm.add_sun(base, d, half, -100.0)):
        with pytest.raises(ValueError):
            bad()


# ---- the walker ---------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_sample_key_is_the_oracles():
    from oracle import oracle_py as orc
    for seed, pixel, samp, d, dim in ((123456, 0, 0, 0, 0), (77, 3014, 3, 2, 3), (1, 96 * 64 - 1, 63, 5, 1)):
        hs = ssm.sample_key(seed, pixel, samp)
        assert ssm.uniform01(hs, d, dim)[()] == f32(orc.uniform(seed, pixel, samp, d, dim))


def test_share_0_and_an_all_zero_map_are_the_sky_walker_bit_for_bit(oracle):
    """on a mirror and a hollow glass ball over a floor, and on the ten spheres: frames and ray counts"""
    import raytracinggpu_amd as rt
    from . import lights_model as lm
    floor = ((0, -1000, 0), 990, (0.5, 0.5, 0.5))
    env = _sun_map(5)
    for spheres, b in (([floor, rt.scenes.DEMO[1], rt.scenes.DEMO[2], rt.scenes.DEMO[3]], 3), (rt.scenes.spheres("demo10"), 2)):
        osc = oracle.Scene()
        for s in spheres:
            osc.add_sphere(s[0], s[1], s[2], *(s[3:] if len(s) > 3 else ()))
        mats = lm.materials(spheres)
        lights = [rt.scenes.LIGHT]
        want = sky.Walker(osc, mats, lights, None, env=env).render(24, 16, 2, b)
        got = ssm.Walker(osc, mats, lights, None, env=env, share=0.0).render(24, 16, 2, b)
        assert (got.view(np.uint32) == want.view(np.uint32)).all()
        dark = np.zeros((5, 5, 3), f32)
        want = sky.Walker(osc, mats, lights, None, env=dark).render(24, 16, 2, b)
        for share in (0.5, 1.0):
            got = ssm.Walker(osc, mats, lights, None, env=dark, share=share).render(24, 16, 2, b)
            assert (got.view(np.uint32) == want.view(np.uint32)).all()
        lit = ssm.Walker(osc, mats, lights, None, env=env, share=0.5).render(24, 16, 2, b)       # the paths are the same: .w is
        plain = sky.Walker(osc, mats, lights, None, env=env).render(24, 16, 2, b)
        assert (lit[..., 3] == plain[..., 3]).all() and (lit[..., :3] != plain[..., :3]).any()
