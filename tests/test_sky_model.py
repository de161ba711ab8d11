"""The model of the environment map (tests/sky_model.py) held to what exists, and the lookup rule held to its own wording (include/raytrace_hip.h "environment").

No map, and an all-zero map: the walker is the walker it rests on and the oracle's Scene.render bit for bit (the cat, the ten spheres, two samples, a posed row share).
The mapping: the six axes land where the rule says; on the seam |px| + |pz| = 1 both hemispheres give the same coordinates; over a lattice of directions with denormal
and huge components a and b stay in [0, 1] and every tap inside the map; zero, NaN and infinite directions meet +0.
The round trip with raytracinggpu_amd/environment.py, whose texel_directions is the inverse mapping: see test_round_trip for the bound and where it comes from."""
import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import environment as envm
from . import lights_model as lm
from . import sky_model as sky
from . import soft_lights_model as sm

f32 = np.float32
P_A, P_B, P_C = (-10.0, 20.0, 40.0), (15.0, 25.0, 30.0), (0.0, 35.0, 5.0)
THREE = [(P_A, 1e10), (P_B, 2e10), (P_C, 5e10)]


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _scene(oracle, oracle_cat, name):
    if name == "cat":
        return oracle.Scene.preset("cpu", oracle_cat), lm.materials(rt.scenes.spheres("cpu"), [dict(albedo=rt.scenes.CAT_ALBEDO, object_slot=6)])
    return oracle.Scene.preset("demo10"), lm.materials(rt.scenes.spheres("demo10"))


@pytest.mark.parametrize("scene,b,spp", [("cat", 2, 1), ("demo10", 3, 1), ("cat", 1, 2)])
def test_no_map_and_a_zero_map_are_the_walker_and_the_oracle(oracle, oracle_cat, scene, b, spp):
    W, H = 32, 24
    sc, mats = _scene(oracle, oracle_cat, scene)
    exp = sc.render(W, H, spp, b, want_rgb8=False)[0]
    assert (exp[..., :3] > 0).any() and exp[..., 3].max() > 2
    np.testing.assert_array_equal(_bits(sm.Walker(sc, mats, [rt.scenes.LIGHT], [0.0]).render(W, H, spp, b)), _bits(exp))
    for env in (None, np.zeros((1, 1, 3), f32), np.zeros((5, 5, 3), f32)):
        np.testing.assert_array_equal(_bits(sky.Walker(sc, mats, [rt.scenes.LIGHT], env=env).render(W, H, spp, b)), _bits(exp))
    for radii in (None, [0.0, 2.0, 5.0]):                             # a list, with and without radii: the walkers underneath
        under = (lm.Walker(sc, mats, THREE) if radii is None else sm.Walker(sc, mats, THREE, radii)).render(W, H, spp, b)
        np.testing.assert_array_equal(_bits(sky.Walker(sc, mats, THREE, radii, env=np.zeros((2, 2, 3), f32)).render(W, H, spp, b)), _bits(under))


def test_a_posed_row_share_without_a_map_is_the_oracle(oracle, oracle_cat):
    W, H, pose = 32, 24, (0.2, 0.1)
    sc, mats = _scene(oracle, oracle_cat, "cat")
    exp = sc.render(W, H, 2, 2, rows=(7, 13), pose=pose, fov=np.pi / 2, want_rgb8=False)[0]
    got = sky.Walker(sc, mats, [rt.scenes.LIGHT], env=np.zeros((2, 2, 3), f32), fov=np.pi / 2).render(W, H, 2, 2, pose=pose, rows=range(7, 13))
    np.testing.assert_array_equal(_bits(got), _bits(exp))
    assert (exp[..., :3] > 0).any()


def test_a_lit_map_changes_the_open_scene_and_only_through_misses(oracle):
    """one diffuse sphere under a constant sky, no light: a camera ray that misses is E, one that hits is rho E after one bounce that always escapes (the sphere is convex)"""
    sc = oracle.Scene()
    rho, E = np.array([0.5, 0.25, 1.0], f32), np.array([2.0, 3.0, 0.5], f32)
    sc.add_sphere((0, 0, 0), 10.0, tuple(rho))
    w = sky.Walker(sc, lm.materials([((0, 0, 0), 10.0, tuple(rho))]), [((0.0, 50.0, 0.0), 0.0)], env=np.broadcast_to(E, (1, 1, 3)))
    W, H = 16, 12
    for b in (0, 1, 3):
        out = w.render(W, H, 1, b)
        miss = out[..., 3] == 1
        assert miss.any() and (~miss).any()
        assert (_bits(out[miss][:, :3]) == _bits(E)).all()
        hit = f32(0) * rho / f32(lm.PI) + rho * E if b > 0 else np.zeros(3, f32)
        assert (_bits(out[~miss][:, :3]) == _bits(hit.astype(f32))).all()
        assert (out[~miss][:, 3] == (3 if b > 0 else 2)).all()           # camera ray, shadow ray, and with a bounce the ray that escapes


def test_the_six_axes():
    n = 64
    axes = np.array([(0, 1, 0), (0, -1, 0), (-1, 0, 0), (1, 0, 0), (0, 0, -1), (0, 0, 1)], f32)
    a, b, ok = sky.oct_coords(axes * f32(3.5))                        # not renormalised: the length does not matter
    assert ok.all()
    assert (a[0], b[0]) == (0.5, 0.5)                                 # +y: the centre
    assert (a[1], b[1]) == (1.0, 1.0)                                 # -y: a corner (sg(+0) = 1) ...
    for sx, sz in ((-1, -1), (-1, 1), (1, -1)):                       # ... and just off the axis the other three
        aa, bb, _ = sky.oct_coords(np.array([sx * 1e-30, -1, sz * 1e-30], f32))
        assert (aa, bb) == ((sx + 1) / 2, (sz + 1) / 2)
    assert (a[2], b[2]) == (0.0, 0.5) and (a[3], b[3]) == (1.0, 0.5)  # -x, +x: the left and right mid-edges
    assert (a[4], b[4]) == (0.5, 0.0) and (a[5], b[5]) == (0.5, 1.0)  # -z: the top mid-edge (row 0); +z: the bottom
    env = np.zeros((n, n, 3), f32)
    env[0, n // 2 - 1:n // 2 + 1] = (1, 2, 3)                         # row 0, the two texels about the middle: -z
    env[n // 2 - 1:n // 2 + 1, n - 1] = (4, 5, 6)                     # the right edge: +x
    E = sky.sky_radiance(env, axes)
    assert E[4].tolist() == [1, 2, 3] and E[3].tolist() == [4, 5, 6] and not E[[0, 1, 2, 5]].any()
    # the direction the fixed camera looks in, seen through texel_directions: row 0's middle texels point at -z and slightly down or up
    d = envm.texel_directions(n)
    assert (d[0, n // 2 - 1:n // 2 + 1, 2] < -0.99).all() and d[n // 2, n // 2, 1] > 0.99 and (d[0, 0, 1] < -0.99)


def test_the_two_hemispheres_agree_on_the_seam():
    """uy = +-0 with |px| + |pz| = 1: the fold maps the seam onto itself.  Exactly so where 1 - |pz| = |px| in binary32: components that are multiples of 2^-12 with a sum
    that is a power of two"""
    k = np.arange(0, 4097, dtype=np.float64)
    for sx in (-1, 1):
        for sz in (-1, 1):
            x, z = sx * k / 4096, sz * (4096 - k) / 4096
            up = np.stack([x, np.zeros_like(x), z], -1).astype(f32)
            a0, b0, ok0 = sky.oct_coords(up)
            lo = up.copy()
            lo[:, 1] = f32(-0.0)                                      # -0 is not < 0: the upper branch
            a1, b1, _ = sky.oct_coords(lo)
            assert (_bits(a0) == _bits(a1)).all() and (_bits(b0) == _bits(b1)).all()
            lo[:, 1] = f32(-1e-45)                                    # the smallest step below the horizon: s is unchanged, the lower branch runs
            a2, b2, ok2 = sky.oct_coords(lo * f32(8))
            assert ok0.all() and ok2.all()
            inner = (k > 0) & (k < 4096)                              # (at the ends sg(+-0) decides the corner: the axes' test)
            assert (_bits(a0)[inner] == _bits(a2)[inner]).all() and (_bits(b0)[inner] == _bits(b2)[inner]).all()


def test_coordinates_and_taps_stay_inside_over_a_lattice():
    mags = np.array([0.0, 1e-45, 1e-40, 1.1754944e-38, 1e-30, 1e-8, 0.3, 1.0, 3.0, 1e8, 1e30, 1e38, 3.4028235e38], f32)
    vals = np.concatenate([mags, -mags])
    u = np.stack(np.meshgrid(vals, vals, vals, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(9)
    u = np.concatenate([u, rng.standard_normal((200_000, 3)).astype(f32), (rng.standard_normal((50_000, 3)) * np.exp2(rng.uniform(-140, 120, (50_000, 1)))).astype(f32)])
    a, b, ok = sky.oct_coords(u)
    assert ok.sum() > 250_000 and (~ok).sum() > 100                   # overflowing 1-norms and the zero vector are in it
    assert (a >= 0).all() and (a <= 1).all() and (b >= 0).all() and (b <= 1).all()
    for n in (1, 2, 5, 64, 1024):
        nf = f32(n)
        sx = ((a * nf).astype(f32) - f32(0.5)).astype(f32)
        assert sx.min() >= -0.5 and sx.max() <= n - 0.5              # floor in [-1, n - 1]: the clamp moves a tap by one texel at the most
        xa, xb, ya, yb, fx, fy = sky.taps(a, b, n)
        for t in (xa, xb, ya, yb):
            assert t.min() >= 0 and t.max() <= n - 1
        assert (fx >= 0).all() and (fx <= 1).all() and (fy >= 0).all() and (fy <= 1).all()   # (1 itself: c - floor(c) of a tiny negative c, rounded; then gx = 0)
        E = sky.sky_radiance(np.full((n, n, 3), np.nextafter(f32(2.0 ** 96), f32(0))), u)
        assert np.isfinite(E).all() and (_bits(E) < 0x70000000).all()  # the bilinear sum of the largest map stays finite with a clear sign bit (below 2^97)


def test_zero_nan_and_infinite_directions_meet_plus_zero():
    env = np.full((5, 5, 3), 7.0, f32)
    bad = np.array([(0, 0, 0), (-0.0, 0, -0.0), (np.nan, 1, 0), (0, np.nan, 0), (1, 0, np.nan), (np.inf, 0, 0), (0, -np.inf, 1), (3e38, 3e38, 0), (np.inf, np.nan, -np.inf)], f32)
    E = sky.sky_radiance(env, bad)
    assert (_bits(E) == 0).all()
    assert (_bits(sky.sky_radiance(env, np.array([1e-45, 0, 0], f32))) == _bits(f32(7))).all()    # the smallest direction there is still has one
    assert sky.sky_radiance(env, np.array(bad[0])).shape == (3,)                                  # a scalar direction


@pytest.mark.parametrize("n", [1, 2, 5, 64])
def test_round_trip(n):
    """sky_radiance(texel_directions(n)[y, x]) of the map with texel (y, x) alone lit, at v, is v within the bilinear weight's distance from 1.
    The bound.  A texel centre has q = (2 x + 1) / n - 1; texel_directions inverts the fold in binary64 and rounds a unit vector to binary32: each component within a
    relative 2^-24.  The lookup: s is two rounded additions of such components and the quotient one more rounding, so p is within 5 * 2^-24 (|p| <= 1); the lower fold adds
    one rounding of 1 - |p|: q within 6 * 2^-24.  a = q / 2 + 1 / 2 halves that and rounds once (a <= 1): within 4 * 2^-24.  sx = a n - 1 / 2: n times that, the product's
    rounding and the difference's, each at most n 2^-24: |sx - x| <= 6 n 2^-24 =: e.  So the lit texel's weight per axis is 1 - e at the least (at a clamped border both
    taps are the lit texel and the weight is gx + fx, within 2^-23 of 1), the two axes multiply, and the five roundings of the combine add 2^-24 each:
        v (1 - e)^2 (1 - 2^-24)^5 <= E <= v (1 + 2^-23)^2 (1 + 2^-24)^5,    relaxed to  |E - v| <= v (2 e + 2^-20).
    Every other texel centre sees at most the weight e of it."""
    v = np.array([3.0, 0.5, 1.9 * 2.0 ** 95], f32)
    e = 6 * n * 2.0 ** -24
    tol = 2 * e + 2.0 ** -20
    d = envm.texel_directions(n)
    assert d.shape == (n, n, 3) and d.dtype == f32 and np.abs(np.linalg.norm(d.astype(np.float64), axis=-1) - 1).max() < 1e-6
    if n <= 5:
        cells = [(y, x) for y in range(n) for x in range(n)]
    else:
        rng = np.random.default_rng(n)
        cells = [(0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1), (0, n // 2), (n // 2, 0), (n - 1, n // 2), (n // 2, n - 1), (n // 2, n // 2), (n // 2 - 1, n // 2 - 1)]
        cells += [tuple(c) for c in rng.integers(0, n, (40, 2))]
    for y, x in cells:
        env = np.zeros((n, n, 3), f32)
        env[y, x] = v
        assert sky.valid_map(env)
        E = sky.sky_radiance(env, d).astype(np.float64)
        assert (np.abs(E[y, x] - v) <= v * tol).all(), (n, y, x, E[y, x])
        E[y, x] = 0
        assert (E <= v * e).all(), (n, y, x)


def test_from_function_of_a_constant_is_constant_and_the_makers_make_valid_maps():
    c = envm.from_function(lambda d: np.array([0.25, 1.0, 4.0]), 7)
    assert c.shape == (7, 7, 3) and c.dtype == f32 and (c == np.array([0.25, 1.0, 4.0], f32)).all() and sky.valid_map(c)
    g = envm.gradient_sky((0.1, 0.3, 1.0), (1.0, 1.0, 1.0), (0.2, 0.1, 0.0), 16)
    assert sky.valid_map(g) and np.allclose(g[8, 8], (0.1, 0.3, 1.0), atol=0.1) and np.allclose(g[0, 0], (0.2, 0.1, 0.0), atol=0.15)
    assert np.allclose(g[0, 8], (1, 1, 1), atol=0.1)                  # the top mid-edge is on the horizon
    img = np.zeros((8, 16, 3))
    img[:, 6:10] = (5.0, 0.0, 0.0)                                    # a band about the centre column: -z, pole to pole
    m = envm.from_latlong(img, 32)
    assert sky.valid_map(m) and m[0, 16, 0] > 4.0 and m[31, 16, 0] < 0.5 and m[16, 0, 0] < 0.5 and m[16, 31, 0] < 0.5
    for bad in (lambda d: -np.ones(3), lambda d: np.full(3, np.inf), lambda d: np.full(3, 2.0 ** 96)):
        with pytest.raises(ValueError):
            envm.from_function(bad, 4)
    with pytest.raises(ValueError):
        envm.texel_directions(0)
    with pytest.raises(ValueError):
        envm.texel_directions(1025)
