"""The model of point lights with a radius (tests/soft_lights_model.py) held to what exists, and the direction rule over what the RNG can return.

Radii 0: the walker is lights_model.Walker bit for bit (the cat with num_bounce 3, the ten-sphere scene with num_bounce 5, 64 x 48, ray counts included).
Direct light: one segment, three lights of radii 0, 2 and 5 -- every pixel is the ORACLE's pixel with its single light at that pixel's L' and at the intensity of all.

The direction.  r1 = m 2^-24, m = 1 .. 2^24, are all values of uniform01; z = 1 - 2 r1 is exact (a multiple of 2^-23 of magnitude <= 1), reaches -1 at m = 2^24 and stays
below 1; z z is rounded once and is <= 1, so 1 - z z >= 0.
The moments, over the lattice r1 = i / n, r2 = j / n, i, j = 1 .. n, n = 1024 (spacing h = 1 / n), in exact arithmetic:
    E z = 1 - 2 E r1 = -1 / n = -h;            E z^2 = 1/3 + 2 h^2 / 3;
    sum_j cos(2 pi j / n) = sum_j sin = sum_j cos sin = 0 and sum_j cos^2 = sum_j sin^2 = n / 2, so E x = E y = E xy = E xz = E yz = 0 and
    E x^2 = E y^2 = (1 - E z^2) / 2 = 1/3 - h^2 / 3.
Rounding: on this lattice z is a multiple of 2^-9, so z z and 1 - z z are exact and s is one correctly rounded square root; x and y are one rounding of a binary64 product
of magnitude <= 1.  Each component is within e = 2^-23 of its exact value (2^-24 from the root, 2^-25 from the narrowing, the rest binary64's), z exactly.  Hence
    | |w|^2 - 1 | <= 2 (|x| + |y|) e + 2 e^2 < 4 e;     first moments within h + e of 0;     second moments within h^2 + 2 e of I / 3."""
import numpy as np
import pytest

import raytracinggpu_amd as rt
from . import lights_model as lm
from . import soft_lights_model as sm

f32 = np.float32
ALL_R = 1 << 24
P_A, P_B, P_C = (-10.0, 20.0, 40.0), (15.0, 25.0, 30.0), (0.0, 35.0, 5.0)
THREE = [(P_A, 1e10), (P_B, 2e10), (P_C, 5e10)]
RADII = [0.0, 2.0, 5.0]


def _scene(oracle, oracle_cat, name):
    if name == "cat":
        return oracle.Scene.preset("cpu", oracle_cat), lm.materials(rt.scenes.spheres("cpu"), [dict(albedo=rt.scenes.CAT_ALBEDO, object_slot=6)])
    return oracle.Scene.preset("demo10"), lm.materials(rt.scenes.spheres("demo10"))


@pytest.mark.parametrize("scene,b", [("cat", 3), ("demo10", 5)])
def test_radii_zero_is_the_point_light_walker(oracle, oracle_cat, scene, b):
    W, H = 64, 48
    sc, mats = _scene(oracle, oracle_cat, scene)
    for lights in ([rt.scenes.LIGHT], THREE):
        exp = lm.Walker(sc, mats, lights)
        got = sm.Walker(sc, mats, lights, [0.0] * len(lights))
        np.testing.assert_array_equal(got.render(W, H, 1, b).view(np.uint32), exp.render(W, H, 1, b).view(np.uint32))
        assert got.picks == exp.picks and len(got.picks) > W * H // 2


def test_one_segment_is_the_oracles_pixel_for_the_light_at_the_shell_point(oracle, oracle_cat):
    W, H = 12, 8
    sc, mats = _scene(oracle, oracle_cat, "cat")
    w = sm.Walker(sc, mats, THREE, RADII)
    got = w.render(W, H, 1, 0)
    moved = 0
    for y in range(H):
        for x in range(W):
            k, Lp = w.light_point(y * W + x, 0, 0)
            assert (RADII[k] == 0) == bool((Lp == np.asarray(THREE[k][0], f32)).all())
            moved += RADII[k] > 0
            sc.set_light([float(v) for v in Lp], float(w.total))        # the oracle's single light: at L', at the intensity of all
            row = sc.render(W, H, 1, 0, rows=(y, y + 1), want_rgb8=False)[0]
            np.testing.assert_array_equal(got[y, x].view(np.uint32), row[0, x].view(np.uint32), err_msg=f"pixel ({x}, {y}) light {k}")
    assert moved > W * H // 2 and (got[..., :3] > 0).any()
    ks = {p[3] for p in w.picks}
    assert ks == {0, 1, 2}                                              # every radius of the list decided some pixel


def test_z_reaches_minus_one_never_one_and_the_root_is_real():
    lo, hi = f32(np.inf), f32(-np.inf)
    for c0 in range(0, ALL_R, 1 << 21):
        r1 = (np.arange(c0 + 1, c0 + (1 << 21) + 1, dtype=np.float64) * 2.0 ** -24).astype(f32)   # exact: m <= 2^24
        z = (f32(1) - (f32(2) * r1).astype(f32)).astype(f32)
        assert (z.astype(np.float64) == 1.0 - 2.0 * r1.astype(np.float64)).all(), "z is exact"
        arg = (f32(1) - (z * z).astype(f32)).astype(f32)
        assert (arg >= 0).all()
        lo, hi = min(lo, z.min()), max(hi, z.max())
    assert lo == f32(-1) and hi == f32(1) - f32(2.0 ** -23)
    x, y, z = sm.direction(f32(1), f32(0.25))                          # r1 = 1: the south pole, whatever r2
    assert z == -1 and x == 0 and y == 0


def test_moments_of_the_direction_over_a_lattice():
    n = 1024
    h, e = 1.0 / n, 2.0 ** -23
    r = (np.arange(1, n + 1, dtype=np.float64) / n).astype(f32)         # exact
    r1, r2 = np.meshgrid(r, r, indexing="ij")
    x, y, z = (c.astype(np.float64) for c in sm.direction(r1, r2))
    n2 = x * x + y * y + z * z
    print(f"| |w|^2 - 1 | <= {np.abs(n2 - 1).max():.3g} (bound {4 * e:.3g})")
    assert np.abs(n2 - 1).max() < 4 * e
    first = np.array([x.mean(), y.mean(), z.mean()])
    second = np.array([[(a * b).mean() for b in (x, y, z)] for a in (x, y, z)])
    print("first moments", first, "bound", h + e)
    print("second moments - I/3", (second - np.eye(3) / 3).ravel(), "bound", h * h + 2 * e)
    assert np.abs(first).max() <= h + e
    assert np.abs(second - np.eye(3) / 3).max() <= h * h + 2 * e


# ---- one occluder above a floor: umbra, lit, penumbra --------------------------------------------------------------------------------------------------------------------------

FLOOR, BALL = ((0.0, -1010.0, 0.0), 1000.0, (0.5, 0.5, 0.5)), ((0.0, -4.0, 0.0), 4.0, (0.5, 0.5, 0.5))
LAMP, RHO = ((0.0, 15.0, 0.0), 3e10), 3.0


def _classify(P, N):
    """-> 'umbra' / 'lit' / None for a floor point, from the cones of the ball and of the shell about P, each with a margin of 1e-3 rad and 1e-2 units (the shadow ray
    leaves P + eps N, eps = 1e-3, at distances above 5: its direction differs from P's by less than 1e-3 rad)"""
    P, N = P.astype(np.float64), N.astype(np.float64)
    C, Q, R = np.array(LAMP[0]), np.array(BALL[0]), BALL[1]
    dC, dQ = np.linalg.norm(C - P), np.linalg.norm(Q - P)
    al, ao = np.arcsin(RHO / dC), np.arcsin(R / dQ)
    a = np.arccos(np.clip(np.dot(C - P, Q - P) / (dC * dQ), -1, 1))
    m = 1e-3
    if a + al < ao - m and dQ + R < dC - RHO - 1e-2:
        return "umbra"                                                  # every direction to the shell meets the ball, and meets it before the shell
    if a - al > ao + m and np.dot(N, C - P) > RHO + 1e-2:
        return "lit"                                                    # no direction to the shell meets the ball, and the whole shell is above the floor's tangent plane
    return None


def test_umbra_is_dark_lit_is_lit_and_a_penumbra_pixel_is_both(oracle):
    W, H, SPP = 48, 32, 16
    sc = oracle.Scene()
    for c, r, a in (FLOOR, BALL):
        sc.add_sphere(c, r, a)
    w = sm.Walker(sc, lm.materials([FLOOR, BALL]), [LAMP], [RHO])
    cam = np.asarray((0, 0, 55), f32)
    n = dict(umbra=0, lit=0, mixed=0)
    for i in range(H // 2, H):
        for j in range(W // 4, 3 * W // 4):
            u0 = sm.camera_dir(W, H, i, j)
            hit, oid, P, N = sc.intersect_all(cam, u0)
            if not hit or oid != 0:
                continue
            cls = _classify(P, N)
            lit = [bool((w.path(cam, u0, 1, i * W + j, s)[0] > 0).all()) for s in range(SPP)]
            if cls == "umbra":
                assert not any(lit), (i, j)
                n["umbra"] += 1
            elif cls == "lit":
                assert all(lit), (i, j)
                n["lit"] += 1
            elif any(lit) and not all(lit):
                n["mixed"] += 1
    print(n)
    assert n["umbra"] >= 3 and n["lit"] >= 50 and n["mixed"] >= 3
