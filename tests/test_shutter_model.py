"""The model of the shutter (tests/shutter_model.py) held to what exists, the draw, the pose, and a streak as a known answer.

Closed shutter: with every displacement +-0 the walker is lens_model.Walker and the oracle's Scene.render bit for bit (ray counts included).

The draw.  uniform01 returns ((h >> 8) + 1) 2^-24 for a 32-bit h: m 2^-24 with m = 1 .. 2^24, so tau lies in (0, 1].  The RNG keys a draw by depth * 4 + dim modulo 2^32.
tau sits at 2^30 + 2; the lens at 2^30 + 0 and 2^30 + 1; the jitter at 2 and 3 (depth 0); the bounce of segment d at 4 d + 0 and 4 d + 1; the pick of segment d at
4 (d + 1) + 2; the shell draws of segment d at 2^31 + 4 d + 0 and + 1.  For segs <= 16 everything but the lens and the shells is below 4 (segs + 1) <= 68.

The streak (shutter_model.py ST_*).  One diffuse sphere of radius rho = 0.5 at depth 20 travels (4, 0, 0) during the exposure; 96 x 64, fov pi / 3, one segment, 64 samples.
A sample hits iff the ray through its pixel's centre passes the sphere's centre of its time tau within rho: the pixel's centre lies in the sphere's projected disc D(tau).
  Where.  D(tau) is centred on the projected centre, which runs along the row y = 0 from x0 = 0 to x1 = |z| 4 / 20 = 16.6 pixels.  Its paraxial radius is a = |z| rho / Dz =
  2.08 pixels; off the axis, at tan(theta) <= 0.21, the image stretches radially by less than 1 / cos^2(theta) < 1.05, so a pixel inside some D(tau) lies within 1.05 a <
  a + 1.5 of the segment.  A pixel whose centre is within a of an end centre is hit by the samples whose tau is near that end: the contributing pixels reach past both.
  How many.  N(tau) = the number of pixel centres in D(tau).  Each sample draws its own tau, so the hits of the frame are sum over pixels and samples of [pixel in D(tau)],
  spp times an average of N over the taus drawn: inside spp [N_min, N_max], the extremes of N over a lattice of 4096 taus, taken with the radius rho (1 -+ 1e-3) so that a
  binary32 rounding at the rim cannot move a count outside.  (An average of 64 x 96 x 64 draws, not a worst case over adversarial ones; the frame is a fixed function of
  the seed and the statement is checked on the model before a kernel sees it.)"""
import numpy as np
import pytest

import raytracinggpu_amd as rt
from . import lens_model as lens
from . import lights_model as lm
from . import shutter_model as shm

f32 = np.float32


def _objs(oracle_cat, name):
    if name == "cat":
        return shm.objects(rt.scenes.spheres("cpu"), {6: oracle_cat}), lm.materials(rt.scenes.spheres("cpu"), [dict(albedo=rt.scenes.CAT_ALBEDO, object_slot=6)])
    return shm.objects(rt.scenes.spheres("demo10")), lm.materials(rt.scenes.spheres("demo10"))


@pytest.mark.parametrize("scene,b", [("cat", 2), ("demo10", 3)])
def test_a_closed_shutter_is_the_lens_walker_and_the_oracle(oracle, oracle_cat, scene, b):
    W, H = 48, 32
    objs, mats = _objs(oracle_cat, scene)
    sc = oracle.Scene.preset("cpu", oracle_cat) if scene == "cat" else oracle.Scene.preset("demo10")
    zeros = ((0.0, -0.0, 0.0), {0: (0.0, 0.0, -0.0), 3: (0.0, 0.0, 0.0)})
    got = shm.Walker(objs, mats, [rt.scenes.LIGHT], shutter=zeros).render(W, H, 2, b)
    exp = lens.Walker(sc, mats, [rt.scenes.LIGHT]).render(W, H, 2, b)
    np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32))
    orc_frame, _, _ = sc.render(W, H, 2, b, want_rgb8=False)
    np.testing.assert_array_equal(got.view(np.uint32), orc_frame.view(np.uint32))
    posed = shm.Walker(objs, mats, [rt.scenes.LIGHT], shutter=zeros, fov=np.pi / 2).render(W, H, 1, 1, pose=(0.2, 0.1), rows=range(8, 16))
    np.testing.assert_array_equal(posed.view(np.uint32), lm.Walker(sc, mats, [rt.scenes.LIGHT], fov=np.pi / 2).render(W, H, 1, 1, pose=(0.2, 0.1), rows=range(8, 16)).view(np.uint32))
    assert (got[..., :3] > 0).any() and got[..., 3].max() > 2


def test_an_open_shutter_moves_the_frame(oracle_cat):
    """the motion does reach the model's frame, through a sphere and through the light alone"""
    objs, mats = _objs(oracle_cat, "demo10")
    still = shm.Walker(objs, mats, [rt.scenes.LIGHT]).render(24, 16, 1, 1)
    w = shm.Walker(objs, mats, [rt.scenes.LIGHT], shutter=((0.0, 0.0, 0.0), {0: (6.0, 0.0, 0.0)}))
    assert (still.view(np.uint32) != w.render(24, 16, 1, 1).view(np.uint32)).any(-1).sum() > 20
    assert len(w.taus) == 24 * 16 and len(set(float(t) for t in w.taus)) > 300      # one tau per path, the pixels' own
    lit = shm.Walker(objs, mats, [rt.scenes.LIGHT], shutter=((8.0, 0.0, 0.0), {})).render(24, 16, 1, 1)
    assert (still.view(np.uint32) != lit.view(np.uint32)).any(-1).sum() > 100


def test_the_draw_lies_in_0_1_and_shares_its_key_with_nothing():
    t = np.array([shm.tau(seed, pixel, samp) for seed in (123456, 7) for pixel in range(0, 3015, 5) for samp in (0, 1, 63)], f32)
    assert t.dtype == f32 and (t > 0).all() and (t <= 1).all()
    m = t.astype(np.float64) * 2.0 ** 24
    assert (m == np.round(m)).all() and m.min() >= 1 and m.max() <= 2 ** 24       # m 2^-24, m = 1 .. 2^24
    assert 0.45 < float(t.mean()) < 0.55 and len(np.unique(t)) > 0.99 * len(t)
    own = (shm.D * 4 + shm.DIM) % 2 ** 32
    assert own == 2 ** 30 + 2
    for segs in range(1, 17):
        others = {(lens.D * 4 + dim) % 2 ** 32 for dim in (0, 1)}                                  # the lens
        others |= {2, 3}                                                                           # the jitter
        others |= {4 * d + dim for d in range(segs) for dim in (0, 1)}                             # the bounces
        others |= {4 * (d + 1) + 2 for d in range(segs)}                                           # the picks
        others |= {((2 ** 29 + d) * 4 + dim) % 2 ** 32 for d in range(segs) for dim in (0, 1)}     # the shells
        assert own not in others
        assert max(k for k in others if k < 2 ** 30) < 4 * (segs + 1)
    # ... and it is the draw it says: the oracle's uniform at that depth and dim, not the lens's
    assert shm.tau(123456, 17, 3) == f32(shm.orc.uniform(123456, 17, 3, np.uint32(1 << 28), 2))
    assert shm.tau(123456, 17, 3) != f32(shm.orc.uniform(123456, 17, 3, np.uint32(1 << 28), 0))


def test_the_pose_is_move_object(oracle):
    rng = np.random.default_rng(5)
    for _ in range(200):
        C, dC = rng.normal(0, 30, 3).astype(f32), rng.normal(0, 5, 3).astype(f32)
        np.testing.assert_array_equal(shm.pose(C, dC, 1).view(np.uint32), oracle.sphere_move(C, dC, 1.0).view(np.uint32))
        t = f32(rng.random())
        exp = (C + (dC * t).astype(f32)).astype(f32)                   # the product first, one rounding each
        np.testing.assert_array_equal(shm.pose(C, dC, t).view(np.uint32), exp.view(np.uint32))
    np.testing.assert_array_equal(shm.pose((1.0, 2.0, 3.0), (0.0, 0.0, 0.0), 0.37), np.asarray((1.0, 2.0, 3.0), f32))


def test_a_streak_of_a_small_sphere():
    frame = shm.st_frame()
    far, bound, lo_x, hi_x, x0, x1, per_sample, n_min, n_max = shm.st_check(frame)
    print(f"contributing pixels within {far:.2f} px of the segment of centres (bound {bound:.2f}), x from {lo_x:.1f} to {hi_x:.1f} (end centres {x0:.2f}, {x1:.2f}); "
          f"{per_sample:.3f} hits per sample, N in [{n_min}, {n_max}]")
    assert n_min >= 8 and n_max <= 2 * n_min
    # with the shutter closed the same scene is a disc about the image centre, and the streak is longer than it by the travel
    still = shm.st_frame(shutter=((0.0, 0.0, 0.0), {}))
    x, _ = shm.st_pixel_xy()
    assert float(x[still[..., 3] > shm.ST_SPP].max()) < 3.0 < x1 <= hi_x
    # the sparse frame is the walker's: one row through the streak, walked in full
    rows = [shm.ST_H // 2]
    full = shm.st_walker().render(shm.ST_W, shm.ST_H, shm.ST_SPP, 0, rows=rows)
    np.testing.assert_array_equal(frame[rows].view(np.uint32), full.view(np.uint32))
    assert (full[..., 3] > shm.ST_SPP).sum() >= 8
