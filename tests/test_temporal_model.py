"""The reference model of rt_temporal_accumulate and rt_denoise_var (tests/temporal_model.py) without a GPU: the properties the formula of include/raytrace_hip.h
promises -- the projection inverts the camera as the kernels write it, a static scene accumulates the running mean, a cut resets, the mask and the two limits do what
they say, a moved sphere's pixels follow it -- and the quality the committed defaults buy on the two scenes of DESIGN.md section 5.8, all on CPU oracle frames and planes."""
import numpy as np
import pytest

import raytracinggpu_amd as rt
from . import denoise_model as dm
from . import temporal_model as tm

F = np.float32
W = H = 128
CAT_SLOT = 6


def _bits_equal(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _albedos(scene):
    return [s[2] for s in rt.scenes.spheres(scene)] + ([rt.scenes.CAT_ALBEDO] if scene == "cpu" else [])


@pytest.fixture(scope="module")
def inputs(oracle, oracle_cat):
    """per scene: eight one-sample b = 3 frames with eight seeds, the 256-sample frame, the planes -- at the size and with the samples of
    test_defaults_reduce_the_error_of_a_one_sample_frame"""
    made = {}

    def get(scene):
        if scene not in made:
            sc = oracle.Scene.preset(scene, oracle_cat if scene == "cpu" else None)
            frames = [sc.render(W, H, 1, 3, want_rgb8=False, seed=1000 + i)[0] for i in range(8)]
            ref = sc.render(W, H, 256, 3, want_rgb8=False, seed=99)[0]
            made[scene] = dict(scene=sc, frames=frames, ref=ref, aov=dm.oracle_aov(sc, _albedos(scene), W, H))
        return made[scene]
    return get


def _angle(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(-1))


def test_projection_round_trip(inputs, oracle):
    """The continuous previous-frame coordinate of every hit point, pushed forward through the camera formula of pixel_dir / posed_dir in binary64, points at the hit
    point to within a quarter of a pixel's angle, 1 / (4 |z|): the nearest-pixel choice tolerates half a pixel.  Derived, not measured."""
    sc = inputs("cpu")["scene"]
    pose_a, pose_b = rt.make_pose(), rt.make_pose(position=(4.0, 2.0, 50.0), yaw=0.15, pitch=0.2)
    planes = {"fixed": inputs("cpu")["aov"]}
    for name, pose in (("a", pose_a), ("b", pose_b)):
        planes[name] = dm.oracle_aov(sc, _albedos("cpu"), W, H, cam=tuple(pose.position), fov=pose.fov, basis=rt.camera_basis(pose))
    cases = [("fixed", dict(camera=((3.0, -2.0, 50.0), None))), ("fixed", dict(camera=((0.0, 0.0, 55.0), 1.3))), ("a", dict(pose=pose_b)), ("b", dict(pose=pose_a)),
             ("fixed", dict(pose=pose_b)), ("a", dict(camera=((0.0, 0.0, 55.0), None)))]
    for cur, prev_cam in cases:
        aov = planes[cur]
        hit = aov[0, ..., 3] >= 0
        P = aov[1, ..., :3]
        k, gx, gy = tm.project(P, W, H, **prev_cam)
        O, bx, by, bz, cx, cy, b = tm.camera_constants(W, **prev_cam)
        posed = "pose" in prev_cam
        z = np.float64(b) - (np.dot(O.astype(np.float64), bz.astype(np.float64)) if posed else 0.0)
        ok = hit & (k > 0)
        assert ok.mean() > 0.5, (cur, prev_cam)
        X, Y = gx.astype(np.float64) - W / 2, H / 2 - gy.astype(np.float64)
        v = X[..., None] * bx.astype(np.float64) + Y[..., None] * by.astype(np.float64) + z * bz.astype(np.float64)
        if posed:
            v = v + O.astype(np.float64)                               # realtime:1115: the position is part of the direction
        ang = _angle(v, P.astype(np.float64) - O.astype(np.float64))[ok]
        assert ang.max() < 1.0 / (4.0 * abs(z)), (cur, prev_cam, ang.max(), 1.0 / (4.0 * abs(z)))
        if posed:                                                      # ... and a textbook camera (direction without the position) would not do
            v0 = v - O.astype(np.float64)
            assert _angle(v0, P.astype(np.float64) - O.astype(np.float64))[ok].max() > 10.0 / abs(z)
    # a camera in its own frame sees every hit point in the pixel it was traced through
    for name, cam in (("fixed", dict(camera=((0.0, 0.0, 55.0), None))), ("a", dict(pose=pose_a)), ("b", dict(pose=pose_b))):
        aov = planes[name]
        hit = aov[0, ..., 3] >= 0
        k, gx, gy = tm.project(aov[1, ..., :3], W, H, **cam)
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        assert (k[hit] > 0).all() and (np.floor(gx)[hit] == xs[hit]).all() and (np.floor(gy)[hit] == ys[hit]).all()


def test_static_scene_accumulates_the_running_mean(inputs, oracle):
    d = inputs("cpu")
    aov, frames = d["aov"], d["frames"]
    ids = aov[0, ..., 3]
    assert (ids >= 0).all() and (ids == CAT_SLOT).sum() > 500
    hist = None
    for i, f in enumerate(frames):
        hist = tm.accumulate(f, aov, None if hist is None else aov, hist, mask=1 << CAT_SLOT)
        n = hist[1, ..., 2]
        assert (n[ids != CAT_SLOT] == i + 1).all()                     # history length = frame index, outside the mask
        assert (n[ids == CAT_SLOT] == 1).all()
        _bits_equal(hist[0][ids == CAT_SLOT], f[ids == CAT_SLOT])
        _bits_equal(hist[0, ..., 3], f[..., 3])
        if i == 1:
            exp = frames[0][..., :3] + (frames[1][..., :3] - frames[0][..., :3]) * F(0.5)
            _bits_equal(hist[0, ..., :3][ids != CAT_SLOT], exp[ids != CAT_SLOT])
    # exactly the running mean: nothing blurred in from a neighbour
    mean = np.mean([f[..., :3].astype(np.float64) for f in frames], axis=0)
    np.testing.assert_allclose(hist[0, ..., :3][ids != CAT_SLOT], mean[ids != CAT_SLOT], rtol=1e-5)
    # the variance: spatial while n < 4 (frames 1 - 3), temporal from then on
    l = tm.lum(np.stack(frames)[..., :3].astype(np.float64))
    far = ids != CAT_SLOT
    np.testing.assert_allclose(hist[1, ..., 0][far], l.mean(0)[far], rtol=1e-5)
    np.testing.assert_allclose(hist[1, ..., 3][far], np.maximum(0, (l * l).mean(0) - l.mean(0) ** 2)[far], rtol=2e-3, atol=1e-6 * float((l * l).max()))


def test_misses_are_copies(oracle, oracle_cat):
    sc = oracle.Scene()
    walls = [s for s in rt.scenes.spheres("cpu") if tuple(s[0]) != (0, 0, -1000)]
    for c, r, a in walls:
        sc.add_sphere(c, r, a)
    sc.add_mesh(oracle_cat)
    w = h = 64
    aov = dm.oracle_aov(sc, [s[2] for s in walls] + [rt.scenes.CAT_ALBEDO], w, h)
    miss = aov[0, ..., 3] == -1
    assert 100 < miss.sum() < w * h - 100
    f0, f1 = (sc.render(w, h, 1, 1, want_rgb8=False, seed=s)[0] for s in (1, 2))
    h0 = tm.accumulate(f0, aov)
    h1 = tm.accumulate(f1, aov, aov, h0)
    for hh, f in ((h0, f0), (h1, f1)):
        _bits_equal(hh[0][miss], f[miss])
        assert not hh[1][miss].any()                                   # n = 0, variance 0
    assert (h1[1, ..., 2][~miss] == 2).all() and (h0[1, ..., 2][~miss] == 1).all()
    out = tm.denoise_var(h1, aov, 3, 2.0, 0.25, 16.0, 16.0, 0.0)
    _bits_equal(out[miss], f1[miss])


def _must_reset(aov, prev, min_dot, max_dist):
    """static camera: pixels none of whose 3 x 3 previous neighbours passes the id, normal and plane tests (binary64, with a margin) -- a superset of the 2 x 2 footprint"""
    N, ID, P = aov[0, ..., :3].astype(np.float64), aov[0, ..., 3], aov[1, ..., :3].astype(np.float64)
    h, w = ID.shape
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    may = np.zeros((h, w), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            qy, qx = np.clip(ys + dy, 0, h - 1), np.clip(xs + dx, 0, w - 1)
            Nq, Pq = prev[0, qy, qx, :3].astype(np.float64), prev[1, qy, qx, :3].astype(np.float64)
            e = (N * (Pq - P)).sum(-1)
            may |= (prev[0, qy, qx, 3] == ID) & ((N * Nq).sum(-1) >= min_dot - 1e-3) & (np.abs(e) <= max_dist * (1 + 1e-3) + 1e-3)
    return (ID >= 0) & ~may


def test_cut_detection(inputs):
    d, other = inputs("cpu"), inputs("demo10")
    aov, (f0, f1) = d["aov"], d["frames"][:2]
    old = np.zeros((2, H, W, 4), np.float32)
    old[0, ..., :3], old[1] = 7.0, (3.0, 10.0, 5.0, 1.0)
    # the planes of another scene as "previous": no pixel passes
    reset = _must_reset(aov, other["aov"], 0.9, 0.5)
    assert reset.all()
    h1 = tm.accumulate(f1, aov, other["aov"], old)
    assert (h1[1, ..., 2][reset] == 1).all()
    _bits_equal(h1[0][reset], f1[reset])
    # its own planes with one test broken per band: the object id, the normal, the plane
    prev = aov.copy()
    prev[0, 8:40, :, 3] += 1
    prev[0, 48:80, :, :3] *= -1
    prev[1, 88:120, :, :3] += 3 * aov[0, 88:120, :, :3]
    reset = _must_reset(aov, prev, 0.9, 0.5)
    for a, b in ((10, 38), (50, 78), (90, 118)):
        assert reset[a:b].all()
    h1 = tm.accumulate(f1, aov, prev, old)
    assert (h1[1, ..., 2][reset] == 1).all()
    _bits_equal(h1[0][reset], f1[reset])
    keep = np.zeros((H, W), bool)
    keep[:7], keep[41:47], keep[81:87], keep[121:] = True, True, True, True
    assert (h1[1, ..., 2][keep] == 6).all()                            # the untouched rows carry on: n_q + 1


def test_mask_max_history_and_alpha_min(inputs):
    d = inputs("cpu")
    aov, f = d["aov"], d["frames"][0]
    ids = aov[0, ..., 3]
    old = np.zeros((2, H, W, 4), np.float32)
    old[0, ..., :3], old[1] = 2.0, (3.0, 10.0, 5.0, 1.0)
    C, l = f[..., :3], tm.lum(f)

    def expect(a):
        a = F(a)
        return F(2) + a * (C - F(2)), F(3) + a * (l - F(3)), F(10) + a * (l * l - F(10))
    h = tm.accumulate(f, aov, aov, old)                                # the defaults: n = 6, a = 1 / 6
    col, m1, m2 = expect(F(1) / F(6))
    assert (h[1, ..., 2] == 6).all()
    _bits_equal(h[0, ..., :3], col)
    _bits_equal(h[1, ..., 0], m1)
    _bits_equal(h[1, ..., 1], m2)
    _bits_equal(h[1, ..., 3], np.maximum(F(0), m2 - m1 * m1))           # n >= 4: the temporal variance
    h = tm.accumulate(f, aov, aov, old, max_history=3)                 # n stops at 3, a at 1 / 3; n < 4: the spatial variance
    assert (h[1, ..., 2] == 3).all()
    _bits_equal(h[0, ..., :3], expect(F(1) / F(3))[0])
    _bits_equal(h[1, ..., 3], tm.accumulate(f, aov)[1, ..., 3])
    h = tm.accumulate(f, aov, aov, old, max_history=1)
    assert (h[1, ..., 2] == 1).all()
    _bits_equal(h[0, ..., :3], expect(1.0)[0])                         # a = 1: H + (C - H), which is C up to rounding
    np.testing.assert_allclose(h[0, ..., :3], C, rtol=1e-6, atol=1e-6)
    h = tm.accumulate(f, aov, aov, old, alpha_min=0.5)                 # the current frame never weighs less than a half
    assert (h[1, ..., 2] == 6).all()
    _bits_equal(h[0, ..., :3], expect(0.5)[0])
    h = tm.accumulate(f, aov, aov, old, alpha_min=0.01)                # a floor below 1 / n changes nothing
    _bits_equal(h[0, ..., :3], expect(F(1) / F(6))[0])
    h = tm.accumulate(f, aov, aov, old, mask=1 << CAT_SLOT)
    assert (h[1, ..., 2][ids == CAT_SLOT] == 1).all() and (h[1, ..., 2][ids != CAT_SLOT] == 6).all()
    _bits_equal(h[0][ids == CAT_SLOT], f[ids == CAT_SLOT])
    h = tm.accumulate(f, aov, aov, old, mask=0xFFFF)
    _bits_equal(h, tm.accumulate(f, aov))                              # everything masked = the first frame


def test_moved_sphere_follows_its_motion_record(oracle):
    w = h = 96
    walls = rt.scenes.spheres("cpu")
    slot = len(walls)
    c0 = np.array([-8.0, -2.0, 18.0], np.float32)
    c1 = c0 + np.array([4.0, 2.0, -1.6], np.float32)
    scenes, planes, frames = [], [], []
    for c in (c0, c1):
        sc = oracle.Scene()
        for s in walls:
            sc.add_sphere(*s)
        sc.add_sphere(tuple(float(x) for x in c), 6.0, (0.8, 0.8, 0.8))
        scenes.append(sc)
        planes.append(dm.oracle_aov(sc, [s[2] for s in walls] + [(0.8, 0.8, 0.8)], w, h))
        frames.append(sc.render(w, h, 1, 1, want_rgb8=False, seed=len(frames) + 1)[0])
    motion = rt.motion_from_spheres(walls + [(c0, 6.0)], walls + [(c1, 6.0)])
    np.testing.assert_array_equal(motion[slot, 9:], c0 - c1)
    h0 = tm.accumulate(frames[0], planes[0])
    taps = {}
    h1 = tm.accumulate(frames[1], planes[1], planes[0], h0, motion=motion, taps=taps)
    on = planes[1][0, ..., 3] == slot
    assert on.sum() > 200
    # where the sphere's old image is (binary64, the fixed camera of cpu:694-699): the pixel, and whether its 3 x 3 neighbourhood shows the sphere
    P = planes[1][1, ..., :3].astype(np.float64) + (c0 - c1).astype(np.float64)
    z = -w / (2 * np.tan(np.float64(F(np.pi / 3)) / 2))
    dd = P - np.array([0.0, 0.0, 55.0])
    px, py = np.floor(dd[..., 0] * z / dd[..., 2] + w / 2).astype(int), np.floor(h / 2 - dd[..., 1] * z / dd[..., 2]).astype(int)
    interior = on & (px >= 1) & (px < w - 1) & (py >= 1) & (py < h - 1)
    pxc, pyc = np.clip(px, 1, w - 2), np.clip(py, 1, h - 2)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            interior &= planes[0][0, pyc + dy, pxc + dx, 3] == slot
    assert interior.sum() > 0.5 * on.sum()
    assert (h1[1, ..., 2][interior] == 2).all()                        # valid history ...
    q = taps["q"][interior]
    assert (np.abs(q[:, 0] - px[interior]) <= 1).all() and (np.abs(q[:, 1] - py[interior]) <= 1).all()   # ... pointing at the sphere's old image
    assert (planes[0][0, q[:, 1], q[:, 0], 3] == slot).all()
    assert (np.hypot(q[:, 0] - np.nonzero(interior)[1], q[:, 1] - np.nonzero(interior)[0]) > 3).all()     # (which is elsewhere)
    # the same frames without the record: no history wherever the sphere's shift takes the old surface out of the tolerances
    h1s = tm.accumulate(frames[1], planes[1], planes[0], h0)
    lost = _must_reset(planes[1], planes[0], 0.9, 0.5) & on
    assert lost.sum() > 0.5 * on.sum()
    assert (h1s[1, ..., 2][lost] == 1).all()
    _bits_equal(h1s[0][lost], frames[1][lost])
    assert (h1s[1, ..., 2][~on & (planes[0][0, ..., 3] != slot)] == 2).all()   # the walls that neither image of the sphere covers are static either way


def _rmse(oracle, a, b):
    return float(np.sqrt(np.mean((oracle.gamma_unit(a[..., :3]) - oracle.gamma_unit(b[..., :3])) ** 2)))


@pytest.mark.parametrize("scene", ["cpu", "demo10"])
def test_error_orderings(inputs, oracle, scene):
    """DESIGN.md section 5.8 at test size: 128 x 128, b = 3, eight static one-sample frames against a 256-sample frame, RMSE in the tonemap's [0, 1] scale.  Two strict
    orderings: the accumulated frame beats the one-sample frame, and accumulation + rt_denoise_var with the committed defaults beats rt_denoise with its defaults on frame
    8 alone.  Measured here (ratios to the one-sample frame's error): cat scene accumulated 0.554, then filtered 0.343, rt_denoise alone 0.375; sphere scene 0.604,
    0.672, 0.882 -- on the sphere scene the filter gives back some of what accumulation won (it smears the reflections the planes do not see), and still beats the
    spatial filter."""
    d = inputs(scene)
    aov, frames, ref = d["aov"], d["frames"], d["ref"]
    hist = None
    for f in frames:
        hist = tm.accumulate(f, aov, None if hist is None else aov, hist)
    v = rt.make_denoise_var_params()
    filtered = tm.denoise_var(hist, aov, v.n_passes, v.k_normal, v.k_position, v.k_albedo, v.k_sigma, v.var_floor)
    p = rt.make_denoise_params()
    spatial = dm.denoise(frames[-1], aov, p.n_passes, p.k_normal, p.k_position, p.k_albedo, p.k_color)
    e_one, e_acc, e_filtered, e_spatial = (_rmse(oracle, x, ref) for x in (frames[-1], hist[0], filtered, spatial))
    print(f"{scene}: rmse one-sample {e_one:.4f}, accumulated {e_acc:.4f} ({e_acc / e_one:.3f}), accumulated + denoise_var {e_filtered:.4f} ({e_filtered / e_one:.3f}), "
          f"denoise on frame 8 alone {e_spatial:.4f} ({e_spatial / e_one:.3f})")
    assert e_acc < e_one
    assert e_filtered < e_spatial
