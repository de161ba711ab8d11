"""Rough mirrors on the device (rt_material_set_roughness, rt_kat_gloss).  -m gpu.  Every case fails on a library without the entries.

  the step       rt_kat_gloss against tests/gloss_model.py step, word for word, on 2^16 items: grazing and normal incidence, rays that arrive from behind the normal,
                 axis-aligned normals and normals with a zero component, rays that are not unit vectors, the four extreme keys, alpha in {2^-12, 1/16, 1/2, 1},
                 segments 0 to 15, items that fold back and items that do not;
  the value      get after set, invalid arguments leave the state untouched, an upload clears, RT_ERR_NO_SCENE before one;
  a closed form  that does not rest on the model: the share of the rays a rough mirror on the axis of a 1 x 1 frame sends into a sphere behind the camera, counted
                 through .w, against the GGX distribution's closed form."""
import ctypes as C

import numpy as np
import pytest

import raytracinggpu_amd as rt
from . import gloss_model as gm
from .test_gloss_model import HS_R1_LEAST, HS_R1_ONE

pytestmark = pytest.mark.gpu

f32 = np.float32
ALPHAS = np.array([2.0 ** -12, 1 / 16, 1 / 2, 1.0], f32)
FLOOR = ((0, -1000, 0), 990, (0.5, 0.5, 0.5))
MIRROR = rt.scenes.DEMO[1]
GLASS = rt.scenes.DEMO[0]


@pytest.fixture(scope="module")
def ctx():
    c_ = rt.Context(0)
    yield c_
    c_.close()


def _items(n=1 << 16, seed=7):
    """-> (dict of the arrays of n items in eight families of n / 8, the family of each)"""
    rng = np.random.default_rng(seed)
    N = rng.normal(size=(n, 3))
    N = N / np.linalg.norm(N, axis=1, keepdims=True)
    fam = np.arange(n) % 8
    axes = np.array([(1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0)], np.float64)
    N[fam == 4] = axes[rng.integers(0, 6, (fam == 4).sum())]            # axis-aligned (+-y: the tangent frame's 0 / 0, a NaN on both sides)
    zx = (fam == 5) & (np.arange(n) // 8 % 2 == 0)                      # a zero x or a zero y component: the other tangent branch
    zy = (fam == 5) & ~zx
    N[zx, 0] = 0
    N[zy, 1] = 0
    N[fam == 5] /= np.linalg.norm(N[fam == 5], axis=1, keepdims=True)
    N = N.astype(f32)
    T = np.cross(N.astype(np.float64), rng.normal(size=(n, 3)))
    T = T / np.linalg.norm(T, axis=1, keepdims=True)
    cos = rng.uniform(0.0, 1.0, n)
    cos[fam == 1] = 10.0 ** rng.uniform(-7, -2, (fam == 1).sum())      # grazing
    sign = np.where(fam == 3, 1.0, -1.0)                                # family 3 arrives from behind the normal: un > 0
    u = (sign * cos)[:, None] * N.astype(np.float64) + np.sqrt(1 - cos * cos)[:, None] * T
    u = np.where((fam == 2)[:, None], -N.astype(np.float64), u)         # normal incidence: u = -N exactly
    u[fam == 6] *= rng.uniform(0.5, 3.0, ((fam == 6).sum(), 1))        # the ray is not renormalised
    alpha = ALPHAS[rng.integers(0, 4, n)]
    hs = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    seg = (np.arange(n) // 8 % 16).astype(np.int32)
    for k, (a, key) in enumerate(((ALPHAS[0], HS_R1_LEAST), (ALPHAS[0], HS_R1_ONE), (ALPHAS[3], HS_R1_LEAST), (ALPHAS[3], HS_R1_ONE))):
        i = 7 + 128 * k                                                 # family 7, segment 0: the four extreme keys
        assert fam[i] == 7 and seg[i] == 0
        alpha[i], hs[i] = a, key
    return dict(alpha=alpha, eps=np.where(fam % 2 == 0, f32(1e-3), f32(1e-4)).astype(f32), P=rng.uniform(-50, 50, (n, 3)).astype(f32), N=N, u=u.astype(f32), hs=hs, seg=seg), fam


def _same(got, want, what):
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), what
    np.testing.assert_array_equal(np.where(nan, f32(0), got).view(np.uint32), np.where(nan, f32(0), want).view(np.uint32), err_msg=what)


def test_the_device_step_equals_the_model_on_65536_items(ctx):
    it, fam = _items()
    h, code, O, u = ctx.kat_gloss(**it)
    mh, mcode, mO, mu = gm.step(**it)
    # the families hold what they are there for
    un = gm._dots(it["u"], it["N"])
    assert (un[fam == 3] > 0).all() and (un[fam == 0] < 0).all() and (np.abs(un[fam == 1]) < 0.011).all()
    assert (mcode == gm.FOLDED).sum() > 2000 and (mcode == gm.PLAIN).sum() > 20000          # both occur
    assert (mcode[fam == 3] == gm.FOLDED).any() and (mcode[fam == 3] == gm.PLAIN).any()
    ynan = (fam == 4) & (it["N"][:, 0] == 0) & (it["N"][:, 2] == 0)
    assert np.isnan(mh[ynan]).all() and ynan.sum() > 1000 and not np.isnan(mh[~ynan]).any() and not np.isnan(mu[~ynan]).any()
    r1, _ = gm.draws(it["hs"][[7, 135, 263, 391]], 0)
    assert r1.tolist() == [2.0 ** -24, 1.0, 2.0 ** -24, 1.0]
    for seg in range(16):
        for a in ALPHAS:
            assert ((it["seg"] == seg) & (it["alpha"] == a)).any(), (seg, a)
        assert ((it["seg"] == seg) & (mcode == gm.FOLDED)).any(), seg
    np.testing.assert_array_equal(code, mcode)
    _same(h, mh, "h")
    _same(O, mO, "O")
    _same(u, mu, "u")
    # one item, and none
    one = {k: v[5:6] for k, v in it.items()}
    assert ctx.kat_gloss(**one)[1][0] == mcode[5]
    assert ctx._L.rt_kat_gloss(ctx._h, 0, None, None) == 0
    assert ctx._L.rt_kat_gloss(ctx._h, 1, None, None) == -1 and ctx._L.rt_kat_gloss(ctx._h, -1, None, None) == -1


def test_the_value_get_after_set_invalid_arguments_uploads_and_no_scene():
    c = rt.Context(0)
    try:
        lib, h = c._L, c._h
        a = C.c_float(-7)
        assert lib.rt_material_set_roughness(h, 0, 0.5) == -4 and lib.rt_material_get_roughness(h, 0, C.byref(a)) == -4 and a.value == -7      # RT_ERR_NO_SCENE
        c.scene_upload([FLOOR, MIRROR, GLASS], None)
        assert [c.roughness(k) for k in range(3)] == [0.0, 0.0, 0.0]
        c.set_roughness(1, 0.25)
        c.set_roughness(0, 1.0)                                         # a diffuse object takes the value too: it is ineffective, not invalid
        c.set_roughness(2, 2.0 ** -12)                                  # ... and so does glass
        assert [c.roughness(k) for k in range(3)] == [1.0, 0.25, 2.0 ** -12]
        for slot in (-1, 3, 16, 31, 32, 1 << 20):
            assert lib.rt_material_set_roughness(h, slot, 0.5) == -1 and b"roughness" in lib.rt_last_error(h), slot
            assert lib.rt_material_get_roughness(h, slot, C.byref(a)) == -1 and a.value == -7, slot
        just_below = float(np.nextafter(f32(2.0 ** -12), f32(0)))
        just_above = float(np.nextafter(f32(1), f32(2)))
        for bad in (just_below, just_above, -0.25, 1e-30, 2.0, float("inf"), -float("inf"), float("nan")):
            assert lib.rt_material_set_roughness(h, 1, bad) == -1 and b"roughness" in lib.rt_last_error(h), bad
        assert lib.rt_material_get_roughness(h, 1, None) == -1
        assert [c.roughness(k) for k in range(3)] == [1.0, 0.25, 2.0 ** -12]
        c.set_roughness(0, 0.0)
        c.set_roughness(0, -0.0)
        assert [c.roughness(k) for k in range(3)] == [0.0, 0.25, 2.0 ** -12] and np.signbit(f32(c.roughness(0))) == False  # noqa: E712
        c.scene_upload([FLOOR, MIRROR, GLASS], None)                    # an upload clears every value
        assert [c.roughness(k) for k in range(3)] == [0.0, 0.0, 0.0]
        c.set_roughness(1, 0.5)
        with pytest.raises(rt.RtError):                                 # a refused upload leaves no scene
            c.scene_upload([FLOOR] * 17, None)
        assert lib.rt_material_get_roughness(h, 1, C.byref(a)) == -4 and a.value == -7
    finally:
        c.close()


# ---- a closed form that does not rest on the model ---------------------------------------------------------------------------------------------------------------------------

D_FAR = 150.0                                        # from the hit point (0, 0, 10) to the centre of the far sphere
R_FAR = 0.6 * D_FAR                                  # R / D = 0.6 = sin(beta): the far sphere fills the cone of half-angle beta about the axis, tan(beta / 2) = 1 / 3
ROUGH_BALL = ((0.0, 0.0, 0.0), 10.0, (0.0, 0.0, 0.0), 1, 1.0, 1.0)      # a mirror on the axis: the camera ray (0, 0, 55) -> -z hits it at (0, 0, 10), N = (0, 0, 1)
FAR_BALL = ((0.0, 0.0, 10.0 + D_FAR), R_FAR, (0.5, 0.5, 0.5))           # diffuse, behind the camera: z from 70 to 250, the camera at z = 55 outside it
EXPECTED = 16 / 25 + 1 / 145


def _rays(c):
    """-> (sum of .w, S) over 64 seeds of 64 samples of the 1 x 1 frame at b = 1"""
    total = S = 0
    for seed in range(64):
        fr = c.render(rt.make_params(1, 1, 64, 1, seed=7000 + seed, **rt.scenes.CPU_LAUNCHER))
        assert fr.shape == (1, 1, 4) and float(fr[0, 0, 3]) == int(fr[0, 0, 3])
        total += int(fr[0, 0, 3])
        S += 64
    return total, S


def test_a_rough_mirror_on_the_axis_sends_the_ggx_share_of_its_rays_into_the_far_sphere():
    """A 1 x 1 frame with sigma = 0: its one camera ray is the axis.  It hits the mirror ball at normal incidence; the facet is theta_h off the axis, the reflected ray
    2 theta_h off it -- or, where 2 theta_h > 90 degrees and the ray is folded back, 180 degrees - 2 theta_h.  Behind the camera a diffuse sphere of radius R at distance D
    from the hit point fills the cone sin(beta) = R / D = 0.6 about the axis, so the ray hits it when 2 theta_h <= beta, tan^2(theta_h) <= tan^2(beta / 2) = 1 / 9, or when
    theta_h >= 90 degrees - beta / 2, tan^2(theta_h) >= 9.  GGX facets drawn with D(h) (n.h) have P(tan^2(theta_h) <= T) = T / (alpha^2 + T); with alpha = 1 / 4:
    (1/9) / (1/16 + 1/9) + 1 - 9 / (1/16 + 9) = 16/25 + 1/145 = 0.6469.
    b = 1: two segments, the reflected ray is the path's last.  A sample whose reflected ray meets the far sphere counts one ray more -- the diffuse hit's shadow ray,
    counted in .w whether it is traced or elided -- than one that misses: sum(.w) = 2 S + hits.  The smooth mirror hits every time: 3 S, exactly.
    The ray leaves from P + eps N, not from P: that moves the cone's apex by eps = 1e-3 against D = 150, the share by about eps / D = 7e-6."""
    S = 64 * 64
    bound = 5 * np.sqrt(EXPECTED * (1 - EXPECTED) / S)
    assert abs(EXPECTED - 0.6469) < 5e-5 and R_FAR / D_FAR == 0.6 and D_FAR >= 10 and FAR_BALL[0][2] - R_FAR > 55
    assert bound < 0.5 * (1 - EXPECTED)                                  # five standard errors are below half the gap between the smooth and the rough figure
    c, smooth = rt.Context(0), rt.Context(0)
    try:
        for c_ in (c, smooth):
            c_.scene_upload([ROUGH_BALL, FAR_BALL], None)               # (the uploaded light, rt.scenes.LIGHT, is outside the far sphere and sees its near side)
        smooth.set_roughness(0, 0.0)
        assert _rays(smooth) == (3 * S, S)
        c.set_roughness(0, 0.25)
        total, s = _rays(c)
        hits = total - 2 * s
        print(f"hit {hits} of {s}: {hits / s:.5f} against {EXPECTED:.5f}, bound {bound:.5f}")
        assert s == S and 0 <= hits <= s
        assert abs(hits / s - EXPECTED) <= bound
        c.set_roughness(0, 0.0)
        assert _rays(c) == (3 * S, S)
    finally:
        c.close()
        smooth.close()
