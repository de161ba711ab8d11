"""tests/emission_model.py held to the mathematics, without a GPU (seconds): the table's counts follow area times radiance and vanish exactly where they must; the draw
stays inside its triangle; the estimate g Le is unbiased for the integral of Le mx cl / d2 over a panel (against a midpoint quadrature, five standard errors plus the
quadrature's own error, both under 1 % of the integral); the walker follows the hit rule and is the walker underneath without an emitter."""
import numpy as np
import pytest

import raytracinggpu_amd as rt
from . import emission_model as em
from . import lights_model as lm
from . import soft_lights_model as slm
from .sky_sample_model import mix32

f32 = np.float32
LE = np.array([10.0, 9.0, 8.0], f32)
# (tilted a little: the reference's box test is strict, so a panel whose box is flat -- an axis-aligned one -- is met by no ray at all; the oracle and the device agree on that)
PANEL = rt.scenes.panel((-6, 14, -6), (12, 0.5, 0), (0, 0.25, 12))


def _keys(n, salt=0x2545F491):
    return mix32(np.arange(n, dtype=np.uint64) ^ np.uint64(salt)).astype(np.uint32)


def _mixed():
    """three meshes' worth of triangles: an emitter with two zero-area triangles among five, a mesh that does not emit, a second emitter of another radiance"""
    rng = np.random.default_rng(7)
    tris = rng.uniform(-5, 5, (12, 3, 3)).astype(f32)
    tris[1, 2] = tris[1, 1]                                             # two corners alike
    tris[3] = tris[3, 0]                                                # a point
    le = np.zeros((12, 3), f32)
    le[:5] = (2.0, 0.0, 1.0)
    le[9:] = (0.0, 0.25, 0.0)
    return tris, le


def test_counts_are_positive_exactly_on_emitting_triangles_with_area_and_prefixes_rise_only_there():
    tris, le = _mixed()
    tb = em.TriTable(tris, le)
    want = np.zeros(12, bool)
    want[[0, 2, 4, 9, 10, 11]] = True
    assert ((tb.c > 0) == want).all()
    assert (tb.A2[[1, 3]] == 0).all() and (tb.A2[want] > 0).all()
    rise = np.diff(np.concatenate([[0], tb.prefix.astype(np.int64)])) > 0
    assert (rise == want).all()
    assert tb.total == int(tb.c.astype(np.uint64).sum()) and tb.c.max() == 1 << 31
    # c follows W = A2 Y to the quantisation's half step
    area2 = np.linalg.norm(np.cross(tris[:, 1].astype(np.float64) - tris[:, 0], tris[:, 2].astype(np.float64) - tris[:, 0]), axis=1)
    w = area2 * le.astype(np.float64).sum(axis=1)
    np.testing.assert_allclose(tb.c[want] / 2.0 ** 31, (w / w.max())[want], rtol=1e-5, atol=2.0 ** -31)
    t, _ = tb.sample(_keys(1 << 14), 0)
    assert want[t].all() and set(np.unique(t)) == set(np.flatnonzero(want))


def test_an_all_black_or_all_degenerate_set_is_empty():
    tris, le = _mixed()
    assert em.TriTable(tris, np.zeros((12, 3), f32)).total == 0
    flat = np.repeat(tris[:, :1], 3, axis=1)
    tb = em.TriTable(flat, le)
    assert tb.total == 0 and not tb.c.any() and not tb.prefix.any()
    assert em.TriTable(np.zeros((0, 3, 3), f32), np.zeros((0, 3), f32)).total == 0


def test_the_point_lies_in_its_triangle_on_65536_keys_and_scalar_and_array_draws_agree():
    tris, le = _mixed()
    tb = em.TriTable(tris, le)
    hs = _keys(1 << 16)
    hs[:4] = (0, 1, 0xFFFFFFFF, 0x80000000)
    seg = (np.arange(1 << 16) % 7).astype(np.int32)
    r1, r2 = tb.barycentrics(hs, seg)
    assert (r1 >= 0).all() and (r1 <= 1).all() and (r2 >= 0).all() and (r2 <= 1).all()
    assert ((r1 + r2).astype(f32) <= 1).all()                           # the rule's own test, in binary32; in the reals the sum may exceed 1 by the one bit that sum drops
    assert (r1.astype(np.float64) + r2.astype(np.float64) <= 1 + 2.0 ** -24).all()
    t, Q = tb.sample(hs, seg)
    # Q against the exact combination of the corners: inside the triangle up to rounding
    A, e1, e2 = tris[t, 0].astype(np.float64), tris[t, 1].astype(np.float64) - tris[t, 0], tris[t, 2].astype(np.float64) - tris[t, 0]
    exact = A + r1[:, None].astype(np.float64) * e1 + r2[:, None].astype(np.float64) * e2
    assert np.abs(Q - exact).max() < 1e-5
    for k in (0, 1, 2, 3, 77, 4096, 65535):
        tk, Qk = tb.sample(int(hs[k]), int(seg[k]))
        assert tk[0] == t[k] and (Qk[0].view(np.uint32) == Q[k].view(np.uint32)).all()


POINTS = [((0.0, 0.0, 0.0), (0.0, 1.0, 0.0)),                           # under the middle of the panel, facing it
          ((5.0, 2.0, -3.0), (0.3, 0.9, 0.1)),                          # off to a side, tilted
          ((-9.0, 10.0, 2.0), (1.0, 0.2, 0.0))]                         # beside it: the panel is seen at grazing angles and part of it lies behind the surface


def _quadrature(P, N, n):
    """midpoint rule over the panel's parameter square, n x n: the integral of Le mx cl / d2 dA, binary64"""
    v = PANEL[0].astype(np.float64)
    c, eu, ev = v[0], v[1] - v[0], v[3] - v[0]
    s = (np.arange(n) + 0.5) / n
    Q = c + s[:, None, None] * eu + s[None, :, None] * ev
    nrm = np.cross(eu, ev)
    dA = np.linalg.norm(nrm) / (n * n)
    nrm = nrm / np.linalg.norm(nrm)
    d = Q - np.asarray(P, np.float64)
    d2 = (d * d).sum(-1)
    wl = d / np.sqrt(d2)[..., None]
    mx = np.maximum(wl @ np.asarray(N, np.float64), 0)
    cl = np.abs(wl @ nrm)
    return LE.astype(np.float64) * (mx * cl / d2).sum() * dA


@pytest.mark.parametrize("P,N", POINTS)
def test_the_estimate_is_unbiased_for_the_integral_over_the_panel(P, N):
    N = (np.asarray(N, np.float64) / np.linalg.norm(N)).astype(f32)
    tb = em.TriTable(em.corners(*PANEL), LE)
    n = 1 << 22
    hs = _keys(n, 0x9E3779B1)
    t, Q = tb.sample(hs, 1)
    g, _, _ = tb.weight(t, Q, np.broadcast_to(np.asarray(P, f32), Q.shape), np.broadcast_to(N, Q.shape))
    est = g.astype(np.float64)[:, None] * LE.astype(np.float64)
    mean, se = est.mean(axis=0), est.std(axis=0) / np.sqrt(n)
    fine = _quadrature(P, N, 2048)
    qerr = np.abs(fine - _quadrature(P, N, 1024))
    thr = 5 * se + qerr
    print("mean", mean, "quadrature", fine, "threshold", thr)
    assert (thr < 0.01 * fine).all(), (thr, fine)
    assert (np.abs(mean - fine) <= thr).all(), (mean, fine, thr)


# ---- the walker ----------------------------------------------------------------------------------------------------------------------------------------------------------

BIG = rt.scenes.panel((-60, 14, -60), (120, 1, 0), (0, 0.5, 120))         # a ceiling no bounce off the floor misses
FLOOR = ((0, -1000, 0), 990, (0.5, 0.25, 0.75))
MIRROR_FLOOR = ((0, -1000, 0), 990, (0.5, 0.5, 0.5), 1, 1.0, 1.0)


def _scene(oracle, floor, panel=BIG):
    osc = oracle.Scene()
    osc.add_sphere(floor[0], floor[1], floor[2], *(floor[3:] if len(floor) > 3 else ()))
    m = oracle.Mesh.from_arrays(*panel).build_bvh()
    osc.add_mesh(m)
    d = dict(vertices=m.vertices, indices=m.triangles, bvh_arr10=m.bvh_array(), albedo=(0.5, 0.5, 0.5), object_slot=1)
    tb = em.TriTable(em.corners(d["vertices"], d["indices"], em.stored_order(d["bvh_arr10"])), LE)
    return osc, lm.materials([floor], [d]), tb, m


def _walker(oracle, floor, share, intensity=3e10, **kw):
    osc, mats, tb, m = _scene(oracle, floor)
    wk = em.Walker(osc, mats, [((-10.0, 5.0, 40.0), intensity)], None, emission={1: LE}, table=tb, share=share, **kw)
    wk._keep = m
    return wk


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_the_camera_sees_le_directly_and_through_a_mirror(oracle):
    up = lm._normalize(lm._v(0.1, 1.0, 0.2))
    for share in (0.0, 0.5, 1.0):
        wk = _walker(oracle, FLOOR, share)
        ans, rays = wk.path(lm._v(0, 0, 0), up, 3, 5, 0)
        assert (_bits(ans) == _bits(LE)).all() and rays == 1
        wm = _walker(oracle, MIRROR_FLOOR, share)
        down = lm._normalize(lm._v(0.1, -1.0, 0.1))
        ans, rays = wm.path(lm._v(0, 5, 0), down, 3, 5, 0)
        assert (_bits(ans) == _bits(LE)).all() and rays == 2           # the mirror's ray ends on the panel: SID[d - 1] == 0xff


def test_behind_a_diffuse_segment_the_emitter_gives_zero_while_sampled_and_le_at_share_0(oracle):
    down = lm._normalize(lm._v(0.1, -1.0, 0.1))
    O = lm._v(0, 5, 0)
    alb = np.asarray(FLOOR[2], f32)
    # lights of intensity 0: the light's term is +0, so at share 0 the answer is alb * Le alone ...
    w0 = _walker(oracle, FLOOR, 0.0, intensity=0.0)
    assert w0.s == 0
    ans, rays = w0.path(O, down, 2, 9, 0)
    assert (_bits(ans) == _bits((alb * LE).astype(f32))).all() and rays == 3
    # ... and at any positive share the effective share is 1: every shadow ray goes to the panel, the bounce's hit on it starts the fold from +0
    w1 = _walker(oracle, FLOOR, 0.5, intensity=0.0)
    assert w1.s == 1 and w1.w_emit == 1
    ans, rays = w1.path(O, down, 2, 9, 0)
    hit, oid, P, N = w1.scene.intersect_all(O, down, 1e-4)
    assert hit and oid == 0
    t, Q = w1.table.sample(em.sample_key(w1.seed, 9, 0), 0)
    g, _, _ = w1.table.weight(t, Q, P, N)
    l3 = (f32(1) * (g[0] * LE).astype(f32)).astype(f32)
    assert g[0] > 0 and rays == 3
    assert (_bits(ans) == _bits(((l3 * alb).astype(f32) / f32(lm.PI)).astype(f32) + (alb * lm._v(0, 0, 0)).astype(f32))).all()
    # a one-segment path never meets the rule
    a0, r0 = w0.path(O, down, 1, 9, 0)
    assert not a0.any() and r0 == 2


def test_ray_counts_do_not_depend_on_the_share_and_no_emitter_is_the_walker_underneath(oracle):
    a = _walker(oracle, FLOOR, 0.5).render(12, 8, 2, 2)
    b = _walker(oracle, FLOOR, 0.0).render(12, 8, 2, 2)
    assert (a[..., 3] == b[..., 3]).all() and a[..., 3].max() >= 5
    assert (_bits(a[..., :3]) != _bits(b[..., :3])).any()
    osc, mats, tb, m = _scene(oracle, FLOOR)
    lights = [((-10.0, 5.0, 40.0), 3e10), ((10.0, 0.0, 30.0), 1e10)]
    plain = slm.Walker(osc, mats, lights, [0.0, 2.0]).render(12, 8, 1, 2)
    for emission in (None, {}, {1: (0.0, 0.0, 0.0)}):
        got = em.Walker(osc, mats, lights, [0.0, 2.0], emission=emission, table=tb, share=0.5).render(12, 8, 1, 2)
        assert (_bits(got) == _bits(plain)).all()
