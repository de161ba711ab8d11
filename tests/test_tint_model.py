"""The model of the tinted mirrors and glass (tests/tint_model.py) held to the rule's closed forms, without a GPU: with no effective flag the walker is the walker
underneath, bit for bit; .w never depends on the flags; a path whose first hit is a tinted mirror of tint t over an untinted remainder X is fl(t X) per channel; a path
through a tinted glass ball head on is fl(t fl(t X))."""
import numpy as np
import pytest

import raytracinggpu_amd as rt
from . import gloss_model as gm
from . import lights_model as lm
from . import tint_model as tn

f32 = np.float32
GOLD = (0.83, 0.61, 0.23)                            # no component is a dyadic rational: every product rounds
FLOOR = ((0, -1000, 0), 990, (0.5, 0.45, 0.4))
WALL = ((0, 0, -1030), 1000, (0.7, 0.5, 0.3))        # behind everything, seen from (0, 0, 55)
DIFFUSE = ((-14, -2, 14), 8, (0.3, 0.6, 0.7))


def _mirror(albedo, centre=(6, 0, 12), radius=10):
    return (centre, radius, albedo, 1, 1.0, 1.0)


def _glass(albedo, centre=(0, 0, 10), radius=9):
    return (centre, radius, albedo, 0, 1.5, 1.0)


def _scene(oracle, spheres):
    osc = oracle.Scene()
    for s in spheres:
        osc.add_sphere(s[0], s[1], s[2], *(s[3:] if len(s) > 3 else ()))
    return osc


def _walker(oracle, spheres, **kw):
    return tn.Walker(_scene(oracle, spheres), lm.materials(spheres), [rt.scenes.LIGHT], **kw)


def _words(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_the_fold_of_a_tinted_segment_is_one_product_per_channel():
    """fl(fl(fl((+0) t) / pi) + fl(t x)) = fl(t x) for t >= +0: the direct term is +0, and +0 + y is y (+0 for y = -0 never arises: t x >= +0)"""
    rng = np.random.default_rng(7)
    t = rng.random((4096, 3)).astype(f32)
    x = (rng.random((4096, 3)) * 8).astype(f32)
    t[:16] = 0
    x[8:24] = 0
    with np.errstate(under="ignore"):
        one = (((f32(0) * t).astype(f32) / f32(lm.PI)).astype(f32) + (t * x).astype(f32)).astype(f32)
    np.testing.assert_array_equal(_words(one), _words((t * x).astype(f32)))
    assert (_words(tn.fold([(f32(0), t[100])])) == 0).all()             # a lone tinted segment over nothing: +0
    seg_x = [(f32(1.5), np.array(GOLD, f32)), (f32(0.75), np.array([0.2, 0.9, 0.4], f32))]
    X = tn.fold(seg_x)
    for tint in (GOLD, (0.0, 0.5, 1.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)):
        tv = np.array(tint, f32)
        np.testing.assert_array_equal(_words(tn.fold([(f32(0), tv)] + seg_x)), _words((tv * X).astype(f32)))
        np.testing.assert_array_equal(_words(tn.fold([(f32(0), tv), (f32(0), tv)] + seg_x)), _words((tv * (tv * X).astype(f32)).astype(f32)))


@pytest.mark.parametrize("case", ["none", "a diffuse object", "white mirror, rough mirror and glass"])
def test_without_an_effective_flag_the_walker_is_the_walker_underneath(oracle, case):
    white = (1.0, 1.0, 1.0)
    spheres = [FLOOR, DIFFUSE, _mirror(white if case.startswith("white") else GOLD), _mirror(white if case.startswith("white") else GOLD, (-2, 12, 4), 6),
               _glass(white if case.startswith("white") else GOLD, (22, 0, 14), 8)]
    rough = {3: 0.25}
    tinted = {"none": (), "a diffuse object": (0, 1), "white mirror, rough mirror and glass": (2, 3, 4)}[case]
    base = gm.Walker(_scene(oracle, spheres), lm.materials(spheres), [rt.scenes.LIGHT], rough=rough).render(24, 16, 2, 3)
    w = _walker(oracle, spheres, rough=rough, tinted=tinted)
    got = w.render(24, 16, 2, 3)
    if case.startswith("white"):
        assert w.tinted == {2, 3, 4} and w.tints > 0 and w.facets > 0   # the flags ARE effective: the words are the same because fl(1 x) is x and +0 + x is x
    else:
        assert not w.tinted and w.tints == 0
    np.testing.assert_array_equal(_words(got), _words(base))            # .w included


def test_w_never_depends_on_the_flags_and_the_colour_does(oracle):
    spheres = [FLOOR, DIFFUSE, _mirror(GOLD), _glass((0.2, 0.8, 0.3), (-4, 10, 6), 6)]
    base = _walker(oracle, spheres).render(24, 16, 2, 3)
    for tinted in ((2,), (3,), (2, 3), (0, 1, 2, 3)):
        w = _walker(oracle, spheres, tinted=tinted)
        got = w.render(24, 16, 2, 3)
        assert w.tinted == set(tinted) - {0, 1} and w.tints > 0
        np.testing.assert_array_equal(_words(got[..., 3]), _words(base[..., 3]))
        assert (_words(got[..., :3]) != _words(base[..., :3])).any()


@pytest.mark.parametrize("tint", [GOLD, (0.0, 0.37, 0.91), (0.0, 0.0, 0.0)])
def test_a_first_hit_on_a_tinted_mirror_is_the_tint_times_the_untinted_remainder(oracle, tint):
    spheres = [FLOOR, DIFFUSE, _mirror(tint)]
    plain, flagged = _walker(oracle, spheres), _walker(oracle, spheres, tinted=(2,))
    cam = np.array([0, 0, 55], f32)
    tv = np.array(tint, f32)
    seen = lit = 0
    for k, (dx, dy) in enumerate([(x, y) for x in (-6, -3, 0, 3, 6) for y in (-5, -1, 3, 7)]):
        u = lm._normalize(lm._v(6 + dx, dy, 12 - 55))
        hit, oid, _, _ = plain.scene.intersect_all(cam, u, 1e-4)
        if not (hit and oid == 2):
            continue
        for segs in (1, 2, 4):
            X, rays = plain.path(cam, u, segs, k, 0)
            before = flagged.tints
            T, rays_t = flagged.path(cam, u, segs, k, 0)
            if flagged.tints - before != 1:                             # the remainder came back to the ball: not this closed form
                continue
            assert rays_t == rays
            np.testing.assert_array_equal(_words(T), _words((tv * X).astype(f32)))
            seen += 1
            lit += int((X > 0).any())
    assert seen >= 20 and lit >= 10


def test_through_a_tinted_glass_ball_head_on_the_tint_applies_twice(oracle):
    spheres = [WALL, _glass(GOLD)]
    plain, flagged = _walker(oracle, spheres), _walker(oracle, spheres, tinted=(1,))
    tv = np.array(GOLD, f32)
    for b in (2, 4):
        X = plain.render(1, 1, 1, b)
        T = flagged.render(1, 1, 1, b)
        assert flagged.tints % 2 == 0 and (X[0, 0, :3] > 0).all()
        assert T[0, 0, 3] == X[0, 0, 3]
        np.testing.assert_array_equal(_words(T[0, 0, :3]), _words((tv * (tv * X[0, 0, :3]).astype(f32)).astype(f32)))
    assert flagged.tints == 4                                           # in and out, at either depth: the wall's bounce does not come back through the ball
    # b = 1: the path ends inside the ball -- two tinted segments over nothing
    assert (_words(flagged.render(1, 1, 1, 1)[0, 0, :3]) == 0).all()


def test_a_material_decides_whether_a_flag_is_effective(oracle):
    spheres = [FLOOR, DIFFUSE, _mirror(GOLD), _glass(GOLD)]
    w = _walker(oracle, spheres, tinted=(0, 1, 2, 3), rough={2: 0.5})
    assert w.tinted == {2, 3} and set(w.rough) == {2}
