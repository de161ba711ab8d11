"""The dead-last permission (raytracinggpu_amd/csrc/rt_deadlast.h: dead_last_permit, compiled into the host library as rth_dead_last_permit -- the text the render path
compiles), checked by brute force on the CPU.

The device rule closes the last continuation ray of a dead path as the hit of the sphere its sphere tests found, whatever the mesh would have said.  The pixel is the
reference's if the last segment's ans = fl(fl(fl(l alb) / pi) + fl(alb (+0))) is FINITE for every object the ray could really have hit and for the sphere shaded in its
place, where l = fl(intensity / (4 pi |L - P|^2) mx) is the direct term at the computed hit point P (direct_term, restated below in binary32 with its binary64 inside).
The permission promises that from the scene alone.  So: wherever it is granted, no point a hit can compute -- on a sphere's surface or in the mesh's root box, off it by
the header's budget 2^-9 S (1 + 2^-7), under the normal that faces the light -- may give a non-finite ans or a direct term outside [+0, 2^96); and wherever one of its
conditions fails it must be refused.  Lights approach a sphere's surface and the root box from both sides, intensities go up to 3e38, albedo components come from
{+0, -0, denormal, 1, > 1, negative, inf, NaN}; the scene that broke the first dead-channel guard (tests/scene_fuzz.py light_edge, seed 19: 3e38 over walls of albedo 4)
is among them."""
import numpy as np
import pytest

from raytracinggpu_amd import hostlib, scenes

from . import scene_fuzz as sf
from .test_dead_channels import DIRECT_END, _bits, f32, fold

BUDGET = 2.0 ** -9 * (1 + 2.0 ** -7)        # rt_deadlast.h: how far a computed hit point lies off its surface, in units of S
GOOD_ALBEDO = [0.0, 1e-45, 1e-40, 0.25, 1.0]
BAD_ALBEDO = [-0.0, np.nextafter(f32(1), f32(2)), 4.0, -0.5, np.inf, -np.inf, np.nan]
INTENSITIES = [0.0, 1.0, 3e10, 1e30, 3e38]


def make(spheres, light, box=None, alb=None, mirror=None, n_in=None, n_out=None):
    """one DeadLastScene: spheres [(centre, R, albedo)], light (x, y, z, intensity), box (lo, hi) with the mesh as the object after the spheres (albedo: the cat's)"""
    s = np.zeros((), hostlib.DEAD_LAST_SCENE)
    n = len(spheres)
    s["n_spheres"], s["n_objects"] = n, n + (box is not None)
    for k, (c, r, a) in enumerate(spheres):
        s["sph"][k] = [c[0], c[1], c[2], r]
        s["alb"][k] = a
    if box is not None:
        s["alb"][n] = scenes.CAT_ALBEDO
        s["have_box"], s["lo"], s["hi"] = 1, box[0], box[1]
    s["n_in"][:], s["n_out"][:] = 1.0, 1.0
    for name, v in (("alb", alb), ("mirror", mirror), ("n_in", n_in), ("n_out", n_out)):
        for k, x in (v or {}).items():
            s[name][k] = x
    s["L"], s["intensity"] = light[:3], light[3]
    return s


def permit(s, **facts):
    return bool(hostlib.dead_last_permit(s, **facts)[0])


def cat_box():
    v, _ = scenes.load_cat_arrays()
    return v.min(0), v.max(0)


def cat_scene(**kw):
    return make([(c, r, a) for c, r, a in scenes.WALLS], list(scenes.LIGHT[0]) + [scenes.LIGHT[1]], cat_box(), **kw)


def direct_term(intensity, L, P, N):
    """direct_term of rt_shade.hip.h over arrays [n, 3]: binary32 outside, binary64 inside"""
    with np.errstate(all="ignore"):
        v = (f32(L) - P).astype(f32)
        n2 = ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]).astype(f32) + v[:, 2] * v[:, 2]).astype(f32)
        wl = (v / np.sqrt(n2).astype(f32)[:, None]).astype(f32)
        dn = ((N[:, 0] * wl[:, 0] + N[:, 1] * wl[:, 1]).astype(f32) + N[:, 2] * wl[:, 2]).astype(f32)
        mx = np.where(dn < 0, f32(0), dn)
        return (np.float64(f32(intensity)) / (4 * np.pi * n2.astype(np.float64)) * mx.astype(np.float64)).astype(f32)


def reachable_points(s, rng, n_random=64):
    """Hit points a ray could compute in scene s, worst cases first: for every surface the point nearest the light, pushed TOWARDS the light by the budget; the same
    away from it; random points of every sphere and of the box, pushed by up to the budget in random directions"""
    L = s["L"].astype(np.float64)
    S = float(np.linalg.norm(L))
    for k in range(int(s["n_spheres"])):
        S = max(S, float(np.linalg.norm(s["sph"][k][:3].astype(np.float64)) + s["sph"][k][3]))
    if s["have_box"]:
        S = max(S, float(np.sqrt((np.maximum(s["lo"].astype(np.float64) ** 2, s["hi"].astype(np.float64) ** 2)).sum())))
    push = BUDGET * S
    pts = []
    unit = lambda v: v / max(np.linalg.norm(v), 1e-300)
    for k in range(int(s["n_spheres"])):
        c, r = s["sph"][k][:3].astype(np.float64), float(s["sph"][k][3])
        d = unit(L - c) if np.linalg.norm(L - c) > 0 else np.array([1.0, 0, 0])
        near = c + r * d
        pts += [near + push * unit(L - near), near - push * unit(L - near), near]
        dirs = rng.normal(size=(n_random, 3)); dirs /= np.linalg.norm(dirs, axis=1)[:, None]
        off = rng.normal(size=(n_random, 3)); off /= np.linalg.norm(off, axis=1)[:, None]
        pts += list(c + r * dirs + push * rng.uniform(0, 1, (n_random, 1)) * off)
    if s["have_box"]:
        lo, hi = s["lo"].astype(np.float64), s["hi"].astype(np.float64)
        near = np.clip(L, lo, hi)
        pts += [near + push * unit(L - near), near]
        pts += list(rng.uniform(lo, hi, (n_random, 3)))
    return np.array(pts).astype(f32)


def assert_finite_everywhere(s, rng):
    """the claim, for a scene whose permission was granted"""
    P = reachable_points(s, rng)
    L = s["L"].astype(f32)
    with np.errstate(all="ignore"):
        v = (L - P).astype(np.float64)
        facing = (v / np.maximum(np.linalg.norm(v, axis=1), 1e-300)[:, None]).astype(f32)    # mx at its largest
    other = rng.normal(size=P.shape); other = (other / np.linalg.norm(other, axis=1)[:, None]).astype(f32)
    for N in (facing, other):
        l = direct_term(s["intensity"], L, P, N)
        assert np.isfinite(l).all(), (s["L"], s["intensity"], l[~np.isfinite(l)][:4])
        assert (_bits(np.abs(l)) < DIRECT_END).all(), (s["L"], s["intensity"], l.max())
        for k in range(int(s["n_objects"])):                          # the last segment's fold for every object's albedo
            alb = np.broadcast_to(s["alb"][k], (len(l), 1, 3)).astype(f32)
            ans, _ = fold(np.ones((len(l), 1), bool), alb, l[:, None])
            assert np.isfinite(ans).all(), (k, s["alb"][k], l[~np.isfinite(ans).all(1)][:4])


def test_the_headline_scene_is_permitted_and_every_fact_is_needed():
    s = cat_scene()
    assert permit(s)
    for fact in ("plain", "anyhit", "deadch", "knob"):
        assert not permit(s, **{fact: 0}), fact
    assert permit(s, knob=7)                                          # any non-zero knob is "on"
    assert_finite_everywhere(s, np.random.default_rng(1))


def test_materials_refuse():
    n = len(scenes.WALLS)
    for k in (0, 3, n):                                               # a wall, another wall, the mesh
        assert not permit(cat_scene(mirror={k: 1})), k
        assert not permit(cat_scene(n_in={k: 1.5})), k
        assert not permit(cat_scene(n_out={k: 1.5})), k
        assert not permit(cat_scene(n_in={k: np.nan}, n_out={k: np.nan})), k      # the kernel's n_in != n_out holds for NaN: glass there, refused here
        assert permit(cat_scene(n_in={k: 1.5}, n_out={k: 1.5})), k               # equal indices: diffuse by the kernel's test
        for c in range(3):
            for a in GOOD_ALBEDO:
                alb = list(cat_scene()["alb"][k]); alb[c] = a
                assert permit(cat_scene(alb={k: alb})), (k, c, a)
            for a in BAD_ALBEDO:
                alb = list(cat_scene()["alb"][k]); alb[c] = a
                assert not permit(cat_scene(alb={k: alb})), (k, c, a)
    s = cat_scene(); s["smooth"] = 1                                  # a mesh that shades with vertex normals: nobody validates them
    assert not permit(s)
    # an object past n_objects is nobody's business
    s = cat_scene(); s["mirror"][n + 1] = 1; s["alb"][n + 2] = [4, 4, 4]
    assert permit(s)


def test_light_refuses():
    base = cat_scene()
    for bad in (-1.0, -0.0, np.inf, -np.inf, np.nan):
        s = base.copy(); s["intensity"] = bad
        assert not permit(s), bad
    for c in range(3):
        for bad in (np.inf, -np.inf, np.nan):
            s = base.copy(); s["L"][c] = bad
            assert not permit(s), (c, bad)
    lo, hi = cat_box()
    for where in ((lo + hi) / 2, lo, hi, [(lo[0] + hi[0]) / 2, hi[1], (lo[2] + hi[2]) / 2]):      # inside the root box, on two corners, on a face
        s = base.copy(); s["L"] = where
        assert not permit(s), where
    c, r, _ = scenes.WALLS[1]                                          # the floor: on its surface, a float step above and below, and within the margin
    top = np.array([0.0, c[1] + r, 0.0])
    for dy in (0.0, 1e-3, -1e-3, 1.0, -1.0, 5.0):
        s = make([(c, r, a) for c, r, a in scenes.WALLS], [top[0], top[1] + dy, top[2], 1.0])
        assert not permit(s), dy
    for r_bad in (0.0, -8.0, np.inf, np.nan):                          # a sphere no margin can be formed for
        s = base.copy(); s["sph"][2][3] = r_bad
        assert not permit(s), r_bad
    s = base.copy(); s["intensity"] = 3e38                              # 51 units from the nearest wall: 3e38 / (4 pi 36^2) is far above 2^96
    assert not permit(s)


@pytest.mark.parametrize("geometry", ["unit_sphere", "walls", "walls_and_box", "box_alone"])
def test_brute_force_lights_towards_a_surface(geometry):
    """lights at S 2^-k from a sphere's surface, inside and outside it, and from the root box, every intensity: granted means finite everywhere, and the sweep must see
    both answers and a refused light that would indeed have broken the guard"""
    rng = np.random.default_rng(7)
    box = None
    if geometry == "unit_sphere":
        spheres = [((0.5, -0.25, 0.125), 1.0, (0.0, 1.0, 0.25))]
    elif geometry == "box_alone":
        spheres, box = [], (np.array([-3.0, -2.0, -1.0], f32), np.array([2.0, 5.0, 4.0], f32))
    else:
        spheres = [(c, r, a) for c, r, a in scenes.WALLS]
        box = cat_box() if geometry == "walls_and_box" else None
    targets = []                                                      # (surface point, outward unit direction)
    if spheres:
        c, r, _ = spheres[0]
        d = np.array([0.6, 0.0, 0.8]) if geometry == "unit_sphere" else -np.array(c, np.float64) / np.linalg.norm(c)     # (a wall: the side that faces the room)
        targets.append((np.array(c, np.float64) + r * d, d))
    if box is not None:
        mid = (box[0].astype(np.float64) + box[1]) / 2
        targets.append((np.array([mid[0], box[1][1], mid[2]]), np.array([0.0, 1.0, 0.0])))                    # the top face
        targets.append((box[1].astype(np.float64), np.ones(3) / np.sqrt(3)))                                      # a corner
    S = max([np.linalg.norm(c) + r for c, r, _ in spheres] + ([float(np.sqrt(np.maximum(box[0] ** 2, box[1] ** 2).sum()))] if box is not None else []))
    granted = refused = broke = 0
    for p, d in targets:
        for k in range(0, 31):
            for side in (1.0, -1.0):
                L = p + side * S * 2.0 ** -k * d
                for inten in INTENSITIES:
                    s = make(spheres, list(L) + [inten], box)
                    if permit(s):
                        granted += 1
                        assert_finite_everywhere(s, rng)
                    else:
                        refused += 1
                        near = np.array([p], np.float64).astype(f32)
                        l = direct_term(inten, s["L"], near, np.array([side * d], np.float64).astype(f32))
                        broke += int(not np.isfinite(l[0]) or _bits(np.abs(l))[0] >= DIRECT_END)
    print(geometry, "granted", granted, "refused", refused, "refused lights whose direct term at the nearest point leaves the guard", broke)
    assert granted > 0 and refused > 0 and broke > 0


def test_light_edge_seed_19():
    """3e38 over walls of albedo 4, a glass ball among them: refused as it is; refused with every object made diffuse (the albedo); and with the albedos brought into
    [0, 1] the answer is the bound's alone -- granted only if every reachable hit is finite"""
    d = sf.scene("light_edge", 19)
    rows = d["spheres"]
    assert float(d["light"][3]) == f32(3e38) and (rows[:, 4:7] == 4).any()
    as_is = make([(r[:3], r[3], r[4:7]) for r in rows], d["light"], mirror={k: int(r[7]) for k, r in enumerate(rows)},
                 n_in={k: r[8] for k, r in enumerate(rows)}, n_out={k: r[9] for k, r in enumerate(rows)})
    assert not permit(as_is)
    diffuse = make([(r[:3], r[3], r[4:7]) for r in rows], d["light"])
    assert not permit(diffuse)
    clamped = make([(r[:3], r[3], np.clip(r[4:7], 0, 1)) for r in rows], d["light"])
    assert not permit(clamped)                                        # a room of 60 units cannot hold a light of 3e38: 3e38 / (4 pi 100^2) > 2^96
    for inten in (3e10, 1e30):
        s = clamped.copy(); s["intensity"] = inten
        if permit(s):
            assert_finite_everywhere(s, np.random.default_rng(19))
    # every scene of the family, as generated: whatever is granted is finite everywhere
    for seed in sf.SEEDS:
        e = sf.scene("light_edge", seed)
        r = e["spheres"]
        s = make([(q[:3], q[3], q[4:7]) for q in r], e["light"], mirror={k: int(q[7]) for k, q in enumerate(r)},
                 n_in={k: q[8] for k, q in enumerate(r)}, n_out={k: q[9] for k, q in enumerate(r)})
        if permit(s):
            assert_finite_everywhere(s, np.random.default_rng(seed))
