"""Generated scenes for the shading step: scene(family, seed) -> a plain description, the same bits for the reference (oracle/ref_harness.cpp `fuzz`), the
oracle and the device.  Pure numpy; every number is binary32-exact and finite, the draw is np.random.default_rng([family_index, seed]).

A description is a dict:
    spheres   float32 [n, 10]: centre(3) radius albedo(3) mirror n_in n_out, in object order (the mesh's slot left out)
    mesh      None, or dict(kind, vertices float32 [nv, 3], triangles int32 [nt, 3], albedo float32 [3], mirror, n_in, n_out, slot)
    light     float32 [4]: position(3) intensity
    cam       float32 [3];  pose: None or float32 [2] (yaw, pitch) for the posed-camera check
    W H spp num_bounce (ints), eps tri_tmin sigma (float32; sigma is 0)
    tied      None, or (i, j): object positions of two coincident spheres (family `ties`)

What each family is for is said at its function.  Camera and light stay outside every sphere unless a family puts them inside on purpose: a camera or a light
inside an opaque ball gives a black frame, which tests nothing.
"""
import numpy as np

F = np.float32
FAMILIES = ("room", "open", "ties", "glass", "light_edge", "odd_spheres", "with_mesh")
SEEDS = range(24)
MAX_OBJECTS = 16                      # RT_MAX_OBJECTS
GLASS_INDICES = (0.7, 1.0, 1.3, 1.5, 2.4)
ALBEDO_STEPS = (0.0, 0.25, 0.5, 1.0)
# the six wall spheres of the reference's scene (cpu_launcher.cpp:673-678): centre, radius; the room is the space between them, |x|, |z| < 60, -10 < y < 60
WALLS = (((0, 0, -1000), 940), ((0, -1000, 0), 990), ((0, 1000, 0), 940), ((-1000, 0, 0), 940), ((1000, 0, 0), 940), ((0, 0, 1000), 940))
CAMERA = (0.0, 0.0, 55.0)
MESH_KINDS = ("three_triangles", "axis_aligned_quads", "soup", "geometric_chain", "flat_faces")


def _row(centre, radius, albedo, mirror=0, n_in=1.0, n_out=1.0):
    return [centre[0], centre[1], centre[2], radius, albedo[0], albedo[1], albedo[2], mirror, n_in, n_out]


def _albedo(rng, steps=ALBEDO_STEPS, p=None):
    return [float(x) for x in rng.choice(steps, 3, p=p)]


def _bright(rng):
    """an albedo with at least one component of 0.5 or more"""
    a = _albedo(rng)
    a[int(rng.integers(3))] = float(rng.choice([0.5, 1.0]))
    return a


def _walls(rng, dark=0.15):
    p = [dark, (1 - dark) * 0.3, (1 - dark) * 0.35, (1 - dark) * 0.35]
    return [_row(c, r, _albedo(rng, p=p)) for c, r in WALLS]


def _material(rng, p=(0.5, 0.2, 0.3)):
    """-> (albedo, mirror, n_in, n_out): diffuse / mirror / glass"""
    k = rng.choice(3, p=p)
    if k == 0:
        return _bright(rng), 0, 1.0, 1.0
    if k == 1:
        return _albedo(rng), 1, 1.0, 1.0
    n_in, n_out = rng.choice(GLASS_INDICES, 2, replace=False)
    return _albedo(rng), 0, float(n_in), float(n_out)


def _outside(points, centre, radius, margin=0.5):
    c = np.asarray(centre, np.float64)
    return all(np.linalg.norm(np.asarray(p, np.float64) - c) > abs(radius) + margin for p in points)


def _free_spheres(rng, n, lo, hi, radii, keep_out, material=_material):
    """n spheres with centres in the box [lo, hi] that contain none of the points keep_out"""
    rows = []
    while len(rows) < n:
        c = [float(F(x)) for x in rng.uniform(lo, hi)]
        r = float(F(rng.uniform(*radii)))
        if _outside(keep_out, c, r):
            rows.append(_row(c, r, *material(rng)))
    return rows


def _free_point(rng, lo, hi, rows):
    while True:
        p = [float(F(x)) for x in rng.uniform(lo, hi)]
        if all(_outside([p], row[:3], row[3]) for row in rows):
            return p


def _finish(rng, rows, light, cam=CAMERA, mesh=None, num_bounce=3, spp=1, eps=1e-3, tied=None, shuffle=False, odd_light=0.2):
    W, H = 64, 48                                                      # scene() makes every third frame 61 x 43
    if rng.random() < odd_light:                                       # a negative or a huge light: negative channels (NaN in the 8-bit image) and overflow in every family
        light = list(light[:3]) + [float(rng.choice([-3e10, 3e38]))]
    order = np.arange(len(rows))
    if shuffle:
        order = rng.permutation(len(rows))
        if tied is not None:
            inv = np.argsort(order)
            tied = (int(inv[tied[0]]), int(inv[tied[1]]))
    d = dict(spheres=np.array([rows[k] for k in order], np.float32).reshape(-1, 10), mesh=mesh, light=np.array(light, np.float32), cam=np.array(cam, np.float32),
             pose=np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.1, 0.4)], np.float32), W=int(W), H=int(H), spp=int(spp), num_bounce=int(num_bounce),
             eps=F(eps), tri_tmin=F(1e-4), sigma=F(0.0), tied=tied)
    assert len(d["spheres"]) + (mesh is not None) <= MAX_OBJECTS
    return d


# ---------------------------------------------------------------------------------------------------------------------------------- the families
def _room(rng):
    """the six walls with albedo components from {0, 0.25, 0.5, 1} and 2 to 9 spheres of random materials, the object order shuffled, the light anywhere in the room"""
    cam = [float(F(x)) for x in (rng.uniform(-10, 10), rng.uniform(-4, 8), rng.uniform(45, 57))]
    balls = _free_spheres(rng, int(rng.integers(2, 10)), (-30, -8, -30), (30, 30, 40), (2, 9), [cam])
    light = _free_point(rng, (-50, -5, -50), (50, 50, 50), balls) + [3e10]
    return _finish(rng, _walls(rng) + balls, light, cam, num_bounce=rng.integers(2, 7), spp=rng.integers(1, 3), shuffle=True)


def _open(rng):
    """no walls: 8 to 16 spheres clustered in the view with the light among them; camera rays and shadow rays miss often (P' = O + 1e9 u, cpu:560)"""
    balls = _free_spheres(rng, int(rng.integers(8, 17)), (-26, -19, -20), (26, 19, 25), (5, 11), [CAMERA], material=lambda g: _material(g, (0.8, 0.08, 0.12)))
    light = _free_point(rng, (-26, -19, 5), (26, 19, 45), balls) + [3e10]
    return _finish(rng, balls, light, num_bounce=rng.integers(1, 6), spp=rng.integers(1, 3), shuffle=True)


def _ties(rng):
    """equal t (the strict '<' of cpu:554 keeps the earlier object): two coincident spheres of different materials in a drawn order, a concentric one, spheres tangent to
    each other and to the floor; every centre on a grid of 4 with power-of-two radii and the camera on a grid point"""
    cam = (0.0, 0.0, 56.0)
    g = lambda lo, hi: float(4 * rng.integers(lo, hi + 1))
    rows = _walls(rng, dark=0.0)
    c, r = (g(-3, 3), g(0, 3), g(-2, 4)), float(rng.choice([4.0, 8.0]))
    mats = [(_bright(rng), 0, 1.0, 1.0), (_albedo(rng), 1, 1.0, 1.0), (_albedo(rng), 0, 1.5, 1.0)]
    a, b = rng.choice(3, 2, replace=False)
    first, second = mats[a], mats[b]
    if rng.random() < 0.4:                                             # two diffuse balls that differ in colour only
        first = (_bright(rng), 0, 1.0, 1.0)
        second = ([(x + 0.5) % 1.25 for x in first[0]], 0, 1.0, 1.0)
    tied = (len(rows), len(rows) + 1)
    rows += [_row(c, r, *first), _row(c, r, *second)]
    rows.append(_row(c, r / 2, _bright(rng)))                          # concentric: seen where the outer one is glass
    c2, r2 = (g(-5, 5), g(0, 4), g(-3, 3)), float(rng.choice([2.0, 4.0]))
    rows.append(_row(c2, r2, *_material(rng)))
    rows.append(_row((c2[0] + 2 * r2, c2[1], c2[2]), r2, *_material(rng)))          # tangent to the previous one at a grid point
    r3 = float(rng.choice([2.0, 4.0, 8.0]))
    rows.append(_row((g(-5, 5), -10.0 + r3, g(-2, 6)), r3, *_material(rng)))        # resting on the floor: tangent to a wall
    for _ in range(int(rng.integers(0, 5))):
        rows.append(_row((g(-6, 6), g(-1, 5), g(-6, 6)), float(rng.choice([1.0, 2.0, 4.0])), *_material(rng)))
    rows = rows[:6] + [q for q in rows[6:] if _outside([cam], q[:3], q[3])]
    light = _free_point(rng, (-40, 0, -20), (40, 50, 50), rows[6:]) + [3e10]
    light = [float(np.round(x)) for x in light[:3]] + [3e10]
    return _finish(rng, rows, light, cam, num_bounce=rng.integers(2, 6), spp=1, tied=tied)


def _glass(rng):
    """nested and overlapping glass with indices from {0.7, 1, 1.3, 1.5, 2.4} on either side: inner glass whose n_out is the outer's n_in (the demo scene's pattern) and inner
    glass where it is not (out2in false on entry), total reflection from the thin side (n_in < n_out), the camera inside a glass ball, two mirror balls and two mirror walls
    facing each other, up to 16 segments"""
    rows = _walls(rng)
    if rng.random() < 0.5:                                             # the side walls as mirrors: paths run between them to the segment limit
        for k in (3, 4):
            rows[k][7] = 1
    cam = list(CAMERA)
    idx = lambda: [float(x) for x in rng.choice(GLASS_INDICES, 2, replace=False)]
    if rng.random() < 0.3:                                             # the camera inside glass
        n_in, n_out = idx()
        rows.append(_row((cam[0] + float(F(rng.uniform(-2, 2))), cam[1], cam[2] - 3.0), 8.0, _albedo(rng), 0, n_in, n_out))
    for _ in range(int(rng.integers(1, 4))):                           # nested pairs
        c = [float(F(x)) for x in rng.uniform((-28, -4, -20), (28, 22, 30))]
        r = float(F(rng.uniform(5, 11)))
        n_in, n_out = idx()
        inner_out = n_in if rng.random() < 0.5 else float(rng.choice([x for x in GLASS_INDICES if x != n_in]))
        inner_in = float(rng.choice([x for x in GLASS_INDICES if x != inner_out]))
        inner = _row([c[0] + float(F(rng.uniform(-1, 1))), c[1], c[2]], float(F(r * rng.uniform(0.4, 0.85))), _albedo(rng), 0, inner_in, inner_out)
        outer = _row(c, r, _albedo(rng), 0, n_in, n_out)
        rows += [inner, outer] if rng.random() < 0.5 else [outer, inner]
    for _ in range(int(rng.integers(1, 4))):                           # lone and overlapping glass
        c = [float(F(x)) for x in rng.uniform((-28, -6, -20), (28, 22, 35))]
        n_in, n_out = idx()
        rows.append(_row(c, float(F(rng.uniform(4, 10))), _albedo(rng), 0, n_in, n_out))
    if rng.random() < 0.6:                                             # two mirror balls facing each other
        y, z, r = float(F(rng.uniform(0, 15))), float(F(rng.uniform(-10, 25))), float(F(rng.uniform(6, 10)))
        rows += [_row((-14.0, y, z), r, _albedo(rng), 1), _row((14.0, y, z), r, _albedo(rng), 1)]
    rows = rows[:6] + rows[6:MAX_OBJECTS]
    keep = [q for q in rows[6:] if q[7] == 0 and q[8] != q[9] or _outside([cam], q[:3], q[3])]
    light = _free_point(rng, (-45, 5, -40), (45, 50, 50), keep) + [3e10]
    return _finish(rng, rows[:6] + keep, light, cam, num_bounce=rng.choice([5, 8, 12, 15, 15]), spp=1)


def _steps(x, k):
    x = F(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
    return float(x)


def _light_edge(rng):
    """the light on a diffuse surface or a few float steps above or below it (wf_anyhit_bound's -inf), at a ball's centre, inside glass, at the camera; intensity 0, negative
    and 3e38; eps 0 and 1e-6; albedo components of 4 over 16 segments (the 2^126 guard of the dead-channel rule) and negative ones"""
    rows = _walls(rng, dark=0.05)
    cam = list(CAMERA)
    balls = _free_spheres(rng, int(rng.integers(2, 6)), (-28, -6, -25), (28, 25, 35), (3, 9), [cam], material=lambda g: _material(g, (0.6, 0.15, 0.25)))
    balls[0][4:10] = _bright(rng) + [0, 1.0, 1.0]                      # ball 0 is diffuse, ball 1 is glass
    balls[1][4:10] = _albedo(rng) + [0, 1.5, 1.0]
    rows += balls
    where = rng.choice(["floor", "ball", "centre", "in_glass", "camera", "free"], p=[0.35, 0.2, 0.08, 0.12, 0.1, 0.15])
    k = int(rng.integers(-3, 4))
    if where == "floor":                                               # on the floor ball's top, +- k float steps: every floor point sees it at mx = 0
        x, z = float(F(rng.uniform(-30, 30))), float(F(rng.uniform(-20, 40)))
        y = np.sqrt(np.float64(990.0) ** 2 - x * x - z * z) - 1000.0
        pos = [x, _steps(y, k), z]
    elif where == "ball":
        c, r = np.array(balls[0][:3], np.float64), balls[0][3]
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        pos = [float(F(v)) for v in c + r * d]
        ax = int(np.argmax(np.abs(d)))
        pos[ax] = _steps(pos[ax], k)
    elif where == "centre":
        pos = list(balls[0][:3])
    elif where == "in_glass":
        pos = [balls[1][0] + float(F(rng.uniform(-1, 1))), balls[1][1], balls[1][2]]
    elif where == "camera":
        pos = list(cam)
    else:
        pos = _free_point(rng, (-45, 0, -40), (45, 50, 50), balls)
    intensity = float(rng.choice([3e10, 0.0, -3e10, 3e38], p=[0.45, 0.1, 0.25, 0.2]))
    eps = float(rng.choice([1e-3, 0.0, 1e-6], p=[0.4, 0.3, 0.3]))
    b = int(rng.choice([2, 4, 15], p=[0.4, 0.3, 0.3]))
    mode = rng.choice(["plain", "four", "negative"], p=[0.4, 0.35, 0.25])
    for q in rows:
        if mode == "four" and rng.random() < 0.7:
            q[4:7] = [float(x) for x in rng.choice([4.0, 1.0, 0.0], 3, p=[0.6, 0.2, 0.2])]
        if mode == "negative" and rng.random() < 0.5:
            q[4 + int(rng.integers(3))] = float(rng.choice([-0.5, -1.0]))
    if mode == "four":
        b = 15
    return _finish(rng, rows, pos + [intensity], cam, num_bounce=b, spp=1, eps=eps, odd_light=0.0)


def _odd_spheres(rng):
    """radius 0, -8, 1e-3 and a ball of 1e6 around everything; the camera exactly on a surface; 16 spheres"""
    cam = list(CAMERA)
    enclosed = rng.random() < 0.4
    rows = [_row((0.0, 0.0, 0.0), 1e6, _bright(rng))] if enclosed else _walls(rng)
    if enclosed and rng.random() < 0.5:
        rows += _walls(rng)[:int(rng.integers(1, 4))]
    spot = lambda: [float(F(x)) for x in rng.uniform((-22, -6, -15), (22, 18, 30))]
    rows.append(_row(spot(), 0.0, _bright(rng)))
    rows.append(_row(spot(), -8.0, *_material(rng)))
    rows.append(_row(spot(), 1e-3, _bright(rng)))
    if rng.random() < 0.6:                                             # the camera on the surface: looking into the ball, or away from it
        r = float(rng.choice([4.0, 10.0]))
        rows.append(_row((0.0, 0.0, 55.0 - r if rng.random() < 0.5 else 55.0 + r), r, *_material(rng, (0.3, 0.1, 0.6))))
    n = MAX_OBJECTS if rng.random() < 0.4 else int(rng.integers(len(rows) + 1, MAX_OBJECTS))
    rows += _free_spheres(rng, n - len(rows), (-26, -8, -20), (26, 20, 30), (2, 7), [cam])
    light = _free_point(rng, (-40, 5, -30), (40, 45, 50), rows[1:] if enclosed else rows[6:]) + [3e10]
    return _finish(rng, rows, light, cam, num_bounce=rng.integers(1, 6), spp=rng.integers(1, 3))


def _with_mesh(rng):
    """one of the small synthetic meshes of test_gpu_parity._synthetic_mesh at a random object slot among walls and spheres, diffuse, mirror or glass; spheres cut through it"""
    from .test_gpu_parity import _synthetic_mesh
    kind = MESH_KINDS[int(rng.integers(len(MESH_KINDS)))]
    v, t = _synthetic_mesh(kind, np.random.default_rng(int(rng.integers(1 << 30))))
    scale, off = F(rng.choice([0.5, 0.75, 1.0])), np.array([rng.integers(-6, 7), rng.integers(0, 9), rng.integers(-4, 13)], np.float32)
    v = ((v.astype(np.float32) * scale).astype(np.float32) + off).astype(np.float32)
    albedo, mirror, n_in, n_out = _material(rng, (0.4, 0.3, 0.3))
    cam = list(CAMERA)
    rows = _walls(rng)
    cut = v[rng.integers(0, len(v), int(rng.integers(1, 4)))]           # balls centred on mesh vertices
    for c in cut:
        r = float(F(rng.uniform(1.5, 4)))
        if _outside([cam], c, r):
            rows.append(_row([float(x) for x in c], r, *_material(rng)))
    rows += _free_spheres(rng, int(rng.integers(0, 4)), (-30, -8, -30), (30, 30, 40), (2, 7), [cam])
    light = _free_point(rng, (-45, 5, -10), (45, 50, 50), rows[6:]) + [3e10]
    d = _finish(rng, rows, light, cam, num_bounce=rng.integers(1, 6), spp=rng.integers(1, 3), shuffle=True)
    d["mesh"] = dict(kind=kind, vertices=v, triangles=np.asarray(t, np.int32), albedo=np.array(albedo, np.float32), mirror=int(mirror), n_in=F(n_in), n_out=F(n_out),
                     slot=int(rng.integers(0, len(rows) + 1)))
    return d


_BUILD = dict(room=_room, open=_open, ties=_ties, glass=_glass, light_edge=_light_edge, odd_spheres=_odd_spheres, with_mesh=_with_mesh)


def scene(family, seed):
    """61 x 43 = 2623 pixels (npix % 4 == 3, partial 8 x 8 tiles) for every third seed, 64 x 48 for the rest"""
    d = _BUILD[family](np.random.default_rng([FAMILIES.index(family), int(seed)]))
    return resized(d, 61, 43) if int(seed) % 3 == 2 else d


def resized(d, W, H, spp=None, eps=None):
    """the same scene with another frame size (and sample count, and eps)"""
    d = dict(d, W=int(W), H=int(H))
    if spp is not None:
        d["spp"] = int(spp)
    if eps is not None:
        d["eps"] = F(eps)
    return d


def swapped(d):
    """family `ties`: the two coincident spheres trade places in the object order"""
    i, j = d["tied"]
    s = d["spheres"].copy()
    s[[i, j]] = s[[j, i]]
    return dict(d, spheres=s)


def animated(family, seed, k):
    """draw k of an animated sequence: scene(family, seed) with its materials, object order and constants, and the light and the spheres' poses moved by the draw
    np.random.default_rng([family_index, seed, k]); k = 0 is the scene itself.  `ties` moves every ball by one common grid step, so that the ties stay."""
    d = scene(family, seed)
    if k == 0:
        return d
    rng = np.random.default_rng([FAMILIES.index(family), int(seed), int(k)])
    s = d["spheres"].copy()
    small = np.abs(s[:, 3]) < 100                                      # the walls stay
    if family == "ties":
        s[small, :3] += (rng.integers(-2, 3, 3) * 0.5).astype(np.float32)
    else:
        s[small, :3] += rng.uniform(-1.5, 1.5, (int(small.sum()), 3)).astype(np.float32)
        s[small, 3] = (s[small, 3] * rng.uniform(0.8, 1.2, int(small.sum())).astype(np.float32)).astype(np.float32)
    light = d["light"].copy()
    light[:3] += rng.uniform(-3, 3, 3).astype(np.float32)
    return dict(d, spheres=s.astype(np.float32), light=light.astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------ description -> the three consumers
def object_order(d):
    """-> list of ("sphere", row) / ("mesh", mesh) in Scene::objects order"""
    out = [("sphere", r) for r in d["spheres"]]
    if d["mesh"] is not None:
        out.insert(d["mesh"]["slot"], ("mesh", d["mesh"]))
    return out


def _py(x):
    return [float(v) for v in x]


def upload_args(d):
    """-> (spheres, mesh, light, camera) for Context.scene_upload; the mesh through the product's own builder (hostlib.build_mesh)"""
    spheres = [(_py(r[:3]), float(r[3]), _py(r[4:7]), int(r[7]), float(r[8]), float(r[9])) for r in d["spheres"]]
    mesh = None
    if d["mesh"] is not None:
        from raytracinggpu_amd import hostlib
        m = d["mesh"]
        mesh = hostlib.build_mesh(m["vertices"], m["triangles"], albedo=_py(m["albedo"]), object_slot=m["slot"])
        mesh.update(mirror=m["mirror"], in_refraction_index=float(m["n_in"]), out_refraction_index=float(m["n_out"]))
    return spheres, mesh, (_py(d["light"][:3]), float(d["light"][3])), (_py(d["cam"]), None)


def oracle_scene(oracle, d):
    s = oracle.Scene()
    for kind, o in object_order(d):
        if kind == "sphere":
            s.add_sphere(o[:3], float(o[3]), o[4:7], int(o[7]), float(o[8]), float(o[9]))
        else:
            s.add_mesh(oracle.Mesh.from_arrays(o["vertices"], o["triangles"], albedo=_py(o["albedo"])).set_material(o["mirror"], float(o["n_in"]), float(o["n_out"])).build_bvh())
    s.set_light(d["light"][:3], float(d["light"][3]))
    return s


def oracle_render(oracle, d, scene=None, pose=None, **kw):
    """the oracle's frame of the description (counter RNG unless kw says otherwise) -> (rgba, third result of Scene.render)"""
    s = scene or oracle_scene(oracle, d)
    args = dict(sigma=float(d["sigma"]), eps=float(d["eps"]), tri_tmin=float(d["tri_tmin"]), cam=_py(d["cam"]), want_rgb8=False)
    if pose is not None:
        args.update(pose=(float(pose[0]), float(pose[1])), fov=np.float32(np.pi / 2))
    args.update(kw)
    rgba, _, third = s.render(d["W"], d["H"], d["spp"], d["num_bounce"], **args)
    return rgba, third


def pack(d):
    """the description as one float32 vector (every integer in it is below 2^24): what oracle/ref_harness.cpp `fuzz` reads and tests/golden/ref_fuzz.npz stores.
    [W H spp num_bounce eps tri_tmin cam(3) light(3) intensity n_spheres mesh_slot] spheres(10 each) then, with a mesh, [albedo(3) mirror n_in n_out nv nt] vertices triangles"""
    m = d["mesh"]
    head = [d["W"], d["H"], d["spp"], d["num_bounce"], d["eps"], d["tri_tmin"], *d["cam"], *d["light"], len(d["spheres"]), -1 if m is None else m["slot"]]
    parts = [np.array(head, np.float32), d["spheres"].reshape(-1)]
    if m is not None:
        parts += [np.array([*m["albedo"], m["mirror"], m["n_in"], m["n_out"], len(m["vertices"]), len(m["triangles"])], np.float32), m["vertices"].reshape(-1),
                  m["triangles"].astype(np.float32).reshape(-1)]
    return np.concatenate(parts).astype(np.float32)
