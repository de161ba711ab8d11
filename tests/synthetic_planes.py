"""Seeded synthetic inputs for rt_denoise, rt_denoise_var and rt_temporal_accumulate (test infrastructure): planes built so that the branches of the kernels run, which
rendered frames leave to the accident of the scene.  tests/test_synthetic_filters_model.py proves on the CPU that they do (the feature minimums below); the same
cases then go to the device in tests/test_gpu_synthetic_filters.py.

The scene.  Every pixel's hit point lies on its camera ray (the ray of denoise_model.camera_rays: direction (j + 0.5 - W / 2, H / 2 - i - 0.5, z)): P = O + v scale(id),
scale a power of two by object id, so every object is a plane of constant z and objects of different scale lie on different planes.  Object ids come in blocks: a few
"mega" blocks wider than 2 * 128 pixels where the frame allows it (ids 0 .. 3: same-id taps exist at every step), with small islands of ids 4 .. 15 and of misses
scattered in them, some placed on multiples of 32 and 8 (the kernel's tile seams at step 1).  Normals tilt by 0.002 and albedos vary by a few percent, gently enough
that the default k_* keep the taps; colours are 1e5-sized levels by object with 1 % noise.

Exactness.  With the camera (O, fov = pi / 2) the constant z is -W / 2 exactly, scale(id) v and O + scale(id) v are exact in binary32, k = b / d.z = 1 / scale exactly
and gx = j + 0.5, gy = i + 0.5 exactly: with nothing moved every pixel reprojects onto itself with a fraction of exactly 0.5, and a motion record that translates by
whole pixels (or by half a pixel) lands exactly where it is meant to."""
import numpy as np

from . import temporal_model as tm

F = np.float32
HALF_PI = float(np.float32(np.pi / 2))
ORIGIN = (0.0, 0.0, 55.0)
N_Q = (1.0, 2.0, 3.0, 2.5, 30.0, 31.0, 32.0, 40.0)                     # previous history lengths: n comes out as 2, 3, 4, 3.5, 31, 32, 32 (clamped from 33) and 32 (from 41)

# ---- the least number of pixels with each feature (conditions on the inputs, asserted on the CPU from the models' stats=) ----
FILTER_MINIMUM = 1000              # per step in (32, 64, 128): far_x, far_y (where 2 s fits in the frame), dropped_by_id
SEAM_MINIMUM = 200                 # across_seam, summed over the passes of a seam case
REPROJECTION_MINIMUMS = dict(tap0=200, tap1=200, tap2=200, tap3=200, no_tap_valid=200, k_not_positive=200, gx_below_alone=200, gx_above_alone=200, gy_below_alone=200,
                             gy_above_alone=200, gx_in_minus1_0=20, gx_in_wminus1_w=20, first_outside_later_inside=200, half_x=200, half_y=200, normal_alone=200,
                             plane_alone=200, id_alone=200)
N_MINIMUM = 200                    # each of n = 2, 3, 4, max_history - 1, max_history
ARITHMETIC_MINIMUM = 100           # pixels on the literal quotient, and on the shared sequence
NAN_CHANNEL_CAP = 0.02             # of the frame's channels


def scale_of(ids):
    """2^-(2 + id mod 3): the planes z = O.z + z / 4, / 8, / 16"""
    return np.ldexp(F(1), -(2 + (np.maximum(ids, 0).astype(np.int64) % 3))).astype(np.float32)


def pixel_vectors(W, H, fov):
    fov = F(np.pi / 3) if fov is None else F(fov)
    z = -F(W) / (F(2) * F(np.tan(np.float64(fov / F(2)))))
    j, i = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    x = ((j - F(W) / F(2)).astype(np.float64) + 0.5).astype(np.float32)
    y = ((F(H) / F(2) - i).astype(np.float64) - 0.5).astype(np.float32)
    return np.stack([x, y, np.full_like(x, z)], axis=-1)


def id_map(W, H, rng, islands=True):
    """mega blocks 0 .. 3 (their seams on the tile seams 288 and 272 where the frame is larger, else off them at 5 / 8 of the frame, so that taps of one object
    cross the tile seams of a small frame), islands 4 .. 15 and -1 in them"""
    sx = 2048 if W > 4000 else 288 if W > 320 else W * 5 // 8
    sy = 272 if H > 300 else H * 5 // 8
    j, i = np.meshgrid(np.arange(W), np.arange(H))
    ids = ((j >= sx).astype(np.int64) + 2 * (i >= sy)).astype(np.float32)
    if not islands:
        return ids
    n = max(W * H // 900, 4)
    iw, ih = (max(1, min(8, W // 6)), max(1, min(8, H // 6)))
    for t in range(n):
        x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
        if t % 3 == 0:                                                 # a third of them on the seams of the 32 x 8 tiles
            x0, y0 = x0 // 32 * 32, y0 // 8 * 8
        ids[y0:y0 + ih, x0:x0 + iw] = -1 if t % 13 == 12 else 4 + t % 12
    return ids


def planes(W, H, seed, fov=None, origin=ORIGIN, ids=None, level=1e5, noise=0.01):
    """-> dict(color [H, W, 4], aov [3, H, W, 4], history [2, H, W, 4], ids): one frame and a history whose plane 0 is the frame"""
    rng = np.random.default_rng(seed)
    ids = id_map(W, H, rng) if ids is None else np.asarray(ids, np.float32)
    hit = ids != -1
    v = pixel_vectors(W, H, fov)
    aov = np.zeros((3, H, W, 4), np.float32)
    j, i = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    n = np.stack([0.002 * np.sin(j / 37), 0.002 * np.cos(i / 29), np.ones_like(j)], axis=-1)
    aov[0, ..., :3] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    aov[0, ..., 3] = ids
    aov[1, ..., :3] = np.asarray(origin, np.float32) + v * scale_of(ids)[..., None]
    aov[1, ..., 3] = 1
    for c in range(3):
        aov[2, ..., c] = 0.5 + 0.05 * np.sin(3 * j / W + 2 * i / H + c + ids)
    aov[:, ~hit] = 0
    aov[0, ..., 3] = ids
    color = np.empty((H, W, 4), np.float32)
    base = level * (0.3 + 0.04 * np.maximum(ids, 0))
    for c in range(3):
        color[..., c] = base * (1 + 0.1 * c) * (1 + noise * rng.standard_normal((H, W)))
    color[..., 3] = rng.integers(1, 4, size=(H, W))
    history = np.zeros((2, H, W, 4), np.float32)
    history[0] = color
    l = tm.lum(color)
    V = ((noise * base) ** 2 * (0.5 + rng.random((H, W)))).astype(np.float32)
    history[1] = np.stack([l, l * l + V, rng.choice(np.asarray(N_Q, np.float32), size=(H, W)), V], axis=-1)
    history[1][~hit] = 0
    return dict(color=color, aov=aov, history=history, ids=ids)


# ---------------------------------------------------------------- the filter's cases ----------------------------------------------------------------
# (W, H, the n_passes the device is asked for, the steps whose far taps must exist along x / along y, seam case)
FILTER_CASES = {
    "517x389": (517, 389, (6, 7, 8), (32, 64, 128), (32, 64, 128), True),
    "4200x24": (4200, 24, (8,), (32, 64, 128), (), True),             # 24 rows: no tap 64 or more rows away exists
    "24x1100": (24, 1100, (8,), (), (32, 64, 128), True),
    "32x8": (32, 8, (1,), (), (), False),                             # one tile exactly: no seam inside
    "64x16": (64, 16, (1,), (), (), True),
    "33x9": (33, 9, (1,), (), (), False),                             # (one column and one row beyond the seam: fewer than 200 pixels reach across it)
    "31x7": (31, 7, (1,), (), (), False),
    "128x32": (128, 32, (3,), (), (), True),
    "127x31": (127, 31, (3,), (), (), True),
    "129x33": (129, 33, (3,), (), (), True),
    "1x700": (1, 700, (8,), (), (), False),
    "700x1": (700, 1, (8,), (), (), False),
    "2x513": (2, 513, (8,), (), (), False),
    "1920x1080": (1920, 1080, (3,), (), (), True),
}


def filter_case(name):
    W, H = FILTER_CASES[name][:2]
    return planes(W, H, seed=sum(map(ord, name)))


# ---------------------------------------------------------------- reprojection ----------------------------------------------------------------
def reprojection_ids(W, H, rng):
    """id_map plus strips of movers along the edges: 8 and 9 on the left, 10 and 11 on the right, 12 at the top, 13 at the bottom, 14 in the middle; 15 in islands"""
    ids = id_map(W, H, rng)
    hy, hx, e = H // 2, W // 2, max(2, min(6, W // 16))
    ids[:hy, :e], ids[hy:, :e] = 8, 9
    ids[:hy, W - e:], ids[hy:, W - e:] = 10, 11
    ids[:e, e:W - e], ids[H - e:, e:W - e] = 12, 13
    ids[hy - 4:hy + 4, hx - max(W // 8, 4):hx + max(W // 8, 4)] = 14
    return ids


def reprojection_motion(W, fov):
    """Records that put gx and gy where the cases want them, in whole and half pixels (a pixel is scale(id) scene units wide on the object's plane):
    8: one pixel left (column 0 -> gx = -0.5: the first tap outside the image, the second inside);  9: three left (columns 0, 1 -> gx < -1);
    10: half a pixel right (the last column -> gx = width exactly);  11: three right (gx > width);  12: three up;  13: three down;
    14: behind the camera (k <= 0);  15: two right, one down."""
    m = np.zeros((16, 12), np.float32)
    m[:, 0] = m[:, 4] = m[:, 8] = 1
    px = lambda i: float(scale_of(np.float32(i)))
    m[8, 9], m[9, 9], m[10, 9], m[11, 9] = -1 * px(8), -3 * px(9), 0.5 * px(10), 3 * px(11)
    m[12, 10], m[13, 10] = 3 * px(12), -3 * px(13)
    m[14, 11] = 4096.0
    m[15, 9], m[15, 10] = 2 * px(15), -1 * px(15)
    return m


def previous_planes(cur, rng):
    """The previous frame's planes 0 and 1: the current ones (nothing else moved) with, at scattered 2 x 2 footprints, 1, 2, 3 or 4 of the four pixels a reprojecting
    pixel (x, y) looks at -- (x, y), (x + 1, y), (x, y + 1), (x + 1, y + 1), in the contract's order when the fraction is exactly 0.5 -- made invalid in one way:
    another id, a normal turned by more than acos(0.9), or a point 5 units off the plane."""
    aov = cur["aov"]
    H, W = aov.shape[1:3]
    prev = aov[:2].copy()
    n = max(W * H // 40, 60)
    xs, ys = rng.integers(1, max(W - 8, 2), size=n) // 3 * 3, rng.integers(1, max(H - 8, 2), size=n) // 3 * 3     # on a grid of 3: footprints do not overlap
    for t, (x, y) in enumerate(zip(xs, ys)):
        how, cnt = t % 3, 1 + (t // 3) % 4
        for qx, qy in ((x, y), (x + 1, y), (x, y + 1), (x + 1, y + 1))[:cnt]:
            if qx >= W or qy >= H or prev[0, qy, qx, 3] == -1:
                continue
            if how == 0:
                prev[0, qy, qx, 3] = (prev[0, qy, qx, 3] + 1) % 16
            elif how == 1:
                prev[0, qy, qx, :3] = np.float32([0.6, 0.0, 0.8])
            else:
                prev[1, qy, qx, 2] += np.float32(5.0)
    return prev


def reprojection_case(W, H, seed, fov=HALF_PI, origin=ORIGIN):
    """-> dict(color, aov, prev_aov, prev_history, motion, ids, fov, origin); the previous camera that fits is the fixed camera (origin, fov)"""
    rng = np.random.default_rng(seed)
    cur = planes(W, H, seed + 1, fov=fov, origin=origin, ids=reprojection_ids(W, H, rng))
    old = planes(W, H, seed + 2, fov=fov, origin=origin, ids=cur["ids"])
    return dict(color=cur["color"], aov=cur["aov"], prev_aov=previous_planes(cur, rng), prev_history=old["history"], motion=reprojection_motion(W, fov), ids=cur["ids"],
                fov=fov, origin=origin)


# ---------------------------------------------------------------- arithmetic edges and non-finite values ----------------------------------------------------------------
AW, AH = 160, 120                                                     # 2 x 2 mega blocks of 96 | 64 by 64 | 56


def arithmetic_case(name, huge=66):
    """-> (planes dict, parameters for the two filters).  Colours of size 1 here.  huge: the binary exponent of the large colours -- 66 for the filters (a pixel's
    sums are at least 9/64 0.3 2^66 > 2^60, squared differences of 1 % stay finite), 61 for rt_temporal_accumulate (25 squared luminances stay below 2^128)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    p = planes(AW, AH, 1000 + len(name), level=1.0)
    ids, c, h = p["ids"], p["color"], p["history"]
    left = np.arange(AW)[None, :] < 96 + np.zeros((AH, 1), np.int64)
    kw = {}
    if name == "zeros":                                               # a third of the channels exactly 0, and every channel of a patch
        c[..., :3][rng.random((AH, AW, 3)) < 0.33] = 0
        c[10:40, 100:150, :3] = 0
    elif name == "denormal":
        c[left, :3] *= F(1e-40)
    elif name == "huge":
        c[left, :3] *= F(2.0 ** huge)
    elif name == "negative":
        c[..., :3][ids % 2 == 1] *= F(-1)
        c[..., 1][left] *= F(-1)
        c[10:40, 100:150, 2] = F(-0.0)                                # a sum of exactly -0: the literal quotient
    elif name == "only_centre":
        c[..., :3][rng.random((AH, AW, 3)) < 0.1] = 0
        kw = dict(k_normal=1e30, k_position=1e30, k_albedo=1e30, k_color=1e30)
    elif name == "variances":                                         # D = 0 V + 0 = 0 beside unequal luminances; the constant quarter forms no dl2 / D at all
        kw = dict(k_sigma=0.0, var_floor=0.0)
    else:
        raise KeyError(name)
    h[0] = c
    l = tm.lum(c)
    with np.errstate(all="ignore"):
        V = h[1, ..., 3].copy()
        if name == "denormal":
            V[left] = F(1e-41)
        if name == "huge":
            V[left] = V[left] * F(2.0 ** huge) * F(2.0 ** huge)
        if name == "variances":
            top = (np.arange(AH)[:, None] < 64) + np.zeros((1, AW), bool)
            V[top & left], V[top & ~left], V[~top & left], V[~top & ~left] = 0, F(1e-41), F(1e30), 1
            c[~top & ~left, :3] = F(0.75)
            h[0] = c
            l = tm.lum(c)
        h[1] = np.stack([l, l * l + V, h[1, ..., 2], V], axis=-1)
        if name == "huge" and huge > 61:
            h[1, ..., 1][left] = 0                                    # (l l is beyond binary32 there; rt_denoise_var reads neither moment)
    h[1][ids == -1] = 0
    return p, kw


def depth_case():
    """A reprojection whose denominator d . bz leaves [2^-60, 2^60]: objects 4 .. 6 at z = -2^61 (k underflows towards 0: gx = width / 2), 7 .. 9 at z = -2^-61
    (k about 1e20: far outside the image), seen from a previous camera at the origin.  Every product stays finite."""
    case = reprojection_case(AW, AH, 4242, fov=None, origin=(0.0, 0.0, 0.0))
    for aov in (case["aov"], case["prev_aov"]):
        ids = case["ids"]
        aov[1, ..., 2][(ids >= 4) & (ids <= 6)] = F(-2.0 ** 61)
        aov[1, ..., 2][(ids >= 7) & (ids <= 9)] = F(-2.0 ** -61)
    return case


ARITHMETIC_CASES = ("zeros", "denormal", "huge", "negative", "only_centre", "variances")
NAN, INF = F(np.nan), F(np.inf)


def nonfinite_filter_case(W=200, H=150, pitch=40):
    """NaN, +Inf and -Inf in a colour channel, NaN in a normal, a position and an albedo, NaN and Inf in the variance: each at isolated pixels, `pitch` apart.
    (The small form, pitch 12, is for the scalar reference: its NaNs meet, which the device's cases avoid.)"""
    p = planes(W, H, 77)
    c, a, h = p["color"], p["aov"], p["history"]
    spots = [(x, y) for y in range(pitch // 2, H, pitch) for x in range(pitch // 2, W, pitch)]
    for t, (x, y) in enumerate(spots):
        if a[0, y, x, 3] == -1:
            continue
        kind = t % 8
        if kind < 3:
            c[y, x, t % 3] = (NAN, INF, -INF)[kind]
        elif kind < 6:
            a[kind - 3, y, x, (t // 8) % 3] = NAN
        else:
            h[1, y, x, 3] = (NAN, INF)[kind - 6]
    h[0] = c
    return p


def nonfinite_history(case):
    """NaN in the previous history's colour, in m1, m2, n and V, and Inf in V, at isolated pixels of a reprojection case's previous history"""
    ph = case["prev_history"].copy()
    H, W = ph.shape[1:3]
    spots = [(x, y) for y in range(9, H - 8, 11) for x in range(9, W - 8, 13)]
    for t, (x, y) in enumerate(spots):
        kind = t % 6
        if kind == 0:
            ph[0, y, x, t % 3] = NAN
        elif kind < 5:
            ph[1, y, x, kind - 1] = NAN
        else:
            ph[1, y, x, 3] = INF
    return ph


def crop(p, x0, x1, y0, y1):
    """the same case on the pixels [x0, x1) x [y0, y1): every plane cut alike (a smaller frame, for the scalar reference)"""
    shape = p["ids"].shape
    out = {}
    for k, v in p.items():
        if isinstance(v, np.ndarray) and v.shape == shape:
            v = v[y0:y1, x0:x1].copy()
        elif isinstance(v, np.ndarray) and v.ndim >= 3 and v.shape[-3:-1] == shape:
            v = v[..., y0:y1, x0:x1, :].copy()
        out[k] = v
    return out


# ---------------------------------------------------------------- the cases the device is held to ----------------------------------------------------------------
def filter_gpu_cases():
    """name -> (build() -> planes dict, the n_passes asked for, rt_denoise's parameters, rt_denoise_var's; {} = the defaults, None = the entry is not run), finite"""
    cases = {}
    for name, (_, _, passes, _, _, _) in FILTER_CASES.items():
        cases[name] = ((lambda name=name: filter_case(name)), passes, {}, {}, True)
    for name in ARITHMETIC_CASES:
        kw = arithmetic_case(name)[1]
        plain = None if name == "variances" else {k: v for k, v in kw.items() if k not in ("k_sigma", "var_floor")}
        cases["arithmetic:" + name] = ((lambda name=name: arithmetic_case(name)[0]), (3,), plain, {k: v for k, v in kw.items() if k != "k_color"}, True)
    cases["nonfinite:k_color=0"] = (nonfinite_filter_case, (2,), dict(k_color=0.0), None, False)
    cases["nonfinite"] = (nonfinite_filter_case, (3,), {}, {}, False)
    return cases


def temporal_gpu_cases(make_pose):
    """name -> (build() -> reprojection case, keywords of temporal_model.accumulate, finite).  make_pose: raytracinggpu_amd.make_pose (the posed case's camera).
    Every case exists at 517 x 389 and at 96 x 64."""
    cases = {}
    for W, H in ((517, 389), (96, 64)):
        base = lambda W=W, H=H: reprojection_case(W, H, 5)
        fixed = lambda c: dict(camera=(c["origin"], c["fov"]), motion=c["motion"])
        t = f"{W}x{H}:"
        cases[t + "movers"] = (base, fixed, True)                                                          # all 16 ids, 15 a mover
        cases[t + "masked"] = (base, lambda c: dict(fixed(c), mask=(1 << 15) | (1 << 2)), True)           # 15 (and 2) masked
        cases[t + "posed"] = (base, lambda c: dict(pose=make_pose(position=(1.5, 0.5, 54.0), yaw=0.04, pitch=0.02), motion=c["motion"]), True)
        cases[t + "fixed_elsewhere"] = (base, lambda c: dict(camera=((1.0, -0.5, 56.0), None), motion=c["motion"]), True)
        cases[t + "no_motion_table"] = (base, lambda c: dict(camera=(c["origin"], c["fov"])), True)
        for mh in (1, 2):
            cases[t + f"max_history={mh}"] = (base, lambda c, mh=mh: dict(fixed(c), max_history=mh), True)
        cases[t + "alpha_min=0.4"] = (base, lambda c: dict(fixed(c), alpha_min=0.4), True)
        cases[t + "alpha_min=0.4,max_history=2"] = (base, lambda c: dict(fixed(c), alpha_min=0.4, max_history=2), True)
        cases[t + "nonfinite_history"] = (lambda base=base: (lambda c: dict(c, prev_history=nonfinite_history(c)))(base()), fixed, False)
    cases["depths"] = (depth_case, lambda c: dict(camera=(c["origin"], c["fov"]), motion=c["motion"]), True)
    for name in ARITHMETIC_CASES:
        def build(name=name):
            p = arithmetic_case(name, huge=61)[0]
            ph = p["history"].copy()                                   # a frame earlier: the same colours one pixel to the left
            ph[0, ..., :3] = np.roll(ph[0, ..., :3], 1, axis=1)
            with np.errstate(all="ignore"):
                l = tm.lum(ph[0])
                ph[1, ..., 0], ph[1, ..., 1] = l, l * l + ph[1, ..., 3]
            return dict(color=p["color"], aov=p["aov"], prev_aov=p["aov"][:2].copy(), prev_history=ph, ids=p["ids"])
        cases["arithmetic:" + name] = (build, lambda c: dict(camera=(ORIGIN, None)), True)
    return cases
