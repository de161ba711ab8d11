"""Seeded synthetic inputs for rt_upsample (test infrastructure, beside tests/synthetic_planes.py): a PAIR of plane sets, w x h and f w x f h, of one scene, built so
that the branches of the kernel run.  tests/test_upsample_model.py proves on the CPU that they do (the feature minimums below); the same cases then go to the device
in tests/test_gpu_upsample.py.

The scene.  Object ids are one function of continuous image coordinates (X, Y) in full-resolution pixel units, evaluated at each resolution's pixel centres
(x + 0.5 and f (j + 0.5)): four blocks with their seams at 5 / 8 of the frame, islands of ids 4 .. 15 and of misses a few low-resolution pixels wide, and THIN islands
half a full-resolution pixel wide around full-resolution pixel centres -- narrower than a low-resolution pixel, so (f = 2, 4: always; f = 3: two times in three) no
low-resolution pixel shows them and their pixels find no tap of their id: the fallback.  Hit points lie on each resolution's own camera ray, as
synthetic_planes.planes builds them, on the plane of constant z of their id: P = O + v scale(id) at full resolution and O + v_low (f scale(id)) at the low one (with
fov = pi / 2, z = -W / 2 and -w / 2: the same plane; exact in binary32 for f = 2 and 4).  Normals tilt by 0.05 with a period of some 60 pixels: gently enough that the default k_* keep the taps, enough that the normal and
plane terms are numbers with a full significand (the association of w = b wn wp shows in the bits).  At scattered low-resolution pixels the normal is
turned by more than the normal term allows, or the point is moved 5 units off its plane: taps dropped by one term alone.

Values.  Two low-resolution planes (a history; plane 0 alone is a colour frame): levels by id times 2^-3 .. 2^3 with noise, a twentieth of the channels exactly 0 and
some denormal, so that both sides of rt_div.h's range are used; plane 0's .w is a ray count of 1 .. 3."""
import numpy as np

from . import synthetic_planes as sp

F = np.float32

# ---- the least number of pixels / taps with each feature on the main case (asserted on the CPU from the model's stats=) ----
COUNTED_MINIMUM = 100              # pixels with exactly 1, 2, 3 and 4 counted taps, each
DROPPED_MINIMUM = 100              # taps dropped by id alone, by the normal term alone, by the plane term alone, and by lying outside the image, each
FALLBACK_MINIMUM = 50              # pixels
FALLBACK_CAP = 0.05                # of the frame

# (full width, full height, factor): tests/test_gpu_upsample.py runs all of them; MAIN is the one the minimums are asserted on
CASES = {"2x2": (2, 2, 2), "4x4": (4, 4, 4), "6x2": (6, 2, 2), "66x18": (66, 18, 2), "140x40": (140, 40, 2), "99x27": (99, 27, 3), "140x40/4": (140, 40, 4)}
MAIN = "140x40"


def islands(W, H, rng):
    """[(x0, y0, x1, y1, id)] in continuous full-resolution pixel coordinates: wide ones first, thin ones on top"""
    out = []
    for t in range(max(W * H // 400, 2)):                             # a few low-resolution pixels wide
        x0, y0 = float(rng.integers(0, W)), float(rng.integers(0, H))
        out.append((x0, y0, x0 + float(rng.integers(3, 9)), y0 + float(rng.integers(3, 7)), -1 if t % 4 == 3 else 4 + t % 12))
    for t in range(max(W * H // 70, 2)):                              # half a pixel wide around the centres of 1 .. 3 pixels in a row or a column
        x0, y0, n = int(rng.integers(0, W)), int(rng.integers(0, H)), int(rng.integers(1, 4))
        lx, ly = (n, 1) if t % 2 else (1, n)
        out.append((x0 + 0.25, y0 + 0.25, x0 + lx - 0.25, y0 + ly - 0.25, -1 if t % 5 == 4 else 4 + (t * 7) % 12))
    return out


def ident(X, Y, W, H, isl):
    ids = ((X >= W * 0.625).astype(np.int64) + 2 * (Y >= H * 0.625)).astype(np.float32)
    for x0, y0, x1, y1, k in isl:
        ids[(X >= x0) & (X < x1) & (Y >= y0) & (Y < y1)] = k
    return ids


def planes_at(w, h, step, isl, W, H):
    """planes 0 and 1 (plane 2 zero) of the w x h grid whose pixel (j, i) has its centre at (step (j + 0.5), step (i + 0.5)) of the W x H frame"""
    j, i = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    X, Y = step * (j + 0.5), step * (i + 0.5)
    ids = ident(X, Y, W, H, isl)
    hit = ids != -1
    aov = np.zeros((3, h, w, 4), np.float32)
    n = np.stack([0.05 * np.sin(X / 11), 0.05 * np.cos(Y / 7), np.ones_like(X)], axis=-1)
    aov[0, ..., :3] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    v = sp.pixel_vectors(w, h, sp.HALF_PI)
    aov[1, ..., :3] = np.asarray(sp.ORIGIN, np.float32) + v * (F(step) * sp.scale_of(ids))[..., None]
    aov[1, ..., 3] = 1
    aov[:, ~hit] = 0
    aov[0, ..., 3] = ids
    return aov, ids


def pair(W, H, f, seed=7):
    """-> dict(low [2, h, w, 4], low_aov [3, h, w, 4], aov [3, H, W, 4], ids [H, W], low_ids [h, w], factor)"""
    assert W % f == 0 and H % f == 0
    w, h = W // f, H // f
    rng = np.random.default_rng(seed + 1000 * f + W)
    isl = islands(W, H, rng)
    aov, ids = planes_at(W, H, 1, isl, W, H)
    low_aov, low_ids = planes_at(w, h, f, isl, W, H)
    hit = low_ids != -1
    how = rng.random((h, w))
    turned, moved = hit & (how < 0.04), hit & (how >= 0.04) & (how < 0.08)
    low_aov[0, turned, :3] = np.float32([0.8, 0.0, 0.6])               # |dN|^2 = 0.8: the normal term is max(0, 1 - 1.6) = 0
    low_aov[1, moved, 2] += F(5.0)                                     # e = 5: the plane term is max(0, 1 - 6.25) = 0
    low = np.empty((2, h, w, 4), np.float32)
    level = 1e3 * (0.3 + 0.04 * np.maximum(low_ids, 0))
    for p in range(2):
        for c in range(4):
            low[p, ..., c] = level * (1 + 0.1 * c + p) * (1 + 0.05 * rng.standard_normal((h, w))) * np.ldexp(1.0, rng.integers(-3, 4, size=(h, w)))
    u = rng.random((2, h, w, 4))
    low[u < 0.05] = 0
    low[(u >= 0.05) & (u < 0.08)] *= F(1e-43)                          # (levels up to 2e4: every product is denormal)
    low[0, ..., 3] = rng.integers(1, 4, size=(h, w))
    return dict(low=low, low_aov=low_aov, aov=aov, ids=ids, low_ids=low_ids, factor=f)


def case(name):
    return pair(*CASES[name])
