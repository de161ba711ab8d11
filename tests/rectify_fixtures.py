"""Seeded synthetic inputs for rt_history_rectify and rt_temporal_accumulate_fast (test infrastructure; tests/synthetic_planes.py builds the planes, this adds what the
clamp's branches need).  tests/test_rectify_model.py proves on the CPU, from the model's stats=, that they reach every branch; tests/test_gpu_rectify.py then holds the
device to the model on the same cases.

The rectifier's case.  All 16 object ids in blocks of 7 x 5 pixels (a seam every few pixels, so windows of every radius lose taps to another id) with islands of misses.
The fast plane is a smooth ramp with 0.3 % noise plus two planted steps of 3 % and 6 % (windows straddle a level change); its length is 4.  The long history's colour is
the fast colour offset per channel independently by -5 %, 0 or +5 % of the level -- the window's deviation is a few tenths of a percent except on a step, so with
k_clamp = 4 an offset channel leaves the band on either side and an unoffset one stays inside: one, two and three channels move.  The history length is 3, 4 (= n_f), 5
(one more) or 32 (far above), so the copy condition is met from both sides."""
import numpy as np

from . import synthetic_planes as sp
from . import temporal_model as tm

F = np.float32
SIZES = ((96, 64), (517, 389))                                         # the project's two sizes
N_F = 4.0
LENGTHS = (3.0, 4.0, 5.0, 32.0)
REACH_MINIMUM = 200
MINIMUMS = ("clamped_low", "clamped_high", "unmoved", "copied_n", "lost_to_id", "moved_1", "moved_2", "moved_3")
EDGES = ("clipped_left", "clipped_right", "clipped_top", "clipped_bottom", "corner_tl", "corner_tr", "corner_bl", "corner_br")


def seam_ids(W, H, rng):
    """ids 0 .. 15 in blocks of 7 x 5, misses in a few islands (none in a corner: the corners' windows must run)"""
    j, i = np.meshgrid(np.arange(W), np.arange(H))
    ids = ((j // 7 + 3 * (i // 5)) % 16).astype(np.float32)
    for _ in range(max(W * H // 1500, 3)):
        x0, y0 = int(rng.integers(4, max(W - 8, 5))), int(rng.integers(4, max(H - 8, 5)))
        ids[y0:y0 + 3, x0:x0 + 4] = -1
    return ids


def rectify_case(W, H, seed=11, nonfinite=False):
    """-> dict(history [2, H, W, 4], fast [H, W, 4], aov [3, H, W, 4], ids)"""
    rng = np.random.default_rng(seed + W)
    ids = seam_ids(W, H, rng) if W >= 16 and H >= 8 else np.full((H, W), 3, np.float32)
    p = sp.planes(W, H, seed, ids=ids, level=1.0)
    hit = ids != -1
    j, i = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ramp = 0.5 * (1 + 0.002 * j + 0.001 * i) * (1 + 0.03 * (j >= W // 2) + 0.06 * (i >= (2 * H) // 3))
    fast = np.zeros((H, W, 4), np.float32)
    for c in range(3):
        fast[..., c] = ramp * (1 + 0.1 * c) * (1 + 0.003 * rng.standard_normal((H, W)))
    fast[..., 3] = np.where(hit, N_F, 0)
    hist = np.zeros((2, H, W, 4), np.float32)
    off = rng.choice(np.asarray([-0.05, 0.0, 0.05]), size=(H, W, 3), p=[0.3, 0.4, 0.3])
    hist[0, ..., :3] = fast[..., :3] + (0.5 * off).astype(np.float32)
    hist[0, ..., 3] = rng.integers(1, 4, size=(H, W))
    l = tm.lum(hist[0])
    V = (1e-4 * (0.5 + rng.random((H, W)))).astype(np.float32)
    hist[1] = np.stack([l, l * l + V, rng.choice(np.asarray(LENGTHS, np.float32), size=(H, W)), V], axis=-1)
    for ys in (slice(0, 3), slice(max(H - 3, 0), H)):                  # the corners' windows run: a long history there
        for xs in (slice(0, 3), slice(max(W - 3, 0), W)):
            hist[1, ys, xs, 2] = 32
    hist[1][~hit] = 0
    if nonfinite:                                                      # isolated pixels, 11 x 13 apart: NaN and +-Inf in F, in H and in the moments
        kinds = [("fast", c, v) for c in range(3) for v in (sp.NAN, sp.INF, -sp.INF)] + [("h0", c, v) for c in range(3) for v in (sp.NAN, sp.INF)] + \
                [("h1", c, sp.NAN) for c in range(3)] + [("h1", 0, sp.INF)]
        spots = [(x, y) for y in range(6, H - 3, 11) for x in range(6, W - 3, 13)]
        for t, (x, y) in enumerate(spots):
            if not hit[y, x]:
                continue
            where, c, v = kinds[t % len(kinds)]
            if where == "fast":
                fast[y, x, c] = v
            elif where == "h0":
                hist[0, y, x, c] = v
            else:
                hist[1, y, x, c] = v
    return dict(history=hist, fast=fast, aov=p["aov"], ids=ids)


def previous_fast(case, seed=3):
    """A previous fast plane for a reprojection case of synthetic_planes: the previous history's colour with 2 % noise, lengths 1 .. 6 and 40 (so that
    min(n + 1, fast_history) clamps for some taps and not for others, and differs from the clamp by max_history)"""
    rng = np.random.default_rng(seed)
    ph = case["prev_history"]
    pf = np.empty(ph.shape[1:], np.float32)
    pf[..., :3] = ph[0, ..., :3] * (1 + 0.02 * rng.standard_normal(ph.shape[1:3] + (3,))).astype(np.float32)
    pf[..., 3] = rng.choice(np.asarray([1, 2, 3, 4, 5, 6, 40], np.float32), size=ph.shape[1:3])
    pf[..., 3][case["prev_aov"][0, ..., 3] == -1] = 0
    return pf
