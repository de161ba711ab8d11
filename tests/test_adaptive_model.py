"""tests/adaptive_model.py against brute-force Python loops: the plan on tiny frames (sizes that are no multiple of the 8 x 8 tile included), the counts formula row by
row with its NaN / Inf / zero-variance cases, and its monotonicity in the variance."""
import math

import numpy as np
import pytest

from . import adaptive_model as am

F = np.float32


def _plan_loops(counts, first):
    H, W = counts.shape
    offs, items = [], []
    for ty in range((H + 7) // 8):
        for tx in range((W + 7) // 8):
            for p in range(64):
                x, y = tx * 8 + p % 8, ty * 8 + p // 8
                offs.append(len(items))
                if x < W and y < H:
                    for s in range(first, min(int(counts[y, x]), 64)):
                        items.append((x, y, s))
    offs.append(len(items))
    return np.array(offs, np.uint32), np.array(items, np.int32).reshape(-1, 3)


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("W,H", [(1, 1), (8, 8), (7, 9), (9, 7), (16, 8), (17, 23), (13, 5)])
def test_plan_equals_the_loops(W, H, first):
    rng = np.random.default_rng(W * 100 + H)
    for counts in (rng.integers(0, 5, (H, W)).astype(np.uint8), np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8),
                   (rng.integers(0, 40, (H, W)) * (rng.random((H, W)) < 0.2) * 7).astype(np.uint8)):
        offs, items = am.plan(counts, first)
        eo, ei = _plan_loops(counts, first)
        np.testing.assert_array_equal(offs, eo)
        np.testing.assert_array_equal(items, ei)
        assert offs.dtype == np.uint32 and items.dtype == np.int32 and items.shape[1] == 3


def test_slot_order_is_the_tile_order():
    x, y = am.slot_pixels(17, 9)
    assert len(x) == 3 * 2 * 64
    assert (x[:8] == np.arange(8)).all() and (y[:8] == 0).all() and (x[8], y[8]) == (0, 1)
    assert (x[64], y[64]) == (8, 0) and (x[3 * 64], y[3 * 64]) == (0, 8)


def _count_loop(m1, n, V, mx, sh, ns, k, fl):
    with np.errstate(all="ignore"):
        m1, n, V, k, fl = F(m1), F(n), F(V), F(k), F(fl)
        if n == 0:
            return 1
        e_n = F(ns - 1) if n < F(sh) else F(0)
        kv = F(k * F(V / F(F(m1 * m1) + fl)))
        e_v = F(math.floor(kv)) if np.isfinite(kv) else kv
        if not e_v >= 1:
            e_v = F(0)
        return int(F(1) + min(F(mx - 1), max(e_n, e_v)))


ROWS = [  # (m1, n, V)
    (0.5, 0.0, 3.0), (0.5, -0.0, 3.0), (0.5, 1.0, 0.0), (0.5, 1.0, 1.0), (0.5, 5.0, 0.0), (0.5, 5.0, 0.24), (0.5, 5.0, 0.26), (0.5, 5.0, 100.0),
    (0.0, 5.0, 0.0), (0.0, 5.0, 1e-3), (0.5, 5.0, np.nan), (np.nan, 5.0, 1.0), (0.5, np.nan, 1.0), (0.5, np.nan, 0.0), (0.5, 5.0, np.inf), (np.inf, 5.0, 1.0),
    (np.inf, 5.0, np.inf), (0.5, 5.0, -1.0), (0.5, 5.0, -np.inf), (1e-30, 3.0, 1e-40), (0.5, 2.0, 0.0), (0.5, 1.999, 0.0), (0.5, np.inf, 0.3), (3e19, 9.0, 1e38)]
PARAMS = [(4, 2, 4, 0.0, 1e-4), (4, 2, 3, 1.0, 1e-4), (64, 3, 8, 16.0, 0.0), (1, 0, 1, 100.0, 1e-4), (8, 0, 1, 4.0, 1e-2), (64, 100, 64, 1e6, 0.0)]


@pytest.mark.parametrize("cp", PARAMS)
def test_counts_rows_equal_the_loop(cp):
    h = np.zeros((2, 1, len(ROWS), 4), F)
    for i, (m1, n, V) in enumerate(ROWS):
        h[1, 0, i] = (m1, 7.0, n, V)
    got = am.sample_counts(h, *cp)
    exp = [_count_loop(m1, n, V, *cp) for m1, n, V in ROWS]
    assert got.dtype == np.uint8 and got[0].tolist() == exp
    assert got.min() >= 1 and got.max() <= cp[0]


def test_the_cases_by_hand():
    cp = (4, 2, 3, 1.0, 0.0)
    one = lambda m1, n, V: int(am.sample_counts(np.array([[[[0, 0, 0, 0]]], [[[m1, 0, n, V]]]], F), *cp)[0, 0])
    assert one(0.5, 0, 9.0) == 1                      # a miss
    assert one(0.5, 1, 0.0) == 3                      # newly revealed
    assert one(0.5, 2, 0.0) == 1                      # no longer short, no variance
    assert one(0.5, 9, 0.25) == 2                     # rel = 1: floor(1) = 1 extra
    assert one(0.5, 9, 0.2499) == 1
    assert one(0.5, 9, 50.0) == 4                     # capped
    assert one(0.5, 9, np.nan) == 1 and one(np.nan, 9, 1.0) == 1
    assert one(0.5, 9, np.inf) == 4 and one(0.0, 9, 1.0) == 4          # rel = +inf asks for everything
    assert one(0.0, 9, 0.0) == 1                      # 0 / 0
    assert one(0.5, np.nan, 0.0) == 1                 # a NaN n is neither a miss nor short


def test_more_variance_never_gives_fewer_samples():
    rng = np.random.default_rng(5)
    V = np.sort(np.concatenate([rng.random(500).astype(F) * F(40), [0, np.inf], F(2) ** rng.integers(-140, 100, 100).astype(F)]).astype(F))
    for cp in PARAMS:
        for m1 in (0.0, 1e-3, 0.7, 30.0):
            for n in (1.0, 6.0):
                h = np.zeros((2, 1, len(V), 4), F)
                h[1, 0, :, 0], h[1, 0, :, 2], h[1, 0, :, 3] = m1, n, V
                c = am.sample_counts(h, *cp)[0].astype(int)
                assert (np.diff(c) >= 0).all(), (cp, m1, n)
