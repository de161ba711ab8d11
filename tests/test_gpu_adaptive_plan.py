"""rt_kat_sample_plan -- the three launches that lay a frame's per-pixel sample counts out as a list (rt_adaptive.hip.h) -- against tests/adaptive_model.py: every
offset and every item.  -m gpu.  Sizes sit on the boundaries the entry reports: the slots one workgroup covers and the slots one round of the scan of workgroup sums
covers."""
import numpy as np
import pytest

import raytracinggpu_amd as rt

from . import adaptive_model as am

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def span(ctx):
    return ctx.kat_sample_plan(np.ones((1, 1), np.uint8))[2]


def _check(ctx, counts, first=0):
    offs, items, span = ctx.kat_sample_plan(counts, first)
    eo, ei = am.plan(counts, first)
    np.testing.assert_array_equal(offs, eo)
    np.testing.assert_array_equal(items, ei)
    return span


def _random(W, H, seed, hi=5):
    return np.random.default_rng(seed).integers(0, hi, (H, W)).astype(np.uint8)


def test_the_span_is_what_the_kernels_are_built_with(span):
    assert span[0] % 64 == 0 and span[0] >= 64 and span[1] % span[0] == 0 and span[1] > span[0]


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("W,H", [(1, 1), (63, 1), (64, 1), (65, 1), (1, 63), (1, 65), (8, 8), (61, 45)])
def test_small_frames(ctx, W, H, first):
    _check(ctx, _random(W, H, W + H), first)
    _check(ctx, np.full((H, W), 3, np.uint8), first)


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_one_tile_below_at_and_above_each_boundary(ctx, span, level, d, first):
    tiles = span[level] // 64 + d                      # a row of 8 x 8 tiles: 64 slots each
    for h in (8, 5):                                   # ... whole, and with three rows of every tile outside the frame
        _check(ctx, _random(8 * tiles - (3 if h == 5 else 0), h, 10 * level + d + 1), first)


def test_two_rounds_of_the_scan_and_a_bit(ctx, span):
    tiles = 2 * span[1] // 64 + 3
    c = _random(8 * tiles, 8, 3, hi=3)
    c[:, -9:] = 64                                     # the carry reaches the last workgroups
    _check(ctx, c)


@pytest.mark.parametrize("first", [0, 1])
def test_all_zero_and_all_max_counts(ctx, first):
    for v in (0, 1, rt.MAX_SAMPLE_COUNT, 255):         # 255 is read as MAX_SAMPLE_COUNT
        offs, items, _ = ctx.kat_sample_plan(np.full((45, 61), v, np.uint8), first)
        eo, ei = am.plan(np.full((45, 61), v, np.uint8), first)
        np.testing.assert_array_equal(offs, eo)
        np.testing.assert_array_equal(items, ei)
        assert len(items) == 45 * 61 * max(min(v, 64) - first, 0)


def test_a_sparse_plane_at_7680_x_4320(ctx):
    rng = np.random.default_rng(8)
    W, H = 7680, 4320
    c = np.zeros((H, W), np.uint8)
    k = rng.integers(0, W * H, 60000)
    c.reshape(-1)[k] = rng.integers(1, 9, len(k)).astype(np.uint8)
    c[-1, -1], c[0, 0], c[H // 2, W // 2] = 64, 200, 64
    _check(ctx, c)
    _check(ctx, c, 1)
