"""Row windows of the traversal queue (csrc/rt_qrows.h, through the host library's rth_qrows_enumerate): the first traversal launch of a chain enumerates the rows
that hold continuation (Y) rays, the last the rows that hold shadow (X) rays.  The queue's layout (wf_slot_to_path of rt_wavefront.hip.h) is restated here in numpy.
CPU only."""
import numpy as np
import pytest

from raytracinggpu_amd import hostlib

N_PATHS = [64, 128, 192, 3072, 9216, 64 * 1013]
LOG2S = list(range(11))
TBLOCKS = [1, 3, 7, 64, 512, 1000]


def slot_to_path(q, log2S, Q, n_groups):
    """wf_slot_to_path: the ray of queue slot q, -1 for padding"""
    gs = q >> 2
    col = gs >> log2S
    g = (gs & ((1 << log2S) - 1)) * Q + col
    return np.where((col < Q) & (g < n_groups), 4 * g + (q & 3), -1)


def geometry(n_paths, log2S):
    n_groups = 2 * n_paths // 4
    S = 1 << log2S
    return n_groups, S, (n_groups + S - 1) // S


@pytest.mark.parametrize("n_paths", N_PATHS)
def test_every_ray_lies_in_its_window(n_paths):
    for log2S in LOG2S:
        n_groups, S, Q = geometry(n_paths, log2S)
        q = np.arange(S * Q * 4, dtype=np.int64)
        r = slot_to_path(q, log2S, Q, n_groups)
        a = (q >> 2) & (S - 1)
        assert np.array_equal(np.sort(r[r >= 0]), np.arange(2 * n_paths))          # the layout holds every ray once
        wy, _, _ = hostlib.qrows_enumerate(n_paths, log2S, Q, 4, 1)
        wx, _, _ = hostlib.qrows_enumerate(n_paths, log2S, Q, 4, 2)
        y0, y1 = (0, S) if wy["rows"] == 0 else (wy["row0"], wy["row0"] + wy["rows"])
        x0, x1 = (0, S) if wx["rows"] == 0 else (wx["row0"], wx["row0"] + wx["rows"])
        is_y, is_x = (r >= 0) & (r < n_paths), r >= n_paths
        assert ((a[is_y] >= y0) & (a[is_y] < y1)).all(), (log2S, wy)
        assert ((a[is_x] >= x0) & (a[is_x] < x1)).all(), (log2S, wx)
        assert y0 == 0 and x1 == S
        assert y1 - x0 <= 1 or S == 1, (log2S, wy, wx)                            # at most the one mixed row is in both
        if S == 1:
            assert wy["rows"] == 0 and wx["rows"] == 0                             # one row: it is mixed, and the window is "every row"
        else:
            assert 0 < wy["rows"] < S and 0 < wx["rows"] < S
        if S > 1 and (n_paths // 4) % Q == 0:
            assert y1 == x0                                                        # no mixed row at all


@pytest.mark.parametrize("n_paths", N_PATHS)
@pytest.mark.parametrize("which", [1, 2])
def test_shares_partition_the_window(n_paths, which):
    for log2S in LOG2S:
        n_groups, S, Q = geometry(n_paths, log2S)
        for tblocks in TBLOCKS:
            none, _, _ = hostlib.qrows_enumerate(n_paths, log2S, Q, tblocks, 0)
            alloc = none["share"] * tblocks                                       # what the queue's buffer holds: S Q 4 slots rounded up to the shares
            w, blk_len, slots = hostlib.qrows_enumerate(n_paths, log2S, Q, tblocks, which)
            if w["rows"] == 0:
                continue                                                           # every row: test_no_window_is_todays_indexing
            assert w["share"] % 4 == 0 and w["total"] == w["rows"] * Q * 4
            assert (blk_len >= 0).all() and (blk_len <= w["share"]).all() and int(blk_len.sum()) == w["total"] == len(slots)
            assert (np.diff(blk_len) <= 0).all()                                   # only the last shares are short
            assert slots.min() >= 0 and slots.max() < alloc
            s = np.sort(slots)
            assert (np.diff(s) > 0).all()                                          # no slot twice
            q = np.arange(S * Q * 4, dtype=np.int64)
            a = (q >> 2) & (S - 1)
            assert np.array_equal(s, q[(a >= w["row0"]) & (a < w["row0"] + w["rows"])])   # exactly the window's rows of the columns [0, Q)
            assert len(slots) < S * Q * 4


@pytest.mark.parametrize("n_paths", N_PATHS)
def test_no_window_is_todays_indexing(n_paths):
    for log2S in LOG2S:
        n_groups, S, Q = geometry(n_paths, log2S)
        for tblocks in TBLOCKS:
            w, blk_len, slots = hostlib.qrows_enumerate(n_paths, log2S, Q, tblocks, 0)
            assert w["row0"] == 0 and w["rows"] == 0
            assert w["share"] == ((S * Q * 4 + tblocks - 1) // tblocks + 3) // 4 * 4   # share_geometry's slots_per_block
            assert (blk_len == w["share"]).all()
            assert np.array_equal(slots, np.arange(tblocks * w["share"]))          # blk_base + k


def test_the_headline_frame_halves_its_first_and_last_scan():
    """half of 1920 x 1080 (one sub-frame) on 256 CUs x 5 workgroups x 2 (oversubscribed), as wf_geometry cuts it"""
    n_paths = 240 * 68 * 64
    n_groups, tblocks = n_paths // 2, 1280
    per = (n_groups + tblocks - 1) // tblocks
    log2S = 0
    while (2 << log2S) <= per and log2S < 16:
        log2S += 1
    Q = (n_groups + (1 << log2S) - 1) >> log2S
    none, _, _ = hostlib.qrows_enumerate(n_paths, log2S, Q, tblocks, 0)
    wy, _, sy = hostlib.qrows_enumerate(n_paths, log2S, Q, tblocks, 1)
    wx, _, sx = hostlib.qrows_enumerate(n_paths, log2S, Q, tblocks, 2)
    assert 2 * n_paths <= len(sy) + len(sx) <= 2 * n_paths + 2 * 4 * Q             # the two windows share at most one row, and X takes the padding rows
    assert len(sy) <= 0.52 * none["share"] * tblocks
