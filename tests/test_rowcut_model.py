"""The cut of a call's rows into sub-frames (RT_PARTS) and into chunks (RT_CHUNK_MPX): csrc/rt_rowcut.h, the text the render path compiles, through the host library's
rth_row_cut / rth_row_chunks, against what tests/rowcut_model.py says a cut has to satisfy.  Exhaustive over heights 1 .. 150, five tile heights (three of them whole wave
tiles), every rank of 1, 2, 3 and 8 interleaved shares, contiguous ranges from rows 0 and 13, 1 .. 9 sub-frames wanted, a counting run or not, a batch cut by frames or
not.  No GPU: a wrong cut writes outside the frame on one."""
import functools

import numpy as np
import pytest

from raytracinggpu_amd import hostlib

from . import rowcut_model as model

HEIGHTS = range(1, 151)
TILE_ROWS = (8, 16, 24, 12, 5)
WORLDS = (1, 2, 3, 8)
WANTS = tuple(range(1, 10))
FLAGS = [(one, whole) for one in (0, 1) for whole in (0, 1)]


def calls(height):
    """the calls of one image height as (row0, n_rows, tile_rows, tile_step): every rank's share at every tile height, and the contiguous ranges from rows 0 and 13
    described as one tile (as rt_render does) and with every tile height (tile_rows of contiguous rows only says how the caller described them)"""
    out = []
    for R in TILE_ROWS:
        for G in WORLDS:
            out.extend(model.shares(height, R, G))
    for row0 in (0, 13):
        n = height - row0
        if n > 0:
            out.extend((row0, n, tr, 1) for tr in (n,) + TILE_ROWS)
    return sorted(set(out))


@functools.lru_cache(maxsize=None)
def cut(height, one, whole):
    """(cases [n, 7], info [n, 4], parts [n, 8, 6]) of every call of `height` and every number of sub-frames wanted"""
    cases = np.array([c + (want, one, whole) for c in calls(height) for want in WANTS], np.int32)
    info, parts = hostlib.row_cut(cases)
    return cases, info, parts


def every_cut():
    for h in HEIGHTS:
        for one, whole in FLAGS:
            yield (h,) + cut(h, one, whole)


def name(height, case):
    return "height %d, rows (row0 %d, n_rows %d, tile_rows %d, tile_step %d), %d parts wanted, one %d, whole %d" % ((height,) + tuple(int(v) for v in case))


def test_the_shares_of_the_model_are_the_package_s():
    from raytracinggpu_amd import _capi
    for h in (1, 43, 131):
        for R in TILE_ROWS:
            for G in WORLDS:
                for rank, s in enumerate(model.shares(h, R, G)):
                    rows, idx = _capi.interleaved_rows(h, R, rank, G)
                    assert s == (rows.row0, rows.n_rows, rows.tile_rows, rows.tile_step)
                    np.testing.assert_array_equal(model.image_row(np.arange(s[1]), s[0], s[2], s[3]), idx)


def test_number_of_parts():
    for h, cases, info, _ in every_cut():
        want = model.parts_expected(cases[:, 1], cases[:, 2], cases[:, 3], cases[:, 4], cases[:, 5])
        bad = np.flatnonzero(info[:, 0] != want)
        assert bad.size == 0, "%s: %d parts, expected %d" % (name(h, cases[bad[0]]), info[bad[0], 0], want[bad[0]])
        R = model.tile_height(cases[:, 2], cases[:, 3])
        np.testing.assert_array_equal(info[:, 1], R)
        np.testing.assert_array_equal(info[:, 3], -(-cases[:, 1] // R))


def test_parts_hold_every_row_of_the_call_once_where_the_call_stores_it():
    """over all sub-frames (whole: in every sub-frame) the pairs (image row, output row) are the call's own {(image row of local row q, q)}, each once"""
    for h, cases, info, parts in every_cut():
        whole = bool(cases[0, 6])
        live = np.arange(model.MAX_PARTS)[None, :] < info[:, :1]
        case_of, j_of = np.nonzero(live)
        p = parts[case_of, j_of].astype(np.int64)
        which, r = model.local_rows(p[:, 1])
        img = model.image_row(r, p[which, 0], p[which, 2], p[which, 3])
        out = model.output_row(r, p[which, 2], p[which, 4], p[which, 5])
        unit = np.arange(len(p)) if whole else case_of              # the set that has to be the call's rows: every sub-frame's / all sub-frames' together
        c = cases[case_of if whole else np.arange(len(cases))].astype(np.int64)
        held = np.bincount(unit[which], minlength=len(c))
        bad = np.flatnonzero(held != c[:, 1])
        assert bad.size == 0, "%s: %d rows in its sub-frames, %d in the call" % (name(h, c[bad[0]]), held[bad[0]], c[bad[0], 1])
        u, q = model.local_rows(c[:, 1])
        order = np.lexsort((out, unit[which]))
        bad = np.flatnonzero((out[order] != q) | (img[order] != model.image_row(q, c[u, 0], c[u, 2], c[u, 3])))
        assert bad.size == 0, "%s: output row %d holds image row %d, expected output row %d with image row %d" % (
            name(h, c[u[bad[0]]]), out[order][bad[0]], img[order][bad[0]], q[bad[0]], model.image_row(q, c[u, 0], c[u, 2], c[u, 3])[bad[0]])
        # ... and sub-frame j holds the call's local tiles j, j + parts, ...
        if not whole:
            R, n = info[case_of, 1][which], info[case_of, 0][which]
            bad = np.flatnonzero((out // R) % n != j_of[which])
            assert bad.size == 0, "%s: sub-frame %d stores into output tile %d" % (name(h, cases[case_of[which[bad[0]]]]), j_of[which[bad[0]]], (out // R)[bad[0]])


def test_no_part_is_empty_and_parts_are_whole_wave_tiles():
    for h, cases, info, parts in every_cut():
        live = np.arange(model.MAX_PARTS)[None, :] < info[:, :1]
        empty = live & (parts[:, :, 1] <= 0) & (info[:, :1] <= info[:, 3:4])
        bad = np.flatnonzero(empty.any(axis=1))
        assert bad.size == 0, "%s: an empty sub-frame among %d of %d tiles" % (name(h, cases[bad[0]]), info[bad[0], 0], info[bad[0], 3])
        ragged = live & (info[:, :1] > 1) & (parts[:, :, 2] % 8 != 0)
        bad = np.flatnonzero(ragged.any(axis=1))
        assert bad.size == 0, "%s: sub-frames of tiles that are no whole wave tiles" % name(h, cases[bad[0]])
        assert not parts[~live].any()


WIDTHS = (61, 8)
CHUNK_PX = (500, 777, 1000, 2000, 9000)


def test_chunks_are_the_call_s_rows_in_order():
    """chunk after chunk: the call's local rows in order, each once, every chunk but the last a multiple of the unit, every chunk inside the image"""
    seen_cut = 0
    for h in HEIGHTS:
        cases = np.array([c + (w, px) for c in calls(h) for w in WIDTHS for px in CHUNK_PX], np.int32)
        info, chunks = hostlib.row_chunks(cases)
        c = cases.astype(np.int64)
        n = info[:, 2]
        needs = c[:, 1] * c[:, 4] > c[:, 5] * 5 // 4
        bad = np.flatnonzero((n > 1) & ~needs | (n < 1))
        assert bad.size == 0, "%s x %d, %d pixels a chunk: %d chunks" % (name(h, tuple(cases[bad[0], :4]) + (0, 0, 0)), cases[bad[0], 4], cases[bad[0], 5], n[bad[0]])
        seen_cut += int((n > 1).sum())
        live = np.arange(chunks.shape[1])[None, :] < n[:, None]
        case_of, k_of = np.nonzero(live)
        ch = chunks[case_of, k_of].astype(np.int64)

        def say(i):
            return "%s x %d, %d pixels a chunk: chunk %d of %d is %s" % (name(h, tuple(cases[case_of[i], :4]) + (0, 0, 0)), cases[case_of[i], 4], cases[case_of[i], 5],
                                                                          k_of[i], n[case_of[i]], tuple(ch[i]))
        # each chunk starts where the chunk before it ended, and the chunks together have the call's rows
        ends = ch[:, 0] + ch[:, 2]
        starts_ok = np.where(k_of == 0, ch[:, 0] == 0, ch[:, 0] == np.roll(ends, 1))
        last = k_of == n[case_of] - 1
        bad = np.flatnonzero(~starts_ok | (last & (ends != c[case_of, 1])) | ((ch[:, 2] <= 0) & (c[case_of, 1] > 0)) | (ch[:, 3] <= 0) | (ch[:, 4] != c[case_of, 3]))
        assert bad.size == 0, say(bad[0])
        # its rows are those local rows of the call, in order
        which, r = model.local_rows(ch[:, 2])
        img = model.image_row(r, ch[which, 1], ch[which, 3], ch[which, 4])
        cc = c[case_of[which]]
        exp = model.image_row(ch[which, 0] + r, cc[:, 0], cc[:, 2], cc[:, 3])
        bad = np.flatnonzero(img != exp)
        assert bad.size == 0, say(which[bad[0]]) + ": its row %d is image row %d, the call's is %d" % (r[bad[0]], img[bad[0]], exp[bad[0]])
        # launch_render_chunk's own check of a chunk
        bad = np.flatnonzero((img < 0) | (img >= h))
        assert bad.size == 0, say(which[bad[0]]) + ": image row %d of %d" % (img[bad[0]], h)
        # all but the last: two sub-frames' worth of whole tiles
        unit = model.chunk_unit(cases[:, 2], cases[:, 3])
        bad = np.flatnonzero(~last & (ch[:, 2] % unit[case_of] != 0))
        assert bad.size == 0, say(bad[0]) + ": no multiple of %d rows" % unit[case_of[bad[0]]]
        np.testing.assert_array_equal(info[n > 1, 0], unit[n > 1])
    assert seen_cut > 10000                                        # (the cases do cut)


@pytest.mark.parametrize("px,rows,expected", [
    (2000, (0, 131, 131, 1), [(0, 0, 48, 48, 1), (48, 48, 48, 48, 1), (96, 96, 35, 35, 1)]),          # the frame of tests/test_gpu_parts.py under RT_CHUNK_MPX=0.002 (61 wide)
    (2000, (13, 105, 105, 1), [(0, 13, 32, 32, 1), (32, 45, 32, 32, 1), (64, 77, 32, 32, 1), (96, 109, 9, 9, 1)]),
    (2000, (8, 48, 8, 3), [(0, 8, 32, 8, 3), (32, 104, 16, 8, 3)]),
])
def test_chunks_by_hand(px, rows, expected):
    info, chunks = hostlib.row_chunks([rows + (61, px)])
    assert info[0, 2] == len(expected)
    assert [tuple(x) for x in chunks[0, :len(expected)]] == expected
