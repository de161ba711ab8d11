"""The cut of a call's rows into sub-frames and chunks, from the definitions alone (a helper module, like lbvh_model.py): what the cut of csrc/rt_rowcut.h has to
satisfy, never how it computes it.

A set of rows is (row0, n_rows, tile_rows, tile_step), include/raytrace_hip.h: local row r is IMAGE row row0 + (r // tile_rows) * tile_rows * tile_step + r % tile_rows
(launch_render_chunk checks the last one against the height).  A sub-frame adds (out_tile0, out_tile_step): its local row r is stored at OUTPUT row
((r // tile_rows) * out_tile_step + out_tile0) * tile_rows + r % tile_rows of the call's buffer (out_index, csrc/rt_kernels.hip.h).  A call's own local row q is stored
at output row q."""
import numpy as np

MAX_PARTS = 8


def image_row(r, row0, tile_rows, tile_step):
    """image row of local row r (numbers or arrays of equal length)"""
    return row0 + (r // tile_rows) * tile_rows * tile_step + r % tile_rows


def output_row(r, tile_rows, out_tile0, out_tile_step):
    """output row of a sub-frame's local row r"""
    return ((r // tile_rows) * out_tile_step + out_tile0) * tile_rows + r % tile_rows


def local_rows(counts):
    """for sets of counts[k] rows each: (k of every row, its local row r), set after set"""
    counts = np.asarray(counts, np.int64)
    which = np.repeat(np.arange(len(counts)), counts)
    first = np.cumsum(counts) - counts
    return which, np.arange(counts.sum(), dtype=np.int64) - first[which]


def shares(height, tile_rows, world):
    """every rank's rows of `height` image rows dealt out as interleaved tiles: tile t (tile_rows rows, the last one what is left) belongs to rank t % world"""
    n_tiles = -(-height // tile_rows)
    for rank in range(world):
        n = sum(min(tile_rows, height - t * tile_rows) for t in range(rank, n_tiles, world))
        yield rank * tile_rows, n, tile_rows, world


def tile_height(tile_rows, tile_step):
    """the height of the tiles the cut deals out: contiguous rows are cut into the kernels' 8-row wave tiles, whatever tile height the caller described them with"""
    return np.where(np.asarray(tile_step) == 1, 8, tile_rows)


def parts_expected(n_rows, tile_rows, tile_step, want, one):
    """how many sub-frames: one for a counting run and for tiles that are not whole wave tiles, else as many as wanted, at most 8 and at most one per tile"""
    R = tile_height(tile_rows, tile_step)
    T = -(-np.asarray(n_rows) // R)
    return np.where((np.asarray(one) != 0) | (R % 8 != 0), 1, np.maximum(1, np.minimum(np.minimum(want, MAX_PARTS), T)))


def chunk_unit(tile_rows, tile_step):
    """what a chunk's rows are a multiple of: two sub-frames' worth of whole tiles (8-row wave tiles for contiguous rows)"""
    return np.where(np.asarray(tile_step) == 1, 16, 2 * np.asarray(tile_rows))
