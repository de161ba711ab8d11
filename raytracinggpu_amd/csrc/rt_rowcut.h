// rt_rowcut.h -- how a call's rows are cut up: into sub-frames of interleaved tiles that run side by side (RT_PARTS), and into sequential chunks of whole tiles (RT_CHUNK_MPX).
//
// A call renders n_rows LOCAL rows: tiles of tile_rows rows, every tile_step-th tile of the image from image row row0 on (rt_rows, include/raytrace_hip.h).  Local row r is
//     image row   row0 + (r / tile_rows) * tile_rows * tile_step + r % tile_rows        (rows_image_row; what launch_render_chunk checks against the image's height)
// and is stored at output row r of the call's buffer.  A sub-frame is such a set of rows again (every `parts`-th local tile), with two more numbers that say where its tiles lie
// in the CALL's output: its local row r goes to
//     output row  ((r / tile_rows) * out_tile_step + out_tile0) * tile_rows + r % tile_rows                                             (out_index, rt_kernels.hip.h)
// The sub-frames of a call together hold every (image row, output row) pair of the call exactly once; with `whole` (a batch cut by frames) every sub-frame holds them all.
// The chunks of a call are consecutive ranges of its local rows, cut at tile boundaries, each described as a call of its own.
// Plain C++, integers only: the library and the host library (rth_row_cut, rth_row_chunks, tests/test_rowcut_model.py) compile the same text.
#pragma once
#include <stdint.h>

namespace rtk {

constexpr int kRowCutMaxParts = 8;                       // rt_ctx::kMaxParts

struct Rows { int row0, n_rows, tile_rows, tile_step; };                                   // rt_rows
struct RowPart { int row0, n_rows, tile_rows, tile_step, out_tile0, out_tile_step; };      // a sub-frame: the row fields of rtk::Frame

inline int64_t rows_image_row(const Rows &rows, int64_t r) { return rows.row0 + (r / rows.tile_rows) * rows.tile_rows * (int64_t)rows.tile_step + (r % rows.tile_rows); }

// The cut of a call's rows into `parts` independent sub-frames of interleaved tiles (R rows high, every G-th tile of the image; T of them in this call)
struct RowCut {
    int parts, R, G, T;
    // sub-frame j's rows (local tiles j, j + parts, ...) and where its tiles lie in the call's output; whole: every sub-frame holds all rows (a batch cut by frames)
    RowPart part(const Rows &rows, int j, bool whole) const {
        const int of = whole ? 1 : parts;
        if (whole) j = 0;
        const int Tj = (T - j + of - 1) / of;
        int n = Tj * R;
        if (Tj > 0 && (T - 1) % of == j) n -= T * R - rows.n_rows;   // the last local tile may be partial
        return RowPart{rows.row0 + j * R * G, n, R, G * of, j, of};
    }
};
inline RowCut split_rows(const Rows &rows, int want, bool one) {
    RowCut c{want < kRowCutMaxParts ? want : kRowCutMaxParts, rows.tile_rows, rows.tile_step, 0};
    if (c.G == 1) c.R = 8;                                        // contiguous rows: any tile height describes them
    c.T = (rows.n_rows + c.R - 1) / c.R;                          // local tiles of this call
    if (c.R % 8 != 0 || one) c.parts = 1;
    if (c.parts > c.T) c.parts = c.T > 0 ? c.T : 1;
    return c;
}

// A call of more than 5/4 of chunk_px pixels is cut into chunks (chunk_px <= 0: never)
inline bool rows_need_chunks(const Rows &rows, int width, int64_t chunk_px) { return chunk_px > 0 && (int64_t)rows.n_rows * width > chunk_px * 5 / 4; }
// The chunks of such a call: `per` local rows each (the last one what is left), a multiple of `unit` -- whole tiles (and whole 8-row wave tiles for contiguous rows), two
// sub-frames' worth at least.  (Contiguous rows: tile_rows only says how the caller described them -- rt_render passes one tile of n_rows -- and every chunk is re-described;
// only interleaved tiles must be cut at tile boundaries.)
struct RowChunks {
    int unit, per, n;
    int first(int k) const { return k * per; }                   // chunk k's first local row: where its output starts in the call's buffer
    Rows chunk(const Rows &rows, int k) const {
        const int a = first(k), nr = per < rows.n_rows - a ? per : rows.n_rows - a;
        if (rows.tile_step == 1) return Rows{rows.row0 + a, nr, nr, 1};       // contiguous rows: one tile of any height describes them
        return Rows{rows.row0 + (a / rows.tile_rows) * rows.tile_rows * rows.tile_step, nr, rows.tile_rows, rows.tile_step};
    }
};
inline RowChunks chunk_rows(const Rows &rows, int width, int64_t chunk_px) {
    RowChunks c{rows.tile_step == 1 ? 16 : rows.tile_rows * 2, 0, 0};
    const int64_t n_chunks = ((int64_t)rows.n_rows * width + chunk_px - 1) / chunk_px;
    c.per = (int)(((int64_t)rows.n_rows + n_chunks - 1) / n_chunks);
    c.per = (c.per + c.unit - 1) / c.unit * c.unit;
    c.n = (rows.n_rows + c.per - 1) / c.per;
    return c;
}

}  // namespace rtk
