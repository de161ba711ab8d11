// rt_qrows.h -- row windows of the traversal queue: which slots a traversal launch has to look at.
//
// The queue holds the rays in slot order: slot group sg = col << log2S | a (four slots each) holds ray group g = a * Q + col, a in [0, S), col in [0, Q)
// (wf_slot_to_path, wf_ray_to_slot).  Continuation (Y) rays are the ray groups g < n_paths / 4, shadow (X) rays the rest, so with
//     a_lo = (n_paths / 4) / Q,   c_lo = (n_paths / 4) % Q
// every row a < a_lo holds Y rays only, every row a > a_lo shadow rays or padding only, and row a_lo is the one mixed row (Y in its columns below c_lo).  Hence
//     the Y window = rows [0, a_lo + (c_lo > 0)),     the X window = rows [a_lo, S).
// A launch that cannot meet a live record of one kind (the first traversal launch of a chain: no shadow ray yet; the last: no continuation ray any more) enumerates
// the other kind's window instead of the whole queue: window-relative slot v stands for column (v >> 2) / rows, row row0 + (v >> 2) % rows.  Workgroup shares are cut
// from the window's slots the way share_geometry cuts them from the queue's; the last shares are clipped at the window's end, so no slot beyond column Q - 1 is
// ever formed.  An all-zero QRows means "every row": the kernel then uses the slot index as it always did.
// Host and device share this file (tests/test_queue_rows.py drives it through the host library's rth_qrows_enumerate).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_QROWS_HD __host__ __device__ __forceinline__
#else
#define RT_QROWS_HD inline
#endif

namespace rtk {

struct QRows { int row0, rows; unsigned int rows_m; };   // rows [row0, row0 + rows) of every column; rows_m = floor(2^32 / rows) (wf_div's magic); rows == 0: no window

RT_QROWS_HD unsigned int qrows_magic(int d) { return d <= 1 ? 0xffffffffu : (unsigned int)(0x100000000ull / (unsigned long long)d); }
// n / d for 0 <= n < 2^32 with m = qrows_magic(d): the estimate mulhi(n, m) is the quotient or one below it (as wf_div)
RT_QROWS_HD int qrows_div(int n, int d, unsigned int m) {
    unsigned int q = (unsigned int)(((unsigned long long)(unsigned int)n * m) >> 32);
    q += ((unsigned int)n - q * (unsigned int)d >= (unsigned int)d) ? 1u : 0u;
    return (int)q;
}
RT_QROWS_HD QRows qrows_make(int row0, int rows, int S) {
    QRows w;
    if (rows >= S) { w.row0 = 0; w.rows = 0; w.rows_m = 0u; }        // every row: today's indexing
    else { w.row0 = row0; w.rows = rows; w.rows_m = qrows_magic(rows); }
    return w;
}
// the rows that can hold a continuation ray / a shadow ray (n_paths need not be a multiple of 4: a group that holds both kinds is in both windows)
RT_QROWS_HD QRows qrows_y(int n_paths, int log2S, int Q) {
    const int ny = (n_paths + 3) / 4, a_lo = ny / Q, c_lo = ny - a_lo * Q;
    return qrows_make(0, a_lo + (c_lo > 0 ? 1 : 0), 1 << log2S);
}
RT_QROWS_HD QRows qrows_x(int n_paths, int log2S, int Q) {
    const int a_lo = (n_paths / 4) / Q;
    return qrows_make(a_lo, (1 << log2S) - a_lo, 1 << log2S);
}
// slots of the window (columns [0, Q): the queue's padding columns are in no window)
RT_QROWS_HD int64_t qrows_slots(const QRows &w, int Q) { return (int64_t)w.rows * Q * 4; }
// slots per workgroup share when `tblocks` workgroups divide `total` slots (a multiple of 4, as share_geometry's)
RT_QROWS_HD int qrows_share(int64_t total, int64_t tblocks) { return (int)(((total + tblocks - 1) / tblocks + 3) / 4 * 4); }
// length of workgroup blk's share: the shares past the window's end are short or empty
RT_QROWS_HD int qrows_share_len(int64_t total, int share, int blk) {
    const int64_t left = total - (int64_t)blk * share;
    return left <= 0 ? 0 : left < share ? (int)left : share;
}
// queue slot of window-relative slot v, 0 <= v < qrows_slots
RT_QROWS_HD int qrows_slot(const QRows &w, int log2S, int v) {
    const int gv = v >> 2;
    const int col = qrows_div(gv, w.rows, w.rows_m), a = w.row0 + (gv - col * w.rows);
    return ((col << log2S | a) << 2) | (v & 3);
}

}  // namespace rtk
