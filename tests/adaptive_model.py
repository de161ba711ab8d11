"""The numpy twin of adaptive sampling (rt_sample_counts*, and the plan of rt_render_counts* that rt_kat_sample_plan returns): the counts a history asks for, in
binary32 with one rounding per operation, and the list of (pixel, sample) items in pixel-slot order with every slot's offset into it."""
import numpy as np

MAX_SAMPLE_COUNT = 64
F = np.float32


def slot_pixels(W, H):
    """-> (x, y) of every pixel slot: 8 x 8 tiles, tiles row-major over the frame, pixels row-major inside a tile; slots past the right or lower edge included"""
    tiles_x, tiles_y = (W + 7) // 8, (H + 7) // 8
    slot = np.arange(tiles_x * tiles_y * 64)
    tile, p = slot >> 6, slot & 63
    return (tile % tiles_x) * 8 + (p & 7), (tile // tiles_x) * 8 + (p >> 3)


def plan(counts, first_sample=0):
    """counts [H, W] uint8 -> (offs [slots + 1] uint32, items [n, 3] int32 of (x, y, sample)): slot-major then sample; samples [first_sample, min(c, 64)) of a pixel"""
    counts = np.asarray(counts)
    H, W = counts.shape
    x, y = slot_pixels(W, H)
    inside = (x < W) & (y < H)
    c = np.zeros(x.shape, np.int64)
    c[inside] = np.minimum(counts[y[inside], x[inside]].astype(np.int64), MAX_SAMPLE_COUNT)
    t = np.maximum(c - first_sample, 0)
    offs = np.zeros(len(t) + 1, np.int64)
    np.cumsum(t, out=offs[1:])
    owner = np.repeat(np.arange(len(t)), t)
    samp = np.arange(offs[-1]) - offs[owner] + first_sample
    items = np.stack([x[owner], y[owner], samp], axis=1).astype(np.int32).reshape(-1, 3)
    return offs.astype(np.uint32), items


def sample_counts(history, max_samples, short_history, new_surface_samples, k_rel, lum_floor):
    """history [2, H, W, 4] (plane 1 = m1, m2, n, V) -> counts [H, W] uint8, the formula of raytrace_hip.h"""
    h = np.asarray(history, F)[1]
    m1, n, V = h[..., 0], h[..., 2], h[..., 3]
    with np.errstate(all="ignore"):
        e_n = np.where(n < F(short_history), F(new_surface_samples - 1), F(0))
        rel = V / (m1 * m1 + F(lum_floor))
        e_v = np.floor(F(k_rel) * rel)
        e_v = np.where(e_v >= F(1), e_v, F(0))                         # a NaN compares false
        count = F(1) + np.minimum(F(max_samples - 1), np.maximum(e_n, e_v))   # neither operand of the max is a NaN here
        count = np.where(n == F(0), F(1), count)
    return count.astype(np.uint8)
