"""Meshes for the LBVH builder's special cases (tests/lbvh_model.py, rt_lbvh.hip.h), shared by the CPU tests of the model and the GPU tests of the device
against it; each as small as its edge allows.  Every generator returns (vertices float32 [nv, 3], triangles int32 [n, 3]) in the order a caller would hand
them to hostlib.build_mesh."""
import numpy as np

SIZES = (5, 6, 33, 63, 64, 65, 257)                                     # below, at and above a wave and a 256-thread block: the tails of the n, n - 1 and 2 n - 1 grids
_CORNERS = np.array([[-1, -1, 1], [1, 0, -1], [0, 1, 0]], np.float64) / 16   # three offsets that sum to zero exactly; extent 0.125 on every axis


def displaced_grid(n, seed=11):
    rng = np.random.default_rng(seed)
    gx, gz = np.meshgrid(np.linspace(-18, 18, n), np.linspace(-14, 22, n), indexing="ij")
    gy = -9.0 + 3.0 * np.sin(gx * 0.45) * np.cos(gz * 0.38) + 0.15 * rng.standard_normal((n, n))
    v = np.stack([gx, gy, gz], -1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a = (i * n + j).reshape(-1)
    t = np.concatenate([np.stack([a, a + 1, a + n], 1), np.stack([a + 1, a + n + 1, a + n], 1)]).astype(np.int32)
    return v, t


def sizes(n):
    """random soup of n triangles over n + 4 vertices (shared vertices, now and then a repeated one: zero area)"""
    rng = np.random.default_rng(100 + n)
    return rng.uniform(-15, 15, (n + 4, 3)).astype(np.float32), rng.integers(0, n + 4, (n, 3)).astype(np.int32)


def one_cell():
    """100 concentric triangles of different sizes whose centroids are bit-equal: ext == 0, every code 0, a tree of positions alone -- and boxes that differ, so the cut still decides"""
    dirs = np.array([[[2, -1, -1], [-1, 2, -1], [-1, -1, 2]], [[2, 0, -1], [-1, 1, 0], [-1, -1, 1]], [[0, 2, -1], [1, -1, -1], [-1, -1, 2]]], np.float64)   # each set sums to zero
    c = np.array([2.0, -4.0, 3.0])
    v = np.concatenate([c + dirs[k % 3] * ((k + 1) / 16) for k in range(100)])   # multiples of 1 / 16 below 32: exact in binary32, and so is A + B + C = 3 c
    return v.astype(np.float32), np.arange(300, dtype=np.int32).reshape(100, 3)


def coincident_cluster():
    """200 random triangles and 40 copies of one of them: equal codes, equal boxes, a range above 32 that cannot become one leaf"""
    rng = np.random.default_rng(21)
    c = rng.uniform(-15, 15, (200, 1, 3))
    v = (c + rng.uniform(-2, 2, (200, 3, 3))).reshape(-1, 3).astype(np.float32)
    t = np.arange(600, dtype=np.int32).reshape(200, 3)
    return v, np.concatenate([t, np.repeat(t[17:18], 40, axis=0)])


def collinear_degenerate():
    """60 zero-area triangles along a line parallel to x: every box has A == 0, wl = wr = 1"""
    rng = np.random.default_rng(22)
    v = np.stack([rng.uniform(-15, 15, 180), np.full(180, 1.5), np.full(180, -2.5)], 1).astype(np.float32)
    return v, np.arange(180, dtype=np.int32).reshape(60, 3)


def planar():
    """300 triangles in the plane y = -3.25: one centroid extent is 0, two are not"""
    rng = np.random.default_rng(23)
    c = rng.uniform(-15, 15, (300, 1, 3))
    v = c + rng.uniform(-1.5, 1.5, (300, 3, 3))
    v[..., 1] = -3.25
    return v.reshape(-1, 3).astype(np.float32), np.arange(900, dtype=np.int32).reshape(300, 3)


def grid_ct1():
    """18 432 triangles: from 16 384 on the cut's triangle cost is 1.0"""
    return displaced_grid(97)


def cat(cat_golden):
    return np.array(cat_golden["vertices"], np.float32), np.array(cat_golden["tri_obj_order"], np.int32)


def _comb(first_bit):
    """Per axis and Morton bit b one tiny triangle whose centroid lies in cell 2^b of that axis and cell 0 of the other two, 40 coincident ones in cell 0 and one at the far
    corner of x that fixes the scale: a radix tree that peels ONE triangle off per level, 3 levels per bit, and then tells the 40 apart by position.  Scaled by 2^-17 (a power
    of two: the cells stay what they are) so that the root box is small."""
    cs = [np.where(np.arange(3) == ax, 2.0 ** b + 0.5, 0.25) for ax in range(3) for b in range(first_bit, 21)]
    cs += [np.full(3, 0.25)] * 40 + [np.array([2097151.0, 0.25, 0.25])]
    v = np.concatenate([c + _CORNERS for c in cs]) * 2.0 ** -17
    return v.astype(np.float32), np.arange(3 * len(cs), dtype=np.int32).reshape(len(cs), 3)


def comb_deep():
    """104 triangles, deeper than both limits of the device-side install (56 in rebuild_part, the 58 path bits of lbvh_walk_kernel's sort key)"""
    return _comb(0)


def comb_shallow():
    """the comb without its three lowest bits: far deeper than any other mesh here, and still installed on the device"""
    return _comb(3)


def all_fixtures(cat_golden):
    out = {f"sizes{n}": sizes(n) for n in SIZES}
    out.update(one_cell=one_cell(), coincident_cluster=coincident_cluster(), collinear_degenerate=collinear_degenerate(), planar=planar(), grid_ct1=grid_ct1(),
               cat=cat(cat_golden), comb_deep=comb_deep(), comb_shallow=comb_shallow())
    return out


NAMES = tuple(f"sizes{n}" for n in SIZES) + ("one_cell", "coincident_cluster", "collinear_degenerate", "planar", "grid_ct1", "cat", "comb_deep", "comb_shallow")
