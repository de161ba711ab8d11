"""A numpy twin of the LBVH builder (raytracinggpu_amd/csrc/rt_lbvh.hip.h; rt_mesh_rebuild_mode(RT_BVH_LBVH)), written top-down and recursively:
no parallel hierarchy emission, no binary searches, no atomics, no prefix sums -- an independent construction of the SAME tree.  The library is compiled
with -ffp-contract=off and correctly rounded division, rocPRIM's radix sort is stable, box merges are min / max and every surface-area decision is a
function of already decided children: the device's bvh_arr10, triangle order and rt_build_stats are a deterministic function of (vertices, uploaded
triangle order, ct), and this file states that function in binary32, operation by operation.

    centroid   ((A + B) + C) * float32(1 / 3) per axis
    bounds     min / max of the centroids per axis; ext = the largest of the three hi - lo (ONE scale: cubic cells)
    cell       u = (c - lo) / ext (0 unless ext > 0), clamped to [0, 1]; q = trunc(float32(u * 2097151)); code = spread(qx) << 2 | spread(qy) << 1 | spread(qz)
    sort       by (code, uploaded index)
    tree       a range of sorted positions splits at the highest differing bit of the augmented key (code, sorted position) of its two ends
    boxes      min / max of the vertex coordinates
    cut        area = dx*dy + dy*dz + dz*dx; wl, wr = area_child / A if A > 0 else 1; inner = (2*cb + wl*cl) + wr*cr; leaf = ct * float(cnt);
               a node is a leaf iff cnt <= 2 or (cnt <= 32 and leaf <= inner); a single triangle costs ct; ct = 1.0 from 16 384 triangles, else 1.6; cb = 1
    numbering  candidates: an internal node has its Karras index (root 0; the children of a split after sorted position g are g and g + 1), the single
               triangle at sorted position k is n - 1 + k; the survivors are numbered in ascending candidate order
    row        [left, right, lo.xyz, hi.xyz, start, end), -1 -1 for a leaf, ranges in sorted positions

Signed zeros: min / max here are numpy's, which may order -0 and +0 either way; the meshes of the tests hold no -0 coordinate."""
import numpy as np

F = np.float32
LEAF, MIN_LEAF = 32, 2                                                   # kLbvhLeaf, kLbvhMinLeaf
CT_SMALL, CT_LARGE, CT_LARGE_FROM, CB = F(1.6), F(1.0), 16384, F(1.0)   # kLbvhCt; the fixed-point pairs' cost, from kQ16AutoNodes triangles on; kLbvhCb
THIRD = F(1.0) / F(3.0)
CELLS = F(2097151.0)                                                     # 2^21 - 1


def centroids(v, tris):
    v = np.asarray(v, F)
    A, B, C = (v[np.asarray(tris)[:, k]] for k in range(3))
    return ((A + B) + C) * THIRD


def cells(v, tris):
    """[n, 3] integer cell of every centroid (21 bits per axis)."""
    c = centroids(v, tris)
    lo, hi = c.min(axis=0), c.max(axis=0)
    ext = (hi - lo).max()
    if not ext > 0:
        return np.zeros(c.shape, np.uint64)
    u = np.minimum(np.maximum((c - lo) / ext, F(0)), F(1))
    return (u * CELLS).astype(np.uint64)                                # (a cast truncates)


def _spread21(x):
    x = x & np.uint64(0x1fffff)
    for s, m in ((32, 0x1f00000000ffff), (16, 0x1f0000ff0000ff), (8, 0x100f00f00f00f00f), (4, 0x10c30c30c30c30c3), (2, 0x1249249249249249)):
        x = (x | x << np.uint64(s)) & np.uint64(m)
    return x


def morton(v, tris):
    q = cells(v, tris)
    return _spread21(q[:, 0]) << np.uint64(2) | _spread21(q[:, 1]) << np.uint64(1) | _spread21(q[:, 2])


def _area(lo, hi):
    dx, dy, dz = hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]
    return dx * dy + dy * dz + dz * dx


class _Node:
    __slots__ = ("cand", "s", "e", "lo", "hi", "cost", "leaf", "l", "r", "depth")


def _split(code, s, e):
    """last sorted position of the left child of the range [s, e] (both ends included)"""
    if code[s] != code[e]:
        bit = (code[s] ^ code[e]).bit_length() - 1
        g = s
        while not (code[g + 1] >> bit) & 1:                             # (sorted: the positions with a 0 in that bit come first)
            g += 1
        return g
    bit = (s ^ e).bit_length() - 1                                      # equal codes: the positions tell them apart
    return ((e >> bit) << bit) - 1


def build(vertices, triangles_uploaded, ct=None):
    """-> (arr10 float32 [n_nodes, 10], order int32 [n], stats).  None for n <= 4: the library runs the reference builder there (rebuild_part)."""
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    tris = np.ascontiguousarray(triangles_uploaded, np.int32).reshape(-1, 3)
    n = len(tris)
    if n <= 4:
        return None
    ct = F(ct) if ct is not None else (CT_LARGE if n >= CT_LARGE_FROM else CT_SMALL)
    order = np.argsort(morton(v, tris), kind="stable").astype(np.int32)  # ties: the uploaded index
    code = [int(c) for c in morton(v, tris)[order]]
    P = v[tris[order]]                                                   # [n, 3 corners, 3]
    tlo, thi = P.min(axis=1), P.max(axis=1)

    def make(s, e, cand):
        nd = _Node()
        nd.cand, nd.s, nd.e, nd.l, nd.r = cand, s, e, None, None
        if s == e:
            nd.lo, nd.hi, nd.cost, nd.leaf = tlo[s], thi[s], ct, True
            return nd
        g = _split(code, s, e)
        L = make(s, g, g if g > s else n - 1 + g)
        R = make(g + 1, e, g + 1 if g + 1 < e else n - 1 + g + 1)
        nd.l, nd.r = L, R
        nd.lo, nd.hi = np.minimum(L.lo, R.lo), np.maximum(L.hi, R.hi)
        cnt = e - s + 1
        A = _area(nd.lo, nd.hi)
        wl = _area(L.lo, L.hi) / A if A > 0 else F(1)
        wr = _area(R.lo, R.hi) / A if A > 0 else F(1)
        inner = (F(2) * CB + wl * L.cost) + wr * R.cost
        leaf = ct * F(cnt)
        nd.leaf = bool(cnt <= MIN_LEAF or (cnt <= LEAF and leaf <= inner))
        nd.cost = leaf if nd.leaf else inner
        return nd

    with np.errstate(all="ignore"):
        root = make(0, n - 1, 0)
    alive = []
    stack = [(root, 0)]
    while stack:                                                         # what hangs below a leaf is gone
        nd, d = stack.pop()
        nd.depth = d
        alive.append(nd)
        if not nd.leaf:
            stack += [(nd.l, d + 1), (nd.r, d + 1)]
    alive.sort(key=lambda nd: nd.cand)
    index = {nd.cand: j for j, nd in enumerate(alive)}
    arr = np.zeros((len(alive), 10), F)
    for j, nd in enumerate(alive):
        arr[j, 0], arr[j, 1] = (-1, -1) if nd.leaf else (index[nd.l.cand], index[nd.r.cand])
        arr[j, 2:5], arr[j, 5:8] = nd.lo, nd.hi
        arr[j, 8], arr[j, 9] = nd.s, nd.e + 1
    leaves = [nd for nd in alive if nd.leaf]
    stats = dict(n_nodes=len(alive), n_leaves=len(leaves), max_leaf_tris=max(nd.e - nd.s + 1 for nd in leaves), max_depth=max(nd.depth for nd in leaves))
    return arr, order, stats


def check_tree(arr, order, n_tris):
    """A proper tree in the reference's flat layout: every node reachable once, leaves of 1..32 triangles covering [0, n) exactly."""
    n = len(arr)
    assert sorted(order.tolist()) == list(range(n_tris))
    seen = np.zeros(n, bool)
    covered = np.zeros(n_tris, np.int32)
    stack = [0]
    leaves = 0
    while stack:
        k = stack.pop()
        assert 0 <= k < n and not seen[k]
        seen[k] = True
        l, r, s, e = int(arr[k, 0]), int(arr[k, 1]), int(arr[k, 8]), int(arr[k, 9])
        assert 0 <= s < e <= n_tris
        assert (arr[k, 2:5] <= arr[k, 5:8]).all()
        if l < 0:
            assert r < 0 and e - s <= 32
            covered[s:e] += 1
            leaves += 1
        else:
            assert e - s > 2
            for c in (l, r):                                            # children nest inside the parent, ranges partition the parent's
                assert (arr[c, 2:5] >= arr[k, 2:5]).all() and (arr[c, 5:8] <= arr[k, 5:8]).all()
            assert {int(arr[l, 8]), int(arr[r, 8])} >= {s} and {int(arr[l, 9]), int(arr[r, 9])} >= {e}
            assert int(arr[l, 9]) - int(arr[l, 8]) + int(arr[r, 9]) - int(arr[r, 8]) == e - s
            stack += [l, r]
    assert seen.all() and (covered == 1).all()
    return leaves
