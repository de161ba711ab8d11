"""tests/lbvh_model.py, the numpy twin of the LBVH builder, checked on its own: a proper tree, boxes and codes against brute force, the cut against an
enumeration of every cut, and the depths the fixtures of tests/lbvh_fixtures.py are there for.  tests/test_gpu_lbvh_model.py then holds the device to it bit for bit."""
import numpy as np
import pytest

from . import lbvh_fixtures as fx
from . import lbvh_model as lm
from .test_gpu_parity import _synthetic_mesh, values_equal

F = np.float32


@pytest.fixture(scope="module")
def meshes(cat_golden):
    return fx.all_fixtures(cat_golden)


@pytest.fixture(scope="module")
def trees(meshes):
    return {k: lm.build(v, t) for k, (v, t) in meshes.items()}


def test_the_names_cover_the_fixtures(meshes):
    assert tuple(meshes) == fx.NAMES


@pytest.mark.parametrize("name", fx.NAMES)
def test_model_builds_a_proper_tree_with_brute_force_boxes(meshes, trees, name):
    v, t = meshes[name]
    arr, order, st = trees[name]
    assert lm.check_tree(arr, order, len(t)) == st["n_leaves"] and st["n_nodes"] == len(arr) == 2 * st["n_leaves"] - 1
    leaf = arr[:, 0] < 0
    assert st["max_leaf_tris"] == int((arr[leaf, 9] - arr[leaf, 8]).max()) <= 32
    P = v[t[order]]
    for k in range(len(arr)):
        s, e = int(arr[k, 8]), int(arr[k, 9])
        np.testing.assert_array_equal(arr[k, 2:5], P[s:e].reshape(-1, 3).min(axis=0))
        np.testing.assert_array_equal(arr[k, 5:8], P[s:e].reshape(-1, 3).max(axis=0))
    depth = np.zeros(len(arr), int)                                       # max_depth: ancestors of the deepest leaf
    for k in np.argsort(arr[:, 9] - arr[:, 8], kind="stable")[::-1]:      # (a parent's range is larger than its children's)
        if arr[k, 0] >= 0:
            depth[int(arr[k, 0])] = depth[int(arr[k, 1])] = depth[k] + 1
    assert st["max_depth"] == depth[leaf].max()
    code = lm.morton(v, t)
    assert (code[order][:-1] <= code[order][1:]).all()                    # sorted by code, ties by uploaded index
    assert all(a < b for a, b, ca, cb in zip(order[:-1], order[1:], code[order][:-1], code[order][1:]) if ca == cb)


@pytest.mark.parametrize("name", fx.NAMES)
def test_codes_equal_a_bit_loop_interleave(meshes, name):
    v, t = meshes[name]
    c = np.stack([((v[t[:, 0], k] + v[t[:, 1], k]) + v[t[:, 2], k]) * (F(1) / F(3)) for k in range(3)], 1)
    assert c.dtype == F
    lo = c.min(axis=0)
    ext = max(F(c[:, k].max() - lo[k]) for k in range(3))
    want = []
    for row in c:
        code = 0
        for k in range(3):
            u = F(row[k] - lo[k]) / ext if ext > 0 else F(0)
            q = int(min(max(u, F(0)), F(1)) * F(2097151))
            for b in range(21):
                code |= (q >> b & 1) << (3 * b + 2 - k)                   # x above y above z
        want.append(code)
    assert [int(x) for x in lm.morton(v, t)] == want


def _radix(keys, s, e):
    """the radix tree over strictly increasing integer keys as nested tuples (s, e, left, right), leaves (s, s, None, None)"""
    if s == e:
        return (s, e, None, None)
    bit = (keys[s] ^ keys[e]).bit_length() - 1
    left = [k for k in range(s, e + 1) if not keys[k] >> bit & 1]
    assert left == list(range(s, left[-1] + 1))
    return (s, e, _radix(keys, s, left[-1]), _radix(keys, left[-1] + 1, e))


def _cuts(node, lo, hi, ct):
    """every cut below `node` -> [(cost in float64, tuple of leaf ranges)]; box of a range from lo / hi of the sorted triangles"""
    s, e, L, R = node
    cnt = e - s + 1

    def area(a, b):
        d = hi[a:b + 1].max(axis=0).astype(np.float64) - lo[a:b + 1].min(axis=0).astype(np.float64)
        return d[0] * d[1] + d[1] * d[2] + d[2] * d[0]
    out = []
    if cnt <= 32:
        out.append((ct * cnt, ((s, e + 1),)))
    if cnt > 2:
        A = area(s, e)
        wl, wr = (area(L[0], L[1]) / A, area(R[0], R[1]) / A) if A > 0 else (1.0, 1.0)
        out += [(2.0 + wl * cl + wr * cr, ll + lr) for cl, ll in _cuts(L, lo, hi, ct) for cr, lr in _cuts(R, lo, hi, ct)]
    return out


def _small_meshes(meshes):
    out = {k: m for k, m in meshes.items() if len(m[1]) <= 12}
    for seed, n in ((1, 7), (2, 9), (3, 11), (4, 12), (5, 12)):
        rng = np.random.default_rng(seed)
        c = rng.uniform(-10, 10, (n, 1, 3))
        out[f"random{seed}"] = ((c + rng.uniform(-3, 3, (n, 3, 3))).reshape(-1, 3).astype(F), np.arange(3 * n, dtype=np.int32).reshape(n, 3))
    v, t = fx.one_cell()
    out["one_cell12"] = (v, t[:12])                                       # equal codes: cut by position
    return out


@pytest.mark.parametrize("ct", [None, 1.0, 4.0])
def test_the_cut_is_the_cheapest_of_all_cuts(meshes, ct):
    small = _small_meshes(meshes)
    assert {"sizes5", "sizes6"} <= set(small)
    for name, (v, t) in small.items():
        arr, order, _ = lm.build(v, t, ct=ct)
        code = lm.morton(v, t)[order]
        keys = [int(c) << 32 | k for k, c in enumerate(code)]
        P = v[t[order]]
        cuts = _cuts(_radix(keys, 0, len(t) - 1), P.min(axis=1), P.max(axis=1), float(F(1.6 if ct is None else ct)))
        mine = tuple(sorted((int(r[8]), int(r[9])) for r in arr if r[0] < 0))
        cost = [c for c, leaves in cuts if tuple(sorted(leaves)) == mine]
        assert len(cost) == 1, name                                       # the model's tree IS a cut of the radix tree
        assert cost[0] == min(c for c, _ in cuts), (name, cost[0], min(c for c, _ in cuts))   # exact ties only
        assert len(cuts) > 1


def test_the_combs_cross_and_respect_the_depth_limits_of_the_device_install(trees):
    """rebuild_part hands a tree deeper than 56 to the host install; lbvh_walk_kernel's breadth-first sort key holds 58 path bits"""
    assert trees["comb_deep"][2]["max_depth"] > 58
    assert 50 <= trees["comb_shallow"][2]["max_depth"] <= 56


def test_what_the_other_fixtures_are_said_to_be(meshes, trees):
    v, t = meshes["one_cell"]
    c = lm.centroids(v, t)
    assert (c.view(np.uint32) == c[0].view(np.uint32)).all() and set(lm.morton(v, t).tolist()) == {0}
    assert len(np.unique(np.concatenate([v[t].min(axis=1), v[t].max(axis=1)], 1), axis=0)) == len(t)   # ... and boxes that differ
    assert 1 < trees["one_cell"][2]["n_leaves"] < len(t)                  # the cut decided: neither every triangle alone nor everything in leaves of 32
    v, t = meshes["collinear_degenerate"]
    arr = trees["collinear_degenerate"][0]
    d = arr[:, 5:8] - arr[:, 2:5]
    assert (d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0] == 0).all()
    c = lm.centroids(*meshes["planar"])
    assert np.ptp(c[:, 1]) == 0 and np.ptp(c[:, 0]) > 0 and np.ptp(c[:, 2]) > 0
    v, t = meshes["coincident_cluster"]
    code = lm.morton(v, t)
    assert (code == code[17]).sum() >= 41                                 # more equal codes than a leaf may hold
    assert len(meshes["grid_ct1"][1]) == 18432 >= lm.CT_LARGE_FROM
    a16 = lm.build(*meshes["grid_ct1"], ct=1.6)[0]
    assert len(a16) != len(trees["grid_ct1"][0])                          # the 1.0 of large meshes decides differently than 1.6 would


@pytest.mark.parametrize("kind,seed", [("axis_aligned_quads", 2), ("soup", 3), ("deep_strip", 4), ("geometric_chain", 5), ("flat_faces", 6)])
def test_the_older_synthetic_meshes_stay_below_the_install_limit(kind, seed):
    assert lm.build(*_synthetic_mesh("three_triangles", np.random.default_rng(1))) is None   # (the reference builder's single leaf)
    v, t = _synthetic_mesh(kind, np.random.default_rng(seed))
    arr, order, st = lm.build(v, t)
    lm.check_tree(arr, order, len(t))
    assert st["max_depth"] < 56
    print(kind, st)


def test_five_triangles_are_the_first_size_the_builder_takes():
    v, t = fx.sizes(5)
    assert lm.build(v, t[:4]) is None and lm.build(v, t) is not None


@pytest.mark.parametrize("name,cap", [("cat", 0.001), ("coincident_cluster", 0.05)])
def test_oracle_on_the_models_tree_renders_the_reference_trees_frame(oracle, meshes, trees, name, cap):
    """the same triangles in another tree: the frames agree except where the nearest hit is a bit-equal tie between two triangles (the scan order decides)"""
    v, t = meshes[name]
    arr, order, _ = trees[name]
    W, H = 160, 100
    ref, _, _ = oracle.Scene.preset("cpu", oracle.Mesh.from_arrays(v, t).build_bvh()).render(W, H, 1, 0, want_rgb8=False)
    got, _, _ = oracle.Scene.preset("cpu", oracle.Mesh.from_arrays(v, t).set_bvh(arr, order)).render(W, H, 1, 0, want_rgb8=False)
    empty, _, _ = oracle.Scene.preset("cpu").render(W, H, 1, 0, want_rgb8=False)
    assert (~values_equal(ref[..., :3], empty[..., :3])).any(-1).mean() > 0.02     # the mesh is in the picture
    np.testing.assert_array_equal(got[..., 3], ref[..., 3])
    diff = (~values_equal(got[..., :3], ref[..., :3])).any(-1)
    assert diff.mean() <= cap, int(diff.sum())
