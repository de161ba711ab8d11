"""Every form of the traversal BOX step on trees unlike the cat's: big leaves, caller-supplied trees that do not hold their triangles or do not nest, inverted boxes, empty
leaves, planar / tiny / huge / far meshes, and forests built at the same edges.  -m gpu.

The form a tree may take is decided on the host (rt_host_scene.hip.h requantize and the layout pass before it):
  * 4-wide fixed-point quads (travq_mode 2): the boxes nest, no leaf is empty, the largest leaf has at most 127 triangles (leaf shift S = 24), every box is ordered and
    within 1e8 of the origin (fast_box);
  * fixed-point pairs (travq_mode 1): the same, except that empty leaves are allowed and leaves may hold up to 2 047 triangles when the mesh has at most 2^20 (S = 20);
  * float pairs (travq_mode 0): every other tree.
Each shape is checked three ways: per-ray results of rt_trace_rays through each production variant and each form asked for, bit for bit against the oracle's
TriangleMesh::intersect walking the SAME tree (Mesh.set_bvh takes the boxes as given, as the reference would); the form that actually ran (so that a silent fall-back is
visible); and, for the shapes that fit in the cpu room, whole frames against the oracle's."""
import os
import zlib

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import hostlib
from .test_gpu_kat import _grazing_rays
from .test_gpu_parity import VARIANTS, linf, values_equal, TOL

pytestmark = pytest.mark.gpu

FORMS = (("qw", {"RT_TRAVQ_QW": "1"}), ("q16", {"RT_TRAVQ_QW": "0", "RT_TRAVQ_Q16": "1"}), ("float", {"RT_TRAVQ_QW": "0", "RT_TRAVQ_Q16": "0"}))
TRACE_VARIANTS = ("wavefront_queue", "path", "wavefront")
# expected travq_mode per form asked for (None = "anything but 2"), by tree class -- requantize's condition, rt_host_scene.hip.h
MODES = {"ok": {"qw": 2, "q16": 1, "float": 0},
         "s20": {"qw": None, "q16": 1, "float": 0},
         "no_shift": {"qw": 0, "q16": 0, "float": 0},
         "no_nest": {"qw": 0, "q16": 0, "float": 0},
         "empty_leaf": {"qw": None, "q16": 1, "float": 0},
         "no_fast_box": {"qw": 0, "q16": 0, "float": 0}}


@pytest.fixture(scope="module")
def forms():
    """One context per form asked for (a context reads its knobs when it is created), and one with the default knobs."""
    out = {}
    for name, env in FORMS:
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            out[name] = rt.Context(0)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    out["default"] = rt.Context(0)
    yield out
    for c in out.values():
        c.close()


# ------------------------------------------------------------------------------------------------------------------------------------------------------------ meshes

def _soup(rng, n, lo, hi, size):
    """n random triangles with corners within `size` of a centre in [lo, hi]^3 (every triangle has its own three vertices)."""
    c = rng.uniform(lo, hi, (n, 1, 3))
    v = (c + rng.uniform(-size, size, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def _cluster(rng, K, c):
    """K triangles (c + p, c + q, c - p - q) with integer c and p, q in eighths: every centroid is exactly c (the float sums are exact), so the reference's midpoint split can
    never separate them and buildBVH makes one leaf of all K.  p, q come from a dozen vectors: vertices repeat, faces repeat (duplicated faces of an OBJ)."""
    S = rng.integers(-6, 7, (12, 3))
    S[np.abs(S).sum(1) == 0] = 1
    S = S * 0.125                                                       # eighths: still exact in binary32, and the cluster spans a few units only
    i = rng.integers(0, 12, K)
    j = (i + rng.integers(1, 12, K)) % 12
    p, q = S[i], S[j]
    c = np.asarray(c, np.float64)
    corners = np.stack([c + p, c + q, c - p - q], 1).reshape(-1, 3).astype(np.float32)
    v, inv = np.unique(corners, axis=0, return_inverse=True)           # shared vertices (the LDS-staged variants hold every vertex)
    return v.astype(np.float32), inv.reshape(K, 3).astype(np.int32)


def _join(*parts):
    vs, ts, off = [], [], 0
    for v, t in parts:
        vs.append(v); ts.append(t + off); off += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(ts).astype(np.int32)


def _leaf_sizes(arr):
    leaves = arr[arr[:, 0] < 0]
    return (leaves[:, 9] - leaves[:, 8]).astype(np.int64)


def _built(v, t):
    m = hostlib.build_mesh(v, t, albedo=rt.scenes.CAT_ALBEDO, object_slot=6)
    m["bvh_arr10"] = np.asarray(m["bvh_arr10"], np.float32).reshape(-1, 10)
    return m


def _big_leaf_mesh(K, seed):
    """A cluster of K coincident-centroid triangles in a soup of 400 ordinary ones, in front of the cpu room's camera; the seed is advanced until the cluster is a leaf of
    its own (an ordinary triangle can end up in the cluster's leaf when a split would leave it alone: cpu:214)."""
    for s in range(seed, seed + 50):
        rng = np.random.default_rng(s)
        v, t = _join(_soup(rng, 400, -14, 14, 1.5), _cluster(rng, K, rng.integers(-5, 6, 3)))
        m = _built(v, t)
        if K in _leaf_sizes(m["bvh_arr10"]):
            return v, t, m
    raise AssertionError(f"no seed gives a leaf of exactly {K} triangles")


def _cat(cat_golden):
    return np.array(cat_golden["vertices"], np.float32), np.array(cat_golden["tri_obj_order"], np.int32)


def _planar(rng, n=600, z=0.0, scale=12.0):
    """n triangles in the plane z = `z`: the root box has extent 0 on z (fixed-point cell size at its floor)."""
    v, t = _soup(rng, n, -scale, scale, scale / 8)
    v[:, 2] = np.float32(z)
    return v, t


def _far_cat(cat_golden, offset):
    """The cat moved by `offset` along x and scaled so that it spans about 2 000 float steps at that offset (near 1e8 the spacing is 8: a unit-size mesh would
    collapse into degenerate triangles)."""
    v, t = _cat(cat_golden)
    ext = float((v.max(0) - v.min(0)).max())
    ulp = float(np.spacing(np.float32(offset)))
    s = max(1.0, 2000.0 * ulp / ext)
    w = (v.astype(np.float64) * s).astype(np.float32)
    w[:, 0] = (w[:, 0].astype(np.float64) + offset).astype(np.float32)
    return w, t


# ------------------------------------------------------------------------------------------------------------------------------------------------------------ caller trees

def _stale(v, m):
    """vertices rotated by 0.05 rad about y and moved a little; the tree keeps the boxes of before the move"""
    a = 0.05
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    w = (v.astype(np.float64) @ R.T + np.array([0.3, 0.0, -0.2])).astype(np.float32)
    return w, dict(m, vertices=w)


def _shrunk_parent(m, rng):
    """one internal node two levels above leaves has its box shrunk to the middle half of itself on every axis: its children stick out of it.  Returns the tree and the
    parts of those children that lie outside the shrunk box (targets for the rays)."""
    arr = m["bvh_arr10"].copy()
    internal = np.flatnonzero(arr[:, 0] >= 0)
    # an internal node whose children are internal too, deep enough that its box is not the root's
    cand = [i for i in internal if i != 0 and arr[int(arr[i, 0]), 0] >= 0 and arr[int(arr[i, 1]), 0] >= 0]
    i = cand[len(cand) // 2]
    lo, hi = arr[i, 2:5].copy(), arr[i, 5:8].copy()
    mid, half = (lo + hi) / 2, (hi - lo) / 4
    arr[i, 2:5] = (mid - half).astype(np.float32); arr[i, 5:8] = (mid + half).astype(np.float32)
    sub, st = [], [i]
    while st:                                                           # the leaves below node i
        k = st.pop()
        if arr[k, 0] >= 0:
            st += [int(arr[k, 0]), int(arr[k, 1])]
        else:
            sub.append(k)
    return dict(m, bvh_arr10=arr), i, sub


def _inverted(m):
    """one internal node's box and one leaf's box inverted on x (lo > hi); the leaf's box is also halved, so that it no longer holds all of its triangles"""
    arr = m["bvh_arr10"].copy()
    internal = np.flatnonzero(arr[:, 0] >= 0)
    leaves = np.flatnonzero(arr[:, 0] < 0)
    i = int(internal[len(internal) // 3])
    arr[i, 2], arr[i, 5] = arr[i, 5], arr[i, 2]
    big = leaves[np.argmax((arr[leaves, 5:8] - arr[leaves, 2:5]).max(1))]
    lo, hi = arr[big, 2], arr[big, 5]
    arr[big, 2], arr[big, 5] = np.float32((lo + hi) / 2), lo
    return dict(m, bvh_arr10=arr), [i, int(big)]


def _empty_leaves(m, n_split=8):
    """n_split leaves of one triangle each become a parent (same box) over that one-triangle leaf and an EMPTY leaf (ts == te, the same box): still a tree"""
    arr = [a for a in m["bvh_arr10"].copy()]
    sizes = _leaf_sizes(m["bvh_arr10"])
    leaves = np.flatnonzero(m["bvh_arr10"][:, 0] < 0)
    pick = leaves[sizes == 1][:n_split]
    if len(pick) < n_split:
        pick = leaves[:n_split]
    for i in pick:
        a = arr[i].copy()
        ts = a[8]
        full = a.copy(); full[0] = full[1] = -1
        empty = a.copy(); empty[0] = empty[1] = -1; empty[8] = empty[9] = ts
        full[9] = a[9]
        n = len(arr)
        arr[i] = a.copy(); arr[i][0] = n; arr[i][1] = n + 1
        arr.append(full); arr.append(empty)
    return dict(m, bvh_arr10=np.array(arr, np.float32))


# ------------------------------------------------------------------------------------------------------------------------------------------------------------ rays

def _rays(arr, rng, n=4000, spread=None, origin_rays=0):
    """half _grazing_rays of test_gpu_kat (aimed at the tree's own leaf faces, edges and corners), half degenerate ones in the style of its _degenerate_rays: zero,
    -0.0, denormal, huge and tiny components, axis-parallel rays, origins on the root box's faces (with u = 0 on that axis)."""
    lo, hi = arr[0, 2:5].astype(np.float64), arr[0, 5:8].astype(np.float64)
    lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
    ext = float((hi - lo).max()) or 1.0
    spread = spread or max(ext, 1e-3)
    g = _grazing_rays(arr, rng, n // 2) if spread == 25.0 else _grazing_scaled(arr, rng, n // 2, spread)
    m = n - n // 2
    c = (lo + hi) / 2
    O = (c + rng.uniform(-1, 1, (m, 3)) * (hi - lo + spread) / 2).astype(np.float32)
    u = rng.normal(size=(m, 3)).astype(np.float32)
    k = rng.integers(0, 3, m)
    r = np.arange(m)
    q = m // 10
    u[r[:3 * q], k[:3 * q]] = np.where(rng.random(3 * q) < 0.5, np.float32(-0.0), np.float32(0.0))   # one zero component (either sign)
    u[r[3 * q:4 * q], k[3 * q:4 * q]] = np.float32(1e-42) * rng.choice([-1, 1], q)
    s = slice(4 * q, 5 * q)
    u[s] = 0.0; u[r[s], k[s]] = rng.choice([-1.0, 1.0], q)             # axis-parallel
    u[5 * q:5 * q + q // 2] *= np.float32(1e20)
    u[5 * q + q // 2:6 * q] *= np.float32(1e-20)
    for j, face in enumerate((lo, hi)):                                 # origins on the root box's faces, travelling along the face or through it
        s = slice(6 * q + 2 * j * q, 6 * q + (2 * j + 1) * q)
        O[r[s], k[s]] = np.float32(face[k[s]])
        s2 = slice(6 * q + (2 * j + 1) * q, 6 * q + (2 * j + 2) * q)
        O[r[s2], k[s2]] = np.float32(face[k[s2]]); u[r[s2], k[s2]] = np.where(rng.random(q) < 0.5, np.float32(-0.0), np.float32(0.0))
    rays = np.concatenate([g, np.concatenate([O, u], 1)]).astype(np.float32)
    if origin_rays:                                                     # rays from the world origin towards the mesh
        tg = (c + rng.uniform(-0.6, 0.6, (origin_rays, 3)) * (hi - lo)).astype(np.float32)
        rays[:origin_rays, :3] = 0.0
        rays[:origin_rays, 3:] = tg
    return rays


def _grazing_scaled(arr, rng, n, spread):
    """_grazing_rays with the origins `spread` (instead of 25 units) around the targets: for meshes far smaller or larger than the cat"""
    leaves = arr[arr[:, 0] < 0]
    pick = leaves[rng.integers(0, len(leaves), n)]
    lo, hi = pick[:, 2:5], pick[:, 5:8]
    w = rng.integers(0, 3, (n, 3))
    tt = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    target = np.where(w == 0, lo, np.where(w == 1, hi, lo + tt * (hi - lo))).astype(np.float32)
    O = (target + rng.normal(size=(n, 3)) * spread).astype(np.float32)
    u = (target - O).astype(np.float32)
    nrm = np.linalg.norm(u.astype(np.float64), axis=1, keepdims=True)
    u[: n // 2] = (u[: n // 2] / nrm[: n // 2]).astype(np.float32)
    k = rng.integers(0, 3, n // 8)
    idx = rng.integers(0, n, n // 8)
    u[idx, k] = 0.0
    return np.concatenate([O, u], axis=1).astype(np.float32)


def _oracle_rows(om, rays, tmin=1e-4):
    exp = np.zeros((len(rays), 5), np.float32)
    for i in range(len(rays)):
        h, tt, N = om.intersect(rays[i, :3], rays[i, 3:], tmin)
        exp[i, 0] = 1.0 if h else 0.0
        exp[i, 1] = tt; exp[i, 2:5] = N
    return exp


def _oracle_mesh(oracle, m):
    """the oracle walking the tree as given: triangles in the tree's order, Mesh.set_bvh"""
    tris = np.asarray(m["indices"])[:, :3]
    return oracle.Mesh.from_arrays(m["vertices"], tris, albedo=m.get("albedo", (0.25, 0.25, 0.25))).set_bvh(m["bvh_arr10"])


def _check_rays_and_forms(forms, m, om, rays, cls, min_hits=50):
    """per-ray results through every form and variant, and the form that ran; returns the measured travq_mode per form"""
    exp = _oracle_rows(om, rays)
    hit = exp[:, 0] != 0
    assert hit.sum() >= min_hits and (~hit).sum() >= 50, int(hit.sum())
    modes = {}
    for name, _ in FORMS:
        c = forms[name]
        c.scene_upload(rt.scenes.spheres("cpu"), dict(m, object_slot=6))
        for variant in TRACE_VARIANTS:
            got = c.trace_rays(rays, 1e-4, variant)
            bad = np.flatnonzero((got[:, 0] != exp[:, 0]) | (hit & (got[:, 1:5].view(np.uint32) != exp[:, 1:5].view(np.uint32)).any(1)))
            assert len(bad) == 0, (name, variant, len(bad), rays[bad[:3]].tolist(), got[bad[:3]].tolist(), exp[bad[:3]].tolist())
        modes[name] = c.stats_after_render(rt.make_params(64, 64, 1, 0, **rt.scenes.CPU_LAUNCHER))["travq_mode"]
        want = MODES[cls][name]
        assert (modes[name] != 2) if want is None else (modes[name] == want), (cls, name, modes[name])
    print(f"travq_mode by form asked for ({cls}): {modes}")
    return modes


def _check_frames(forms, oracle, m, om):
    """whole frames in the cpu room: b = 0 through every variant bit for bit with the oracle, work counters of the counting (float-pair) instantiation equal to the
    oracle's, and one b = 2 frame (sigma = 0: every channel bit-identical, L-inf within the tolerance)"""
    c = forms["default"]
    c.scene_upload(rt.scenes.spheres("cpu"), dict(m, object_slot=6))
    osc = oracle.Scene.preset("cpu", om)
    W, H = 320, 200
    exp0, _, cnt0 = osc.render(W, H, 1, 0, want_rgb8=False)
    for variant in tuple(VARIANTS) + ("lds_top", "lds_verts", "lds_all"):
        p = rt.make_params(W, H, 1, 0, variant=variant, **rt.scenes.CPU_LAUNCHER)
        got = c.render(p)
        assert values_equal(got[..., :3], exp0[..., :3]).all(), variant
        np.testing.assert_array_equal(got[..., 3], exp0[..., 3])
    for variant in ("wavefront_queue", "wavefront", "lockstep"):
        got_work = c.count_work(rt.make_params(W, H, 1, 0, variant=variant, **rt.scenes.CPU_LAUNCHER))
        assert got_work == {k: cnt0[k] for k in ("rays", "box_tests", "nodes", "tri_tests")}, variant
    exp2, _, _ = osc.render(W, H, 2, 2, want_rgb8=False)
    got2 = c.render(rt.make_params(W, H, 2, 2, **rt.scenes.CPU_LAUNCHER))
    assert linf(oracle, got2, exp2) <= TOL
    assert values_equal(got2[..., :3], exp2[..., :3]).all()
    np.testing.assert_array_equal(got2[..., 3], exp2[..., 3])


# ------------------------------------------------------------------------------------------------------------------------------------------------------------ B: single trees

@pytest.mark.parametrize("K", [127, 128, 129, 1000, 2047, 2048, 5000])
def test_big_leaves_from_the_reference_builder(forms, oracle, K):
    """Leaves of K triangles made by buildBVH itself (coincident centroids: the midpoint split fails, cpu:214).  K <= 127: S = 24, every form; 128 .. 2 047: S = 20
    (leaf word 1 << 31 | count << 20 | first), no quads; 2 048 and more: only the float pairs can hold the leaf."""
    v, t, m = _big_leaf_mesh(K, 1000 + K)
    arr = m["bvh_arr10"]
    sizes = _leaf_sizes(arr)
    assert sizes.max() == K, (sizes.max(), K)                           # the intended leaf occurs and is the largest: the case cannot vanish with a change of builder
    cls = "ok" if K <= 127 else ("s20" if K <= 2047 else "no_shift")
    om = _oracle_mesh(oracle, m)
    rng = np.random.default_rng(K)
    rays = _rays(arr, rng, spread=25.0)
    cl = arr[arr[:, 0] < 0][np.argmax(sizes)]                           # and rays through the big leaf's box itself
    tg = (cl[2:5] + rng.uniform(0, 1, (600, 3)) * (cl[5:8] - cl[2:5])).astype(np.float32)
    O = (tg + rng.normal(size=(600, 3)) * 25).astype(np.float32)
    rays[-600:] = np.concatenate([O, (tg - O).astype(np.float32)], 1)
    _check_rays_and_forms(forms, m, om, rays, cls)
    _check_frames(forms, oracle, m, om)


def test_more_than_2_20_triangles_with_a_leaf_of_128(forms, oracle):
    """2^20 + 1 triangles and one leaf of 128: neither leaf shift fits (S = 24 needs leaves <= 127, S = 20 needs <= 2^20 triangles): the float pairs, whatever is asked."""
    rng = np.random.default_rng(20)
    n = (1 << 20) + 1 - 128
    g = np.arange(n)
    c = np.stack([(g % 128) * 0.25 - 16, (g // 128 % 128) * 0.25 - 16, (g // 16384) * 0.25 - 8], 1) + rng.uniform(-0.05, 0.05, (n, 3))
    v = (c[:, None, :] + rng.uniform(-0.1, 0.1, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
    v, t = _join((v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)), _cluster(rng, 128, (0, 0, 40)))
    assert len(t) == (1 << 20) + 1
    m = _built(v, t)
    sizes = _leaf_sizes(m["bvh_arr10"])
    assert sizes.max() == 128, sizes.max()
    om = _oracle_mesh(oracle, m)
    _check_rays_and_forms(forms, m, om, _rays(m["bvh_arr10"], rng, spread=25.0), "no_shift")


def _cat_mesh(cat_golden):
    return dict(vertices=np.array(cat_golden["vertices"], np.float32), indices=np.asarray(cat_golden["tri_bvh_order"]),
                bvh_arr10=np.asarray(cat_golden["bvh_arr10"], np.float32).reshape(-1, 10), albedo=rt.scenes.CAT_ALBEDO, object_slot=6)


@pytest.mark.parametrize("shape", ["stale", "shrunk_parent", "inverted", "empty_leaves"])
def test_caller_trees(forms, oracle, cat_golden, shape):
    """Trees the caller supplies, used as given (as the reference uses them): a stale tree (vertices moved after the build), a parent box shrunk inside its children's
    union, inverted boxes, empty leaves.  The frame must still be the reference's -- triangles whose leaf the reference never reaches stay invisible, and a triangle
    accepted in a flagged leaf counts only if the reference's test of the leaf's REAL box says hit."""
    m = _cat_mesh(cat_golden)
    v = m["vertices"]
    rng = np.random.default_rng(zlib.crc32(shape.encode()))
    arr0 = m["bvh_arr10"]
    extra = None
    if shape == "stale":
        v, m = _stale(v, m)
        cls = "ok"
    elif shape == "shrunk_parent":
        m, i, sub = _shrunk_parent(m, rng)
        arr = m["bvh_arr10"]
        lo, hi = arr[i, 2:5], arr[i, 5:8]
        pick = np.array(sub)[rng.integers(0, len(sub), 1500)]          # points in the leaves below the shrunk node, outside its box
        tg = arr[pick, 2:5] + rng.uniform(0, 1, (1500, 3)) * (arr[pick, 5:8] - arr[pick, 2:5])
        out = ((tg < lo) | (tg > hi)).any(1)
        tg = tg[out].astype(np.float32)
        O = (tg + rng.normal(size=tg.shape) * 25).astype(np.float32)
        extra = np.concatenate([O, (tg - O).astype(np.float32)], 1)
        assert len(extra) > 300
        cls = "no_nest"
    elif shape == "inverted":
        m, nodes = _inverted(m)
        arr = m["bvh_arr10"]
        tg = np.concatenate([arr0[k, 2:5] + rng.uniform(0, 1, (700, 3)) * (arr0[k, 5:8] - arr0[k, 2:5]) for k in nodes]).astype(np.float32)
        O = (tg + rng.normal(size=tg.shape) * 25).astype(np.float32)
        extra = np.concatenate([O, (tg - O).astype(np.float32)], 1)
        cls = "no_fast_box"
    else:
        m = _empty_leaves(m)
        assert (_leaf_sizes(m["bvh_arr10"]) == 0).sum() == 8
        cls = "empty_leaf"
    om = _oracle_mesh(oracle, m)
    rays = _rays(m["bvh_arr10"] if shape != "inverted" else arr0, rng, spread=25.0)
    if extra is not None:
        rays[-len(extra):] = extra[: len(rays)]
    _check_rays_and_forms(forms, m, om, rays, cls)
    _check_frames(forms, oracle, m, om)


@pytest.mark.parametrize("shape", ["planar", "tiny", "huge", "far_1e4", "far_1e6", "far_9.9e7", "far_1.5e8"])
def test_planar_and_extreme_scales(forms, oracle, cat_golden, shape):
    """The fixed-point grid (65 000 cells per axis over the root box, cell size at least 1e-30: q16_grid) and the error-bounded box filters at the edges of their
    argument: a root box of extent 0 on one axis, a mesh of extent 1e-3, one of extent 1e6, and the cat far from the origin (1e4, 1e6, 9.9e7: still within fast_box's
    1e8; 1.5e8: beyond it, where the float pairs must take over).  Rays are built around each mesh, and for the far ones also from the world origin."""
    rng = np.random.default_rng(zlib.crc32(shape.encode()))
    origin_rays = 0
    cls = "ok"
    if shape == "planar":
        v, t = _planar(rng, z=-3.0)
    elif shape == "tiny":
        v, t = _soup(rng, 500, -5e-4, 5e-4, 5e-5)
        v = (v + np.float32(0.125)).astype(np.float32)
    elif shape == "huge":
        v, t = _soup(rng, 500, -5e5, 5e5, 5e4)
    else:
        off = float(shape.split("_")[1])
        v, t = _far_cat(cat_golden, off)
        origin_rays = 500
        cls = "ok" if off < 1e8 else "no_fast_box"
    m = _built(v, t)
    arr = m["bvh_arr10"]
    if shape == "planar":
        assert arr[0, 4] == arr[0, 7]                                  # root extent 0 on z
    om = _oracle_mesh(oracle, m)
    ext = float((arr[0, 5:8] - arr[0, 2:5]).max())
    rays = _rays(arr, rng, spread=max(ext, 1e-3), origin_rays=origin_rays)
    # a planar mesh is invisible to the reference: its root box has no thickness, and BoundingBox::intersect never hits such a box (strict '>', cpu:156) unless the ray
    # lies in the plane -- and then it is parallel to every triangle (cpu:230).  Every ray must miss it on the device too.
    _check_rays_and_forms(forms, m, om, rays, cls, min_hits=0 if shape == "planar" else 50)
    if shape == "planar":                                              # where the cat sits: whole frames too
        _check_frames(forms, oracle, m, om)


# ------------------------------------------------------------------------------------------------------------------------------------------------------------ C: forests

def _forest_rays(rng, members, planes, n=4000):
    """camera-like rays at the members' triangles, degenerate ones, and origins exactly on the shared planes and on the union box's faces with u = +-0 on that axis"""
    allv = np.concatenate([m["vertices"] for m in members])
    lo, hi = allv.min(0), allv.max(0)
    ext = float((hi - lo).max())
    O = (lo + rng.uniform(-0.5, 1.5, (n, 3)) * (hi - lo)).astype(np.float32)
    tg = allv[rng.integers(0, len(allv), n)] + rng.normal(scale=0.02 * ext, size=(n, 3))
    u = (tg - O).astype(np.float32)
    u[: n // 2] = (u[: n // 2] / np.linalg.norm(u[: n // 2], axis=1, keepdims=True)).astype(np.float32)
    k = rng.integers(0, 3, n)
    r = np.arange(n)
    u[r[2000:2200], k[2000:2200]] = np.float32(1e-42)
    u[2200:2300] *= np.float32(1e20)
    faces = [(a, float(lo[a])) for a in range(3)] + [(a, float(hi[a])) for a in range(3)] + list(planes)
    s = 2300
    per = (n - s) // len(faces)
    for a, val in faces:
        sl = slice(s, s + per)
        O[sl, a] = np.float32(val)
        u[sl, a] = np.where(rng.random(per) < 0.5, np.float32(-0.0), np.float32(0.0))
        s += per
    return np.concatenate([O, u], 1).astype(np.float32)


def _check_forest(forms, oracle, members, oms, planes, cls, seed):
    rng = np.random.default_rng(seed)
    osc = oracle.Scene()
    for om in oms:
        osc.add_mesh(om)
    rays = _forest_rays(rng, members, planes)
    exp = [osc.intersect_all(rays[i, :3], rays[i, 3:], 1e-4) for i in range(len(rays))]
    eh = np.array([e[0] for e in exp])
    eP = np.array([e[2] for e in exp], np.float32)
    eN = np.array([e[3] for e in exp], np.float32)
    assert eh.sum() >= 50 and (~eh).sum() >= 50, int(eh.sum())
    meshes = [dict(mm, object_slot=j) for j, mm in enumerate(members)]
    modes = {}
    for name, _ in FORMS:
        c = forms[name]
        c.scene_upload([], meshes)
        for variant in TRACE_VARIANTS:
            got = c.trace_rays(rays, 1e-4, variant)
            gP = (rays[:, :3] + (got[:, 1:2] * rays[:, 3:]).astype(np.float32)).astype(np.float32)   # P = O + t u, as intersect_all forms it
            bad = np.flatnonzero(((got[:, 0] != 0) != eh) | (eh & ((gP.view(np.uint32) != eP.view(np.uint32)).any(1) | (got[:, 2:5].view(np.uint32) != eN.view(np.uint32)).any(1))))
            assert len(bad) == 0, (name, variant, len(bad), rays[bad[:3]].tolist(), got[bad[:3]].tolist(), eh[bad[:3]].tolist())
        modes[name] = c.stats_after_render(rt.make_params(64, 64, 1, 0, **rt.scenes.CPU_LAUNCHER))["travq_mode"]
        want = MODES[cls][name]
        assert (modes[name] != 2) if want is None else (modes[name] == want), (cls, name, modes[name])
    print(f"forest travq_mode by form asked for ({cls}): {modes}")
    return rays, eh


def test_forest_small_root_inside_a_large_one(forms, oracle):
    rng = np.random.default_rng(31)
    a, b = _built(*_soup(rng, 500, -14, 14, 1.5)), _built(*_soup(rng, 200, -2, 2, 0.4))
    _check_forest(forms, oracle, [a, b], [_oracle_mesh(oracle, a), _oracle_mesh(oracle, b)], [], "ok", 31)


def test_forest_roots_sharing_a_face_plane(forms, oracle):
    """two meshes whose root boxes touch in the plane z = 0 exactly (each has vertices on it)"""
    rng = np.random.default_rng(32)
    va, ta = _soup(rng, 300, -10, 10, 1.5); va[:, 2] = -np.abs(va[:, 2]); va[0, 2] = 0.0
    vb, tb = _soup(rng, 300, -10, 10, 1.5); vb[:, 2] = np.abs(vb[:, 2]); vb[0, 2] = 0.0
    a, b = _built(va, ta), _built(vb, tb)
    assert a["bvh_arr10"][0, 7] == 0.0 and b["bvh_arr10"][0, 4] == 0.0
    _check_forest(forms, oracle, [a, b], [_oracle_mesh(oracle, a), _oracle_mesh(oracle, b)], [(2, 0.0)], "ok", 32)


def test_forest_planar_mesh_beside_an_ordinary_one(forms, oracle):
    """a planar mesh (z = -3) on the union box's minimum z face, an ordinary mesh above it -- and the same planar mesh's tree kept while its triangles are tilted through
    the plane (a stale caller tree: a FLAT root box whose triangles cross it).  Rays in that plane with u.z = -0.0 see NaN, NaN on z for the flat root (skipped by
    min_element / max_element) but NaN, -inf for a union box sharing the plane: the union node must be widened for the reference's hits there (tests/test_box_nesting.py)."""
    rng = np.random.default_rng(33)
    vp, tp = _planar(rng, n=300, z=-3.0)
    p = _built(vp, tp)
    vo, to = _soup(rng, 300, -10, 10, 1.5)
    vo[:, 2] = np.abs(vo[:, 2]) + np.float32(1.0)
    o = _built(vo, to)
    _check_forest(forms, oracle, [p, o], [_oracle_mesh(oracle, p), _oracle_mesh(oracle, o)], [(2, -3.0)], "ok", 33)
    tilt = np.array(p["vertices"], np.float32)
    tilt[:, 2] = (tilt[:, 2] + np.float32(0.05) * tilt[:, 0]).astype(np.float32)   # every triangle crosses z = -3 (or touches it); the boxes stay flat at z = -3
    ps = dict(p, vertices=tilt)
    rays, eh = _check_forest(forms, oracle, [ps, o], [_oracle_mesh(oracle, ps), _oracle_mesh(oracle, o)], [(2, -3.0)], "ok", 34)
    in_plane = (rays[:, 2] == np.float32(-3.0)) & (rays[:, 5] == 0) & np.signbit(rays[:, 5])
    assert (in_plane & eh).sum() >= 20                                 # the reference does hit tilted triangles along the flat root's plane with u.z = -0.0


@pytest.mark.parametrize("member", ["big_leaf", "shrunk_parent"])
def test_forest_with_a_member_at_an_edge(forms, oracle, cat_golden, member):
    """a forest whose second member has a leaf of 128 triangles (S = 20 for the whole forest) or a non-nesting caller tree (float pairs for the whole forest)"""
    rng = np.random.default_rng(35)
    a = _cat_mesh(cat_golden)
    if member == "big_leaf":
        _, _, b = _big_leaf_mesh(128, 7000)
        cls = "s20"
    else:
        b, _, _ = _shrunk_parent(_built(*_soup(rng, 600, -10, 10, 1.0)), rng)
        cls = "no_nest"
    arr = b["bvh_arr10"].copy()                                        # moved beside the cat, boxes with it (rounding is monotone: nesting is kept)
    arr[:, [2, 5]] = (arr[:, [2, 5]] + np.float32(20)).astype(np.float32)
    b = dict(b, vertices=(np.asarray(b["vertices"], np.float32) + np.float32([20, 0, 0])).astype(np.float32), bvh_arr10=arr)
    _check_forest(forms, oracle, [a, b], [_oracle_mesh(oracle, a), _oracle_mesh(oracle, b)], [], cls, 36)
