"""Reference model of rt_mesh_compute_normals[_of] and of the previous shading normal of rt_render_aov_motion (test infrastructure, like tests/motion_model.py).

numpy binary32 throughout, every operation one rounding in the order include/raytrace_hip.h states: the face normals are the N of tests/texture_model.py's triangle
records, a vertex's sum starts as the first incident face normal and takes the others one by one in the triangle order handed in, and the normalisation is the one
the other models use.  The reference has no such computation; this file is the yardstick.  Nothing here is code under test."""
import numpy as np

from . import motion_model as mm
from . import texture_model as xm

F = np.float32


def incidence(n_vertices, triangles, order=None):
    """per vertex the list of triangles (positions in `triangles`) of the corners that name it: ascending in `order` (a permutation of the triangles: the order the
    sums run in; None = as listed), corners 0, 1, 2 within a triangle, a triangle that names a vertex twice listed twice"""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    out = [[] for _ in range(int(n_vertices))]
    for ti in (range(len(t)) if order is None else np.asarray(order, np.int64)):
        for k in range(3):
            out[t[ti, k]].append(int(ti))
    return out


def vertex_sums(vertices, triangles, order=None, dtype=np.float32):
    """S(v) -> [nv, 3] and the valence of every vertex.  dtype=np.float64: the same sums of the same (binary32) vertices in binary64, for the error bound."""
    v = np.asarray(vertices, np.float32).astype(dtype)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    A, B, Cc = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    with np.errstate(all="ignore"):
        N = xm._cross(B - A, Cc - A)                                   # triangle_records' N, in dtype
    if dtype == np.float32:
        assert N.dtype == np.float32
        np.testing.assert_array_equal(N.view(np.uint32), xm.triangle_records(vertices, t)[3].view(np.uint32))
    inc = incidence(len(v), t, order)
    S = np.zeros((len(v), 3), dtype)
    with np.errstate(all="ignore"):
        for i, tl in enumerate(inc):
            if not tl:
                continue
            s = N[tl[0]].copy()                                        # the first face normal as it is (a -0 stays -0)
            for ti in tl[1:]:
                s = s + N[ti]                                          # one rounding per component and face
            S[i] = s
    return S, np.array([len(x) for x in inc])


def vertex_normals(vertices, triangles, order=None):
    """n(v) -> [nv, 3] float32: normalize(S), zeros where !(dot(S, S) > 0)"""
    S, _ = vertex_sums(vertices, triangles, order)
    with np.errstate(all="ignore"):
        d = xm._dot(S, S)
        n = mm._normalize(S)
    out = np.where((d > 0)[:, None], n, F(0)).astype(np.float32)
    assert S.dtype == np.float32 and d.dtype == np.float32
    return out


def vertex_normals_f64(vertices, triangles):
    """the same formula evaluated in binary64 (unnormalised sums and unit normals): what the binary32 result is an approximation of"""
    S, val = vertex_sums(vertices, triangles, dtype=np.float64)
    with np.errstate(all="ignore"):
        n = S / np.sqrt((S * S).sum(-1))[:, None]
    return S, n, val


def smooth_normal(alpha, beta, gamma, na, nb, nc):
    """get_smooth_normal's last line: normalize((alpha n_a + beta n_b) + gamma n_c)"""
    with np.errstate(all="ignore"):
        return mm._normalize(mm.barycentric_point(alpha, beta, gamma, na, nb, nc))


def previous_planes(tr, snapshots=None, motion=None, normal_snapshots=None, branch=None):
    """out_prev of rt_render_aov_motion with normal snapshots: motion_model.previous_planes, then on every hit of an object of normal_snapshots =
    {object id: dict(mesh=the oracle Mesh of the CURRENT shape, normals=[nn, 3] the normals the mesh shaded with at the snapshot, nidx=[nt, 3] their indices per
    triangle in the mesh's current triangle order)} N' = smooth_normal over the snapshot's corner normals with the CURRENT triangle's barycentrics."""
    out = mm.previous_planes(tr, snapshots, motion, branch=branch)
    for oid, s in (normal_snapshots or {}).items():
        on = tr["id"] == oid
        if not on.any():
            continue
        mesh = s["mesh"]
        tris = np.asarray(mesh.triangles, np.int64)
        tri = tr["tri"][on]
        assert (tri >= 0).all(), "trace() was not given this mesh"
        A, e1, e2, Nt = (x[tri] for x in xm.triangle_records(mesh.vertices, tris))
        alpha, beta, gamma = xm.barycentrics(A, e1, e2, Nt, tr["O"], tr["u"][on])
        nn, ni = np.asarray(s["normals"], np.float32), np.asarray(s["nidx"], np.int64)
        out[0, ..., :3][on] = smooth_normal(alpha, beta, gamma, nn[ni[tri, 0]], nn[ni[tri, 1]], nn[ni[tri, 2]])
    assert out.dtype == np.float32
    return out


def rotate_about_axis(v, theta, centre):
    """the vertices turned by theta about the vertical (y) axis through `centre` (binary64 inside, narrowed once)"""
    v = np.asarray(v, np.float32).astype(np.float64)
    c, s = np.cos(theta), np.sin(theta)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return ((v - centre) @ R.T + centre).astype(np.float32)


def fan(n_triangles=5000, spread=20):
    """a fan of n triangles around vertex 0 whose areas are spread over 2^spread, in no monotone order: the summation order shows in the bits of n(0)
    -> (vertices [2 n + 1, 3], triangles [n, 3])"""
    k = np.arange(n_triangles)
    size = np.exp2(((k * 7919) % n_triangles) * (spread / 2.0) / (n_triangles - 1))          # edge lengths over 2^(spread / 2): areas over 2^spread
    a = 2 * np.pi * k / n_triangles
    b = a + 2 * np.pi / n_triangles * 0.9
    rim1 = np.stack([size * np.cos(a), size * np.sin(a), 0.01 * size * np.cos(3 * a)], -1)
    rim2 = np.stack([size * np.cos(b), size * np.sin(b), 0.01 * size * np.sin(5 * a)], -1)
    v = np.concatenate([[[0.0, 0.0, 0.25]], rim1, rim2]).astype(np.float32)
    t = np.stack([np.zeros(n_triangles, np.int64), 1 + k, 1 + n_triangles + k], -1).astype(np.int32)
    return v, t
