"""The numpy model of rt_mesh_compute_normals and of the previous shading normal (tests/normals_model.py), checked alone: no GPU, no library call.

The model is the yardstick of tests/test_gpu_normals.py (the reference has no normal computation), so it is held to what it approximates -- the same sums in
binary64 -- within a bound derived below, to geometry (a closed surface's normals point outwards), and to the fixtures' preconditions the GPU tests lean on."""
import numpy as np
import pytest

import raytracinggpu_amd as rt

from . import motion_model as mm
from . import normals_model as nm
from . import temporal_model as tm

U = 2.0 ** -24                                                          # the unit roundoff of binary32
SLOT = 6
THETA_DEG, SEQ_W, SEQ_H = 35.0, 96, 64                                  # the rotating sequence: cos 35 deg = 0.819 < min_normal_dot = 0.9


def _cat(cat_golden):
    return np.asarray(cat_golden["vertices"], np.float32), np.ascontiguousarray(np.asarray(cat_golden["tri_bvh_order"])[:, :3], np.int32)


TETRA_V = np.float32([[0, 0, 0], [4, 0, 0], [0, 3, 0], [0, 0, 5]])
TETRA_T = np.int32([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])        # every face counter-clockwise seen from outside


def test_the_cat_meets_the_preconditions_of_the_fixture(cat_golden):
    v, t = _cat(cat_golden)
    assert len(v) == 2247
    S, val = nm.vertex_sums(v, t)
    assert val.max() <= 12 and val.min() >= 1                           # valence at most 12, no unreferenced vertex
    N = nm.xm.triangle_records(v, t)[3]
    assert (nm.xm._dot(N, N) > 0).all()                                 # no degenerate triangle
    assert (nm.xm._dot(S, S) > 0).all()                                 # no zero sum
    assert (t[:, 0] != t[:, 1]).all() and (t[:, 1] != t[:, 2]).all() and (t[:, 0] != t[:, 2]).all()
    n = nm.vertex_normals(v, t)
    assert n.dtype == np.float32 and np.isfinite(n).all()
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() < 4 * U


def test_every_cat_normal_lies_within_the_derived_bound_of_the_binary64_sums(cat_golden):
    """The bound, per component of n(v), with k = the valence, e1 = B - A, e2 = C - A of an incident face and M = sum over the faces of |e1| |e2| (binary64):
      * a face normal's component is a difference of two products of differences: each factor carries one rounding (relative u), each product one, the difference
        one -- at most gamma_4 (|e1y e2z| + |e1z e2y|) <= gamma_4 |e1| |e2| (Cauchy-Schwarz), gamma_n = n u / (1 - n u);
      * the k - 1 additions each round a partial sum that is at most M in magnitude: together with the above gamma_(k+3) M per component, sqrt(3) times that as a vector;
      * normalising a vector perturbed by d turns it by at most 2 |d| / |S|;
      * the normalisation's own roundings: the sum of three squares carries gamma_3, its root half of that and one rounding, the quotient one more: below 4 u
        per component of a unit vector.
    So |n32 - n64| <= 2 sqrt(3) gamma_(k+3) M / |S| + 4 u.  Nothing in it is fitted to what the model gives."""
    v, t = _cat(cat_golden)
    n32 = nm.vertex_normals(v, t).astype(np.float64)
    S64, n64, val = nm.vertex_normals_f64(v, t)
    v64 = v.astype(np.float64)
    e1, e2 = v64[t[:, 1]] - v64[t[:, 0]], v64[t[:, 2]] - v64[t[:, 0]]
    m = np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)
    M = np.zeros(len(v))
    for k in range(3):
        np.add.at(M, t[:, k], m)
    gamma = (val + 3) * U / (1 - (val + 3) * U)
    bound = 2 * np.sqrt(3) * gamma * M / np.linalg.norm(S64, axis=1) + 4 * U
    err = np.abs(n32 - n64).max(axis=1)
    print("largest error / bound over the cat's vertices: %.3g, largest error %.3g, largest bound %.3g" % ((err / bound).max(), err.max(), bound.max()))
    assert (err <= bound).all()
    assert bound.max() < 1e-3                                           # ... and the bound says something: no vertex of the cat is near a cancellation


def test_a_closed_tetrahedron_has_outward_normals():
    n = nm.vertex_normals(TETRA_V, TETRA_T)
    out = TETRA_V.astype(np.float64) - TETRA_V.astype(np.float64).mean(0)
    assert ((n.astype(np.float64) * out).sum(1) > 0).all()
    # and a vertex's normal is the area-weighted mean: vertex 0 sees the three faces in the coordinate planes, areas 6, 10, 7.5 -> (-7.5, -10, -6) normalised
    np.testing.assert_allclose(n[0], np.float64([-7.5, -10, -6]) / np.linalg.norm([-7.5, -10, -6]), rtol=0, atol=4 * U)


def test_special_vertices():
    v = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [9, 9, 9], [0, -1, 0]])
    # vertex 3 is named by nobody; vertices 0 and 1 by two faces that cancel exactly; (0, 0, 1): vertex 0 twice, a degenerate face
    t = np.int32([[0, 1, 2], [0, 1, 4], [0, 0, 1]])
    n = nm.vertex_normals(v, t)
    np.testing.assert_array_equal(n[[0, 1, 3]], 0)
    np.testing.assert_array_equal(n[2], [0, 0, 1])
    np.testing.assert_array_equal(n[4], [0, 0, -1])
    # a face normal with a -0 component that is the FIRST of its vertex keeps the sign; added to a +0 it would not
    v2 = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    s, _ = nm.vertex_sums(v2, np.int32([[0, 2, 1]]))                    # N = (0, 0, -1): x = 1 * 0 - 0 * 0 ... the signs of the zeros are the products'
    n2 = nm.vertex_normals(v2, np.int32([[0, 2, 1]]))
    np.testing.assert_array_equal(np.signbit(n2[0]), np.signbit(s[0]))
    # a NaN vertex: zeros at every vertex whose sum it reaches, the model's value elsewhere
    v3 = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [1, 1, 0], [2, 1, 1]])
    n3 = nm.vertex_normals(v3, np.int32([[0, 1, 2], [1, 3, 4], [2, 1, 4], [4, 1, 5]]))
    np.testing.assert_array_equal(n3[[1, 3, 4]], 0)
    assert np.isfinite(n3).all() and (n3[[0, 2, 5]] != 0).any(1).all()


def test_the_summation_order_shows_in_the_bits_of_the_fan():
    v, t = nm.fan()
    assert len(t) == 5000
    N = nm.xm.triangle_records(v, t)[3].astype(np.float64)
    area = np.linalg.norm(N, axis=1)
    assert area.max() / area.min() >= 0.99 * 2.0 ** 20 and np.isfinite(N).all()
    fwd = nm.vertex_normals(v, t)
    rev = nm.vertex_normals(v, t, order=np.arange(len(t))[::-1])
    assert (fwd[0].view(np.uint32) != rev[0].view(np.uint32)).any()    # the hub: a wrong order on the device cannot pass for the right one
    np.testing.assert_array_equal(fwd[1:].view(np.uint32), rev[1:].view(np.uint32))   # the rim's vertices have one face each
    np.testing.assert_allclose(fwd[0], rev[0], rtol=0, atol=1e-3)      # ... and both are the same normal to the precision the sum has


def sequence_planes(oracle, cat_golden, frames=6, theta_deg=THETA_DEG, w=SEQ_W, h=SEQ_H):
    """the rotating smooth cat, frame 0 (unturned) to frames - 1: per frame (vertices, vertex normals, the oracle's mesh, the trace, the current planes, and the
    previous-frame planes without / with the normal snapshot; None for frame 0)"""
    v0, t = _cat(cat_golden)
    arr = np.asarray(cat_golden["bvh_arr10"], np.float32).reshape(-1, 10)
    centre = v0.astype(np.float64).mean(0)
    out, last = [], None
    for f in range(frames):
        v = nm.rotate_about_axis(v0, f * np.deg2rad(theta_deg), centre)
        vn = nm.vertex_normals(v, t)
        om = oracle.Mesh.from_arrays(v, t, albedo=tuple(rt.scenes.CAT_ALBEDO)).set_bvh(arr, None).refit()
        om.set_normals(vn, t)
        tr = mm.trace(oracle.Scene.preset("cpu", om), w, h, meshes={SLOT: om})
        wo = wi = None
        if last is not None:
            snap = {SLOT: dict(mesh=om, previous=last[0], smooth=True)}
            wo = mm.previous_planes(tr, snap)
            wi = nm.previous_planes(tr, snap, normal_snapshots={SLOT: dict(mesh=om, normals=last[1], nidx=t)})
        out.append(dict(v=v, vn=vn, mesh=om, tr=tr, cur=mm.planes(tr), without=wo, with_=wi))
        last = (v, vn)
    return out


def kept(history, cat):
    return (history[1, ..., 2] > 1) & cat


def test_the_rotating_sequence_is_decided_by_the_normal_snapshot(oracle, cat_golden):
    """35 degrees a frame about the vertical axis through the cat's centroid, 96 x 64, min_normal_dot 0.9: from frame 2 on, strictly more cat pixels keep their
    history with the normal snapshot than without, and each side -- with, without, and with-but-not-without -- has at least 200 pixels (the colours play no part
    in the history lengths: zeros here)."""
    seq = sequence_planes(oracle, cat_golden)
    C = np.zeros((SEQ_H, SEQ_W, 4), np.float32)
    h_with = h_without = tm.accumulate(C, seq[0]["cur"][:2])
    for f in range(1, len(seq)):
        s, cat = seq[f], seq[f]["tr"]["id"] == SLOT
        on = cat
        np.testing.assert_array_equal(s["with_"][1].view(np.uint32), s["without"][1].view(np.uint32))          # P' does not depend on the normals
        turned = (s["with_"][0][on][:, :3] != s["without"][0][on][:, :3]).any(-1)
        assert turned.mean() > 0.9                                      # N' differs from N all over the cat
        h_with = tm.accumulate(C, s["with_"], seq[f - 1]["cur"][:2], h_with)
        h_without = tm.accumulate(C, s["without"], seq[f - 1]["cur"][:2], h_without)
        kw, kwo = kept(h_with, cat), kept(h_without, cat)
        print(f"frame {f}: cat pixels {int(cat.sum())}, history kept with the normal snapshot {int(kw.sum())}, without {int(kwo.sum())}, with only {int((kw & ~kwo).sum())}")
        if f >= 2:
            assert kw.sum() > kwo.sum()
            assert kw.sum() >= 200 and kwo.sum() >= 200 and (kw & ~kwo).sum() >= 200


def test_the_previous_normal_is_the_previous_frames_normal_at_the_same_barycentric_point(oracle, cat_golden):
    """N' of frame f == the smooth normal of frame f - 1's mesh evaluated at the same triangle and barycentrics; for a rigid turn that is the current normal turned
    back, to rounding"""
    seq = sequence_planes(oracle, cat_golden, frames=2)
    s = seq[1]
    on = s["tr"]["id"] == SLOT
    Np = s["with_"][0][on][:, :3].astype(np.float64)
    a = -np.deg2rad(THETA_DEG)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    back = s["cur"][0][on][:, :3].astype(np.float64) @ R.T
    assert on.sum() >= 200 and np.abs(Np - back).max() < 1e-4
