"""Pins the CPU restatement (oracle/rt_oracle.c) to the reference.

Every expected value below was produced by the reference's own code
(/root/reference/cpu_launcher.cpp compiled by oracle/Makefile, dumped by
oracle/make_golden.py).  All comparisons are bit-exact unless stated.
"""
import hashlib

import numpy as np
import pytest

from .conftest import load_golden

SHA_CAT_1_0 = "d0424aef9bbf5dc3052b21a9bdcfcde559024086ef88cdcbe433bf70908a1b13"   # SURVEY 8c / BASELINE.md


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_bvh_build_matches_reference(oracle_cat, cat_golden):
    # buildBVH (cpu:190-224): same in-place partition => same triangle order, same nodes
    assert oracle_cat.num_nodes == len(cat_golden["bvh_arr10"]) == 2019
    assert oracle_cat.max_depth == 24
    np.testing.assert_array_equal(oracle_cat.triangles, cat_golden["tri_bvh_order"])
    np.testing.assert_array_equal(bits(oracle_cat.bvh_array()), bits(cat_golden["bvh_arr10"]))


def test_obj_reader_matches_reference(oracle, tmp_path):
    # an OBJ in the cat's exporter layout and counts (seeded numbers) and what the reference's readOBJ made of it (tests/golden/ref_obj.npz)
    g = load_golden("ref_obj.npz")
    p = tmp_path / "cat.obj"
    p.write_bytes(g["obj_text"].tobytes())
    m = oracle.Mesh.from_obj(str(p))        # readOBJ (cpu:315-493) incl. the in-parser 0.8 / (0,-10,0)
    np.testing.assert_array_equal(bits(m.vertices), bits(g["vertices"]))
    np.testing.assert_array_equal(m.triangles, g["tri_obj_order"])


def test_obj_reader_missing_file_gives_empty_mesh(oracle, capfd):
    m = oracle.Mesh.from_obj("/nonexistent/cat.obj")      # cpu:322-325
    assert m.status == -1 and len(m.vertices) == 0 and len(m.triangles) == 0
    assert "Error opening file!" in capfd.readouterr().out


def test_obj_reader_face_forms(oracle, tmp_path):
    # v/vt/vn, v/vt, v, v//vn, negative indices and polygon fan triangulation (cpu:369-488)
    p = tmp_path / "t.obj"
    p.write_text("v 0 0 0\r\nv 1 0 0\r\nv 1 1 0\r\nv 0 1 0\r\nv 0.5 2 0 1 0 0\r\nvn 0 0 1\r\nvt 0 0\r\n"
                 "f 1/1/1 2/1/1 3/1/1 4/1/1\r\nf 1/1 2/1 3/1\r\nf 1 2 3 4 5\r\nf 1//1 2//1 3//1\r\nf -5 -4 -3\r\n")
    m = oracle.Mesh.from_obj(str(p), scale=2.0, offset=(1, 0, 0))
    v = m.vertices
    np.testing.assert_array_equal(v[1], [3, 0, 0])           # transformed
    np.testing.assert_array_equal(v[4], [0.5, 2, 0])         # 6-number vertex: untouched (cpu:344-350)
    assert m.triangles.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 1, 2], [0, 1, 2]]


def test_kat_sphere(oracle):
    g = load_golden("kat.npz")
    L = oracle.lib()
    import ctypes as C
    fp = C.POINTER(C.c_float)
    for row, exp in zip(g["sphere_in"], g["sphere_out"]):
        row = np.ascontiguousarray(row)
        t = C.c_float(0); N = np.zeros(3, np.float32)
        hit = L.or_sphere_intersect(row[0:3].ctypes.data_as(fp), float(row[3]), row[4:7].ctypes.data_as(fp),
                                    row[7:10].ctypes.data_as(fp), C.byref(t), N.ctypes.data_as(fp))
        assert hit == int(exp[0])
        if hit:
            assert bits(np.float32(t.value)) == bits(exp[1])
            np.testing.assert_array_equal(bits(N), bits(exp[2:5]))
    assert 0.05 < g["sphere_out"][:, 0].mean() < 0.95


def test_kat_box(oracle):
    g = load_golden("kat.npz")
    L = oracle.lib()
    import ctypes as C
    fp = C.POINTER(C.c_float)
    got = []
    for row in g["box_in"]:
        row = np.ascontiguousarray(row)
        got.append(L.or_box_intersect(row[0:3].ctypes.data_as(fp), row[3:6].ctypes.data_as(fp),
                                      row[6:9].ctypes.data_as(fp), row[9:12].ctypes.data_as(fp)))
    np.testing.assert_array_equal(np.array(got, np.float32), g["box_out"])
    assert 0.05 < g["box_out"].mean() < 0.95
    zero_dir = (g["box_in"][:, 9:12] == 0).any(axis=1)
    assert zero_dir.sum() > 500      # the inf/nan slab cases are exercised


def test_kat_triangle(oracle):
    g = load_golden("kat.npz")
    L = oracle.lib()
    import ctypes as C
    fp = C.POINTER(C.c_float)
    for row, exp in zip(g["tri_in"], g["tri_out"]):
        row = np.ascontiguousarray(row)
        t = C.c_float(0); N = np.zeros(3, np.float32)
        hit = L.or_moller_trumbore(row[0:3].ctypes.data_as(fp), row[3:6].ctypes.data_as(fp), row[6:9].ctypes.data_as(fp),
                                   row[9:12].ctypes.data_as(fp), row[12:15].ctypes.data_as(fp), C.byref(t),
                                   N.ctypes.data_as(fp))
        assert hit == int(exp[0])
        np.testing.assert_array_equal(bits(N), bits(exp[2:5]))
        if hit:
            assert bits(np.float32(t.value)) == bits(exp[1])
    assert 0.2 < g["tri_out"][:, 0].mean() < 0.9


def test_kat_mesh_traversal(oracle_cat):
    g = load_golden("kat.npz")
    nhit = 0
    for row, exp in zip(g["mesh_in"], g["mesh_out"]):
        hit, t, N = oracle_cat.intersect(row[0:3], row[3:6])
        assert hit == bool(exp[0])
        if hit:
            nhit += 1
            assert bits(np.float32(t)) == bits(exp[1])
            np.testing.assert_array_equal(bits(N), bits(exp[2:5]))
    assert nhit > 1500


def test_png_bytes_of_unmodified_reference_binary(oracle, oracle_cat):
    """`./cpu 1 0` (the reference program itself, 512x512) vs the restatement's 8-bit output."""
    g = load_golden("ref_cpu_png_1_0.npz")
    assert hashlib.sha256(g["cat"].tobytes()).hexdigest() == SHA_CAT_1_0
    _, rgb8, cnt = oracle.Scene.preset("cpu", oracle_cat).render(512, 512, 1, 0)
    np.testing.assert_array_equal(rgb8, g["cat"])
    assert hashlib.sha256(rgb8.tobytes()).hexdigest() == SHA_CAT_1_0
    # OBJ missing => the reference renders the spheres-only scene (cpu:322-325)
    _, rgb8, _ = oracle.Scene.preset("spheres").render(512, 512, 1, 0)
    np.testing.assert_array_equal(rgb8, g["spheres"])
    # num_rays does not matter at num_bounce=0, sigma=0
    _, rgb8b, _ = oracle.Scene.preset("cpu", oracle_cat).render(512, 512, 3, 0, rows=(200, 232))
    np.testing.assert_array_equal(rgb8b, g["cat"][200:232])


@pytest.mark.parametrize("name,scene", [("cpu_512_direct", "cpu"), ("cpu_1080p_direct", "cpu"),
                                        ("spheres_512_direct", "spheres"), ("demo10_256_direct", "demo10"),
                                        ("cpu_512_b3_spp2", "cpu"), ("demo10_256_b5", "demo10")])
def test_float_render_matches_reference_getColor(oracle, oracle_cat, name, scene):
    """Linear float colour from the reference's Scene::getColor; the stochastic cases replay the
    reference's mt19937 stream (clock()==0, one thread) through rng_mode=1: bit-exact."""
    g = load_golden("ref_render.npz")
    W, H, spp, b, stride = (int(x) for x in g[name + "_cfg"])
    s = oracle.Scene.preset(scene, oracle_cat if scene == "cpu" else None)
    rgba, _, _ = s.render(W, H, spp, b, rng_mode=1, stride=stride, threads=1, want_rgb8=False)
    exp = g[name + "_color"]
    assert rgba.shape[:2] == exp.shape[:2]
    np.testing.assert_array_equal(bits(rgba[..., :3]), bits(exp))
    assert np.isfinite(exp).all() and exp.max() > 1.0


@pytest.mark.parametrize("name", ["cpu_mirror_256_b3", "cpu_glass_256_b5", "two_cats_256_b3", "two_cats_512_direct", "two_cats_diffuse_256_b1"])
def test_mesh_materials_and_several_meshes_match_reference_getColor(oracle, cat_golden, name):
    """Scenes the reference's classes accept and its main() never builds: a TriangleMesh with mirror = 1 / with refraction indices 1.5 / 1 (Geometry's public members,
    cpu:113-116, read by getColor for whichever object was hit, cpu:573-606) and TWO meshes in one Scene::objects, one of them in the middle of the order (cpu:538-564).
    Golden: the reference TU itself with those members set (oracle/ref_harness.cpp add_material_scene), mt19937(0) replayed: colours bit-exact, primary hit ids equal."""
    from . import material_scenes as ms
    g = load_golden("ref_materials.npz")
    W, H, spp, b, stride = (int(x) for x in g[name + "_cfg"])
    scene = name.rsplit("_", 2)[0]                                  # "two_cats_256_b3" -> "two_cats"
    s = ms.oracle_scene(oracle, scene, cat_golden["vertices"], cat_golden["tri_obj_order"])
    rgba, _, _ = s.render(W, H, spp, b, rng_mode=1, stride=stride, threads=1, want_rgb8=False)
    exp = g[name + "_color"]
    np.testing.assert_array_equal(bits(rgba[..., :3]), bits(exp))
    assert np.isfinite(exp).all() and exp.max() > 1.0
    rec = g[name + "_hit"]
    tan_h = np.float32(np.tan(np.float64(np.float32(np.float32(np.pi / 3) / np.float32(2)))))
    z = np.float32(np.float32(-W) / np.float32(np.float32(2) * tan_h))
    ids = set()
    for ii in range(0, rec.shape[0], 5):
        for jj in range(0, rec.shape[1], 5):
            i, j = ii * stride, jj * stride
            u = np.array([np.float32(j) - np.float32(W) / 2 + 0.5, np.float32(H) / 2 - i - 0.5, z], np.float32)
            n = np.sqrt(np.float32(np.float32(u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]))
            u = (u / n).astype(np.float32)
            hit, oid, P, N = s.intersect_all([0, 0, 55], u)
            assert oid == int(rec[ii, jj, 0])
            np.testing.assert_array_equal(bits(P), bits(rec[ii, jj, 1:4]))
            if hit:
                np.testing.assert_array_equal(bits(N), bits(rec[ii, jj, 4:7]))
            ids.add(oid)
    n_meshes = sum(1 for o in ms.describe(scene, cat_golden["vertices"]) if o[0] == "mesh")
    mesh_ids = {k for k, o in enumerate(ms.describe(scene, cat_golden["vertices"])) if o[0] == "mesh"}
    if scene == "two_cats_diffuse":
        assert 0 in ids and 7 not in ids                            # the same geometry twice: every hit is an exact tie and the EARLIER object keeps it (strict '<', cpu:554)
    else:
        assert mesh_ids <= ids, (ids, n_meshes)                     # every mesh is seen by some primary ray


@pytest.mark.parametrize("name,scene", [("cpu_512_direct", "cpu"), ("demo10_256_direct", "demo10")])
def test_primary_hit_records(oracle, oracle_cat, name, scene):
    g = load_golden("ref_render.npz")
    W, H, spp, b, stride = (int(x) for x in g[name + "_cfg"])
    s = oracle.Scene.preset(scene, oracle_cat if scene == "cpu" else None)
    rec = g[name + "_hit"]
    # correctly rounded float tangent (the reference's is constant-folded by g++, see rt_oracle.c or_render)
    tan_h = np.float32(np.tan(np.float64(np.float32(np.float32(np.pi / 3) / np.float32(2)))))
    z = np.float32(np.float32(-W) / np.float32(np.float32(2) * tan_h))
    ids = set()
    for ii in range(0, rec.shape[0], 3):
        for jj in range(0, rec.shape[1], 3):
            i, j = ii * stride, jj * stride
            u = np.array([np.float32(j) - np.float32(W) / 2 + 0.5, np.float32(H) / 2 - i - 0.5, z], np.float32)
            n = np.sqrt(np.float32(np.float32(u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]))
            u = (u / n).astype(np.float32)
            hit, oid, P, N = s.intersect_all([0, 0, 55], u)
            assert oid == int(rec[ii, jj, 0])
            np.testing.assert_array_equal(bits(P), bits(rec[ii, jj, 1:4]))
            if hit:
                np.testing.assert_array_equal(bits(N), bits(rec[ii, jj, 4:7]))
            ids.add(oid)
    assert len(ids) >= 4


def test_counter_rng_statistics_vs_reference_rng(oracle, oracle_cat):
    """The counter RNG replaces the reference's clock()-seeded mt19937: the estimator must
    agree statistically with the reference's own 256-spp mean (per-pixel standard error kept)."""
    g = load_golden("ref_stat.npz")
    W, H, spp, b, stride = (int(x) for x in g["cfg"])
    s = oracle.Scene.preset("cpu", oracle_cat)
    rgba, _, _ = s.render(W, H, spp, b, stride=stride, want_rgb8=False)
    mean, sem = g["mean"].astype(np.float64), g["sem"].astype(np.float64)
    # both sides are 256-sample means => difference has variance 2*sem^2
    zscore = (rgba[..., :3] - mean) / np.sqrt(2 * sem ** 2 + 1e-12)
    ok = sem > 0
    assert ok.mean() > 0.3            # pure-colour walls have exactly-zero channels
    assert np.abs(zscore[ok]).mean() < 1.0           # E|z| = 0.8 for a unit normal
    assert (np.abs(zscore[ok]) > 5).mean() < 2e-3
    assert abs(zscore[ok].mean()) < 0.15             # no bias (an mt19937 stream with another seed gives 0.08)
    rel = np.abs(rgba[..., :3].mean() - mean.mean()) / mean.mean()
    assert rel < 5e-3


def test_counter_rng_properties(oracle):
    u = np.array([oracle.uniform(123456, p, s, d, k) for p in range(40) for s in range(3) for d in range(4)
                  for k in range(4)])
    assert (u > 0).all() and (u <= 1).all()
    assert abs(u.mean() - 0.5) < 0.02 and abs(u.var() - 1 / 12) < 0.01
    assert len(np.unique(u)) > 0.99 * len(u)
    assert oracle.uniform(1, 2, 3, 4, 1) == oracle.uniform(1, 2, 3, 4, 1)


def test_render_is_thread_and_tile_independent(oracle, oracle_cat):
    s = oracle.Scene.preset("cpu", oracle_cat)
    full, _, c_full = s.render(256, 144, 2, 2, threads=4, want_rgb8=False)
    one, _, c_one = s.render(256, 144, 2, 2, threads=1, want_rgb8=False)
    np.testing.assert_array_equal(bits(full), bits(one))
    assert c_full == c_one
    part, _, _ = s.render(256, 144, 2, 2, rows=(40, 72), want_rgb8=False)
    np.testing.assert_array_equal(bits(part), bits(full[40:72]))
    assert c_full["rays"] == int(full[..., 3].sum())
