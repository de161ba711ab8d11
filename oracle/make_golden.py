#!/usr/bin/env python3
"""TEST INFRASTRUCTURE -- generates tests/golden/*.npz from the REAL reference.

Run in the build container only (needs /root/reference and `make -C oracle ref`):

    python oracle/make_golden.py

What it does
  * runs oracle/_ref/cpu (= /root/reference/cpu_launcher.cpp built exactly as the
    reference Makefile:38 says) as `cpu 1 0` in a scratch directory, once with the
    cat OBJ reachable and once without (spheres-only), decodes the PNGs and stores
    the RGB bytes + SHA-256;
  * runs oracle/_ref/ref_harness (oracle/ref_harness.cpp + the reference TU) to dump
    the parsed mesh, the BVH, primitive known-answer tests, float renders (direct
    lighting, and mt19937(0)-replayable stochastic renders) and a statistical mean;
  * runs oracle/_ref/realtime_harness (oracle/realtime_harness.cpp + the device code of the reference's
    realtime_render.cu as host functions) for the posed camera, the progressive output, smooth normals,
    the transform kernel and the motions (`realtime`; oracle/realtime_fixture.py);
  * packs everything as numpy .npz (no pickles) under tests/golden/.

The fixtures are data: inputs and the reference's outputs.  No reference source
text is stored.  The cat mesh (cadnav.com, see tests/golden/README.md for the
attribution its readme asks for) is stored as the float32 vertex array and the
int32 index array the reference's own parser produced.
"""
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("RT_REFERENCE", "/root/reference")
GOLD = os.path.join(ROOT, "tests", "golden")
CPU = os.path.join(HERE, "_ref", "cpu")
HARNESS = os.path.join(HERE, "_ref", "ref_harness")


def run(cmd, cwd, env=None):
    e = dict(os.environ)
    if env:
        e.update(env)
    r = subprocess.run(cmd, cwd=cwd, env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        print(r.stdout)
        raise SystemExit(f"{cmd} failed with {r.returncode}")
    return r.stdout


def f32(path, cols=None):
    a = np.fromfile(path, dtype="<f4")
    return a.reshape(-1, cols) if cols else a


def i32(path, cols=None):
    a = np.fromfile(path, dtype="<i4")
    return a.reshape(-1, cols) if cols else a


def norm_rows(v):
    """float32 normalisation in the reference's operation order (cpu:58-63)."""
    v = v.astype(np.float32)
    n2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]).astype(np.float32) + v[:, 2] * v[:, 2]
    n = np.sqrt(n2.astype(np.float32)).astype(np.float32)
    return (v / n[:, None]).astype(np.float32)


def make_kat_inputs(rng, verts, tris):
    cam = np.array([0, 0, 55], np.float32)
    # ---- spheres: [C R O u]
    walls = np.array([[0, 0, -1000, 940], [0, -1000, 0, 990], [0, 1000, 0, 940], [-1000, 0, 0, 940],
                      [1000, 0, 0, 940], [0, 0, 1000, 940], [0, 0, 0, 10], [-20, 0, 0, 10], [20, 0, 0, 9]], np.float32)
    rows = []
    for _ in range(4000):
        s = walls[rng.integers(len(walls))]
        O = cam if rng.random() < 0.5 else rng.uniform(-50, 50, 3).astype(np.float32)
        u = norm_rows(rng.normal(size=(1, 3)))[0]
        rows.append(np.concatenate([s, O, u]))
    for s in walls[6:]:  # tangent / through-centre / inside / behind
        C, Rr = s[:3], s[3]
        for O in (cam, C.copy(), (C + np.array([0, 0, Rr / 2], np.float32)).astype(np.float32)):
            for tgt in (C, C + np.array([Rr, 0, 0], np.float32), C + np.array([0, Rr, 0], np.float32),
                        C + np.array([Rr * 1.0000001, 0, 0], np.float32)):
                d = (tgt - O).astype(np.float32)
                if not d.any():
                    d = np.array([0, 0, -1], np.float32)
                u = norm_rows(d[None])[0]
                rows.append(np.concatenate([s, O, u]))
                rows.append(np.concatenate([s, O, -u]))
    sph = np.array(rows, np.float32)
    # ---- boxes: [mn mx O u]
    rows = []
    for _ in range(6000):
        a = rng.uniform(-30, 30, 3); b = a + rng.uniform(0, 20, 3) * (rng.random(3) > 0.1)
        O = cam if rng.random() < 0.5 else rng.uniform(-60, 60, 3)
        u = norm_rows(rng.normal(size=(1, 3)))[0].astype(np.float64)
        if rng.random() < 0.7:   # aim at a point in (or just around) the box so that hits are common
            tgt = a + (b - a) * rng.uniform(-0.15, 1.15, 3)
            u = norm_rows((tgt - O)[None])[0].astype(np.float64)
        k = rng.random()
        if k < 0.15:
            u[rng.integers(3)] = 0.0  # axis-parallel slab => inf / nan
        if k < 0.03:
            u[:] = 0; u[rng.integers(3)] = 1.0
        if 0.15 <= k < 0.25:  # origin exactly on a slab plane with zero direction component => 0/0
            ax = rng.integers(3); O = np.array(O, np.float64); O[ax] = a[ax]; u[ax] = 0.0
        if 0.25 <= k < 0.35:  # aim exactly at a corner
            corner = np.where(rng.random(3) < 0.5, a, b)
            u = norm_rows((corner - O)[None])[0]
        rows.append(np.concatenate([a, b, O, u]))
    box = np.array(rows, np.float32)
    # ---- triangles: [A B C O u]
    rows = []
    for _ in range(6000):
        A, B, C = rng.uniform(-20, 20, (3, 3)).astype(np.float32)
        O = cam if rng.random() < 0.5 else rng.uniform(-60, 60, 3).astype(np.float32)
        k = rng.random()
        if k < 0.5:   # aim inside the triangle
            w = rng.dirichlet([1, 1, 1]); tgt = w[0] * A + w[1] * B + w[2] * C
        elif k < 0.6:  # exactly at a vertex
            tgt = (A, B, C)[rng.integers(3)]
        elif k < 0.75:  # exactly on an edge
            s = rng.random(); tgt = s * A + (1 - s) * B
        else:
            tgt = rng.uniform(-25, 25, 3)
        u = norm_rows((np.asarray(tgt, np.float32) - O)[None])[0]
        if k > 0.97:   # ray parallel to the plane: u = e1 direction
            u = norm_rows((B - A)[None])[0]
        if k > 0.985:  # degenerate triangle
            C = A.copy()
        rows.append(np.concatenate([A, B, C, O, u]))
    # real cat triangles hit through vertices / edge midpoints from the camera
    for ti in rng.integers(0, len(tris), 800):
        A, B, C = verts[tris[ti]]
        for tgt in (A, ((A + B) / 2).astype(np.float32), ((A + B + C) / 3).astype(np.float32)):
            u = norm_rows((tgt - cam)[None])[0]
            rows.append(np.concatenate([A, B, C, cam, u]))
    tri = np.array(rows, np.float32)
    # ---- whole mesh: [O u]
    rows = []
    L = np.array([-10, 20, 40], np.float32)
    for _ in range(3000):
        tgt = verts[rng.integers(len(verts))] + rng.normal(scale=0.3, size=3).astype(np.float32)
        u = norm_rows((tgt - cam)[None])[0]
        rows.append(np.concatenate([cam, u]))
    for vi in rng.integers(0, len(verts), 600):   # exactly through mesh vertices
        u = norm_rows((verts[vi] - cam)[None])[0]
        rows.append(np.concatenate([cam, u]))
    for _ in range(2000):                          # shadow-like rays towards the light
        O = rng.uniform([-30, -10, -10], [30, 30, 20]).astype(np.float32)
        u = norm_rows((L - O)[None])[0]
        rows.append(np.concatenate([O, u]))
    for _ in range(1000):                          # axis-parallel and random
        u = np.zeros(3, np.float32); u[rng.integers(3)] = rng.choice([-1, 1])
        O = rng.uniform(-30, 30, 3).astype(np.float32)
        rows.append(np.concatenate([O, u]))
    mesh = np.array(rows, np.float32)
    return sph, box, tri, mesh


MATERIAL_RENDERS = [  # name, scene (oracle/ref_harness.cpp add_material_scene), W, H, spp, bounce, stride
    ("cpu_mirror_256_b3", "cpu_mirror", 256, 256, 1, 3, 2),
    ("cpu_glass_256_b5", "cpu_glass", 256, 256, 1, 5, 2),
    ("two_cats_256_b3", "two_cats", 256, 256, 1, 3, 2),
    ("two_cats_512_direct", "two_cats", 512, 512, 1, 0, 4),
    ("two_cats_diffuse_256_b1", "two_cats_diffuse", 256, 256, 1, 1, 2),
]


def make_materials():
    """tests/golden/ref_materials.npz alone (`python oracle/make_golden.py materials`): mesh materials and several meshes per scene through the reference's own
    Scene::getColor / intersect_all (single thread, mt19937(0)); the other fixtures stay as committed (ref_stat.npz is not reproducible run to run)."""
    tmp = tempfile.mkdtemp(prefix="rt_golden_")
    try:
        with_cat = os.path.join(tmp, "with_cat"); os.makedirs(with_cat)
        os.symlink(os.path.join(REF, "cadnav.com_model"), os.path.join(with_cat, "cadnav.com_model"))
        out = {}
        for name, scene, W, H, spp, b, stride in MATERIAL_RENDERS:
            base = os.path.join(tmp, name)
            run([HARNESS, "render", scene, str(W), str(H), str(spp), str(b), str(stride), base], with_cat, {"OMP_NUM_THREADS": "1"})
            nh, nw = (H + stride - 1) // stride, (W + stride - 1) // stride
            out[name + "_color"] = f32(base + ".color.f32").reshape(nh, nw, 3)
            out[name + "_hit"] = f32(base + ".hit.f32").reshape(nh, nw, 7)
            out[name + "_cfg"] = np.array([W, H, spp, b, stride], np.int32)
            print("render", name, out[name + "_color"].shape)
        np.savez_compressed(os.path.join(GOLD, "ref_materials.npz"), **out)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def obj_text(rng, n_v=2247, n_vn=2152, n_vt=2032, n_f=3954):
    """An OBJ in the layout of the cat's exporter (comment header, mtllib, `v  x y z` with four decimals, vn / vt blocks, g / usemtl / s,
    `f v/vt/vn v/vt/vn v/vt/vn ` with a trailing blank, CRLF line ends) with the cat's counts but seeded numbers and faces of our own."""
    L = ["# Wavefront OBJ written by oracle/make_golden.py", "# the layout of a 3ds Max export", "", "mtllib synthetic.mtl", "", "#", "# object synthetic_001", "#", ""]
    v = np.round(rng.uniform(-32.0, 32.0, (n_v, 3)), 4)
    v[rng.integers(0, n_v, 40), rng.integers(0, 3, 40)] = 0.0             # exact zeros, printed as 0.0000 / -0.0000 below
    L += ["v  %.4f %.4f %.4f" % tuple(r) for r in v]
    L[len(L) - 20] = "v  %.4f %.4f %.4f" % (-0.0, 7.0, -0.0)
    L += ["# %d vertices" % n_v, ""]
    L += ["vn %.4f %.4f %.4f" % tuple(r) for r in np.round(rng.uniform(-1, 1, (n_vn, 3)), 4)] + ["# %d vertex normals" % n_vn, ""]
    L += ["vt %.4f %.4f %.4f" % tuple(r) for r in np.round(rng.uniform(0, 1, (n_vt, 3)) * [1, 1, 0], 4)] + ["# %d texture coords" % n_vt, ""]
    L += ["g synthetic_001", "usemtl synthetic", "s off"]
    for _ in range(n_f):
        vi = rng.choice(n_v, 3, replace=False) + 1
        L.append("f " + " ".join("%d/%d/%d" % (a, rng.integers(1, n_vt + 1), rng.integers(1, n_vn + 1)) for a in vi) + " ")
    L += ["# %d faces" % n_f, "", ""]
    return "\r\n".join(L).encode()


def make_obj():
    """tests/golden/ref_obj.npz alone (`python oracle/make_golden.py obj`): a seeded OBJ in the cat's exporter layout (obj_text()) and what the reference's own
    TriangleMesh::readOBJ makes of it (`ref_harness mesh` with that file where the reference looks for the cat): the OBJ reader tests need no asset from outside."""
    text = obj_text(np.random.default_rng(20261016))
    tmp = tempfile.mkdtemp(prefix="rt_golden_")
    try:
        od = os.path.join(tmp, "cadnav.com_model", "Models_F0202A090"); os.makedirs(od)
        with open(os.path.join(od, "cat.obj"), "wb") as f:
            f.write(text)
        md = os.path.join(tmp, "mesh"); os.makedirs(md)
        print(run([HARNESS, "mesh", md], tmp).strip())
        np.savez_compressed(os.path.join(GOLD, "ref_obj.npz"), obj_text=np.frombuffer(text, np.uint8),
                            vertices=f32(os.path.join(md, "vertices.f32"), 3), tri_obj_order=i32(os.path.join(md, "tri_obj_order.i32"), 3))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


FUZZ_SEEDS, FUZZ_W, FUZZ_H = range(8), 32, 24


def fuzz_scene(family, seed):
    """scene(family, seed) of tests/scene_fuzz.py as the fixture holds it: 32 x 24, one sample, the family's own num_bounce, and the reference's own eps
    (a literal 1e-3 in Scene::getColor, cpu:575, 582, 610: the scenes of `light_edge` that ask for 0 or 1e-6 are held to the reference at 1e-3)"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from tests import scene_fuzz
    return scene_fuzz.resized(scene_fuzz.scene(family, seed), FUZZ_W, FUZZ_H, spp=1, eps=1e-3)


def make_fuzz():
    """tests/golden/ref_fuzz.npz alone (`python oracle/make_golden.py fuzz`): seeds 0 to 7 of every family of tests/scene_fuzz.py through the reference's own
    Sphere, TriangleMesh, Scene and Scene::getColor (`ref_harness fuzz`, one process per scene: single thread, mt19937(0)); the packed descriptions and the frames."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from tests import scene_fuzz
    keys = [(f, k) for f in scene_fuzz.FAMILIES for k in FUZZ_SEEDS]
    packed = [scene_fuzz.pack(fuzz_scene(f, k)) for f, k in keys]
    tmp = tempfile.mkdtemp(prefix="rt_golden_")
    try:
        src = os.path.join(tmp, "scenes.f32")
        np.concatenate([np.array([len(packed)], np.float32)] + packed).astype("<f4").tofile(src)
        out = {}
        for i, (f, k) in enumerate(keys):
            dst = os.path.join(tmp, "frame.f32")
            run([HARNESS, "fuzz", src, str(i), dst], tmp, {"OMP_NUM_THREADS": "1"})
            out[f"{f}_{k}_desc"] = packed[i]
            out[f"{f}_{k}_frame"] = f32(dst).reshape(FUZZ_H, FUZZ_W, 3)
        np.savez_compressed(os.path.join(GOLD, "ref_fuzz.npz"), **out)
        print("fuzz", len(keys), "scenes", os.path.getsize(os.path.join(GOLD, "ref_fuzz.npz")), "bytes")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def make_realtime():
    """tests/golden/ref_realtime.npz alone (`python oracle/make_golden.py realtime`): the posed camera and its rays, the progressive output, smooth normals, the
    `transform` kernel and the light's and spheres' motions as the device code of the reference's realtime_render.cu computes them, run as host functions by
    oracle/_ref/realtime_harness; inputs and the run are oracle/realtime_fixture.py's.  The same bytes on every run."""
    if HERE not in sys.path:
        sys.path.insert(0, HERE)
    import realtime_fixture
    if not os.path.exists(realtime_fixture.HARNESS):
        raise SystemExit("build the reference first: make -C oracle ref")
    path = os.path.join(GOLD, "ref_realtime.npz")
    realtime_fixture.save(path, realtime_fixture.build())
    print("realtime", os.path.getsize(path), "bytes", hashlib.sha256(open(path, "rb").read()).hexdigest())


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "realtime":
        os.makedirs(GOLD, exist_ok=True)
        return make_realtime()
    if not (os.path.exists(CPU) and os.path.exists(HARNESS)):
        raise SystemExit("build the reference first: make -C oracle ref")
    os.makedirs(GOLD, exist_ok=True)
    if len(sys.argv) > 1 and sys.argv[1] == "materials":
        return make_materials()
    if len(sys.argv) > 1 and sys.argv[1] == "obj":
        return make_obj()
    if len(sys.argv) > 1 and sys.argv[1] == "fuzz":
        return make_fuzz()
    tmp = tempfile.mkdtemp(prefix="rt_golden_")
    try:
        with_cat = os.path.join(tmp, "with_cat"); os.makedirs(with_cat)
        no_cat = os.path.join(tmp, "no_cat"); os.makedirs(no_cat)
        os.symlink(os.path.join(REF, "cadnav.com_model"), os.path.join(with_cat, "cadnav.com_model"))

        # 1. the unmodified reference binary, deterministic setting `1 0`
        imgs = {}
        for name, cwd in (("cat", with_cat), ("spheres", no_cat)):
            run([CPU, "1", "0"], cwd, {"OMP_NUM_THREADS": "8"})
            rgb = np.array(Image.open(os.path.join(cwd, "image.png")).convert("RGB"), np.uint8)
            imgs[name] = rgb
            print(name, rgb.shape, hashlib.sha256(rgb.tobytes()).hexdigest())
        np.savez_compressed(os.path.join(GOLD, "ref_cpu_png_1_0.npz"),
                            cat=imgs["cat"], spheres=imgs["spheres"],
                            cat_sha256=np.frombuffer(hashlib.sha256(imgs["cat"].tobytes()).digest(), np.uint8),
                            spheres_sha256=np.frombuffer(hashlib.sha256(imgs["spheres"].tobytes()).digest(), np.uint8))

        # 2. mesh + BVH as the reference parses / builds them
        md = os.path.join(tmp, "mesh"); os.makedirs(md)
        print(run([HARNESS, "mesh", md], with_cat).strip())
        verts = f32(os.path.join(md, "vertices.f32"), 3)
        tri_obj = i32(os.path.join(md, "tri_obj_order.i32"), 3)
        tri_bvh = i32(os.path.join(md, "tri_bvh_order.i32"), 3)
        arr10 = f32(os.path.join(md, "bvh_arr10.f32"), 10)
        np.savez_compressed(os.path.join(ROOT, "raytracinggpu_amd", "data", "cat_mesh.npz"), vertices=verts, tri_obj_order=tri_obj,
                            tri_bvh_order=tri_bvh, bvh_arr10=arr10)

        # 3. primitive KATs
        rng = np.random.default_rng(20261004)
        sph, box, tri, mesh = make_kat_inputs(rng, verts, tri_obj)
        kd = os.path.join(tmp, "kat"); os.makedirs(kd)
        sph.tofile(os.path.join(kd, "kat_sphere_in.f32")); box.tofile(os.path.join(kd, "kat_box_in.f32"))
        tri.tofile(os.path.join(kd, "kat_tri_in.f32")); mesh.tofile(os.path.join(kd, "kat_mesh_in.f32"))
        run([HARNESS, "kat", kd], with_cat)
        np.savez_compressed(os.path.join(GOLD, "kat.npz"),
                            sphere_in=sph, sphere_out=f32(os.path.join(kd, "kat_sphere_out.f32"), 5),
                            box_in=box, box_out=f32(os.path.join(kd, "kat_box_out.f32")),
                            tri_in=tri, tri_out=f32(os.path.join(kd, "kat_tri_out.f32"), 5),
                            mesh_in=mesh, mesh_out=f32(os.path.join(kd, "kat_mesh_out.f32"), 5))

        # 4. float renders through the reference's Scene::getColor (single thread, mt19937(0))
        renders = [  # name, scene, W, H, spp, bounce, stride
            ("cpu_512_direct", "cpu", 512, 512, 1, 0, 4),
            ("cpu_1080p_direct", "cpu", 1920, 1080, 1, 0, 8),
            ("spheres_512_direct", "spheres", 512, 512, 1, 0, 4),
            ("cpu_512_b3_spp2", "cpu", 512, 512, 2, 3, 8),
            ("demo10_256_b5", "demo10", 256, 256, 1, 5, 2),
            ("demo10_256_direct", "demo10", 256, 256, 1, 0, 2),
        ]
        out = {}
        for name, scene, W, H, spp, b, stride in renders:
            base = os.path.join(tmp, name)
            run([HARNESS, "render", scene, str(W), str(H), str(spp), str(b), str(stride), base], with_cat,
                {"OMP_NUM_THREADS": "1"})
            nh, nw = (H + stride - 1) // stride, (W + stride - 1) // stride
            out[name + "_color"] = f32(base + ".color.f32").reshape(nh, nw, 3)
            out[name + "_hit"] = f32(base + ".hit.f32").reshape(nh, nw, 7)
            out[name + "_cfg"] = np.array([W, H, spp, b, stride], np.int32)
            print("render", name, out[name + "_color"].shape)
        np.savez_compressed(os.path.join(GOLD, "ref_render.npz"), **out)

        # 5. statistical golden of the stochastic estimator (reference RNG, 8 threads)
        base = os.path.join(tmp, "stat")
        W, H, spp, b, stride = 512, 512, 256, 3, 8
        run([HARNESS, "stat", str(W), str(H), str(spp), str(b), str(stride), base], with_cat, {"OMP_NUM_THREADS": "8"})
        nh, nw = (H + stride - 1) // stride, (W + stride - 1) // stride
        np.savez_compressed(os.path.join(GOLD, "ref_stat.npz"),
                            mean=f32(base + ".mean.f32").reshape(nh, nw, 3),
                            sem=f32(base + ".sem.f32").reshape(nh, nw, 3),
                            cfg=np.array([W, H, spp, b, stride], np.int32))
        print("stat done")
        make_materials()
        make_obj()
        make_fuzz()
        make_realtime()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for fn in sorted(os.listdir(GOLD)):
        print(f"{os.path.getsize(os.path.join(GOLD, fn)):9d}  {fn}")


if __name__ == "__main__":
    sys.exit(main())
