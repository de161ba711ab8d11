"""Pins what the oracle (oracle/rt_oracle.c) and the library's host code restate from the reference's realtime_render.cu to that program itself.

tests/golden/ref_realtime.npz was written by the reference's OWN device code -- Camera::rotate, KernelLaunch, TriangleMesh::get_smooth_normal, transform,
MoveLightSource, MoveObject -- run as host functions (oracle/realtime_harness.cpp over the stand-in CUDA headers of oracle/ref_stubs/; inputs:
oracle/realtime_fixture.py).  Every comparison is bit for bit, as uint32: a NaN equals a NaN only where the fixture has one, and -0 is not +0.

One recorded deviation (DESIGN.md "Numerics"): KernelLaunch evaluates tan(pov / 2) with a run-time tanf (realtime:1112); the oracle and rt_render_pose use the
correctly rounded binary32 tangent, which no C library can change.  test_camera_rays holds every fov at which the two agree to the fixture as it is, and
the others to the fixture once the oracle is handed the fixture's z: only the tangent may differ.
"""
import os

import numpy as np
import pytest

import raytracinggpu_amd as rt

from .conftest import load_golden


INTENSITY = float(np.float32(3e10))                                   # KernelInit's (realtime:1024)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, exp, what):
    g, e = bits(got), bits(exp)
    assert g.shape == e.shape, what
    bad = np.argwhere(g != e)
    assert len(bad) == 0, f"{what}: {len(bad)} of {g.size} words differ, first at {tuple(bad[0])}: got {np.asarray(got).ravel()[np.flatnonzero(g != e)[0]]!r}, " \
                          f"reference {np.asarray(exp).ravel()[np.flatnonzero(g != e)[0]]!r}"


@pytest.fixture(scope="module")
def ref():
    return load_golden("ref_realtime.npz")


def correctly_rounded_tan_half(fov):
    """the binary32 nearest to tan(fov / 2) of the binary32 fov / 2: binary64 tan is within an ulp of binary64, far finer than the binary32 grid unless the
    true value sits within 2^-29 relative of a binary32 midpoint, which none of the fixture's four does (checked against the fixture below)"""
    return np.float32(np.tan(np.float64(np.float32(fov) / np.float32(2))))


def test_camera_basis(oracle, ref):
    """Camera::rotate (realtime:825-847) at 200 (yaw, pitch): the oracle's restatement and the library's host function"""
    for k, ((yaw, pitch), exp) in enumerate(zip(ref["basis_in"], ref["basis_out"])):
        same(np.array(oracle.camera_basis(float(yaw), float(pitch))), exp, f"or_camera_basis({yaw!r}, {pitch!r}) (row {k})")
        same(np.array(rt.camera_basis(rt.make_pose(yaw=float(yaw), pitch=float(pitch)))), exp, f"rt_camera_basis({yaw!r}, {pitch!r}) (row {k})")


def oracle_rays(oracle, case, jitter, sigma, z=None):
    W, H, fov = int(case[0]), int(case[1]), float(case[2])
    out = np.zeros((len(jitter), H, W, 6), np.float32)
    for j, (r1, r2) in enumerate(jitter):
        for y in range(H):
            for x in range(W):
                O, u = oracle.posed_ray(W, H, fov, case[3:6], float(case[6]), float(case[7]), x, y, float(r1), float(r2), sigma=sigma, z=z)
                out[j, y, x, :3], out[j, y, x, 3:] = O, u
    return out


def test_camera_rays(oracle, ref):
    """KernelLaunch's camera ray (realtime:1112-1128) as a probe object saw it: every pixel of 16 x 12 and 13 x 7 frames, five poses, four fovs, once with
    r1 = 1 (jitter exactly +-0) and with eight (r1, r2) pairs.  Cases whose run-time tanf is the correctly rounded tangent are held as they are; the others
    (pi / 3 alone) are held with the fixture's z handed to the oracle, and their own z must differ from the fixture's exactly as the two tangents do."""
    cases, jitter, sigma = ref["ray_cases"], ref["ray_jitter"], float(ref["ray_sigma"][0])
    set_aside = []
    for k, case in enumerate(cases):
        W, fov = int(case[0]), case[2]
        t_ref, t_cr = ref["ray_tan"][k], correctly_rounded_tan_half(fov)
        exp = ref[f"rays_{k:02d}"]
        what = f"case {k} ({W} x {int(case[1])}, fov {fov!r}, C {case[3:6]}, yaw {case[6]!r}, pitch {case[7]!r})"
        if bits(t_ref) == bits(t_cr):
            same(oracle_rays(oracle, case, jitter, sigma), exp, what)
        else:
            set_aside.append(float(fov))
            assert bits(ref["ray_z"][k]) == bits(np.float32(-W) / (np.float32(2) * t_ref)), what                 # the fixture's z is its own tangent's
            z_own = np.float32(-W) / (np.float32(2) * t_cr)
            assert bits(z_own) != bits(ref["ray_z"][k]), what
            same(oracle_rays(oracle, case, jitter, sigma, z=float(ref["ray_z"][k])), exp, what + ", the fixture's z")
            assert np.any(bits(oracle_rays(oracle, case, jitter[:1], sigma)) != bits(exp[:1])), what + ": the deviation no longer shows; drop it from DESIGN.md"
    # at most the fovs where the two tangents differ are set aside: pi / 3 alone, three of the four stay in
    assert set(np.float32(f) for f in set_aside) <= {np.float32(np.pi / 3)}, set_aside
    assert len({float(c[2]) for c in cases} - set(set_aside)) >= 3


def test_progressive_output(oracle, ref):
    """accumbuffer += colour; accumbuffer / framenumber; (unsigned char)min(powf(c, 1 / 2.2f), 255.) (realtime:1136-1147) on values at every 8-bit code
    boundary, denormals, > 255^2.2, inf and NaN, frame numbers 1, 2, 3, 7, 1000.  The kernel's colour is the probe's miss: 0."""
    for n in ref["prog_frames"]:
        acc_in, exp_acc, exp_disp, exp_bytes = (ref[f"prog_{n}_{k}"] for k in ("accum_in", "accum_out", "display", "bytes"))
        assert np.array_equal(exp_bytes[:, 3], np.ones(len(exp_bytes), np.uint8))                               # make_uchar4(..., 1)
        assert len(np.unique(exp_bytes[:, :3])) == 256                                                          # every code is met
        accum = np.zeros((len(acc_in), 4), np.float32); accum[:, :3] = acc_in
        disp, rgb8 = oracle.progressive_accumulate(accum, np.zeros_like(accum), int(n))
        same(accum[:, :3], exp_acc, f"accumbuffer after frame {n}")
        same(disp[:, :3], exp_disp, f"display values, frame {n}")
        bad = np.argwhere(rgb8 != exp_bytes[:, :3])
        assert len(bad) == 0, f"frame {n}: {len(bad)} bytes differ, first at {tuple(bad[0])}: display {disp[bad[0][0], bad[0][1]]!r}"


def patch_mesh(oracle, verts, normals, tris):
    """the oracle's mesh of the patch with its BVH built and normals set, and to_fixture[k] = the fixture's index of the triangle now at position k"""
    m = oracle.Mesh.from_arrays(verts, tris[:, :3]).build_bvh()
    key = {tuple(t[:3]): i for i, t in enumerate(tris)}
    to_fixture = np.array([key[tuple(t)] for t in m.triangles])
    assert sorted(to_fixture) == list(range(len(tris)))
    m.set_normals(normals, tris[to_fixture, 3:])
    return m, to_fixture


def check_smooth(oracle, m, to_fixture, rays, exp, what, tri_tmin=1e-4):
    """exp[r, t]: get_smooth_normal of ray r and triangle t.  Compared: the pairs (ray, the triangle the oracle reports as its nearest hit) -> their share"""
    hits = 0
    for r, ray in enumerate(rays):
        hit, _, N, tri = m.intersect_tri(ray[:3], ray[3:], tri_tmin)
        if hit:
            hits += 1
            same(N, exp[r, to_fixture[tri]], f"{what}: ray {r} {ray!r}, triangle {to_fixture[tri]}")
    return hits / len(rays)


def test_smooth_normals(oracle, ref):
    """get_smooth_normal (realtime:221-245) for 768 recorded camera rays x the 8 triangles of the patch (non-unit, mutually inconsistent vertex normals), read
    through the oracle's mesh intersect: bit for bit for the triangle the oracle hits, and at least 80 % of the rays take part (here: all of them)"""
    m, to_fixture = patch_mesh(oracle, ref["patch_verts"], ref["patch_normals"], ref["patch_tris"])
    rays = np.concatenate([ref[f"rays_{k:02d}"][0].reshape(-1, 6) for k in ref["smooth_cases"]])
    share = check_smooth(oracle, m, to_fixture, rays, ref["smooth_N"].reshape(len(rays), len(to_fixture), 3), "patch")
    print(f"smooth normals: {share:.3f} of {len(rays)} rays hit the patch")
    assert share >= 0.8


def test_smooth_normals_edge_cases(oracle, ref):
    """rays through a vertex, through the middle of an edge (beta or gamma exactly 0) and grazing a triangle's plane: whichever triangle the oracle settles on,
    its normal is the reference's for that pair.  The straight rays have two zero direction components, so those on the rim of a BVH box miss it
    (BoundingBox::intersect's strict '>' and 0 / 0); of each kind -- vertex, edge AB, edge AC -- some hit."""
    m, to_fixture = patch_mesh(oracle, ref["patch_verts"], ref["patch_normals"], ref["patch_tris"])
    rays, exp = ref["smooth_edge_rays"], ref["smooth_edge_N"]
    for kind in range(3):
        share = check_smooth(oracle, m, to_fixture, rays[kind::4], exp[kind::4], ("vertex", "edge AB", "edge AC")[kind])
        print(f"edge cases, kind {kind}: {share:.2f} of the rays hit")
        assert share > 0
    check_smooth(oracle, m, to_fixture, rays[3::4], exp[3::4], "grazing")


def test_smooth_normals_after_transform(oracle, ref):
    """or_mesh_transform on the patch WITH normals, then the smooth normal: the reference's transform (which translates the normals too) and its
    get_smooth_normal over the moved arrays"""
    m, to_fixture = patch_mesh(oracle, ref["patch_verts"], ref["patch_normals"], ref["patch_tris"])
    T = ref["patch_transform"]
    m.transform(T[:9], T[9:]).refit()
    same(m.vertices, ref["patch_verts_moved"], "patch vertices after transform")
    rays = np.concatenate([ref[f"rays_{k:02d}"][0].reshape(-1, 6) for k in ref["smooth_cases"]])
    share = check_smooth(oracle, m, to_fixture, rays, ref["smooth_N_moved"].reshape(len(rays), len(to_fixture), 3), "moved patch")
    assert share >= 0.8


def test_transform(oracle, ref):
    """the `transform` kernel (realtime:415-432) over 37 vertices and 41 normals: a rotation, a matrix that is not orthogonal, the identity with -0 entries,
    translations large enough to round.  The oracle keeps normals per mesh, so they ride on a mesh whose triangles index them."""
    verts, normals = ref["transform_verts"], ref["transform_normals"]
    tris = np.array([[0, 1, 2]], np.int32)
    for k, case in enumerate(ref["transform_cases"]):
        m = oracle.Mesh.from_arrays(verts, tris)
        m.set_normals(normals, tris)
        m.transform(case[:9], case[9:])
        same(m.vertices, ref["transform_verts_out"][k], f"vertices, case {k}")
        same(m.shading_normals, ref["transform_normals_out"][k], f"normals, case {k}")


def test_light_motion(oracle, ref):
    """MoveLightSource (realtime:1072-1090) for 100 lights (on the axis, across atan2f's branch cut), several speeds and dt, and 20 chained steps: the
    oracle's restatement and rt_light_orbit, the host function behind rt_scene_move_light"""
    for k, (row, exp) in enumerate(zip(ref["light_in"], ref["light_out"])):
        same(oracle.light_orbit(row[:3], float(row[3]), float(row[4])), exp, f"or_light_orbit, light {k} {row!r}")
        pos, inten = rt.light_orbit((tuple(float(x) for x in row[:3]), INTENSITY), float(row[3]), float(row[4]))
        same(np.array(pos, np.float32), exp, f"rt_light_orbit, light {k} {row!r}")
        assert inten == INTENSITY
    row = ref["light_chain_in"][0]
    a, b = row[:3].copy(), (tuple(float(x) for x in row[:3]), INTENSITY)
    for k, exp in enumerate(ref["light_chain_out"]):
        a = oracle.light_orbit(a, float(row[3]), float(row[4]))
        b = rt.light_orbit(b, float(row[3]), float(row[4]))
        same(a, exp, f"or_light_orbit, chained step {k}")
        same(np.array(b[0], np.float32), exp, f"rt_light_orbit, chained step {k}")


def test_sphere_motion(oracle, ref):
    """MoveObject (realtime:1092-1098): C + v * dt with -0 velocities, a dt that rounds the product and centres that round the sum"""
    for k, (row, exp) in enumerate(zip(ref["object_in"], ref["object_out"])):
        same(oracle.sphere_move(row[:3], row[3:6], float(row[6])), exp, f"or_sphere_move, row {k} {row!r}")


def test_fixture_is_what_the_harness_writes(ref):
    """where oracle/_ref/realtime_harness has been built (it needs the reference): its output today is the committed fixture, byte for byte"""
    from oracle import realtime_fixture
    if not os.path.exists(realtime_fixture.HARNESS):
        pytest.skip("oracle/_ref/realtime_harness is not built (make -C oracle ref, where the reference is)")
    fresh = realtime_fixture.build()
    assert sorted(fresh) == sorted(ref.files)
    for k in sorted(fresh):
        a, b = np.ascontiguousarray(fresh[k]), ref[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
