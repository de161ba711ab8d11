"""TEST INFRASTRUCTURE -- the inputs of tests/golden/ref_realtime.npz and the run of oracle/_ref/realtime_harness that answers them.

build() -> {name: array}: every input below (seeded, so the same on every run) and what the reference's own device code -- Camera::rotate, KernelLaunch,
TriangleMesh::get_smooth_normal, transform, MoveLightSource, MoveObject of realtime_render.cu, run as host functions by oracle/realtime_harness.cpp --
makes of it.  `python oracle/make_golden.py realtime` stores it; tests/test_realtime_pinned.py re-runs it where the binary exists and compares.
Arrays only; no reference text.
"""
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HARNESS = os.path.join(HERE, "_ref", "realtime_harness")
F = np.float32
PI = np.pi

FOVS = np.array([PI / 2, PI / 3, 1.0, 0.7], F)                         # realtime's own pov, this project's default, two more
# (C, yaw, pitch): the launcher's default; two oblique ones; |yaw| > 2 pi.  Every C != 0; all four keep the patch below in view.
POSES = np.array([[0, 0, 55, 0, 0.3], [12, -4, 60, 0.25, -0.2], [-15, 8, 48, -0.35, 0.15], [3.5, 2.25, 52, 6.5, -0.05]], F)
POSE_STEEP = np.array([1, 2, 3, -2.0, PI / 2], F)                      # looking straight down: rays only
SIGMA = F(0.2)                                                         # KernelLaunch's own (realtime:1123)


def basis_inputs(rng):
    hp = F(PI / 2)
    rows = [(0.0, 0.3), (0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0), (0.0, hp), (0.0, -hp), (1.0, hp), (-2.5, -hp), (0.3, np.nextafter(hp, F(0))),
            (0.3, np.nextafter(hp, F(2))), (7.0, 0.1), (-6.5, -0.2), (100.0, 1.0), (-1e4, 0.5), (1e-8, 1e-8), (-1e-20, 1e-30), (1e-45, -1e-45), (1e-3, -1e-3),
            (PI, 0.0), (-PI, PI), (PI / 2, 0.25), (-PI / 2, -0.25), (2 * PI, 2 * PI), (0.5, 3.0), (0.5, -3.0)]
    rows += [tuple(p[3:5]) for p in POSES] + [tuple(POSE_STEEP[3:5])]
    more = np.stack([rng.uniform(-7, 7, 200 - len(rows)), rng.uniform(-1.7, 1.7, 200 - len(rows))], 1)
    return np.concatenate([np.array(rows, F), more.astype(F)])


def ray_cases():
    """rows of (W, H, fov, Cx, Cy, Cz, yaw, pitch): 16 x 12 at pose p with fovs p and p + 1 (every fov at two poses), then 13 x 7 at pose p with fov p + 2 and
    at the steep pose"""
    rows = [[16, 12, FOVS[(k + d) % 4], *p] for k, p in enumerate(POSES) for d in (0, 1)]
    rows += [[13, 7, FOVS[(k + 2) % 4], *p] for k, p in enumerate(POSES)] + [[13, 7, FOVS[1], *POSE_STEEP]]
    return np.array(rows, F)


def jitter_pairs(rng):
    """(r1, r2): r1 = 1 makes the jitter exactly +-0; then eight pairs with the edges of curand_uniform's range (0, 1]"""
    fixed = [(1.0, 0.3), (2.0 ** -24, 0.25), (0.5, 0.5), (0.9, 1.0)]
    return np.concatenate([np.array(fixed, F), rng.uniform(2.0 ** -24, 1.0, (5, 2)).astype(F)])


def patch(rng):
    """a 2 x 2 grid of quads (8 triangles, 9 vertices) across z ~ 120, where the rays of POSES go: KernelLaunch adds the camera's POSITION to the direction
    (realtime:1115), so at 16 x 12 every ray leaves C roughly along C itself.  Pose 0 looks at the middle vertex, the others at other quads.  x and y are dyadic so
    that the edge cases below are exact, and z is whole for the same reason.  11 normals, non-unit, and each triangle corner picks its own: mutually inconsistent."""
    gx, gy = np.array([-64.0, 0.0, 48.0]), np.array([-32.0, 4.0, 40.0])
    verts = np.array([[x, y, 0] for y in gy for x in gx], np.float64)
    verts[:, 2] = 120 + rng.integers(-6, 7, 9)
    tris = []
    for j in range(2):
        for i in range(2):
            a = j * 3 + i
            tris += [[a, a + 1, a + 4], [a, a + 4, a + 3]]
    normals = rng.normal(size=(11, 3)) * 0.5 + [0, 0, -1]
    normals *= rng.uniform(0.3, 3.0, (11, 1))
    nidx = rng.integers(0, 11, (8, 3))
    return verts.astype(F), normals.astype(F), np.concatenate([np.array(tris), nidx], 1).astype(np.int32)


def edge_rays(verts, tris):
    """per triangle: through vertex A (beta = gamma = 0), through the middle of AB (gamma = 0) and of AC (beta = 0), along the dyadic direction (1/4, 1/8, 1) from
    dyadic origins: with the patch's whole coordinates every product in get_smooth_normal's numerators is exact in binary32, so the zeros are exact (the direction is
    not of unit length: the expressions do not ask for it).  Then a ray that grazes the triangle's plane through its centroid (dot(u, N) tiny)."""
    rows = []
    v = verts.astype(np.float64)
    d0 = np.array([0.25, 0.125, 1.0])
    for t in tris:
        A, B, C = v[t[0]], v[t[1]], v[t[2]]
        for P in (A, (A + B) / 2, (A + C) / 2):
            rows.append([*(P - 56 * d0), *d0])
        N = np.cross(B - A, C - A); N /= np.linalg.norm(N)
        d = (B - A) / np.linalg.norm(B - A) - 1e-6 * N
        d /= np.linalg.norm(d)
        O = (A + B + C) / 3 - 300 * d
        rows.append([*O, *d])
    return np.array(rows, F)


def rotation(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]); Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (Rz @ Ry @ Rx).reshape(9)


PATCH_TRANSFORM = np.concatenate([rotation(0.05, -0.04, 0.1), [5, -3, -10]]).astype(F)      # keeps the patch in every frame of POSES


def transform_inputs(rng):
    verts = rng.uniform(-40, 40, (37, 3)); verts[:5] *= 1e4; verts[5] = 0; verts[6] = [-0.0, 1e-40, 1]
    normals = rng.normal(size=(41, 3)); normals[0] = [0, 0, 1]; normals[1] = 0
    ident = np.array([1, -0.0, 0, -0.0, 1, -0.0, 0, 0, 1.0])
    cases = [np.concatenate([rotation(0.3, -1.1, 2.0), [1.5, -2.25, 7]]),
             np.concatenate([rng.normal(size=9) * 2, [0.1, 0.2, 0.3]]),                      # not orthogonal
             np.concatenate([ident, [-0.0, 0.0, -0.0]]),
             np.concatenate([ident, [1e7, -3e6, 12345.678]]),                                # translations that round the sums
             np.concatenate([rotation(-2.0, 0.4, 0.01), [16777216.0, 1e-3, -65536.5]]),
             PATCH_TRANSFORM]
    return verts.astype(F), normals.astype(F), np.array(cases, F)


def progressive_inputs(rng):
    """1536 display values c (512 pixels x 3 channels) around every 8-bit code boundary of (unsigned char)min(powf(c, 1 / 2.2f), 255.), and the edges of
    binary32; frame number n then gets accumbuffer = fl(c * n)"""
    k = np.arange(1, 256, dtype=np.float64)
    b = (k ** 2.2).astype(F)
    d1 = np.nextafter(b, F(0)); d2 = np.nextafter(d1, F(0))
    u1 = np.nextafter(b, F(np.inf)); u2 = np.nextafter(u1, F(np.inf))
    vals = [d2, d1, b, u1, u2]
    special = np.array([0.0, -0.0, 1e-45, 1e-42, 1e-39, 1.1754944e-38, 1e-30, 0.5, 1.0, 196964.0, 196965.0, 2e5, 1e30, 3e38, np.inf, np.nan, -1.0, -np.inf, -1e-45], F)
    vals = np.concatenate(vals + [special])
    fill = np.exp(rng.uniform(np.log(1e-6), np.log(4e5), 1536 - len(vals))).astype(F)
    return np.concatenate([vals, fill]).astype(F).reshape(512, 3)


PROG_FRAMES = np.array([1, 2, 3, 7, 1000], np.int32)


def light_inputs(rng):
    """rows of (Lx, Ly, Lz, angular speed, dt)"""
    L = rng.uniform(-60, 60, (100, 3))
    L[0] = [0, 15, 40]                                                                       # KernelInit's light
    L[1] = [0, 20, 0]; L[2] = [-0.0, 20, 0]; L[3] = [0, 20, -0.0]; L[4] = [-0.0, -5, -0.0]   # on the axis
    L[5] = [-30, 10, 0]; L[6] = [-30, 10, -0.0]; L[7] = [-30, 10, 1e-30]; L[8] = [-30, 10, -1e-30]; L[9] = [-1e-3, 1, 1e-38]   # atan2f's branch cut
    L[10] = [25, 0, 0]; L[11] = [0, 3, -17]; L[12] = [1e20, 0, 1e20]; L[13] = [1e-25, 0, -1e-25]
    L[14:30, 0] = -np.abs(L[14:30, 0])
    speed = rng.choice([0.75, -2.0, 6.0, 2.5, 0.0, 4.0, 1e3], 100)
    dt = rng.choice([2e-2, 0.1, 0.5, 1 / 3, 0.04], 100)
    return np.concatenate([L, speed[:, None], dt[:, None]], 1).astype(F)


LIGHT_CHAIN = np.array([[0, 15, 40, 2.5, 2e-2]], F)                                          # 20 steps from KernelInit's light at MoveLightSource's own dt
LIGHT_CHAIN_STEPS = 20


def object_inputs(rng):
    """rows of (C, v, dt)"""
    rows = np.concatenate([rng.uniform(-30, 30, (40, 3)), rng.uniform(-25, 25, (40, 3)), rng.choice([0.2, 0.25, 1 / 3, 0.125], (40, 1))], 1)
    rows[0] = [0, -1000, 0, 0, -0.6, 0, 0.2]                                                 # the floor sinks at MoveObject's own dt
    rows[1] = [0, 0, 0, -0.0, 0.0, -0.0, 0.2]; rows[2] = [-0.0, -0.0, -0.0, -0.0, 1, -0.0, 0.2]
    rows[3] = [1e7, -1e7, 16777216, 1.5, 0.75, 1, 0.2]                                       # the sum rounds
    rows[4] = [20, 10, -8, 0.1, 0.7, 1e-20, 1 / 3]                                           # the product rounds
    return rows.astype(F)


def run(args):
    r = subprocess.run([HARNESS] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"realtime_harness {args[0]} failed with {r.returncode}: {r.stdout}")


def build():
    rng = np.random.default_rng(20261019)
    tmp = tempfile.mkdtemp(prefix="rt_realtime_")
    out = {}

    def put(name, a):
        path = os.path.join(tmp, name)
        np.ascontiguousarray(a).tofile(path)
        return path

    def get(name, shape, dtype="<f4"):
        return np.fromfile(os.path.join(tmp, name), dtype=dtype).reshape(shape)

    try:
        # camera basis
        out["basis_in"] = basis_inputs(rng)
        run(["basis", put("basis_in", out["basis_in"]), os.path.join(tmp, "basis_out")])
        out["basis_out"] = get("basis_out", (-1, 3, 3))
        # camera rays
        cases, jit = ray_cases(), jitter_pairs(rng)
        out["ray_cases"], out["ray_jitter"], out["ray_sigma"] = cases, jit, np.array([SIGMA], F)
        run(["rays", put("cases", cases), put("jit", jit), os.path.join(tmp, "r")])
        tans = get("r.tan.f32", (-1, 2))
        out["ray_tan"], out["ray_z"] = tans[:, 0].copy(), tans[:, 1].copy()
        rays = get("r.rays.f32", (-1, 6))
        at = 0
        for k, c in enumerate(cases):
            n = len(jit) * int(c[0]) * int(c[1])
            out[f"rays_{k:02d}"] = rays[at:at + n].reshape(len(jit), int(c[1]), int(c[0]), 6).copy()
            at += n
        assert at == len(rays)
        # progressive output
        disp = progressive_inputs(rng)
        out["prog_frames"] = PROG_FRAMES
        for n in PROG_FRAMES:
            with np.errstate(over="ignore", invalid="ignore"):
                acc = (disp.astype(np.float64) * float(n)).astype(F)
            run(["prog", put("acc", acc), int(n), os.path.join(tmp, "p")])
            out[f"prog_{n}_accum_in"] = acc
            out[f"prog_{n}_accum_out"] = get("p.accum.f32", (-1, 3))
            out[f"prog_{n}_display"] = get("p.disp.f32", (-1, 3))
            out[f"prog_{n}_bytes"] = get("p.bytes.u8", (-1, 4), np.uint8)
        # transform
        tv, tn, tc = transform_inputs(rng)
        out["transform_verts"], out["transform_normals"], out["transform_cases"] = tv, tn, tc
        run(["transform", put("tv", tv), put("tn", tn), put("tc", tc), os.path.join(tmp, "t")])
        out["transform_verts_out"] = get("t.v.f32", (len(tc), -1, 3))
        out["transform_normals_out"] = get("t.n.f32", (len(tc), -1, 3))
        # smooth normals: the patch as it is, and after the reference's own transform
        pv, pn, pt = patch(rng)
        out["patch_verts"], out["patch_normals"], out["patch_tris"], out["patch_transform"] = pv, pn, pt, PATCH_TRANSFORM
        run(["transform", put("pv", pv), put("pn", pn), put("pc", PATCH_TRANSFORM), os.path.join(tmp, "pt")])
        out["patch_verts_moved"], out["patch_normals_moved"] = get("pt.v.f32", (-1, 3)), get("pt.n.f32", (-1, 3))
        smooth_cases = np.array([0, 3, 4, 6], np.int32)      # 16 x 12, each pose once, at a fov whose run-time tangent is the correctly rounded one: the jitter-free rays
        out["smooth_cases"] = smooth_cases
        srays = np.concatenate([out[f"rays_{k:02d}"][0].reshape(-1, 6) for k in smooth_cases])
        erays = edge_rays(pv, pt)
        out["smooth_edge_rays"] = erays
        tri_path = put("pt_i", pt)
        for tag, v, n in (("", pv, pn), ("_moved", out["patch_verts_moved"], out["patch_normals_moved"])):
            run(["smooth", put("sv", v), put("sn", n), tri_path, put("sr", srays), os.path.join(tmp, "s")])
            out["smooth_N" + tag] = get("s", (len(smooth_cases), 12, 16, len(pt), 3))
        run(["smooth", put("sv", pv), put("sn", pn), tri_path, put("sr", erays), os.path.join(tmp, "s")])
        out["smooth_edge_N"] = get("s", (len(erays), len(pt), 3))
        # motions
        out["light_in"] = light_inputs(rng)
        run(["light", put("li", out["light_in"]), 0, os.path.join(tmp, "lo")])
        out["light_out"] = get("lo", (-1, 3))
        out["light_chain_in"] = LIGHT_CHAIN
        run(["light", put("lc", LIGHT_CHAIN), LIGHT_CHAIN_STEPS, os.path.join(tmp, "lco")])
        out["light_chain_out"] = get("lco", (LIGHT_CHAIN_STEPS, 3))
        out["object_in"] = object_inputs(rng)
        run(["object", put("oi", out["object_in"]), os.path.join(tmp, "oo")])
        out["object_out"] = get("oo", (-1, 3))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return out


def save(path, arrays):
    """an .npz (deflated, as numpy.savez_compressed writes it) whose bytes depend on the arrays alone: every member carries the same fixed date"""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.ascontiguousarray(arrays[name]), allow_pickle=False)
