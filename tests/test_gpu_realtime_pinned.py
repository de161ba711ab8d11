"""The device's posed camera, smooth normals, mesh transform, progressive output and light motion against tests/golden/ref_realtime.npz: what the reference's own
realtime_render.cu computes (its device code run as host functions, oracle/realtime_harness.cpp).  -m gpu.  Every frame is at most 16 x 12.

The smooth-normal tests hold the device to the reference DIRECTLY, not through the oracle: the fixture has get_smooth_normal of every recorded camera ray against every
triangle of an 8-triangle patch, and the AOV normal of a pixel must be, bit for bit, the fixture's for the triangle that pixel's ray hits.  Which triangle that is comes
from the geometry in binary64; a pixel whose ray passes within 1e-6 (barycentric) of an edge may show either neighbour's normal.  Those rays were recorded at fovs whose
run-time tangent is the correctly rounded one, so the one recorded deviation (DESIGN.md "Numerics", tests/test_realtime_pinned.py) does not enter."""
import numpy as np
import pytest

import raytracinggpu_amd as rt

from .conftest import load_golden

pytestmark = pytest.mark.gpu

SHELL = [((0.0, 0.0, 0.0), 5000.0, (0.5, 0.5, 0.5))]                  # one sphere around everything: every ray that leaves the patch still hits something
PATCH_SLOT = 1
INTENSITY = float(np.float32(3e10))                                   # KernelInit's (realtime:1024)


@pytest.fixture(scope="module")
def ctx():
    c_ = rt.Context(0)
    yield c_
    c_.close()


@pytest.fixture(scope="module")
def ref():
    return load_golden("ref_realtime.npz")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pose_of(case):
    return rt.make_pose(tuple(float(x) for x in case[3:6]), float(case[6]), float(case[7]), case[2])


def params(case, **kw):
    return rt.make_params(int(case[0]), int(case[1]), 1, 0, **dict(rt.scenes.CPU_LAUNCHER, **kw))


def upload_patch(ctx, oracle, ref):
    """the patch, in the triangle order and with the tree of the oracle's buildBVH, and its normals; -> to_fixture[k] = the fixture's index of uploaded triangle k"""
    tris = ref["patch_tris"]
    m = oracle.Mesh.from_arrays(ref["patch_verts"], tris[:, :3]).build_bvh()
    key = {tuple(t[:3]): i for i, t in enumerate(tris)}
    to_fixture = np.array([key[tuple(t)] for t in m.triangles])
    ctx.scene_upload(SHELL, dict(vertices=ref["patch_verts"], indices=m.triangles, bvh_arr10=m.bvh_array(), albedo=(0.25, 0.25, 0.25), object_slot=PATCH_SLOT))
    ctx.mesh_set_normals(ref["patch_normals"], tris[to_fixture, 3:])
    return to_fixture


def candidates(verts, tris, ray, tol=1e-6):
    """in binary64: the triangle the ray hits first, and with it every triangle whose edge the ray passes within tol of at no greater distance + tol"""
    O, u = ray[:3].astype(np.float64), ray[3:].astype(np.float64)
    found = []
    for k, t in enumerate(tris):
        A, B, C = (verts[i].astype(np.float64) for i in t[:3])
        e1, e2 = B - A, C - A
        N = np.cross(e1, e2)
        den = u @ N
        if den == 0:
            continue
        beta, gamma = e2 @ np.cross(A - O, u) / den, -(e1 @ np.cross(A - O, u)) / den
        dist = (A - O) @ N / den
        if min(beta, gamma, 1 - beta - gamma) >= -tol and dist > 0:
            found.append((dist, k))
    if not found:
        return []
    nearest = min(found)[0]
    return [k for dist, k in found if dist <= nearest * (1 + 1e-6)]


def check_patch_normals(ctx, ref, verts, exp_N, what):
    """AOV plane 0 at every smooth-normal pose: a patch pixel's normal is the fixture's for its triangle -> the number of pixels held"""
    held = 0
    for s, k in enumerate(ref["smooth_cases"]):
        case = ref["ray_cases"][k]
        got = ctx.render_aov(params(case), pose=pose_of(case))
        rays = ref[f"rays_{k:02d}"][0]                                 # r1 = 1: the pixel-centre rays, as the reference's kernel built them
        on_patch = got[0, ..., 3] == PATCH_SLOT
        for y, x in zip(*np.nonzero(on_patch)):
            cand = candidates(verts, ref["patch_tris"], rays[y, x])
            assert cand, f"{what}, case {k}, pixel ({x}, {y}): the device hit the patch, binary64 geometry does not"
            ok = [np.array_equal(bits(got[0, y, x, :3]), bits(exp_N[s, y, x, t])) for t in cand]
            assert any(ok), f"{what}, case {k}, pixel ({x}, {y}), triangle {cand}: device {got[0, y, x, :3]!r}, reference {[exp_N[s, y, x, t] for t in cand]!r}"
            held += 1
        # and no patch pixel is lost: where binary64 sees a clear hit, the device reports the patch
        for y in range(rays.shape[0]):
            for x in range(rays.shape[1]):
                if not on_patch[y, x]:
                    assert not candidates(verts, ref["patch_tris"], rays[y, x], tol=-1e-6), f"{what}, case {k}, pixel ({x}, {y}): a clear hit the device missed"
    return held


def test_smooth_normals_equal_the_references(ctx, oracle, ref):
    """smooth_normal and posed_dir on the device: rt_render_aov of the patch under each recorded pose"""
    upload_patch(ctx, oracle, ref)
    held = check_patch_normals(ctx, ref, ref["patch_verts"], ref["smooth_N"], "patch")
    total = len(ref["smooth_cases"]) * 12 * 16
    print(f"smooth normals: {held} of {total} pixels on the patch")
    assert held >= 0.8 * total


@pytest.mark.parametrize("per_mesh", [False, True])
def test_smooth_normals_after_transform(ctx, oracle, ref, per_mesh):
    """rt_mesh_transform / rt_mesh_transform_of on the patch with normals: the AOV normals are the reference's get_smooth_normal over the vertices and normals its
    own transform kernel produced -- the kernel ADDS the translation to the normals, and so must the device"""
    upload_patch(ctx, oracle, ref)
    T = ref["patch_transform"]
    ctx.mesh_transform(T[:9], T[9:], object_slot=PATCH_SLOT if per_mesh else None)
    held = check_patch_normals(ctx, ref, ref["patch_verts_moved"], ref["smooth_N_moved"], "moved patch")
    total = len(ref["smooth_cases"]) * 12 * 16
    assert held >= 0.8 * total
    assert not np.array_equal(bits(ref["smooth_N_moved"]), bits(ref["smooth_N"]))


def test_posed_rendering_at_every_recorded_pose(ctx, oracle, ref):
    """rt_render_pose on the walls and one sphere at every recorded (frame, pose, fov): the oracle's frame word for word (direct lighting, no jitter: nothing but the
    camera, the intersections and the shading, all of them pinned)"""
    spheres = rt.scenes.spheres("cpu") + [((4.0, -3.0, -6.0), 9.0, (0.75, 0.5, 0.25))]
    ctx.scene_upload(spheres)
    sc = oracle.Scene.preset("spheres")
    sc.add_sphere(*spheres[-1])
    frames = []
    for k, case in enumerate(ref["ray_cases"]):
        W, H = int(case[0]), int(case[1])
        got = ctx.render_pose(params(case), pose_of(case))
        exp, _, _ = sc.render(W, H, 1, 0, sigma=0.0, fov=case[2], cam=tuple(float(x) for x in case[3:6]), pose=(float(case[6]), float(case[7])), want_rgb8=False,
                              **{k_: v for k_, v in rt.scenes.CPU_LAUNCHER.items() if k_ in ("eps", "tri_tmin")})
        assert np.array_equal(bits(got), bits(exp)), f"case {k} {case!r}: {int((bits(got) != bits(exp)).sum())} words differ"
        frames.append(got[..., :3].tobytes())
    assert len(set(frames)) == len(frames)                            # every pose and fov gives its own picture


def test_progressive_output(ctx, oracle, ref):
    """rt_progressive_frame over three frames at 16 x 12: display values and bytes are realtime:1136-1147 (or_progressive_accumulate, held to the fixture by
    tests/test_realtime_pinned.py) applied to the frames rt_render_pose gives for the same seeds.  Walls of mixed colours under a dim light: the bytes spread over
    the middle of the 8-bit range instead of saturating at 0 and 255."""
    case = ref["ray_cases"][0]
    W, H = int(case[0]), int(case[1])
    albedos = [(0.8, 0.5, 0.3), (0.3, 0.6, 0.9), (0.9, 0.2, 0.4), (0.5, 0.9, 0.6), (0.7, 0.7, 0.2), (0.6, 0.35, 0.85)]
    spheres = [(c, r, a) for (c, r, _), a in zip(rt.scenes.spheres("cpu"), albedos)] + [((0.0, 4.0, 56.0), 3.0, (0.9, 0.8, 0.7))]
    ctx.scene_upload(spheres, light=((-10.0, 20.0, 40.0), 2e9))
    pose = pose_of(case)
    kw = dict(rt.scenes.CPU_LAUNCHER, sigma=0.2)
    ctx.progressive_reset()
    accum = np.zeros((H, W, 4), np.float32)
    for frame in (1, 2, 3):
        one = ctx.render_pose(rt.make_params(W, H, 2, 2, **dict(kw, seed=oracle.wang_hash(frame))), pose)
        disp, rgb8 = ctx.progressive_frame(rt.make_params(W, H, 2, 2, **kw), pose)
        assert ctx.progressive_frames() == frame
        edisp, ergb8 = oracle.progressive_accumulate(accum, one, frame)
        assert np.array_equal(bits(disp), bits(edisp)), f"frame {frame}: display"
        assert np.array_equal(rgb8, ergb8), f"frame {frame}: bytes differ at {np.argwhere(rgb8 != ergb8)[:4].tolist()}"
        print(f"frame {frame}: {len(np.unique(rgb8))} byte values, {rgb8.min()} to {rgb8.max()}")
        assert len(np.unique(rgb8)) > 32 and 0 < rgb8.min() and rgb8.max() < 255


def test_light_motion_chain(ctx, ref):
    """rt_scene_move_light 20 times from KernelInit's light: rt_scene_get_light after every step is MoveLightSource's own result"""
    row = ref["light_chain_in"][0]
    ctx.scene_upload(rt.scenes.spheres("cpu"), light=(tuple(float(x) for x in row[:3]), INTENSITY))
    for k, exp in enumerate(ref["light_chain_out"]):
        ctx.move_light(float(row[3]), float(row[4]))
        pos, inten = ctx.light()
        assert np.array_equal(bits(np.array(pos, np.float32)), bits(exp)), f"step {k}: {pos!r}, reference {exp!r}"
        assert inten == INTENSITY
