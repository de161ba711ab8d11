"""Reference model of rt_render_aov_motion's previous-frame planes (test infrastructure, like tests/temporal_model.py).

numpy binary32 throughout, every operation one rounding in the order include/raytrace_hip.h states.  Built from what existed before the entry: the pixel-centre camera
rays of tests/denoise_model.py, the CPU oracle's Scene.intersect_all for the winning object, its point and its normal, Mesh.intersect_tri for the triangle, the
barycentrics and triangle records of tests/texture_model.py, and tests/temporal_model.py's `moved` for the rigid branch.  Nothing here is code under test."""
import numpy as np

from . import denoise_model as dm
from . import temporal_model as tm
from . import texture_model as xm

F = np.float32
MISS, SNAPSHOT, RIGID, STATIC = 0, 1, 2, 3                             # the branch a pixel took


def trace(scene, W, H, meshes=None, tri_tmin=1e-4, **camera):
    """The first hit of every pixel-centre camera ray (camera: denoise_model.camera_rays' keywords) -> dict O [3], u, P, N [n_rows, W, 3], id [n_rows, W] (-1: a miss)
    and tri [n_rows, W]: for a hit on an object of meshes = {object id: oracle Mesh in the scene}, the triangle's position in that mesh's CURRENT order, else -1."""
    O, u = dm.camera_rays(W, H, **camera)
    n = u.shape[0]
    out = dict(O=O, u=u, P=np.zeros((n, W, 3), np.float32), N=np.zeros((n, W, 3), np.float32), id=np.full((n, W), -1, np.int64), tri=np.full((n, W), -1, np.int64))
    for r in range(n):
        for c in range(W):
            hit, oid, P, N = scene.intersect_all(O, u[r, c], tri_tmin)
            if not hit:
                continue
            out["P"][r, c], out["N"][r, c], out["id"][r, c] = P, N, oid
            if meshes and oid in meshes:
                found, _, _, tri = meshes[oid].intersect_tri(O, u[r, c], tri_tmin)
                assert found and tri >= 0
                out["tri"][r, c] = tri
    return out


def planes(tr, albedos=None):
    """planes 0 and 1 of rt_render_aov from a trace (and plane 2 where albedos[id] is given, else zeros) -> [3, n_rows, W, 4]"""
    hit = tr["id"] >= 0
    out = np.zeros((3,) + tr["id"].shape + (4,), np.float32)
    out[0, ..., :3], out[0, ..., 3] = tr["N"], tr["id"]
    out[1, ..., :3], out[1, ..., 3] = tr["P"], hit
    if albedos is not None:
        out[2, ..., :3][hit] = np.asarray(albedos, np.float32)[tr["id"][hit]]
    return out


def _normalize(v):
    with np.errstate(all="ignore"):
        n = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
        return v / n[..., None]


def barycentric_point(alpha, beta, gamma, A, B, Cc):
    """(alpha A + beta B) + gamma C per component; dtype follows the inputs (binary32 for the model, binary64 for its check)"""
    return (alpha[..., None] * A + beta[..., None] * B) + gamma[..., None] * Cc


def previous_planes(tr, snapshots=None, motion=None, branch=None):
    """out_prev of rt_render_aov_motion -> [2, n_rows, W, 4].  snapshots = {object id: dict(mesh=the oracle Mesh of the CURRENT shape (the one trace was given),
    previous=[nv, 3] the vertices at the snapshot, smooth=the mesh shades with interpolated normals)}; motion: the [16, 12] table or None.  A snapshot takes precedence
    over the object's record.  branch: an optional dict that receives `of` [n_rows, W] (MISS / SNAPSHOT / RIGID / STATIC)."""
    snapshots = snapshots or {}
    ids = tr["id"]
    hit = ids >= 0
    cur = planes(tr)
    Pm, Nm = tm.moved(cur, motion)                                     # the rigid branch (motion None: P, N themselves)
    Pp, Np_ = Pm.copy(), Nm.copy()
    of = np.where(hit, RIGID if motion is not None else STATIC, MISS).astype(np.int8)
    for oid, s in snapshots.items():
        on = ids == oid
        if not on.any():
            continue
        mesh = s["mesh"]
        tris = np.asarray(mesh.triangles, np.int64)
        tri = tr["tri"][on]
        assert (tri >= 0).all(), "trace() was not given this mesh"
        A, e1, e2, Nt = (x[tri] for x in xm.triangle_records(mesh.vertices, tris))
        alpha, beta, gamma = xm.barycentrics(A, e1, e2, Nt, tr["O"], tr["u"][on])
        vp = np.asarray(s["previous"], np.float32)
        Ap, Bp, Cp = vp[tris[tri, 0]], vp[tris[tri, 1]], vp[tris[tri, 2]]
        with np.errstate(all="ignore"):
            Pp[on] = barycentric_point(alpha, beta, gamma, Ap, Bp, Cp)
            Np_[on] = tr["N"][on] if s.get("smooth") else _normalize(xm._cross(Bp - Ap, Cp - Ap))
        of[on] = SNAPSHOT
    out = np.zeros((2,) + ids.shape + (4,), np.float32)
    out[0, ..., 3] = -1
    out[0, ..., :3][hit], out[0, ..., 3][hit] = Np_[hit], ids[hit]
    out[1, ..., :3][hit], out[1, ..., 3][hit] = Pp[hit], 1
    if branch is not None:
        branch["of"] = of
    assert out.dtype == np.float32
    return out


def sine_deform(v, frame, amplitude=3.0, wavelength=20.0, rate=0.5):
    """v.x += A sin(2 pi v.y / wavelength + rate frame): the deformation of the sequences (binary64 inside, narrowed once)"""
    v = np.asarray(v, np.float32)
    out = v.copy()
    out[:, 0] = (v[:, 0].astype(np.float64) + amplitude * np.sin(2 * np.pi * v[:, 1].astype(np.float64) / wavelength + rate * frame)).astype(np.float32)
    return out
