"""Reference model of rt_temporal_accumulate and rt_denoise_var (test infrastructure, like tests/denoise_model.py).

numpy binary32 throughout: every operation one rounding, in the order include/raytrace_hip.h states, so the device's histories and frames are held to it bit for bit.
The four reprojection taps and the 25 taps of a pass are vectorised over the image; their order (the first valid tap wins; dy outer, dx inner) is the contract's."""
import numpy as np

import raytracinggpu_amd as rt
from .denoise_model import H3, _sqdiff, _term

F = np.float32


def lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def _dot(a, b):
    return (a[..., 0] * b[0] + a[..., 1] * b[1]) + a[..., 2] * b[2]


def camera_constants(W, camera=None, pose=None):
    """What the library derives from the previous camera: (O, bx, by, bz, cx, cy, b), all binary32.  pose: a CameraPose; else camera = (position, fov or None)."""
    if pose is not None:
        O = np.asarray(list(pose.position), np.float32)
        bx, by, bz = (np.asarray(v, np.float32) for v in rt.camera_basis(pose))
        fov = F(pose.fov)
        z = -F(W) / (F(2) * F(np.tan(np.float64(fov / F(2)))))
        return O, bx, by, bz, _dot(O, bx), _dot(O, by), _dot(O, bz) + z
    pos, fov = camera if camera is not None else ((0.0, 0.0, 55.0), None)
    fov = F(np.pi / 3) if fov is None else F(fov)
    z = -F(W) / (F(2) * F(np.tan(np.float64(fov / F(2)))))
    eye = np.eye(3, dtype=np.float32)
    return np.asarray(pos, np.float32), eye[0], eye[1], eye[2], F(0), F(0), z


def moved(aov, motion):
    """(P', N') of every pixel: the hit point and the normal taken to the previous frame by the pixel's object's motion record (motion None: themselves)."""
    N, ID, P = aov[0, ..., :3], aov[0, ..., 3], aov[1, ..., :3]
    if motion is None:
        return P, N
    m = np.asarray(motion, np.float32)[np.where(ID >= 0, ID, 0).astype(np.int64) & 15]          # [H, W, 12]
    Pm = np.stack([((m[..., 3 * r] * P[..., 0] + m[..., 3 * r + 1] * P[..., 1]) + m[..., 3 * r + 2] * P[..., 2]) + m[..., 9 + r] for r in range(3)], axis=-1)
    Nm = np.stack([(m[..., 3 * r] * N[..., 0] + m[..., 3 * r + 1] * N[..., 1]) + m[..., 3 * r + 2] * N[..., 2] for r in range(3)], axis=-1)
    return Pm, Nm


def project(Pm, W, H, camera=None, pose=None):
    """The previous camera's coordinates of the points Pm: (k, gx, gy); previous pixel (i, j)'s centre is gx = i + 0.5, gy = j + 0.5; k <= 0: behind the camera."""
    O, bx, by, bz, cx, cy, b = camera_constants(W, camera, pose)
    with np.errstate(all="ignore"):
        d = Pm - O
        k = b / _dot(d, bz)
        X = _dot(d, bx) * k - cx
        Y = _dot(d, by) * k - cy
        gx = X + F(W) / F(2)
        gy = F(H) / F(2) - Y
    assert gx.dtype == np.float32 and gy.dtype == np.float32 and k.dtype == np.float32
    return k, gx, gy


def accumulate(C, aov, prev_aov=None, prev_history=None, camera=None, pose=None, motion=None, mask=0, max_history=32, alpha_min=0.0, min_normal_dot=0.9,
               max_plane_dist=0.5, taps=None):
    """rt_temporal_accumulate -> the history [2, H, W, 4].  taps: an optional dict that receives `q` [H, W, 2] = the previous pixel (x, y) each pixel took its
    history from, (-1, -1) where it took none."""
    C = np.ascontiguousarray(C, np.float32)
    aov = np.ascontiguousarray(aov, np.float32)
    Hh, W = C.shape[:2]
    ID = aov[0, ..., 3]
    hit = ID != F(-1)
    l = lum(C)
    n = np.ones((Hh, W), np.float32)
    col = C[..., :3].copy()
    m1, m2 = l.copy(), l * l
    took = np.full((Hh, W, 2), -1, np.int64)
    with np.errstate(all="ignore"):
        if prev_aov is not None:
            pa = np.ascontiguousarray(prev_aov, np.float32)
            ph = np.ascontiguousarray(prev_history, np.float32)
            pN, pID, pP = pa[0, ..., :3], pa[0, ..., 3], pa[1, ..., :3]
            Pm, Nm = moved(aov, motion)
            k, gx, gy = project(Pm, W, Hh, camera, pose)
            idi = np.where(hit, ID, 0).astype(np.int64)
            masked = ((int(mask) >> (idi & 31)) & 1).astype(bool)
            cand = hit & ~masked & (k > 0) & (gx >= F(-1)) & (gx <= F(W)) & (gy >= F(-1)) & (gy <= F(Hh))
            gx, gy = np.where(cand, gx, F(0)), np.where(cand, gy, F(0))
            fx, fy = np.floor(gx), np.floor(gy)
            ix, iy = fx.astype(np.int64), fy.astype(np.int64)
            jx = np.where(gx - fx >= F(0.5), ix + 1, ix - 1)
            jy = np.where(gy - fy >= F(0.5), iy + 1, iy - 1)
            found = np.zeros((Hh, W), bool)
            mpd2 = F(max_plane_dist) * F(max_plane_dist)
            for t in range(4):
                qx, qy = (jx if t & 1 else ix), (jy if t & 2 else iy)
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < Hh)
                qxc, qyc = np.clip(qx, 0, W - 1), np.clip(qy, 0, Hh - 1)
                Nq, Pq = pN[qyc, qxc], pP[qyc, qxc]
                nd = (Nm[..., 0] * Nq[..., 0] + Nm[..., 1] * Nq[..., 1]) + Nm[..., 2] * Nq[..., 2]
                e = (Nm[..., 0] * (Pq[..., 0] - Pm[..., 0]) + Nm[..., 1] * (Pq[..., 1] - Pm[..., 1])) + Nm[..., 2] * (Pq[..., 2] - Pm[..., 2])
                valid = cand & ~found & inside & (pID[qyc, qxc] == ID) & (nd >= F(min_normal_dot)) & (e * e <= mpd2)
                H0, H1 = ph[0][qyc, qxc], ph[1][qyc, qxc]
                nn = np.minimum(H1[..., 2] + F(1), F(max_history))
                al = np.maximum(F(1) / nn, F(alpha_min))
                col = np.where(valid[..., None], H0[..., :3] + al[..., None] * (C[..., :3] - H0[..., :3]), col)
                m1 = np.where(valid, H1[..., 0] + al * (l - H1[..., 0]), m1)
                m2 = np.where(valid, H1[..., 1] + al * (l * l - H1[..., 1]), m2)
                n = np.where(valid, nn, n)
                took[valid] = np.stack([qx, qy], axis=-1)[valid]
                found |= valid
        var = np.maximum(F(0), m2 - m1 * m1)
        # the spatial estimate while the history is short: the 5 x 5 current-frame neighbours of the same object
        ys, xs = np.meshgrid(np.arange(Hh), np.arange(W), indexing="ij")
        s1, s2, cnt = (np.zeros((Hh, W), np.float32) for _ in range(3))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + dy, xs + dx
                inside = (qy >= 0) & (qy < Hh) & (qx >= 0) & (qx < W)
                qy, qx = np.clip(qy, 0, Hh - 1), np.clip(qx, 0, W - 1)
                ok = inside & (ID[qy, qx] == ID)
                lq = l[qy, qx]
                s1 = np.where(ok, s1 + lq, s1)
                s2 = np.where(ok, s2 + lq * lq, s2)
                cnt = np.where(ok, cnt + F(1), cnt)
        e1, e2 = s1 / cnt, s2 / cnt
        var = np.where(n < F(4), np.maximum(F(0), e2 - e1 * e1), var)
    out = np.zeros((2, Hh, W, 4), np.float32)
    out[0] = C
    out[0, ..., :3][hit] = col[hit]
    out[1][hit] = np.stack([m1, m2, n, var], axis=-1)[hit]
    if taps is not None:
        took[~hit] = -1
        taps["q"] = took
    assert out.dtype == np.float32
    return out


def denoise_var_pass(C, V, aov, s, k_normal, k_position, k_albedo, k_sigma, var_floor):
    """One pass with step s over colour C [H, W, 4] and variance V [H, W] -> (colour, variance)."""
    C = np.ascontiguousarray(C, np.float32)
    V = np.ascontiguousarray(V, np.float32)
    aov = np.ascontiguousarray(aov, np.float32)
    Hh, W = C.shape[:2]
    N, ID, P, A = aov[0, ..., :3], aov[0, ..., 3], aov[1, ..., :3], aov[2, ..., :3]
    ys, xs = np.meshgrid(np.arange(Hh), np.arange(W), indexing="ij")
    S = np.zeros((Hh, W, 3), np.float32)
    Wt = np.zeros((Hh, W), np.float32)
    Sv = np.zeros((Hh, W), np.float32)
    L = lum(C)
    with np.errstate(all="ignore"):
        D = F(k_sigma) * V + F(var_floor)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + dy * s, xs + dx * s
                inside = (qy >= 0) & (qy < Hh) & (qx >= 0) & (qx < W)
                qy, qx = np.clip(qy, 0, Hh - 1), np.clip(qx, 0, W - 1)
                ok = inside & (ID[qy, qx] == ID)
                w = np.full((Hh, W), H3[abs(dy)] * H3[abs(dx)], np.float32)
                t = _term(_sqdiff(N, N[qy, qx]), k_normal)
                if t is not None:
                    w = w * t
                if F(k_position) != 0:
                    Pq = P[qy, qx]
                    e = (N[..., 0] * (Pq[..., 0] - P[..., 0]) + N[..., 1] * (Pq[..., 1] - P[..., 1])) + N[..., 2] * (Pq[..., 2] - P[..., 2])
                    w = w * _term(e * e, k_position)
                t = _term(_sqdiff(A, A[qy, qx]), k_albedo)
                if t is not None:
                    w = w * t
                dl = L - L[qy, qx]
                dl2 = dl * dl
                w = np.where(dl2 == 0, w, w * np.maximum(F(0), F(1) - dl2 / D))          # equal luminance: the term is exactly 1
                take = ok & (w > 0)                                    # False for a NaN weight
                Cq = C[qy, qx, :3]
                S = np.where(take[..., None], S + w[..., None] * Cq, S)
                Wt = np.where(take, Wt + w, Wt)
                Sv = np.where(take, Sv + (w * w) * V[qy, qx], Sv)
        rgb = S / Wt[..., None]
        vo = Sv / (Wt * Wt)
    out = C.copy()
    hit = ID != F(-1)
    out[hit, :3] = rgb[hit]
    Vo = V.copy()
    Vo[hit] = vo[hit]
    assert out.dtype == np.float32 and Vo.dtype == np.float32
    return out, Vo


def denoise_var(history, aov, n_passes, k_normal, k_position, k_albedo, k_sigma, var_floor):
    """rt_denoise_var: pass k = 0 .. n_passes - 1 with step 2^k over history plane 0, the variance starting as .w of history plane 1 -> the filtered colour."""
    assert 1 <= n_passes <= 8
    history = np.ascontiguousarray(history, np.float32)
    out, V = history[0], history[1, ..., 3]
    for k in range(n_passes):
        out, V = denoise_var_pass(out, V, aov, 1 << k, k_normal, k_position, k_albedo, k_sigma, var_floor)
    return out
