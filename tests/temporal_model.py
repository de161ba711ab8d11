"""Reference model of rt_temporal_accumulate and rt_denoise_var (test infrastructure, like tests/denoise_model.py).

numpy binary32 throughout: every operation one rounding, in the order include/raytrace_hip.h states, so the device's histories and frames are held to it bit for bit.
The four reprojection taps and the 25 taps of a pass are vectorised over the image; their order (the first valid tap wins; dy outer, dx inner) is the contract's.  min and max are minNum and maxNum (np.fmin, np.fmax), as the header states."""
import numpy as np

import raytracinggpu_amd as rt
from .denoise_model import atrous_pass, div_in_range, lum, luminance_term

F = np.float32


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
               max_plane_dist=0.5, taps=None, stats=None):
    """rt_temporal_accumulate -> the history [2, H, W, 4].  taps: an optional dict that receives `q` [H, W, 2] = the previous pixel (x, y) each pixel took its
    history from, (-1, -1) where it took none.  stats: an optional dict that receives how many pixels took each branch of the reprojection (the keys are listed in
    tests/synthetic_planes.py, REPROJECTION_MINIMUMS) and `n`, the history lengths written, as {value: pixels}."""
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
    st = {} if stats is None else stats
    fast = np.ones((Hh, W), bool)                                      # every quotient of the pixel took rt_div.h's shared sequence
    with np.errstate(all="ignore"):
        if prev_aov is not None:
            pa = np.ascontiguousarray(prev_aov, np.float32)
            ph = np.ascontiguousarray(prev_history, np.float32)
            pN, pID, pP = pa[0, ..., :3], pa[0, ..., 3], pa[1, ..., :3]
            Pm, Nm = moved(aov, motion)
            k, gx, gy = project(Pm, W, Hh, camera, pose)
            O, _, _, bz, _, _, b = camera_constants(W, camera, pose)
            idi = np.where(hit, ID, 0).astype(np.int64)
            masked = ((int(mask) >> (idi & 31)) & 1).astype(bool)
            live = hit & ~masked
            bounds = [gx >= F(-1), gx <= F(W), gy >= F(-1), gy <= F(Hh)]
            cand = live & (k > 0) & bounds[0] & bounds[1] & bounds[2] & bounds[3]
            fast &= ~live | (div_in_range(b) & div_in_range(_dot(Pm - O, bz)))
            st["k_not_positive"] = int((live & ~(k > 0)).sum())
            for i, name in enumerate(("gx_below", "gx_above", "gy_below", "gy_above")):
                st[name + "_alone"] = int((live & (k > 0) & ~bounds[i] & np.logical_and.reduce([bounds[j] for j in range(4) if j != i])).sum())
            st["gx_in_minus1_0"] = int((cand & (gx < F(0))).sum())
            st["gx_in_wminus1_w"] = int((cand & (gx > F(W - 1))).sum())
            gx, gy = np.where(cand, gx, F(0)), np.where(cand, gy, F(0))
            fx, fy = np.floor(gx), np.floor(gy)
            ix, iy = fx.astype(np.int64), fy.astype(np.int64)
            st["half_x"], st["half_y"] = int((cand & (gx - fx == F(0.5))).sum()), int((cand & (gy - fy == F(0.5))).sum())
            jx = np.where(gx - fx >= F(0.5), ix + 1, ix - 1)
            jy = np.where(gy - fy >= F(0.5), iy + 1, iy - 1)
            found = np.zeros((Hh, W), bool)
            first_outside = np.zeros((Hh, W), bool)
            alone = {name: np.zeros((Hh, W), bool) for name in ("id", "normal", "plane")}
            mpd2 = F(max_plane_dist) * F(max_plane_dist)
            for t in range(4):
                qx, qy = (jx if t & 1 else ix), (jy if t & 2 else iy)
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < Hh)
                qxc, qyc = np.clip(qx, 0, W - 1), np.clip(qy, 0, Hh - 1)
                Nq, Pq = pN[qyc, qxc], pP[qyc, qxc]
                nd = (Nm[..., 0] * Nq[..., 0] + Nm[..., 1] * Nq[..., 1]) + Nm[..., 2] * Nq[..., 2]
                e = (Nm[..., 0] * (Pq[..., 0] - Pm[..., 0]) + Nm[..., 1] * (Pq[..., 1] - Pm[..., 1])) + Nm[..., 2] * (Pq[..., 2] - Pm[..., 2])
                looked = cand & ~found & inside
                ok_id, ok_n, ok_p = pID[qyc, qxc] == ID, nd >= F(min_normal_dot), e * e <= mpd2
                valid = looked & ok_id & ok_n & ok_p
                alone["id"] |= looked & ~ok_id & ok_n & ok_p
                alone["normal"] |= looked & ok_id & ~ok_n & ok_p
                alone["plane"] |= looked & ok_id & ok_n & ~ok_p
                if t == 0:
                    first_outside = cand & ~inside
                H0, H1 = ph[0][qyc, qxc], ph[1][qyc, qxc]
                nn = np.fmin(H1[..., 2] + F(1), F(max_history))       # minNum and maxNum, as the kernel's fminf and fmaxf: a NaN n_q gives max_history
                al = np.fmax(F(1) / nn, F(alpha_min))
                fast &= ~valid | div_in_range(nn)
                col = np.where(valid[..., None], H0[..., :3] + al[..., None] * (C[..., :3] - H0[..., :3]), col)
                m1 = np.where(valid, H1[..., 0] + al * (l - H1[..., 0]), m1)
                m2 = np.where(valid, H1[..., 1] + al * (l * l - H1[..., 1]), m2)
                n = np.where(valid, nn, n)
                took[valid] = np.stack([qx, qy], axis=-1)[valid]
                st[f"tap{t}"] = int(valid.sum())
                st[f"alpha_is_alpha_min_tap{t}"] = int((valid & (F(1) / nn < F(alpha_min))).sum())
                found |= valid
            st["no_tap_valid"] = int((cand & ~found).sum())
            st["first_outside_later_inside"] = int((first_outside & found).sum())
            st["alpha_min_above"] = sum(st.pop(f"alpha_is_alpha_min_tap{t}") for t in range(4))
            st["alpha_min_below"] = int(found.sum()) - st["alpha_min_above"]
            st["reprojected"] = int(found.sum())
            for name, m in alone.items():
                st[name + "_alone"] = int(m.sum())
        var = np.fmax(F(0), m2 - m1 * m1)
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
        var = np.where(n < F(4), np.fmax(F(0), e2 - e1 * e1), var)
        fast &= ~(n < F(4)) | (div_in_range(s1) & div_in_range(s2))
    st["shared"], st["literal"] = int((fast & hit).sum()), int((~fast & hit).sum())
    vals, cts = np.unique(n[hit & (n == n)], return_counts=True)
    st["n"] = {float(v): int(c) for v, c in zip(vals, cts)}
    out = np.zeros((2, Hh, W, 4), np.float32)
    out[0] = C
    out[0, ..., :3][hit] = col[hit]
    out[1][hit] = np.stack([m1, m2, n, var], axis=-1)[hit]
    if taps is not None:
        took[~hit] = -1
        taps["q"] = took
    assert out.dtype == np.float32
    return out


def denoise_var_pass(C, V, aov, s, k_normal, k_position, k_albedo, k_sigma, var_floor, stats=None):
    """One pass with step s over colour C [H, W, 4] and variance V [H, W] -> (colour, variance).  stats: as denoise_model.denoise_pass."""
    C = np.ascontiguousarray(C, np.float32)
    V = np.ascontiguousarray(V, np.float32)
    with np.errstate(all="ignore"):
        D = F(k_sigma) * V + F(var_floor)
    return atrous_pass(C, np.ascontiguousarray(aov, np.float32), s, k_normal, k_position, k_albedo, luminance_term(C, D), V=V, stats=stats)


def denoise_var(history, aov, n_passes, k_normal, k_position, k_albedo, k_sigma, var_floor, stats=None, keep=None):
    """rt_denoise_var: pass k = 0 .. n_passes - 1 with step 2^k over history plane 0, the variance starting as .w of history plane 1 -> the filtered colour.
    stats, keep: as denoise_model.denoise."""
    assert 1 <= n_passes <= 8
    history = np.ascontiguousarray(history, np.float32)
    out, V = history[0], history[1, ..., 3]
    for k in range(n_passes):
        out, V = denoise_var_pass(out, V, aov, 1 << k, k_normal, k_position, k_albedo, k_sigma, var_floor, stats=stats)
        if keep is not None:
            keep[k + 1] = out
    return out
