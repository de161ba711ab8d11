"""A second, scalar reference of rt_denoise, rt_temporal_accumulate and rt_denoise_var, written from the contract in include/raytrace_hip.h alone (test infrastructure).

One pixel at a time, np.float32 scalars, one rounding per operation, `continue` where the contract says "skipped" and `break` where it says "the first valid one wins".
Nothing here is vectorised and nothing is shared with tests/denoise_model.py and tests/temporal_model.py but the stencil weights and camera_constants: its job is to make
those two models trustworthy on inputs that reach every branch, before the device is held to them.  It is slow (a few hundred microseconds per pixel and pass): frames
of a few thousand pixels.

min and max are minNum and maxNum (the operand that is not NaN), as the header states.

mutant= (tests only) changes one thing a broken kernel would plausibly change; tests/test_synthetic_filters_model.py proves that the synthetic inputs tell every one of
them from the contract."""
import numpy as np

from .denoise_model import H3
from .temporal_model import camera_constants

F = np.float32
ZERO, ONE = F(0), F(1)
MUTANTS = ("halo1", "dx_outer", "half_gt", "gx_lt_width", "tap_order", "no_clamp", "no_alpha_min", "n_le_4", "var_lag", "div_seq", "k_color_unscaled", "w_ge_0")
DIV_LO, DIV_HI = F(2.0 ** -60), F(2.0 ** 60)


def fmax(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a >= b else b


def fmin(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a <= b else b


def _fma(a, b, c):
    return F(np.float64(a) * np.float64(b) + np.float64(c))


def _in_range(x):
    return DIV_LO <= abs(x) <= DIV_HI


def shared_sequence(n, d):
    """rt_div.h's q = n r1, two residual steps, with r = fl(1 / d); binary32, fma emulated in binary64"""
    r = ONE / d
    r1 = _fma(_fma(-d, r, ONE), r, r)
    q = n * r1
    q1 = _fma(_fma(-d, q, n), r1, q)
    return _fma(_fma(-d, q1, n), r1, q1)


def quot(n, d, mutant=None):
    """the correctly rounded quotient; mutant div_seq: the shared sequence where the kernel must take the literal quotient"""
    if mutant == "div_seq" and not (_in_range(n) and _in_range(d)):
        return shared_sequence(n, d)
    return n / d


def lum(c):
    return (F(0.2126) * c[0] + F(0.7152) * c[1]) + F(0.0722) * c[2]


def _sq3(a, b):
    x, y, z = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return (x * x + y * y) + z * z


def _pass(C, V, aov, s, k_normal, k_position, k_albedo, k_color, var, k_sigma, var_floor, mutant):
    Hh, W = C.shape[:2]
    out = C.copy()
    Vo = None if V is None else V.copy()
    reach = 1 if (mutant == "halo1" and s >= 32) else 2
    order = [(dy, dx) for dy in range(-2, 3) for dx in range(-2, 3)]
    if mutant == "dx_outer":
        order = [(dy, dx) for dx in range(-2, 3) for dy in range(-2, 3)]
    for y in range(Hh):
        for x in range(W):
            idp = aov[0, y, x, 3]
            if idp == F(-1):
                continue
            Np, Pp, Ap, Cp = aov[0, y, x], aov[1, y, x], aov[2, y, x], C[y, x]
            if var:
                lp = lum(Cp)
                D = k_sigma * V[y, x] + var_floor
            Sx = Sy = Sz = Wt = Sv = ZERO
            for dy, dx in order:
                qx, qy = x + dx * s, y + dy * s
                if qx < 0 or qx >= W or qy < 0 or qy >= Hh:
                    continue
                if abs(dx) > reach or abs(dy) > reach:
                    continue
                Nq = aov[0, qy, qx]
                if Nq[3] != idp:
                    continue
                w = H3[abs(dy)] * H3[abs(dx)]
                if k_normal != 0:
                    w = w * fmax(ZERO, ONE - _sq3(Np, Nq) * k_normal)
                if k_position != 0:
                    Pq = aov[1, qy, qx]
                    e = (Np[0] * (Pq[0] - Pp[0]) + Np[1] * (Pq[1] - Pp[1])) + Np[2] * (Pq[2] - Pp[2])
                    w = w * fmax(ZERO, ONE - (e * e) * k_position)
                if k_albedo != 0:
                    w = w * fmax(ZERO, ONE - _sq3(Ap, aov[2, qy, qx]) * k_albedo)
                Cq = C[qy, qx]
                if var:
                    dl = lp - lum(Cq)
                    dl2 = dl * dl
                    if dl2 != 0:
                        w = w * fmax(ZERO, ONE - quot(dl2, D, mutant))
                elif k_color != 0:
                    w = w * fmax(ZERO, ONE - _sq3(Cp, Cq) * k_color)
                if not (w >= 0 if mutant == "w_ge_0" else w > 0):
                    continue
                Sx, Sy, Sz = Sx + w * Cq[0], Sy + w * Cq[1], Sz + w * Cq[2]
                Wt = Wt + w
                if var:
                    Sv = Sv + (w * w) * V[qy, qx]
            out[y, x, 0], out[y, x, 1], out[y, x, 2] = quot(Sx, Wt, mutant), quot(Sy, Wt, mutant), quot(Sz, Wt, mutant)
            if var:
                Vo[y, x] = quot(Sv, Wt * Wt, mutant)
    return out, Vo


def denoise(C, aov, n_passes, k_normal, k_position, k_albedo, k_color, mutant=None):
    assert mutant is None or mutant in MUTANTS
    out = np.ascontiguousarray(C, np.float32)
    aov = np.ascontiguousarray(aov, np.float32)
    with np.errstate(all="ignore"):
        for k in range(n_passes):
            kc = F(k_color) if mutant == "k_color_unscaled" else F(k_color) * F(4 ** k)
            out, _ = _pass(out, None, aov, 1 << k, F(k_normal), F(k_position), F(k_albedo), kc, False, None, None, mutant)
    return out


def denoise_var(history, aov, n_passes, k_normal, k_position, k_albedo, k_sigma, var_floor, mutant=None):
    assert mutant is None or mutant in MUTANTS
    history = np.ascontiguousarray(history, np.float32)
    aov = np.ascontiguousarray(aov, np.float32)
    out = history[0]
    planes = [np.ascontiguousarray(history[1, ..., 3])]                # planes[k] = the variance pass k reads
    with np.errstate(all="ignore"):
        for k in range(n_passes):
            V = planes[k - 1] if (mutant == "var_lag" and k >= 2) else planes[k]
            out, Vo = _pass(out, V, aov, 1 << k, F(k_normal), F(k_position), F(k_albedo), None, True, F(k_sigma), F(var_floor), mutant)
            planes.append(Vo)
    return out


TAPS = ((0, 0), (1, 0), (0, 1), (1, 1))


def accumulate(C, aov, prev_aov=None, prev_history=None, camera=None, pose=None, motion=None, mask=0, max_history=32, alpha_min=0.0, min_normal_dot=0.9,
               max_plane_dist=0.5, taps=None, mutant=None):
    assert mutant is None or mutant in MUTANTS
    C = np.ascontiguousarray(C, np.float32)
    aov = np.ascontiguousarray(aov, np.float32)
    Hh, W = C.shape[:2]
    out = np.zeros((2, Hh, W, 4), np.float32)
    took = np.full((Hh, W, 2), -1, np.int64)
    have_prev = prev_aov is not None
    if have_prev:
        pa = np.ascontiguousarray(prev_aov, np.float32)
        ph = np.ascontiguousarray(prev_history, np.float32)
        O, bx, by, bz, cx, cy, b = camera_constants(W, camera, pose)
        mot = None if motion is None else np.asarray(motion, np.float32)
    max_hist, a_min, min_nd = F(max_history), F(alpha_min), F(min_normal_dot)
    mpd2 = F(max_plane_dist) * F(max_plane_dist)
    half_w, half_h = F(W) / F(2), F(Hh) / F(2)
    tap_order = (TAPS[3], TAPS[1], TAPS[2], TAPS[0]) if mutant == "tap_order" else TAPS
    with np.errstate(all="ignore"):
        L = np.empty((Hh, W), np.float32)
        for y in range(Hh):
            for x in range(W):
                L[y, x] = lum(C[y, x])
        for y in range(Hh):
            for x in range(W):
                Cp, Np = C[y, x], aov[0, y, x]
                idp = Np[3]
                out[0, y, x] = Cp
                if idp == F(-1):
                    continue
                l = L[y, x]
                n, col, m1, m2 = ONE, [Cp[0], Cp[1], Cp[2]], l, l * l
                oid = int(idp)
                if have_prev and not (int(mask) >> (oid & 31)) & 1:
                    P, N = aov[1, y, x], Np
                    if mot is not None:
                        m = mot[oid & 15]
                        P = [((m[3 * r] * P[0] + m[3 * r + 1] * P[1]) + m[3 * r + 2] * P[2]) + m[9 + r] for r in range(3)]
                        N = [(m[3 * r] * N[0] + m[3 * r + 1] * N[1]) + m[3 * r + 2] * N[2] for r in range(3)]
                    d = [P[0] - O[0], P[1] - O[1], P[2] - O[2]]
                    k = quot(b, (d[0] * bz[0] + d[1] * bz[1]) + d[2] * bz[2], mutant)
                    X = ((d[0] * bx[0] + d[1] * bx[1]) + d[2] * bx[2]) * k - cx
                    Y = ((d[0] * by[0] + d[1] * by[1]) + d[2] * by[2]) * k - cy
                    gx, gy = X + half_w, half_h - Y
                    right = gx < F(W) if mutant == "gx_lt_width" else gx <= F(W)
                    if k > 0 and gx >= F(-1) and right and gy >= F(-1) and gy <= F(Hh):
                        fx, fy = np.floor(gx), np.floor(gy)
                        ix, iy = int(fx), int(fy)
                        if mutant == "half_gt":
                            jx, jy = (ix + 1 if gx - fx > F(0.5) else ix - 1), (iy + 1 if gy - fy > F(0.5) else iy - 1)
                        else:
                            jx, jy = (ix + 1 if gx - fx >= F(0.5) else ix - 1), (iy + 1 if gy - fy >= F(0.5) else iy - 1)
                        for tx, ty in tap_order:
                            qx, qy = (jx if tx else ix), (jy if ty else iy)
                            if qx < 0 or qx >= W or qy < 0 or qy >= Hh:
                                continue
                            Nq = pa[0, qy, qx]
                            if Nq[3] != idp:
                                continue
                            if not ((N[0] * Nq[0] + N[1] * Nq[1]) + N[2] * Nq[2] >= min_nd):
                                continue
                            Pq = pa[1, qy, qx]
                            e = (N[0] * (Pq[0] - P[0]) + N[1] * (Pq[1] - P[1])) + N[2] * (Pq[2] - P[2])
                            if not (e * e <= mpd2):
                                continue
                            H0, H1 = ph[0, qy, qx], ph[1, qy, qx]
                            n = H1[2] + ONE if mutant == "no_clamp" else fmin(H1[2] + ONE, max_hist)
                            a = quot(ONE, n, mutant) if mutant == "no_alpha_min" else fmax(quot(ONE, n, mutant), a_min)
                            col = [H0[c] + a * (Cp[c] - H0[c]) for c in range(3)]
                            m1 = H1[0] + a * (l - H1[0])
                            m2 = H1[1] + a * (l * l - H1[1])
                            took[y, x] = (qx, qy)
                            break
                V = fmax(ZERO, m2 - m1 * m1)
                if (n <= F(4)) if mutant == "n_le_4" else (n < F(4)):
                    s1 = s2 = cnt = ZERO
                    for dy in range(-2, 3):
                        for dx in range(-2, 3):
                            qx, qy = x + dx, y + dy
                            if qx < 0 or qx >= W or qy < 0 or qy >= Hh:
                                continue
                            if aov[0, qy, qx, 3] != idp:
                                continue
                            lq = L[qy, qx]
                            s1, s2, cnt = s1 + lq, s2 + lq * lq, cnt + ONE
                    e1, e2 = quot(s1, cnt, mutant), quot(s2, cnt, mutant)
                    V = fmax(ZERO, e2 - e1 * e1)
                out[0, y, x, 0], out[0, y, x, 1], out[0, y, x, 2] = col
                out[1, y, x] = (m1, m2, n, V)
    if taps is not None:
        taps["q"] = took
    return out
