"""The environment map, restated (a helper module, like soft_lights_model.py): the rule of include/raytrace_hip.h "environment" -- the octahedral coordinates (a, b) of a
direction, the clamped bilinear lookup E = sky_radiance(u) -- in numpy binary32, for scalars and arrays, and a path walker that is soft_lights_model.Walker with its path
restated so that a miss starts the fold from E.  With every radius 0 that walker is lights_model.Walker; without a map, or with an all-zero one, it is the walker it rests
on bit for bit (tests/test_sky_model.py holds it to that, and to the oracle, before any kernel is held to it).  sigma stays 0, as in the models it rests on."""
import math

import numpy as np

from oracle import oracle_py as orc
from . import soft_lights_model as sm
from .lights_model import PI, _cross, _dot, _norm2, _normalize, _v, f32

TEXEL_END = 0x6f800000                               # bits of 2^96: a texel's bits are below it (finite, sign bit clear)


def _sg(v):
    return np.where(v < 0, f32(-1), f32(1)).astype(f32)


def oct_coords(u):
    """u [..., 3] binary32 -> (a, b, ok): steps 1 to 4 of the rule; where ok is false (s not a finite number above 0) a and b are 0.5 and nobody reads them"""
    u = np.asarray(u, f32)
    ux, uy, uz = u[..., 0], u[..., 1], u[..., 2]
    with np.errstate(all="ignore"):
        s = ((np.abs(ux) + np.abs(uy)).astype(f32) + np.abs(uz)).astype(f32)
        ok = (s > 0) & (s < np.inf)
        sd = np.where(ok, s, f32(1)).astype(f32)
        px = (np.where(ok, ux, f32(0)).astype(f32) / sd).astype(f32)
        pz = (np.where(ok, uz, f32(0)).astype(f32) / sd).astype(f32)
        fx = ((f32(1) - np.abs(pz)).astype(f32) * _sg(px)).astype(f32)
        fz = ((f32(1) - np.abs(px)).astype(f32) * _sg(pz)).astype(f32)
        low = ok & (uy < 0)
        qx, qz = np.where(low, fx, px).astype(f32), np.where(low, fz, pz).astype(f32)
        a = ((qx * f32(0.5)).astype(f32) + f32(0.5)).astype(f32)
        b = ((qz * f32(0.5)).astype(f32) + f32(0.5)).astype(f32)
    return a, b, ok


def tex_floor(c):
    """-> (floor(c) as int64, c - floor(c)); outside [-2^31, 2^31), NaN included: (0, 0)"""
    c = np.asarray(c, f32)
    with np.errstate(all="ignore"):
        ok = (c >= f32(-2147483648.0)) & (c < f32(2147483648.0))
        cc = np.where(ok, c, f32(0)).astype(f32)
        fl = np.floor(cc).astype(f32)
        return fl.astype(np.int64), (cc - fl).astype(f32)


def taps(a, b, n):
    """step 5 up to the clamp: -> (xa, xb, ya, yb, fx, fy)"""
    nf = f32(n)
    x0, fx = tex_floor(((a * nf).astype(f32) - f32(0.5)).astype(f32))
    y0, fy = tex_floor(((b * nf).astype(f32) - f32(0.5)).astype(f32))
    cl = lambda i: np.clip(i, 0, n - 1)
    return cl(x0), cl(x0 + 1), cl(y0), cl(y0 + 1), fx, fy


def sky_radiance(env, u):
    """env [n, n, 3] binary32 (row 0 first), u [..., 3] -> E [..., 3]"""
    env = np.asarray(env, f32)
    n = env.shape[0]
    assert env.shape == (n, n, 3) and 1 <= n <= 1024
    a, b, ok = oct_coords(u)
    xa, xb, ya, yb, fx, fy = taps(a, b, n)
    gx, gy = (f32(1) - fx).astype(f32)[..., None], (f32(1) - fy).astype(f32)[..., None]
    fx, fy = fx[..., None], fy[..., None]
    t00, t10, t01, t11 = env[ya, xa], env[ya, xb], env[yb, xa], env[yb, xb]
    top = ((t00 * gx).astype(f32) + (t10 * fx).astype(f32)).astype(f32)
    bot = ((t01 * gx).astype(f32) + (t11 * fx).astype(f32)).astype(f32)
    E = ((top * gy).astype(f32) + (bot * fy).astype(f32)).astype(f32)
    return np.where(ok[..., None], E, f32(0)).astype(f32)


def valid_map(env):
    """what rt_scene_set_environment accepts: every texel's bits below 2^96's"""
    return bool((np.ascontiguousarray(env, f32).view(np.uint32) < TEXEL_END).all())


class Walker(sm.Walker):
    """soft_lights_model.Walker under the environment env ([n, n, 3], or None: a miss is black); radii None: point lights"""

    def __init__(self, scene, mats, lights, radii=None, env=None, **kw):
        super().__init__(scene, mats, lights, [0.0] * len(lights) if radii is None else radii, **kw)
        self.env = None if env is None else np.asarray(env, f32)

    def path(self, O, u, segs, pixel, samp):
        sc, eps = self.scene, self.eps
        refr = f32(1)
        seg = []
        rays = 0
        E = _v(0, 0, 0)
        for d in range(segs):
            rays += 1
            hit, oid, P, N = sc.intersect_all(O, u, self.tri_tmin)
            if not hit:
                if self.env is not None:
                    E = sky_radiance(self.env, np.asarray(u, f32))       # the direction as the ray holds it
                break
            alb, mirror, n_in, n_out = self.mats[oid]
            if mirror:
                O = P + eps * N
                u = u - f32(2 * _dot(u, N)) * N
            elif n_in != n_out:
                out2in = refr == n_out
                if out2in:
                    ratio = f32(n_out / n_in)
                else:
                    ratio = f32(n_in / n_out)
                    N = -N
                un = _dot(u, N)
                k = f32(f32(ratio * ratio) * f32(f32(1) - f32(un * un)))
                if ((out2in and refr > n_in) or (not out2in and refr > n_out)) and k > 1:
                    O = P + eps * N
                    u = u - f32(2 * un) * N
                else:
                    O = P - eps * N
                    u = f32(-np.sqrt(f32(f32(1) - k))) * N + ratio * (u - un * N)
                    refr = n_in if out2in else n_out
            else:
                if self.surface is not None:
                    alb = self.surface(oid, O, u, alb)
                k, L = self.light_point(pixel, samp, d)
                Pa = P + eps * N
                to = L - Pa
                rays += 1
                shit, _, Pp, _ = sc.intersect_all(Pa, to / np.sqrt(_norm2(to)), self.tri_tmin)
                hidden = shit and _norm2(Pp - Pa) <= _norm2(L - Pa)
                mx = max(_dot(N, _normalize(L - P)), f32(0))
                lvis = f32(float(self.total) / (4 * PI * float(_norm2(L - P))) * float(mx))
                seg.append((f32(0) if hidden else lvis, alb))
                self.picks.append((pixel, samp, d, k, bool(not hidden and lvis > 0)))
                if d + 1 >= segs:
                    break
                r1, r2 = f32(orc.uniform(self.seed, pixel, samp, d, 0)), f32(orc.uniform(self.seed, pixel, samp, d, 1))
                s1 = np.sqrt(f32(f32(1) - r2))
                x = f32(math.cos(2 * PI * float(r1)) * float(s1))
                y = f32(math.sin(2 * PI * float(r1)) * float(s1))
                z = np.sqrt(r2)
                T1 = _normalize(_v(-N[1], N[0], 0) if (N[1] != 0 and N[0] != 0) else _v(-N[2], 0, N[0]))
                T2 = _cross(N, T1)
                u = (x * T1 + y * T2) + z * N
                O = Pa
                refr = f32(1)
        ans = E                                                          # the fold starts from what the path's last ray met
        for l, alb in reversed(seg):
            ans = (l * alb) / f32(PI) + alb * ans
        return ans, rays
