"""Rough mirrors, restated (a helper module, like fresnel_model.py): the rule of include/raytrace_hip.h "roughness" -- the facet normal h of steps 2 to 4, the whole hit
on explicit items, and a path walker that is soft_lights_model.Walker whose mirror branch takes the step for the objects in `rough` -- in numpy binary32, one rounding
per operation, on sky_sample_model.uniform01.  Written from the header, not from the kernel.  With no effective roughness the walker calls the walker underneath
(tests/test_gloss_model.py holds it to that, and the facets to the GGX distribution, before any kernel is held to it)."""
import math

import numpy as np

from oracle import oracle_py as orc
from . import soft_lights_model as slm
from .lights_model import PI, _cross, _dot, _norm2, _normalize, _v, f32
from .sky_sample_model import sample_key, uniform01

D = 1 << 25                                          # the draws of segment d sit at depth D + d: (D + d) * 4 + dim = 2^27 + 4 d + dim
PLAIN, FOLDED = 0, 1
ALPHA_MIN = f32(2.0 ** -12)


def _a(x):
    return np.asarray(x, f32)


def _dots(a, b):
    return (((a[:, 0] * b[:, 0]).astype(f32) + (a[:, 1] * b[:, 1]).astype(f32)).astype(f32) + (a[:, 2] * b[:, 2]).astype(f32)).astype(f32)


def polar(alpha, r1):
    """step 3: (c2, c, s) of the facet's polar angle from alpha and the draw r1; binary32 scalars or arrays"""
    alpha, r1 = _a(alpha), _a(r1)
    a2 = (alpha * alpha).astype(f32)
    m = (a2 - f32(1)).astype(f32)
    c2 = ((f32(1) - r1).astype(f32) / (f32(1) + (m * r1).astype(f32)).astype(f32)).astype(f32)
    return c2, np.sqrt(c2).astype(f32), np.sqrt((f32(1) - c2).astype(f32)).astype(f32)


def frame(N):
    """cosine_bounce's tangent frame about N [k, 3] -> (T1, T2): T1 = normalize((-Ny, Nx, 0)) if Nx != 0 and Ny != 0 else normalize((-Nz, 0, Nx)), T2 = cross(N, T1)"""
    N = _a(N)
    t1a = (N[:, 1] != 0) & (N[:, 0] != 0)
    p, q = np.where(t1a, -N[:, 1], -N[:, 2]).astype(f32), N[:, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.sqrt(((p * p).astype(f32) + (q * q).astype(f32)).astype(f32)).astype(f32)   # (the third square is +0: the sum is unchanged)
        op, oq = (p / n).astype(f32), (q / n).astype(f32)
        zero = (f32(0) / n).astype(f32)
    T1 = np.where(t1a[:, None], np.stack([op, oq, zero], 1), np.stack([op, zero, oq], 1)).astype(f32)
    T2 = np.stack([((N[:, 1] * T1[:, 2]).astype(f32) - (N[:, 2] * T1[:, 1]).astype(f32)).astype(f32),
                   ((N[:, 2] * T1[:, 0]).astype(f32) - (N[:, 0] * T1[:, 2]).astype(f32)).astype(f32),
                   ((N[:, 0] * T1[:, 1]).astype(f32) - (N[:, 1] * T1[:, 0]).astype(f32)).astype(f32)], 1)
    return T1, T2


def facet_from(alpha, N, r1, r2):
    """steps 3 and 4 from the two draws: h [k, 3] and c2 [k]"""
    N = _a(N).reshape(-1, 3)
    c2, c, s = polar(alpha, r1)
    a = 2 * PI * np.asarray(r2, f32).astype(np.float64)
    if a.size == 1:                                                     # the walker: libm's, as soft_lights_model.direction
        cs, sn = np.float64(math.cos(float(a.ravel()[0]))), np.float64(math.sin(float(a.ravel()[0])))
    else:
        cs, sn = np.cos(a), np.sin(a)
    x = np.asarray(cs * s.astype(np.float64)).astype(f32).reshape(-1)
    y = np.asarray(sn * s.astype(np.float64)).astype(f32).reshape(-1)
    c = np.broadcast_to(c, x.shape)
    with np.errstate(invalid="ignore"):
        T1, T2 = frame(N)
        h = (((x[:, None] * T1).astype(f32) + (y[:, None] * T2).astype(f32)).astype(f32) + (c[:, None] * N).astype(f32)).astype(f32)
    return h, np.broadcast_to(c2, x.shape)


def draws(hs, seg):
    hs = np.asarray(hs, np.uint32).ravel()
    depth = np.uint64(D) + np.broadcast_to(np.asarray(seg, np.int64), hs.shape).astype(np.uint64)
    return uniform01(hs, depth, 0), uniform01(hs, depth, 1)


def facet(alpha, N, hs, seg):
    """steps 2 to 4 on k items: alpha and seg broadcast, N [k, 3], hs uint32 [k] -> h [k, 3]"""
    r1, r2 = draws(hs, seg)
    return facet_from(alpha, N, r1, r2)[0]


def step_from(alpha, eps, P, N, u, r1, r2):
    """the whole hit from the two draws -> (h, code, O, u')"""
    P, N, u = (_a(x).reshape(-1, 3) for x in (P, N, u))
    k_ = P.shape[0]
    eps = np.broadcast_to(_a(eps), (k_,)).astype(f32)
    with np.errstate(invalid="ignore", over="ignore"):
        un = _dots(u, N)
        O = (P + (eps[:, None] * N).astype(f32)).astype(f32)
        h, _ = facet_from(alpha, N, r1, r2)
        uh = _dots(u, h)
        v = (u - ((f32(2) * uh).astype(f32)[:, None] * h).astype(f32)).astype(f32)
        vn = _dots(v, N)
        fold = (vn != 0) & ((vn < 0) == (un < 0))
        w = (v - ((f32(2) * vn).astype(f32)[:, None] * N).astype(f32)).astype(f32)
        v = np.where(fold[:, None], w, v).astype(f32)
    return h, np.where(fold, FOLDED, PLAIN).astype(np.int32), O, v


def step(alpha, eps, P, N, u, hs, seg):
    """the whole hit on k items: alpha, eps and seg broadcast, P, N, u [k, 3], hs uint32 [k] -> (h [k, 3], code [k], O [k, 3], u' [k, 3])"""
    r1, r2 = draws(hs, seg)
    return step_from(alpha, eps, P, N, u, r1, r2)


class Walker(slm.Walker):
    """soft_lights_model.Walker in which the objects of `rough` ({object id: alpha}) have a roughness; radii None: point lights.  A roughness is effective on a mirror
    alone (alpha > 0 and mirror != 0); with no effective roughness every path is the walker's underneath.  facets counts the facets drawn, folded those folded back."""

    def __init__(self, scene, mats, lights, radii=None, rough=None, **kw):
        super().__init__(scene, mats, lights, [0.0] * len(lights) if radii is None else radii, **kw)
        self.rough = {int(k): f32(a) for k, a in (rough or {}).items() if f32(a) > 0 and self.mats[int(k)][1]}
        self.facets = 0
        self.folded = 0

    def path(self, O, u, segs, pixel, samp):
        if not self.rough:
            return super().path(O, u, segs, pixel, samp)
        sc, eps = self.scene, self.eps
        refr = f32(1)
        seg = []
        rays = 0
        hs = np.uint32(sample_key(self.seed, pixel, samp))
        for d in range(segs):
            rays += 1
            hit, oid, P, N = sc.intersect_all(O, u, self.tri_tmin)
            if not hit:
                break
            alb, mirror, n_in, n_out = self.mats[oid]
            if mirror and oid in self.rough:                             # the rule's hit
                _, code, O1, u1 = step(self.rough[oid], eps, P, N, u, [hs], d)
                O, u = O1[0], u1[0]
                self.facets += 1
                self.folded += int(code[0])
            elif mirror:
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
                    with np.errstate(invalid="ignore"):
                        u = f32(-np.sqrt(f32(f32(1) - k))) * N + ratio * (u - un * N)
                    refr = n_in if out2in else n_out
            else:                                                        # the diffuse branch of soft_lights_model.Walker
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
        ans = _v(0, 0, 0)
        for l, alb in reversed(seg):
            ans = (l * alb) / f32(PI) + alb * ans
        return ans, rays
