"""Fresnel dielectrics, restated (a helper module, like soft_lights_model.py): the rule of include/raytrace_hip.h "fresnel" -- the reflectance R of steps 1 and 2, the
whole step on explicit items, and a path walker that is soft_lights_model.Walker with steps 2 to 4 added to the refraction branch of the flagged objects -- in numpy
binary32, one rounding per operation.  With no effective flag the walker calls the walker underneath (tests/test_fresnel_model.py holds it to that, and R to a binary64
evaluation of the Fresnel equations, before any kernel is held to it)."""
import math

import numpy as np

from oracle import oracle_py as orc
from . import soft_lights_model as slm
from .lights_model import PI, _cross, _dot, _norm2, _normalize, _v, f32
from .sky_sample_model import uniform01

D = 1 << 26                                          # the draw of segment d sits at depth D + d: (D + d) * 4 = 2^28 + 4 d
REFRACTED, REFLECTED, TOTAL = 0, 1, 2


def _a(x):
    return np.asarray(x, f32)


def reflectance(n1, n2, un):
    """R of a ray that comes from the side of index n1 and meets the side of index n2 with un = dot(u, N); binary32 scalars or arrays.  NaN where the radicand is
    negative (k > 1: total reflection, or the reference's quirk) or at 0 / 0"""
    n1, n2, un = _a(n1), _a(n2), _a(un)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = (n1 / n2).astype(f32)
        k = ((ratio * ratio).astype(f32) * (f32(1) - (un * un).astype(f32)).astype(f32)).astype(f32)
        ci = np.abs(un)
        ct = np.sqrt((f32(1) - k).astype(f32)).astype(f32)
        a, b, c, e = (n1 * ci).astype(f32), (n2 * ct).astype(f32), (n1 * ct).astype(f32), (n2 * ci).astype(f32)
        rs = ((a - b).astype(f32) / (a + b).astype(f32)).astype(f32)
        rp = ((c - e).astype(f32) / (c + e).astype(f32)).astype(f32)
        return (f32(0.5) * ((rs * rs).astype(f32) + (rp * rp).astype(f32)).astype(f32)).astype(f32)


def _dots(a, b):
    return (((a[:, 0] * b[:, 0]).astype(f32) + (a[:, 1] * b[:, 1]).astype(f32)).astype(f32) + (a[:, 2] * b[:, 2]).astype(f32)).astype(f32)


def step(n_in, n_out, refr, eps, P, N, u, hs, seg):
    """the whole hit on k items: scalars broadcast, P, N, u [k, 3], hs uint32 [k], seg ints -> (R [k] (+0 under total reflection), code [k], O [k, 3], u [k, 3],
    the index after [k])"""
    hs = np.asarray(hs, np.uint32).ravel()
    k_ = hs.size
    n_in, n_out, refr, eps = (np.broadcast_to(_a(x), (k_,)).astype(f32) for x in (n_in, n_out, refr, eps))
    P, N, u = (_a(x).reshape(k_, 3) for x in (P, N, u))
    seg = np.broadcast_to(np.asarray(seg, np.int64), (k_,))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        out2in = refr == n_out
        ratio = np.where(out2in, (n_out / n_in).astype(f32), (n_in / n_out).astype(f32)).astype(f32)
        N = np.where(out2in[:, None], N, -N).astype(f32)
        un = _dots(u, N)
        k = ((ratio * ratio).astype(f32) * (f32(1) - (un * un).astype(f32)).astype(f32)).astype(f32)
        total = ((out2in & (refr > n_in)) | (~out2in & (refr > n_out))) & (k > 1)
        n1, n2 = np.where(out2in, n_out, n_in).astype(f32), np.where(out2in, n_in, n_out).astype(f32)
        R = reflectance(n1, n2, un)
        # (reflectance forms ratio as fl(n1 / n2): the same quotient)
        r_f = uniform01(hs, (np.uint64(D) + seg.astype(np.uint64)), 0)
        reflect = ~total & (r_f <= R)
        code = np.where(total, TOTAL, np.where(reflect, REFLECTED, REFRACTED)).astype(np.int32)
        R = np.where(total, f32(0), R).astype(f32)
        mirror = total | reflect
        epsN = (eps[:, None] * N).astype(f32)
        O = np.where(mirror[:, None], (P + epsN).astype(f32), (P - epsN).astype(f32)).astype(f32)
        u_refl = (u - ((f32(2) * un).astype(f32)[:, None] * N).astype(f32)).astype(f32)
        ct = np.sqrt((f32(1) - k).astype(f32)).astype(f32)
        Nc = ((-ct)[:, None] * N).astype(f32)
        Tc = (ratio[:, None] * (u - (un[:, None] * N).astype(f32)).astype(f32)).astype(f32)
        u_refr = (Nc + Tc).astype(f32)
        u_new = np.where(mirror[:, None], u_refl, u_refr).astype(f32)
        after = np.where(mirror, refr, np.where(out2in, n_in, n_out)).astype(f32)
    return R, code, O, u_new, after


class Walker(slm.Walker):
    """soft_lights_model.Walker in which the objects of `fresnel` (object ids) are flagged; radii None: point lights.  A flag is effective on glass alone (mirror == 0 and
    n_in != n_out); with no effective flag every path is the walker's underneath.  reflected counts the draws that reflected."""

    def __init__(self, scene, mats, lights, radii=None, fresnel=(), **kw):
        super().__init__(scene, mats, lights, [0.0] * len(lights) if radii is None else radii, **kw)
        self.flagged = {int(k) for k in fresnel if not self.mats[int(k)][1] and self.mats[int(k)][2] != self.mats[int(k)][3]}
        self.reflected = 0

    def path(self, O, u, segs, pixel, samp):
        if not self.flagged:
            return super().path(O, u, segs, pixel, samp)
        sc, eps = self.scene, self.eps
        refr = f32(1)
        seg = []
        rays = 0
        for d in range(segs):
            rays += 1
            hit, oid, P, N = sc.intersect_all(O, u, self.tri_tmin)
            if not hit:
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
                reflect = ((out2in and refr > n_in) or (not out2in and refr > n_out)) and k > 1
                if not reflect and oid in self.flagged:                  # steps 2 to 4 of the rule
                    R = reflectance(n_out if out2in else n_in, n_in if out2in else n_out, un)
                    r_f = f32(orc.uniform(self.seed, pixel, samp, np.uint32(D + d), 0))
                    reflect = bool(r_f <= R)                             # (a NaN R refracts)
                    self.reflected += int(reflect)
                if reflect:
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
