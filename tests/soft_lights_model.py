"""Point lights with a radius, restated (a helper module, like lights_model.py): the rule of include/raytrace_hip.h "soft shadows" -- the direction w(r1, r2), the point
L' = L_k + rho_k w of the picked light's shell -- in numpy binary32, and a path walker that is lights_model.Walker with L' in place of L in the diffuse branch.  With every
radius 0 it is that walker bit for bit (tests/test_soft_lights_model.py holds it to that, and to the oracle for direct light, before any kernel is held to it)."""
import math

import numpy as np

from oracle import oracle_py as orc
from . import lights_model as lm
from .lights_model import PI, _cross, _dot, _norm2, _normalize, _v, f32

D = 1 << 29                                          # the draws of segment d sit at depth D + d: (D + d) * 4 + dim = 2^31 + 4 d + dim modulo 2^32


def direction(r1, r2):
    """w(r1, r2): z = 1 - 2 r1, s = sqrt(1 - z z), x = (float)(cos(2 pi r2) s), y = (float)(sin(2 pi r2) s); binary32 scalars or arrays -> (x, y, z)"""
    r1, r2 = np.asarray(r1, f32), np.asarray(r2, f32)
    z = (f32(1) - (f32(2) * r1).astype(f32)).astype(f32)
    s = np.sqrt((f32(1) - (z * z).astype(f32)).astype(f32)).astype(f32)
    a = 2 * PI * r2.astype(np.float64)
    if a.ndim == 0:
        cs, sn = math.cos(float(a)), math.sin(float(a))             # the walker: libm's, as lights_model's bounce
    else:
        cs, sn = np.cos(a), np.sin(a)
    x = np.asarray(cs * s.astype(np.float64)).astype(f32)
    y = np.asarray(sn * s.astype(np.float64)).astype(f32)
    return x, y, z


def shell_point(L, rho, r1, r2):
    """L' = L + rho w per component, the product first; rho == 0: L itself (the addition is skipped)"""
    L = np.asarray(L, f32)
    if not f32(rho) > 0:
        return L
    x, y, z = direction(f32(r1), f32(r2))
    return _v(f32(L[0] + f32(f32(rho) * x)), f32(L[1] + f32(f32(rho) * y)), f32(L[2] + f32(f32(rho) * z)))


def camera_dir(W, H, i, j, fov=None):
    """the direction of pixel (row i, column j)'s camera ray with sigma == 0, as lights_model.Walker.render forms it"""
    z = lm.camera_z(W, f32(np.pi / 3) if fov is None else f32(fov))
    return _normalize(_v(f32(float(f32(f32(j) - f32(W) / f32(2))) + 0.5), f32(float(f32(f32(H) / f32(2) - f32(i))) - 0.5), z))


class Walker(lm.Walker):
    """lights_model.Walker whose light k has the radius radii[k]"""

    def __init__(self, scene, mats, lights, radii, **kw):
        super().__init__(scene, mats, lights, **kw)
        assert len(radii) == len(lights)
        self.radii = [f32(r) for r in radii]
        self.soft = any(r > 0 for r in self.radii)
        if len(lights) == 1:                         # a list of one takes whatever rt_scene_set_light takes: the pick is that light, the total its intensity
            self.light_of = lambda pixel, samp, d: 0
        self.surface = None                          # surface(oid, O, u, albedo) -> the albedo at the hit of the ray (O, u) on object oid: a textured mesh (texture_model.py)

    def light_point(self, pixel, samp, d):
        """-> (k, L'): the light segment d picks and the point of its shell the segment sees"""
        k = self.light_of(pixel, samp, d)
        if not self.soft:
            return k, self.pos[k]
        r1 = f32(orc.uniform(self.seed, pixel, samp, np.uint32(D + d), 0))
        r2 = f32(orc.uniform(self.seed, pixel, samp, np.uint32(D + d), 1))
        return k, shell_point(self.pos[k], self.radii[k], r1, r2)

    def path(self, O, u, segs, pixel, samp):
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
                if ((out2in and refr > n_in) or (not out2in and refr > n_out)) and k > 1:
                    O = P + eps * N
                    u = u - f32(2 * un) * N
                else:
                    O = P - eps * N
                    u = f32(-np.sqrt(f32(f32(1) - k))) * N + ratio * (u - un * N)
                    refr = n_in if out2in else n_out
            else:                                                        # the diffuse branch on the operand L'
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
