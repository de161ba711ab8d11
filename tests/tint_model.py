"""Tinted mirrors and glass, restated (a helper module, like gloss_model.py): the rule of include/raytrace_hip.h "tint" as a path walker that is gloss_model.Walker whose
specular arms -- the smooth mirror's, the rough mirror's, the glass's -- record a segment (sid = the object, l = +0) for the objects in `tinted`, where the walker
underneath records nothing.  The fold is the existing restatement, per channel fl(fl(fl(l alb) / pi) + fl(alb ans)); the intersections are the oracle's; numpy binary32,
one rounding per operation.  Written from the header, not from the kernel.  With no effective flag the walker calls the walker underneath
(tests/test_tint_model.py holds it to that and to the closed forms before any kernel is held to it)."""
import math

import numpy as np

from oracle import oracle_py as orc
from . import gloss_model as glm
from .lights_model import PI, _cross, _dot, _norm2, _normalize, _v, f32
from .sky_sample_model import sample_key


def fold(segments):
    """the existing fold, back to front over (l, alb) pairs: ans = fl(fl(l alb) / pi) + fl(alb ans) per channel, from +0"""
    ans = _v(0, 0, 0)
    for l, alb in reversed(segments):
        ans = (l * alb) / f32(PI) + alb * ans
    return ans


class Walker(glm.Walker):
    """gloss_model.Walker in which the objects of `tinted` (object ids) carry the flag.  A flag is effective on an object that takes a specular arm alone (mirror != 0,
    smooth or rough, or n_in != n_out); with no effective flag every path is the walker's underneath.  The colour is the object's material albedo: the surface hook
    (a texture) is asked at diffuse hits alone.  tints counts the tinted segments recorded."""

    def __init__(self, scene, mats, lights, radii=None, rough=None, tinted=(), **kw):
        super().__init__(scene, mats, lights, radii, rough=rough, **kw)
        self.tinted = {int(k) for k in tinted if self.mats[int(k)][1] or self.mats[int(k)][2] != self.mats[int(k)][3]}
        self.tints = 0

    def path(self, O, u, segs, pixel, samp):
        if not self.tinted:
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
            specular = bool(mirror) or n_in != n_out
            if mirror and oid in self.rough:                             # gloss_model's hit
                _, code, O1, u1 = glm.step(self.rough[oid], eps, P, N, u, [hs], d)
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
            if specular and oid in self.tinted:                          # the rule's hit: the same ray, no shadow ray, a segment of the object's albedo and l = +0
                seg.append((f32(0), alb))
                self.tints += 1
        return fold(seg), rays
