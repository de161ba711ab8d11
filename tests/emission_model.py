"""Emissive meshes, restated (a helper module, like sky_sample_model.py, on which it is built): the rule of include/raytrace_hip.h "emissive meshes" -- the table over
the scene's triangles in numpy binary32 and Python integers, the draw sample(hs, d) for scalars and arrays, and the estimate's factor g in binary64.  The device is held to
this word for word (tests/test_gpu_emission.py); tests/test_emission_model.py holds THIS to the mathematics: the areas, the barycentrics, the unbiasedness against a
quadrature over the panel."""
import numpy as np

from .sky_sample_model import M32, f32, uniform01, uniform24

KAPPA = f32(2.0 ** -10)                                                 # the shadow ray aims at L' = Q + KAPPA (Pa - Q)


def stored_order(bvh_arr10):
    """the order in which an upload stores a mesh's triangles: the leaves of the tree as the traversal reaches them -- pre-order, the RIGHT child before the left --
    ascending inside a leaf -> indices into the uploaded triangle array"""
    a = np.asarray(bvh_arr10, f32).reshape(-1, 10)
    if len(a) == 0:
        return np.zeros(0, np.int64)
    out, stack = [], [0]
    while stack:
        i = stack.pop()
        left, right = int(a[i, 0]), int(a[i, 1])
        if left == -1:
            out.extend(range(int(a[i, 8]), int(a[i, 9])))
        else:
            stack.append(left)                                          # popped second
            stack.append(right)
    return np.array(out, np.int64)


def corners(vertices, indices, order=None):
    """[nt, 3, 3] binary32: the corners A, B, C of every triangle, in `order` (indices into `indices`) if given"""
    v, t = np.asarray(vertices, f32), np.asarray(indices)[:, :3].astype(np.int64)
    if order is not None:
        t = t[np.asarray(order, np.int64)]
    return v[t]


def _cross(a, b):
    return np.stack([((a[..., 1] * b[..., 2]).astype(f32) - (a[..., 2] * b[..., 1]).astype(f32)).astype(f32),
                     ((a[..., 2] * b[..., 0]).astype(f32) - (a[..., 0] * b[..., 2]).astype(f32)).astype(f32),
                     ((a[..., 0] * b[..., 1]).astype(f32) - (a[..., 1] * b[..., 0]).astype(f32)).astype(f32)], axis=-1)


def _dot(a, b):
    return (((a[..., 0] * b[..., 0]).astype(f32) + (a[..., 1] * b[..., 1]).astype(f32)).astype(f32) + (a[..., 2] * b[..., 2]).astype(f32)).astype(f32)


class TriTable:
    """the sampling table of the triangles tris [nt, 3, 3] (corners A, B, C in stored order) whose meshes have the radiances le [nt, 3] (a row per triangle; zeros: its mesh
    does not emit): W [nt] binary32, c [nt] uint32, prefix [nt] uint64 (inclusive), total (a Python int; 0: the table is empty)"""

    def __init__(self, tris, le):
        tris = np.ascontiguousarray(tris, f32).reshape(-1, 3, 3)
        self.nt = len(tris)
        self.le = np.ascontiguousarray(np.broadcast_to(np.asarray(le, f32), (self.nt, 3)), f32)
        self.A = tris[:, 0]
        self.e1 = (tris[:, 1] - tris[:, 0]).astype(f32)
        self.e2 = (tris[:, 2] - tris[:, 0]).astype(f32)
        self.Nt = _cross(self.e1, self.e2)
        self.A2 = np.sqrt(_dot(self.Nt, self.Nt)).astype(f32)           # twice the area
        self.Y = ((self.le[:, 0] + self.le[:, 1]).astype(f32) + self.le[:, 2]).astype(f32)
        self.W = np.where(self.Y > 0, (self.A2 * self.Y).astype(f32), f32(0)).astype(f32)
        wmax = self.W.max() if self.nt else f32(0)
        if not wmax > 0:
            self.c = np.zeros(self.nt, np.uint32)
        else:
            k = ((self.W / wmax).astype(f32) * f32(2.0 ** 31)).astype(f32).astype(np.uint64)
            self.c = np.where(self.W > 0, np.maximum(k, np.uint64(1)), np.uint64(0)).astype(np.uint32)
        self.prefix = np.cumsum(self.c.astype(np.uint64), dtype=np.uint64)
        self.total = int(self.prefix[-1]) if self.nt else 0

    def pick(self, ka, kb):
        """the triangle of the 24-bit integers (ka, kb): K = ka 2^24 + kb, X = ((K total) >> 48) + 1, the least t with prefix[t] >= X (the sky table's pick)"""
        ka, kb = np.atleast_1d(np.asarray(ka, np.uint64)), np.atleast_1d(np.asarray(kb, np.uint64))
        K = (ka << np.uint64(24)) | kb
        if K.size <= 4096:                                              # Python integers: the product is exact as written
            X = np.array([((int(k) * self.total) >> 48) + 1 for k in K], np.uint64)
        else:                                                           # the same in 64-bit pieces (sky_sample_model.Table.pick says why it is exact)
            tl, th = np.uint64(self.total & 0xFFFFFF), np.uint64(self.total >> 24)
            mid = ka * tl + kb * th + ((kb * tl) >> np.uint64(24))
            X = ka * th + (mid >> np.uint64(24)) + np.uint64(1)
        return np.searchsorted(self.prefix, X, side="left").astype(np.int64), X

    def barycentrics(self, hs, d):
        """(r1, r2) of the draw after the fold: binary32, r1 + r2 <= 1 up to the rounding of the fold's own subtractions"""
        hs = np.atleast_1d(np.asarray(hs, np.uint64))
        depth = (np.uint64(1 << 27) + np.broadcast_to(np.asarray(d, np.uint64), hs.shape)) & M32
        r1, r2 = uniform01(hs, depth, 2), uniform01(hs, depth, 3)
        fold = (r1 + r2).astype(f32) > 1
        r1 = np.where(fold, (f32(1) - r1).astype(f32), r1).astype(f32)
        r2 = np.where(fold, (f32(1) - r2).astype(f32), r2).astype(f32)
        return r1, r2

    def sample(self, hs, d):
        """the draw of segment d of sample key hs (scalars or arrays) -> (t, Q [.., 3] binary32)"""
        hs = np.atleast_1d(np.asarray(hs, np.uint64))
        depth = (np.uint64(1 << 27) + np.broadcast_to(np.asarray(d, np.uint64), hs.shape)) & M32
        t, _ = self.pick(uniform24(hs, depth, 0), uniform24(hs, depth, 1))
        r1, r2 = self.barycentrics(hs, d)
        Q = ((self.A[t] + (r1[:, None] * self.e1[t]).astype(f32)).astype(f32) + (r2[:, None] * self.e2[t]).astype(f32)).astype(f32)
        return t, Q

    def weight(self, t, Q, P, N):
        """g of the draw (t, Q) at the diffuse hit P with normal N: (mx cl A2 total) / (2 c d2) in binary64, rounded to binary32 once -> (g, wl, d2)"""
        t = np.atleast_1d(np.asarray(t, np.int64))
        Q, P, N = np.asarray(Q, f32).reshape(-1, 3), np.asarray(P, f32).reshape(-1, 3), np.asarray(N, f32).reshape(-1, 3)
        v = (Q - P).astype(f32)
        d2 = _dot(v, v)
        wl = (v / np.sqrt(d2).astype(f32)[:, None]).astype(f32)
        mx = np.maximum(_dot(N, wl), f32(0))
        nn = (self.Nt[t] / self.A2[t][:, None]).astype(f32)
        cl = np.abs(_dot(nn, wl))
        num = ((mx.astype(np.float64) * cl.astype(np.float64)) * self.A2[t].astype(np.float64)) * float(self.total)
        den = (2.0 * self.c[t].astype(np.float64)) * d2.astype(np.float64)
        return (num / den).astype(f32), wl, d2

    def aim(self, Q, Pa):
        """L' = Q + KAPPA (Pa - Q) per component: where the shadow ray to Q ends"""
        Q, Pa = np.asarray(Q, f32), np.asarray(Pa, f32)
        return (Q + (KAPPA * (Pa - Q).astype(f32)).astype(f32)).astype(f32)


import math  # noqa: E402

from oracle import oracle_py as _orc  # noqa: E402
from . import soft_lights_model as _slm  # noqa: E402
from .lights_model import PI as _PI, _cross as _c3, _dot as _d3, _norm2 as _n2, _normalize as _nz, _v  # noqa: E402
from .sky_sample_model import sample_key  # noqa: E402


def effective_share(share, table, total_intensity):
    """0 if there is no table, it is empty or the share is 0; 1 if the lights give nothing; the share otherwise"""
    if table is None or table.total == 0 or not share > 0:
        return f32(0)
    return f32(1) if float(total_intensity) == 0.0 else f32(share)


class Walker(_slm.Walker):
    """soft_lights_model.Walker with emitters: emission = {object id: (r, g, b)} and the table of the scene's triangles in stored order (a TriTable whose rows carry the
    radiance of their mesh).  A continuation ray whose nearest object emits ends the path there and starts the fold from E (the hit rule); a diffuse segment's one
    shadow ray goes to a point of an emitter iff uniform01(hs, d + 1, 3) <= s and is then a point light's shadow ray to L' = Q + KAPPA (Pa - Q); the fold runs per
    channel.  The intersections are the oracle's.  With no emitter it calls the walker underneath: bit for bit soft_lights_model.Walker."""

    def __init__(self, scene, mats, lights, radii=None, emission=None, table=None, share=0.5, **kw):
        super().__init__(scene, mats, lights, [0.0] * len(lights) if radii is None else radii, **kw)
        self.emission = {int(k): np.asarray(v, f32) for k, v in (emission or {}).items() if np.asarray(v, f32).any()}
        self.table = table if self.emission else None
        self.s = effective_share(share, self.table, self.total)
        self.w_emit = f32(1) / self.s if self.s > 0 else f32(0)
        self.w_light = f32(1) / (f32(1) - self.s) if self.s < 1 else f32(0)

    def path(self, O, u, segs, pixel, samp):
        if not self.emission:
            return super().path(O, u, segs, pixel, samp)
        sc, eps = self.scene, self.eps
        hs = sample_key(self.seed, pixel, samp)
        refr = f32(1)
        seg = []
        rays = 0
        E = _v(0, 0, 0)
        after_diffuse = False
        for d in range(segs):
            rays += 1
            hit, oid, P, N = sc.intersect_all(O, u, self.tri_tmin)
            if not hit:
                break
            if oid in self.emission:                                    # the path ends on the emitter
                if not (after_diffuse and self.s > 0):
                    E = self.emission[oid]
                break
            alb, mirror, n_in, n_out = self.mats[oid]
            after_diffuse = False
            if mirror:
                O = P + eps * N
                u = u - f32(2 * _d3(u, N)) * N
            elif n_in != n_out:
                out2in = refr == n_out
                if out2in:
                    ratio = f32(n_out / n_in)
                else:
                    ratio = f32(n_in / n_out)
                    N = -N
                un = _d3(u, N)
                k = f32(f32(ratio * ratio) * f32(f32(1) - f32(un * un)))
                if ((out2in and refr > n_in) or (not out2in and refr > n_out)) and k > 1:
                    O = P + eps * N
                    u = u - f32(2 * un) * N
                else:
                    O = P - eps * N
                    u = f32(-np.sqrt(f32(f32(1) - k))) * N + ratio * (u - un * N)
                    refr = n_in if out2in else n_out
            else:
                after_diffuse = True
                if self.surface is not None:
                    alb = self.surface(oid, O, u, alb)
                Pa = P + eps * N
                rays += 1
                r_s = f32(_orc.uniform(self.seed, pixel, samp, d + 1, 3))
                if r_s <= self.s:
                    t, Q = self.table.sample(hs, d)
                    g, _, _ = self.table.weight(t, Q, P, N)
                    l3 = (self.w_emit * (g[0] * self.table.le[t[0]]).astype(f32)).astype(f32)
                    L = self.table.aim(Q[0], Pa)
                else:
                    _, L = self.light_point(pixel, samp, d)
                    mx = max(_d3(N, _nz(L - P)), f32(0))
                    lvis = f32(float(self.total) / (4 * _PI * float(_n2(L - P))) * float(mx))
                    lv = f32(lvis * self.w_light)
                    l3 = _v(lv, lv, lv)
                to = L - Pa
                shit, _, Pp, _ = sc.intersect_all(Pa, to / np.sqrt(_n2(to)), self.tri_tmin)
                blocked = shit and _n2(Pp - Pa) <= _n2(L - Pa)
                seg.append((_v(0, 0, 0) if blocked else l3, alb))
                if d + 1 >= segs:
                    break
                r1, r2 = f32(_orc.uniform(self.seed, pixel, samp, d, 0)), f32(_orc.uniform(self.seed, pixel, samp, d, 1))
                s1 = np.sqrt(f32(f32(1) - r2))
                x = f32(math.cos(2 * _PI * float(r1)) * float(s1))
                y = f32(math.sin(2 * _PI * float(r1)) * float(s1))
                z = np.sqrt(r2)
                T1 = _nz(_v(-N[1], N[0], 0) if (N[1] != 0 and N[0] != 0) else _v(-N[2], 0, N[0]))
                T2 = _c3(N, T1)
                u = (x * T1 + y * T2) + z * N
                O = Pa
                refr = f32(1)
        ans = E
        for l3, alb in reversed(seg):
            ans = (l3 * alb) / f32(_PI) + alb * ans
        return ans, rays
