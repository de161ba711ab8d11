"""Sky sampling, restated (a helper module, like sky_model.py): the rule of include/raytrace_hip.h "sky sampling" -- the table of an environment map in numpy binary32
and Python integers, the draw sample(hs, d) for scalars and arrays, and the estimate's factor g in binary64.  numpy rounds every binary32 operation once, its quotients
and square roots are the correctly rounded ones.  The device is held to this word for word (tests/test_gpu_sky_sample.py); tests/test_sky_sample_model.py holds THIS to
the mathematics: the solid angles, the unbiasedness against a quadrature of sky_model.sky_radiance.  The Walker is sky_model.Walker with the share draw, the sky ray, the miss rule and the three-channel fold."""
import math

import numpy as np

from .sky_model import sky_radiance  # noqa: F401  (what the estimate multiplies)

f32 = np.float32
M32 = 0xFFFFFFFF


def mix32(x):
    """the counter RNG's mixer on uint32 arrays (csrc/rt_kernels.hip.h mix32)"""
    x = np.asarray(x, np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & M32
    x ^= x >> np.uint64(16)
    return x


def uniform24(hs, depth, dim):
    """the 24-bit integer k behind a draw: uniform01 = (k + 1) 2^-24.  hs, depth: uint32 arrays or scalars"""
    key = ((np.asarray(depth, np.uint64) * np.uint64(4) + np.uint64(dim)) & M32) * np.uint64(0x85EBCA77) & M32
    return mix32(np.asarray(hs, np.uint64) ^ key) >> np.uint64(8)


def uniform01(hs, depth, dim):
    return ((uniform24(hs, depth, dim) + np.uint64(1)).astype(f32) * f32(2.0 ** -24)).astype(f32)


def _sg(v):
    return np.where(v < 0, f32(-1), f32(1)).astype(f32)


def oct_q(xs, n):
    """q = fl(2 fl(xs / n) - 1) for binary32 xs"""
    a = (np.asarray(xs, f32) / f32(n)).astype(f32)
    return ((a * f32(2)).astype(f32) - f32(1)).astype(f32)


def oct_point(qx, qz):
    """-> (px, py, pz, m): the octahedral point of 1-norm 1 and m = fl(fl(px px + py py) + pz pz)"""
    qx, qz = np.asarray(qx, f32), np.asarray(qz, f32)
    h = ((f32(1) - np.abs(qx)).astype(f32) - np.abs(qz)).astype(f32)
    low = h < 0
    px = np.where(low, ((f32(1) - np.abs(qz)).astype(f32) * _sg(qx)).astype(f32), qx).astype(f32)
    pz = np.where(low, ((f32(1) - np.abs(qx)).astype(f32) * _sg(qz)).astype(f32), qz).astype(f32)
    m = (((px * px).astype(f32) + (h * h).astype(f32)).astype(f32) + (pz * pz).astype(f32)).astype(f32)
    return px, h, pz, m


class Table:
    """the sampling table of env [n, n, 3]: W [n * n] binary32, c [n * n] uint32, prefix [n * n] uint64 (inclusive), total (a Python int; 0: the table is empty)"""

    def __init__(self, env):
        env = np.ascontiguousarray(env, f32)
        n = env.shape[0]
        assert env.shape == (n, n, 3) and 1 <= n <= 1024
        self.n, self.env = n, env
        Y = ((env[..., 0] + env[..., 1]).astype(f32) + env[..., 2]).astype(f32)
        idx = np.arange(n)
        b9 = None
        for dy in (-1, 0, 1):
            yy = np.clip(idx + dy, 0, n - 1)
            for dx in (-1, 0, 1):
                xx = np.clip(idx + dx, 0, n - 1)
                term = Y[np.ix_(yy, xx)]
                b9 = term.copy() if b9 is None else (b9 + term).astype(f32)
        q = oct_q((idx.astype(f32) + f32(0.5)).astype(f32), n)
        qx, qz = np.meshgrid(q, q, indexing="xy")                       # [row (z), column (x)]
        _, _, _, m = oct_point(qx, qz)
        self.m_centre = m
        self.B9 = b9
        self.W = (b9 / (m * np.sqrt(m).astype(f32)).astype(f32)).astype(f32).ravel()
        wmax = self.W.max()
        if wmax == 0:
            self.c = np.zeros(n * n, np.uint32)
        else:
            k = ((self.W / wmax).astype(f32) * f32(2.0 ** 31)).astype(f32).astype(np.uint64)
            self.c = np.where(self.W > 0, np.maximum(k, np.uint64(1)), np.uint64(0)).astype(np.uint32)
        self.prefix = np.cumsum(self.c.astype(np.uint64), dtype=np.uint64)
        self.total = int(self.prefix[-1])

    def pick(self, ka, kb):
        """the texel of the 24-bit integers (ka, kb): K = ka 2^24 + kb, X = ((K total) >> 48) + 1, the least t with prefix[t] >= X.  Python integers: the product is exact."""
        ka, kb = np.atleast_1d(np.asarray(ka, np.uint64)), np.atleast_1d(np.asarray(kb, np.uint64))
        K = (ka << np.uint64(24)) | kb
        if K.size <= 4096:                                              # Python integers: the product is exact as written
            X = np.array([((int(k) * self.total) >> 48) + 1 for k in K], np.uint64)
        else:
            # the same in 64-bit pieces: total = th 2^24 + tl (th < 2^28), K total = ka th 2^48 + (ka tl + kb th) 2^24 + kb tl, so
            # floor(K total / 2^48) = ka th + floor((ka tl + kb th + floor(kb tl / 2^24)) / 2^24); every product is below 2^52 and every sum below 2^54
            tl, th = np.uint64(self.total & 0xFFFFFF), np.uint64(self.total >> 24)
            mid = ka * tl + kb * th + ((kb * tl) >> np.uint64(24))
            X = ka * th + (mid >> np.uint64(24)) + np.uint64(1)
        return np.searchsorted(self.prefix, X, side="left").astype(np.int64), X

    def sample(self, hs, d):
        """the draw of segment d of sample key hs (scalars or arrays) -> (t, w [.., 3] binary32, m, r)"""
        hs = np.atleast_1d(np.asarray(hs, np.uint64))
        depth = (np.uint64(3 << 28) + np.broadcast_to(np.asarray(d, np.uint64), hs.shape)) & M32
        t, _ = self.pick(uniform24(hs, depth, 0), uniform24(hs, depth, 1))
        y, x = t // self.n, t % self.n
        jx, jz = uniform01(hs, depth, 2), uniform01(hs, depth, 3)
        qx = oct_q((x.astype(f32) + jx).astype(f32), self.n)
        qz = oct_q((y.astype(f32) + jz).astype(f32), self.n)
        px, py, pz, m = oct_point(qx, qz)
        r = np.sqrt(m).astype(f32)
        w = np.stack([(px / r).astype(f32), (py / r).astype(f32), (pz / r).astype(f32)], axis=-1)
        return t, w, m, r

    def weight(self, t, m, r, mx=1.0):
        """g = mx / pdf: binary64, rounded to binary32 once"""
        num = (np.asarray(mx, f32).astype(np.float64) * 4.0) * float(self.total)
        den = ((self.c[t].astype(np.float64) * float(self.n * self.n)) * np.asarray(m, f32).astype(np.float64)) * np.asarray(r, f32).astype(np.float64)
        return (num / den).astype(f32)


def sample_key(seed, pixel, samp):
    """the sample key hs of (seed, pixel, sample): the oracle's or_uniform hashes depth and dim into this"""
    h = mix32(np.uint64(pixel) ^ mix32(np.uint64(seed)))
    return int(mix32(h ^ ((np.uint64(samp) * np.uint64(0x9E3779B1)) & M32)))


def effective_share(share, table, total_intensity):
    """0 if there is no table or it is empty, 1 if the lights give nothing, the share otherwise"""
    if table is None or table.total == 0 or not share > 0:
        return f32(0)
    return f32(1) if float(total_intensity) == 0.0 else f32(share)


from oracle import oracle_py as _orc  # noqa: E402
from . import sky_model as _sky  # noqa: E402
from .lights_model import PI as _PI, _cross, _dot, _norm2, _normalize, _v  # noqa: E402


class Walker(_sky.Walker):
    """sky_model.Walker with the share draw: a diffuse segment's one shadow ray goes to the sky iff uniform01(hs, d + 1, 3) <= s -- blocked iff anything at all is hit --
    and otherwise to the list's light, weighted; a miss behind a diffuse segment starts the fold from +0; the fold runs per channel.  With s == 0 it calls the walker
    underneath: bit for bit sky_model.Walker."""

    def __init__(self, scene, mats, lights, radii=None, env=None, share=0.0, **kw):
        super().__init__(scene, mats, lights, radii, env=env, **kw)
        self.table = Table(self.env) if (self.env is not None and share > 0) else None
        self.s = effective_share(share, self.table, self.total)
        self.w_sky = f32(1) / self.s if self.s > 0 else f32(0)
        self.w_light = f32(1) / (f32(1) - self.s) if 0 < self.s < 1 else f32(0)

    def path(self, O, u, segs, pixel, samp):
        if not self.s > 0:
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
                if not after_diffuse:
                    E = sky_radiance(self.env, np.asarray(u, f32))
                break
            alb, mirror, n_in, n_out = self.mats[oid]
            after_diffuse = False
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
                after_diffuse = True
                if self.surface is not None:
                    alb = self.surface(oid, O, u, alb)
                Pa = P + eps * N
                rays += 1
                r_s = f32(_orc.uniform(self.seed, pixel, samp, d + 1, 3))
                if r_s <= self.s:
                    t, w, m, r = self.table.sample(hs, d)
                    w = w[0]
                    dn = _dot(N, w)
                    g = self.table.weight(t, m, r, f32(0) if dn < 0 else dn)[0]
                    Es = sky_radiance(self.env, w)
                    l3 = (self.w_sky * (g * Es)).astype(f32)
                    blocked, _, _, _ = sc.intersect_all(Pa, w, self.tri_tmin)
                else:
                    _, L = self.light_point(pixel, samp, d)
                    to = L - Pa
                    shit, _, Pp, _ = sc.intersect_all(Pa, to / np.sqrt(_norm2(to)), self.tri_tmin)
                    blocked = shit and _norm2(Pp - Pa) <= _norm2(L - Pa)
                    dn = _dot(N, _normalize(L - P))
                    lvis = f32(float(self.total) / (4 * _PI * float(_norm2(L - P))) * float(max(dn, f32(0))))
                    lv = f32(lvis * self.w_light)
                    l3 = _v(lv, lv, lv)
                seg.append((_v(0, 0, 0) if blocked else l3, alb))
                if d + 1 >= segs:
                    break
                r1, r2 = f32(_orc.uniform(self.seed, pixel, samp, d, 0)), f32(_orc.uniform(self.seed, pixel, samp, d, 1))
                s1 = np.sqrt(f32(f32(1) - r2))
                x = f32(math.cos(2 * _PI * float(r1)) * float(s1))
                y = f32(math.sin(2 * _PI * float(r1)) * float(s1))
                z = np.sqrt(r2)
                T1 = _normalize(_v(-N[1], N[0], 0) if (N[1] != 0 and N[0] != 0) else _v(-N[2], 0, N[0]))
                T2 = _cross(N, T1)
                u = (x * T1 + y * T2) + z * N
                O = Pa
                refr = f32(1)
        ans = E
        for l3, alb in reversed(seg):
            ans = (l3 * alb) / f32(_PI) + alb * ans
        return ans, rays
