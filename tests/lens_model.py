"""The thin lens, restated (a helper module, like soft_lights_model.py): the rule of include/raytrace_hip.h "thin lens" -- the point (dx, dy) of the unit disc, the ray
(O', u') from the lens point through the pinhole ray's point on the plane of focus -- in numpy binary32, and a path walker that is soft_lights_model.Walker (with every
radius 0: lights_model.Walker) started on that ray.  With R == 0 it is that walker bit for bit (tests/test_lens_model.py holds it to that, and to the oracle, before any
kernel is held to it).  sigma stays 0: the walkers it rests on do not restate the jitter."""
import math

import numpy as np

from oracle import oracle_py as orc
from . import lights_model as lm
from . import soft_lights_model as sm
from .lights_model import PI, _normalize, _v, f32

D = 1 << 28                                          # the two draws sit at depth D: D * 4 + dim = 2^30 + dim
FIXED = (_v(1, 0, 0), _v(0, 1, 0), _v(0, 0, -1))     # (ex, ey, a) of the fixed camera


def disc(r1, r2):
    """s = sqrt(r1), dx = (float)(cos(2 pi r2) s), dy = (float)(sin(2 pi r2) s); binary32 scalars or arrays -> (dx, dy, s)"""
    r1, r2 = np.asarray(r1, f32), np.asarray(r2, f32)
    s = np.sqrt(r1).astype(f32)
    a = 2 * PI * r2.astype(np.float64)
    if a.ndim == 0:
        cs, sn = math.cos(float(a)), math.sin(float(a))             # the walker: libm's, as lights_model's bounce
    else:
        cs, sn = np.cos(a), np.sin(a)
    dx = np.asarray(cs * s.astype(np.float64)).astype(f32)
    dy = np.asarray(sn * s.astype(np.float64)).astype(f32)
    return dx, dy, s


def lens_ray(O, u, basis, R, f, r1, r2):
    """-> (O', u').  O [3]; u [..., 3]; basis (ex, ey, a); r1, r2 broadcast against u's leading shape.  One rounding per operation; where !(c > 0) the ray stays (O, u)."""
    O, u = np.asarray(O, f32), np.asarray(u, f32)
    ex, ey, a = (np.asarray(b, f32) for b in basis)
    R, f = f32(R), f32(f)
    with np.errstate(all="ignore"):
        c = ((u[..., 0] * a[0]).astype(f32) + (u[..., 1] * a[1]).astype(f32)).astype(f32) + (u[..., 2] * a[2]).astype(f32)
        c = np.asarray(c, f32)
        t = np.asarray(f / c, f32)
        F = (O + (t[..., None] * u).astype(f32)).astype(f32)
        dx, dy, _ = disc(r1, r2)
        lx, ly = np.asarray(R * dx, f32), np.asarray(R * dy, f32)
        O2 = ((O + (lx[..., None] * ex).astype(f32)).astype(f32) + (ly[..., None] * ey).astype(f32)).astype(f32)
        d = (F - O2).astype(f32)
        n2 = ((d[..., 0] * d[..., 0]).astype(f32) + (d[..., 1] * d[..., 1]).astype(f32)).astype(f32) + (d[..., 2] * d[..., 2]).astype(f32)
        u2 = (d / np.sqrt(np.asarray(n2, f32))[..., None]).astype(f32)
    ok = np.asarray(c > 0)[..., None]
    return np.where(ok, O2, np.broadcast_to(O, O2.shape)).astype(f32), np.where(ok, u2, np.broadcast_to(u, u2.shape)).astype(f32)


def pixel_dir(W, H, i, j, z):
    """the un-normalised direction of pixel (row i, column j), as lights_model.Walker.render forms it"""
    return _v(f32(float(f32(f32(j) - f32(W) / f32(2))) + 0.5), f32(float(f32(f32(H) / f32(2) - f32(i))) - 0.5), z)


class Walker(sm.Walker):
    """soft_lights_model.Walker behind a lens = (R, f); radii None: point lights"""

    def __init__(self, scene, mats, lights, radii=None, lens=(0.0, 1.0), **kw):
        super().__init__(scene, mats, lights, [0.0] * len(lights) if radii is None else radii, **kw)
        self.R, self.f = f32(lens[0]), f32(lens[1])

    def camera_ray(self, u0, basis, pixel, samp):
        """-> (O', u') of sample samp of the pixel whose pinhole direction is u0"""
        if not self.R > 0:
            return self.cam, u0
        r1 = f32(orc.uniform(self.seed, pixel, samp, np.uint32(D), 0))
        r2 = f32(orc.uniform(self.seed, pixel, samp, np.uint32(D), 1))
        return lens_ray(self.cam, u0, basis, self.R, self.f, r1, r2)

    def render(self, W, H, spp=1, num_bounce=0, pose=None, rows=None):
        """lights_model.Walker.render with each sample's own camera ray"""
        z = lm.camera_z(W, self.fov)
        basis = orc.camera_basis(*pose) if pose is not None else None
        lens_basis = (basis[0], basis[1], -basis[2]) if pose is not None else FIXED
        rows = list(range(H)) if rows is None else list(rows)
        out = np.zeros((len(rows), W, 4), f32)
        inv_n = f32(1.0 / spp)
        for ii, i in enumerate(rows):
            for j in range(W):
                uc = pixel_dir(W, H, i, j, z)
                if basis is not None:
                    uc = ((self.cam + basis[2] * uc[2]) + basis[0] * uc[0]) + basis[1] * uc[1]
                u0 = _normalize(uc)                                      # sigma == 0: the jitter is exactly +-0
                tot, nrays = _v(0, 0, 0), 0
                for s in range(spp):
                    O, u = self.camera_ray(u0, lens_basis, i * W + j, s)
                    c, r = self.path(O, u, num_bounce + 1, i * W + j, s)
                    tot = tot + (c * inv_n if basis is not None else c)
                    nrays += r
                out[ii, j, :3] = tot if basis is not None else tot / f32(spp)
                out[ii, j, 3] = nrays
        return out


# ---- the circle of confusion as a known answer: one small diffuse sphere on the axis, in front of nothing ---------------------------------------------------------------------
# 96 x 64, fov pi / 3: |z| = 96 / (2 tan(pi / 6)) = 83.14 pixels.  The sphere of radius COC_RHO sits at depth COC_DZ in front of the camera at (0, 0, 55), the lens of radius
# COC_R focuses at COC_F.  Paraxial: the pinhole image has the radius |z| rho / Dz = 2.08 pixels, a point at depth Dz spreads over a disc of radius
# |z| R |Dz - f| / (Dz f) = 5.20 pixels (>= 4, as the test wants it).
COC_W, COC_H, COC_SPP = 96, 64, 64
COC_CAM = (0.0, 0.0, 55.0)
COC_RHO, COC_DZ, COC_R, COC_F = 0.5, 20.0, 2.5, 40.0
COC_SPHERE = ((0.0, 0.0, COC_CAM[2] - COC_DZ), COC_RHO, (0.5, 0.5, 0.5))
COC_LIGHT = ((0.0, 10.0, 55.0), 3e10)


def coc_radii():
    """-> (pinhole image radius, circle-of-confusion radius) in pixels"""
    z = abs(float(lm.camera_z(COC_W, f32(np.pi / 3))))
    return z * COC_RHO / COC_DZ, z * COC_R * abs(COC_DZ - COC_F) / (COC_DZ * COC_F)


def coc_pixel_radius():
    """[H, W] distance of every pixel's centre from the image centre, in pixels"""
    x = np.arange(COC_W, dtype=np.float64) - COC_W / 2 + 0.5
    y = COC_H / 2 - np.arange(COC_H, dtype=np.float64) - 0.5
    return np.hypot(x[None, :], y[:, None])


def coc_check(frame):
    """the two statements about a frame of the scene above (one segment, COC_SPP samples); a pixel contributes when one of its samples hit the sphere (it then counts a
    shadow ray: .w > spp).  -> (largest radius of a contributing pixel, the bound it stays under, the radius it must reach)"""
    a, b = coc_radii()
    assert b >= 4.0
    r = coc_pixel_radius()
    hit = frame[..., 3] > COC_SPP
    assert hit.any()
    reach = float(r[hit].max())
    assert reach <= a + b + 1.5, (reach, a + b + 1.5)
    assert reach >= a + b / 2, (reach, a + b / 2)
    assert ((frame[..., :3] > 0).any(-1) <= hit).all()               # colour only where the sphere was hit
    return reach, a + b + 1.5, a + b / 2


def coc_walker(oracle, lens=(COC_R, COC_F)):
    sc = oracle.Scene()
    sc.add_sphere(*COC_SPHERE)
    return Walker(sc, lm.materials([COC_SPHERE]), [COC_LIGHT], lens=lens, cam=COC_CAM)


def coc_frame(oracle, lens=(COC_R, COC_F)):
    """Walker.render(96, 64, 64, 0) of the scene above without walking the paths that cannot meet the sphere: a sample whose ray passes the centre at more than
    rho (1 + 1e-3) -- in binary64, from a vectorised evaluation of the rule whose rays differ from the walker's by a few binary32 ulps, 1e-6 of rho -- is a miss: one ray,
    colour +0, and x + 0 = x leaves the pixel's sum what the walker's is.  Every other sample is walked by the walker itself, on its own (scalar) ray."""
    W, H, spp = COC_W, COC_H, COC_SPP
    w = coc_walker(oracle, lens)
    z = lm.camera_z(W, w.fov)
    u0 = np.zeros((H, W, 3), f32)
    for i in range(H):
        for j in range(W):
            u0[i, j] = _normalize(pixel_dir(W, H, i, j, z))
    if w.R > 0:
        r = np.array([[orc.uniform(w.seed, p, s, np.uint32(D), dim) for dim in (0, 1)] for p in range(H * W) for s in range(spp)], f32).reshape(H, W, spp, 2)
        O, u = lens_ray(w.cam, u0[:, :, None, :], FIXED, w.R, w.f, r[..., 0], r[..., 1])
    else:
        O, u = np.broadcast_to(w.cam, (H, W, spp, 3)), np.broadcast_to(u0[:, :, None, :], (H, W, spp, 3))
    to = np.asarray(COC_SPHERE[0], np.float64) - O.astype(np.float64)
    ud = u.astype(np.float64)
    along = (to * ud).sum(-1) / np.sqrt((ud * ud).sum(-1))
    dist = np.sqrt(np.maximum((to * to).sum(-1) - along * along, 0.0))
    near = dist <= COC_RHO * (1 + 1e-3)
    out = np.zeros((H, W, 4), f32)
    out[..., 3] = spp
    for i, j in zip(*np.nonzero(near.any(-1))):
        tot, nrays = _v(0, 0, 0), 0
        for s in range(spp):
            if near[i, j, s]:
                Os, us = w.camera_ray(u0[i, j], FIXED, i * W + j, s)
                c, n = w.path(Os, us, 1, i * W + j, s)
            else:
                c, n = _v(0, 0, 0), 1
            tot = tot + c
            nrays += n
        out[i, j, :3] = tot / f32(spp)
        out[i, j, 3] = nrays
    return out
