"""The shutter, restated (a helper module, like lens_model.py): the rule of include/raytrace_hip.h "shutter" -- the time tau of a sample, the pose C + d tau of a
sphere centre and of the light -- and a path walker that is lens_model.Walker walking every sample's path in the scene AT THAT SAMPLE'S POSE: a fresh oracle Scene of the
moved spheres and the same Mesh objects, in object order, so that the reference's own intersect_all stays the judge of every hit.  With every displacement +-0 the shutter
is closed and the walker is lens_model.Walker bit for bit (tests/test_shutter_model.py holds it to that, and to the oracle, before any kernel is held to it).  sigma stays 0:
the walkers it rests on do not restate the jitter."""
import numpy as np

from oracle import oracle_py as orc
from . import lens_model as lens
from . import lights_model as lm
from .lights_model import _normalize, _v, f32

D = lens.D                                           # the draw sits at depth D, dim 2: D * 4 + 2 = 2^30 + 2, beside the lens's two
DIM = 2


def tau(seed, pixel, samp):
    """the time of sample samp of the pixel, in (0, 1]: uniform01(hs, 1 << 28, 2)"""
    return f32(orc.uniform(seed, pixel, samp, np.uint32(D), DIM))


def pose(C, dC, t):
    """C + dC t per component, the product first, one rounding each: MoveObject's arithmetic, the oracle's own"""
    return orc.sphere_move(np.asarray(C, f32), np.asarray(dC, f32), float(f32(t)))


def objects(spheres, meshes=None):
    """the scene's objects in the order of Scene::objects: ("mesh", Mesh) at the slots of meshes = {object_slot: oracle Mesh}, ("sphere", upload tuple) in the places left"""
    meshes = dict(meshes or {})
    n = len(spheres) + len(meshes)
    it = iter(spheres)
    return [("mesh", meshes[k]) if k in meshes else ("sphere", tuple(next(it))) for k in range(n)]


def scene_of(objs, motion=None, t=None):
    """a fresh oracle Scene of objs with every sphere at its pose of time t under motion = {object_slot: displacement} (a slot that is not named does not move: its
    displacement is +0, and C + 0 t is formed all the same, as the kernel forms it)"""
    sc = orc.Scene()
    for slot, (kind, o) in enumerate(objs):
        if kind == "mesh":
            sc.add_mesh(o)
            continue
        c = o[0] if motion is None else pose(o[0], motion.get(slot, (0.0, 0.0, 0.0)), t)
        sc.add_sphere(c, o[1], o[2], *o[3:])
    return sc


def is_on(light, motion):
    return bool(any(float(x) != 0 for x in light) or any(float(x) != 0 for v in motion.values() for x in v))


class Walker(lens.Walker):
    """lens_model.Walker over objs = objects(...) whose spheres travel motion[slot] and whose one light travels `light` over the exposure; mats as lights_model.materials"""

    def __init__(self, objs, mats, lights, shutter=((0.0, 0.0, 0.0), {}), **kw):
        assert len(lights) == 1                      # the shutter forms are built for the Scene's one point light
        super().__init__(scene_of(objs), mats, lights, **kw)
        self.objs = objs
        self.dL = tuple(shutter[0]) if shutter[0] is not None else (0.0, 0.0, 0.0)
        self.motion = {int(k): tuple(v) for k, v in (shutter[1] or {}).items()}
        self.on = is_on(self.dL, self.motion)
        self.L0 = self.pos[0]
        self.taus = []                               # every tau drawn

    def path(self, O, u, segs, pixel, samp):
        if not self.on:
            return super().path(O, u, segs, pixel, samp)
        t = tau(self.seed, pixel, samp)
        self.taus.append(t)
        self.scene = scene_of(self.objs, self.motion, t)            # one path sees one instant
        self.pos = [pose(self.L0, self.dL, t)]
        return super().path(O, u, segs, pixel, samp)


# ---- a streak as a known answer: one small diffuse sphere that crosses the view during the exposure --------------------------------------------------------------------------
# 96 x 64, fov pi / 3: |z| = 96 / (2 tan(pi / 6)) = 83.14 pixels.  The sphere of radius RHO starts on the axis at depth DZ in front of the camera at (0, 0, 55) and travels
# DC = (4, 0, 0): its centre's image runs from the image centre 83.14 * 4 / 20 = 16.6 pixels to the right; the paraxial image radius is |z| rho / Dz = 2.08 pixels.
ST_W, ST_H, ST_SPP = 96, 64, 64
ST_CAM = (0.0, 0.0, 55.0)
ST_RHO, ST_DZ = 0.5, 20.0
ST_DC = (4.0, 0.0, 0.0)
ST_SPHERE = ((0.0, 0.0, ST_CAM[2] - ST_DZ), ST_RHO, (0.5, 0.5, 0.5))
ST_LIGHT = ((0.0, 10.0, 55.0), 3e10)
ST_SHUTTER = ((0.0, 0.0, 0.0), {0: ST_DC})


def st_z():
    return abs(float(lm.camera_z(ST_W, f32(np.pi / 3))))


def st_pixel_xy():
    """([H, W] x, [H, W] y) of every pixel's centre on the image plane at distance |z|, in pixels from the image centre"""
    x = np.arange(ST_W, dtype=np.float64) - ST_W / 2 + 0.5
    y = ST_H / 2 - np.arange(ST_H, dtype=np.float64) - 0.5
    return np.broadcast_to(x[None, :], (ST_H, ST_W)), np.broadcast_to(y[:, None], (ST_H, ST_W))


def st_inside(t, rho):
    """[..., H, W]: does the ray through a pixel's centre pass the sphere's centre at time t (binary64 array, C + DC t) within rho?  The exact projected disc."""
    t = np.asarray(t, np.float64)
    c = np.asarray(ST_SPHERE[0], np.float64) - np.asarray(ST_CAM, np.float64) + t[..., None] * np.asarray(ST_DC, np.float64)      # centre as seen from the camera
    x, y = st_pixel_xy()
    d = np.stack([x, y, np.full_like(x, -st_z())], -1)
    d = d / np.sqrt((d * d).sum(-1, keepdims=True))
    cc = c[..., None, None, :]
    along = (cc * d).sum(-1)
    dist2 = (cc * cc).sum(-1) - along * along
    return (along > 0) & (dist2 <= rho * rho)


def st_count_bounds(n=4096):
    """(N_min, N_max): the least number of pixel centres inside the projected disc of radius rho (1 - 1e-3) and the greatest inside that of radius rho (1 + 1e-3), over the
    lattice tau = k / n, k = 1 .. n"""
    t = np.arange(1, n + 1, dtype=np.float64) / n
    lo = min(int(st_inside(t[k:k + 256], ST_RHO * (1 - 1e-3)).sum((-1, -2)).min()) for k in range(0, n, 256))
    hi = max(int(st_inside(t[k:k + 256], ST_RHO * (1 + 1e-3)).sum((-1, -2)).max()) for k in range(0, n, 256))
    return lo, hi


def st_check(frame):
    """the statements about a frame of the scene above (one segment, ST_SPP samples); a pixel contributes when one of its samples hit the sphere (it then counts a shadow
    ray: .w > spp).  -> (largest distance of a contributing pixel from the segment of centres, its bound, least and greatest x of a contributing pixel, the projected end
    centres, hits per sample, N_min, N_max)"""
    z = st_z()
    a = z * ST_RHO / ST_DZ                                             # paraxial image radius
    x0, x1 = 0.0, z * ST_DC[0] / ST_DZ                                 # the projected end centres, on the row y = 0
    x, y = st_pixel_xy()
    hit = frame[..., 3] > ST_SPP
    assert hit.any()
    dist = np.hypot(x - np.clip(x, x0, x1), y)                         # distance from the segment [(x0, 0), (x1, 0)]
    far = float(dist[hit].max())
    assert far <= a + 1.5, (far, a + 1.5)
    lo_x, hi_x = float(x[hit].min()), float(x[hit].max())
    assert lo_x <= x0 and hi_x >= x1, (lo_x, hi_x, x0, x1)             # the contributing pixels reach at least to both projected end centres
    n_min, n_max = st_count_bounds()
    hits = float(frame[..., 3].astype(np.float64).sum() - ST_SPP * ST_W * ST_H)
    assert ST_SPP * n_min <= hits <= ST_SPP * n_max, (hits / ST_SPP, n_min, n_max)
    assert ((frame[..., :3] > 0).any(-1) <= hit).all()                 # colour only where the sphere was hit
    return far, a + 1.5, lo_x, hi_x, x0, x1, hits / ST_SPP, n_min, n_max


def st_walker(shutter=ST_SHUTTER):
    return Walker(objects([ST_SPHERE]), lm.materials([ST_SPHERE]), [ST_LIGHT], shutter=shutter, cam=ST_CAM)


def st_frame(shutter=ST_SHUTTER):
    """Walker.render(96, 64, 64, 0) of the scene above without walking the paths that cannot meet the sphere, as lens_model.coc_frame does it: a sample whose ray passes
    the centre of its time at more than rho (1 + 1e-3), in binary64 from the walker's own binary32 tau and pose, is a miss -- one ray, colour +0, and x + 0 = x leaves the
    pixel's sum what the walker's is.  Every other sample is walked by the walker itself."""
    W, H, spp = ST_W, ST_H, ST_SPP
    w = st_walker(shutter)
    z = lm.camera_z(W, w.fov)
    x, y = st_pixel_xy()
    d = np.stack([x, y, np.full_like(x, -st_z())], -1)
    d = d / np.sqrt((d * d).sum(-1, keepdims=True))
    out = np.zeros((H, W, 4), f32)
    out[..., 3] = spp
    # a pixel further than the image radius and a margin from the segment of centres meets the sphere at no time
    a = st_z() * ST_RHO / ST_DZ
    x1 = st_z() * abs(ST_DC[0]) / ST_DZ
    cand = np.hypot(x - np.clip(x, 0.0, x1), y) <= a + 4.0 if w.on else np.hypot(x, y) <= a + 4.0
    cam = np.asarray(ST_CAM, np.float64)
    for i, j in zip(*np.nonzero(cand)):
        u0 = _normalize(lens.pixel_dir(W, H, i, j, z))
        tot, nrays = _v(0, 0, 0), 0
        for s in range(spp):
            c = np.asarray(ST_SPHERE[0], f32) if not w.on else pose(ST_SPHERE[0], w.motion.get(0, (0.0, 0.0, 0.0)), tau(w.seed, i * W + j, s))
            cc = c.astype(np.float64) - cam
            along = float((cc * d[i, j]).sum())
            near = along > 0 and float((cc * cc).sum()) - along * along <= (ST_RHO * (1 + 1e-3)) ** 2
            if near:
                col, n = w.path(w.cam, u0, 1, i * W + j, s)
            else:
                col, n = _v(0, 0, 0), 1
            tot = tot + col
            nrays += n
        out[i, j, :3] = tot / f32(spp)
        out[i, j, 3] = nrays
    return out
