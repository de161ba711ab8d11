"""Several point lights, restated (a helper module, like still_view.py): the rule of include/raytrace_hip.h "several point lights" -- prefix, pick -- and a scalar path
walker that applies it: Scene::getColor (cpu:566-648) over the oracle's Scene.intersect_all and oracle_py.uniform, in numpy binary32, with the bounce, the fold and the ray
count of csrc/rt_shade.hip.h.  The oracle's scene knows geometry only through intersect_all, so the walker carries the materials itself: one (albedo, mirror, n_in, n_out)
per object id, in the order the objects were added.  With one light it is Scene.render bit for bit (tests/test_lights_model.py holds it to that first)."""
import math

import numpy as np

from oracle import oracle_py as orc

f32 = np.float32
PI = 3.14159265358979323846


def prefix(intensities):
    """prefix[0] = I_0, prefix[k] = fl(prefix[k - 1] + I_k)"""
    out = np.zeros(len(intensities), f32)
    acc = f32(0)
    for k, i in enumerate(intensities):
        acc = f32(i) if k == 0 else f32(acc + f32(i))
        out[k] = acc
    return out


def pick(pre, r):
    """the least k with prefix[k] >= x and prefix[k] > 0 for x = fl(r * total); r a binary32 scalar or array in (0, 1]"""
    pre = np.asarray(pre, f32)
    x = (np.asarray(r, f32) * pre[-1]).astype(f32)
    ok = (pre >= x[..., None]) & (pre > 0)
    assert ok.any(axis=-1).all()
    return np.argmax(ok, axis=-1)


def materials(spheres, meshes=()):
    """per object id (albedo, mirror, n_in, n_out) of a scene_upload argument list: the meshes at their object_slot, the spheres in the places left"""
    n = len(spheres) + len(meshes)
    out = [None] * n
    for m in meshes:
        out[m["object_slot"]] = (np.asarray(m["albedo"], f32), int(m.get("mirror", 0)), f32(m.get("in_refraction_index", 1.0)),
                                 f32(m.get("out_refraction_index", 1.0)))
    it = iter(spheres)
    for k in range(n):
        if out[k] is None:
            s = next(it)
            out[k] = (np.asarray(s[2], f32), int(s[3]) if len(s) > 3 else 0, f32(s[4]) if len(s) > 4 else f32(1), f32(s[5]) if len(s) > 5 else f32(1))
    return out


def _v(*a):
    return np.array(a, f32)


def _dot(a, b):
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def _norm2(a):
    return _dot(a, a)


def _normalize(a):
    return a / np.sqrt(_norm2(a))


def _cross(a, b):
    return _v(a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def camera_z(W, fov):
    return f32(-f32(W) / f32(2 * f32(math.tan(float(f32(fov / f32(2)))))))


class Walker:
    """scene: an oracle Scene (its own light is not read); mats: materials(); lights: [(position, intensity)]"""

    def __init__(self, scene, mats, lights, eps=1e-3, tri_tmin=1e-4, seed=123456, cam=(0, 0, 55), fov=None):
        self.scene, self.mats = scene, mats
        self.pos = [np.asarray(p, f32) for p, _ in lights]
        self.pre = prefix([i for _, i in lights])
        self.total = self.pre[-1]
        self.eps, self.tri_tmin, self.seed = f32(eps), tri_tmin, seed
        self.cam = np.asarray(cam, f32)
        self.fov = f32(np.pi / 3) if fov is None else f32(fov)
        self.picks = []                              # (pixel, sample, segment, light, lit) of every diffuse segment walked

    def light_of(self, pixel, samp, d):
        r = f32(orc.uniform(self.seed, pixel, samp, d + 1, 2))
        return int(pick(self.pre, r))

    def path(self, O, u, segs, pixel, samp):
        """-> (colour, rays): segments 0 .. segs - 1 of the path that starts with the ray (O, u)"""
        sc, eps = self.scene, self.eps
        refr = f32(1)
        seg = []                                      # (l, albedo) of the diffuse segments, front to back
        rays = 0
        for d in range(segs):
            rays += 1
            hit, oid, P, N = sc.intersect_all(O, u, self.tri_tmin)
            if not hit:
                break
            alb, mirror, n_in, n_out = self.mats[oid]
            if mirror:                                                   # cpu:573-579
                O = P + eps * N
                u = u - f32(2 * _dot(u, N)) * N
            elif n_in != n_out:                                          # cpu:580-604
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
            else:                                                        # cpu:605-645, the light picked by the rule
                k = self.light_of(pixel, samp, d)
                L = self.pos[k]
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
        for l, alb in reversed(seg):                                     # fold_segment, back to front
            ans = (l * alb) / f32(PI) + alb * ans
        return ans, rays

    def render(self, W, H, spp=1, num_bounce=0, pose=None, rows=None):
        """-> [rows, W, 4] as Scene.render gives it (cpu_launcher's depth convention: num_bounce + 1 segments); pose = (yaw, pitch): realtime_render.cu's camera;
        rows: the image rows to render (default: all)"""
        z = camera_z(W, self.fov)
        basis = orc.camera_basis(*pose) if pose is not None else None
        rows = list(range(H)) if rows is None else list(rows)
        out = np.zeros((len(rows), W, 4), f32)
        inv_n = f32(1.0 / spp)
        for ii, i in enumerate(rows):
            for j in range(W):
                uc = _v(f32(float(f32(f32(j) - f32(W) / f32(2))) + 0.5), f32(float(f32(f32(H) / f32(2) - f32(i))) - 0.5), z)
                if basis is not None:
                    uc = ((self.cam + basis[2] * uc[2]) + basis[0] * uc[0]) + basis[1] * uc[1]
                u0 = _normalize(uc)                                      # sigma == 0: the jitter is exactly +-0
                tot, nrays = _v(0, 0, 0), 0
                for s in range(spp):
                    c, r = self.path(self.cam, u0, num_bounce + 1, i * W + j, s)
                    tot = tot + (c * inv_n if basis is not None else c)
                    nrays += r
                out[ii, j, :3] = tot if basis is not None else tot / f32(spp)
                out[ii, j, 3] = nrays
        return out
