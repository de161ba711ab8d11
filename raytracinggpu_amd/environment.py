"""Environment maps for Context.set_environment (rt_scene_set_environment; the rule: include/raytrace_hip.h "environment").

A map is an [n, n, 3] float32 array of radiances, row 0 first, in the octahedral layout with +y as the pole: the centre of the map is the zenith, its corners are the
nadir, the left and right mid-edges are -x and +x, the top mid-edge (row 0) is -z -- the way the fixed camera looks -- and the bottom mid-edge +z.  The device looks a
direction up bilinearly, clamped at the border.  Everything here is host-side numpy that MAKES maps; nothing in it is bit-critical.

  texel_directions(n)                         the unit direction of every texel centre, [n, n, 3] (the inverse of the device's mapping)
  from_function(f, n)                         f(directions [n, n, 3]) -> radiances [n, n, 3] (or anything that broadcasts to it), sampled at the texel centres
  from_latlong(img, n)                        an equirectangular float image [H, W, 3] (row 0 = +y, the centre column = -z, +x to its right), resampled bilinearly
  gradient_sky(zenith, horizon, ground, n)    a sky that fades from the horizon's colour to the zenith's above and to the ground's below"""
import numpy as np

MAX_N = 1024                                         # RT_MAX_ENVIRONMENT
TEXEL_END = np.float32(2.0 ** 96)                    # a radiance is finite, not negative and below this


def _check_n(n):
    if not (isinstance(n, (int, np.integer)) and 1 <= n <= MAX_N):
        raise ValueError(f"an environment has n x n texels with 1 <= n <= {MAX_N}, not n = {n!r}")
    return int(n)


def texel_directions(n):
    """[n, n, 3] float32: the unit direction whose lookup lands on the centre of texel (row y, column x)"""
    n = _check_n(n)
    c = (np.arange(n, dtype=np.float64) + 0.5) / n * 2.0 - 1.0          # q = 2 a - 1 at the centres
    qx, qz = np.meshgrid(c, c, indexing="xy")                            # [row (z), column (x)]
    upper = np.abs(qx) + np.abs(qz) <= 1.0
    sg = lambda v: np.where(v < 0, -1.0, 1.0)
    px = np.where(upper, qx, (1.0 - np.abs(qz)) * sg(qx))
    pz = np.where(upper, qz, (1.0 - np.abs(qx)) * sg(qz))
    py = np.where(upper, 1.0 - np.abs(qx) - np.abs(qz), -(np.abs(qx) + np.abs(qz) - 1.0))
    d = np.stack([px, py, pz], axis=-1)
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)


def _as_map(rgb, n):
    a = np.broadcast_to(np.asarray(rgb, np.float32), (n, n, 3)).copy()
    if not (np.isfinite(a).all() and (a >= 0).all() and (a < TEXEL_END).all()):
        raise ValueError("an environment's radiances are finite, not negative and below 2^96")
    return np.abs(a)                                                    # (-0 -> +0: the sign bit is clear)


def from_function(f, n):
    """the map of a radiance function of the direction: f takes [n, n, 3] unit directions"""
    n = _check_n(n)
    return _as_map(f(texel_directions(n)), n)


def from_latlong(img, n):
    """an equirectangular image [H, W, 3], resampled bilinearly at the texel centres' directions: longitude wraps, latitude clamps"""
    n = _check_n(n)
    img = np.asarray(img, np.float64)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"a lat-long image is [H, W, 3], not {img.shape}")
    H, W = img.shape[:2]
    d = texel_directions(n).astype(np.float64)
    lon = np.arctan2(d[..., 0], -d[..., 2])                              # 0 at -z, +pi/2 at +x
    lat = np.arccos(np.clip(d[..., 1], -1.0, 1.0))                       # 0 at +y
    sx = (lon / (2 * np.pi) + 0.5) * W - 0.5
    sy = lat / np.pi * H - 0.5
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = (sx - x0)[..., None], (sy - y0)[..., None]
    xa, xb = x0.astype(int) % W, (x0.astype(int) + 1) % W
    ya, yb = np.clip(y0.astype(int), 0, H - 1), np.clip(y0.astype(int) + 1, 0, H - 1)
    out = (img[ya, xa] * (1 - fx) + img[ya, xb] * fx) * (1 - fy) + (img[yb, xa] * (1 - fx) + img[yb, xb] * fx) * fy
    return _as_map(out, n)


def texel_solid_angles(n):
    """[n, n] float64: the solid angle of every texel, (4 / n^2) / |p|^3 at its centre (p the octahedral point of 1-norm 1); the sum tends to 4 pi"""
    n = _check_n(n)
    c = (np.arange(n, dtype=np.float64) + 0.5) / n * 2.0 - 1.0
    qx, qz = np.meshgrid(c, c, indexing="xy")
    py = 1.0 - np.abs(qx) - np.abs(qz)
    low = py < 0
    px = np.where(low, (1.0 - np.abs(qz)) * np.where(qx < 0, -1.0, 1.0), qx)
    pz = np.where(low, (1.0 - np.abs(qx)) * np.where(qz < 0, -1.0, 1.0), qz)
    return (4.0 / (n * n)) / (px * px + py * py + pz * pz) ** 1.5


def add_sun(rgb, direction, half_angle, radiance):
    """a copy of the map rgb [n, n, 3] with a disc of `radiance` (a number or three) added: every texel whose centre lies within half_angle (radians) of `direction`.
    A disc that holds no centre goes to the nearest texel, its radiance scaled by the disc's solid angle over the texel's: the energy stays what was asked for."""
    a = np.array(rgb, np.float32)
    if a.ndim != 3 or a.shape[0] != a.shape[1] or a.shape[2] != 3:
        raise ValueError(f"an environment is an [n, n, 3] array, not {a.shape}")
    n = _check_n(a.shape[0])
    d = np.asarray(direction, np.float64)
    if d.shape != (3,) or not np.isfinite(d).all() or not np.linalg.norm(d) > 0:
        raise ValueError("the sun's direction is three finite numbers, not all zero")
    if not 0 < half_angle <= np.pi:
        raise ValueError("the sun's half-angle lies in (0, pi]")
    d = d / np.linalg.norm(d)
    rad = np.broadcast_to(np.asarray(radiance, np.float64), (3,))
    cosang = texel_directions(n).astype(np.float64) @ d
    inside = cosang >= np.cos(half_angle)
    if inside.any():
        a[inside] = (a[inside].astype(np.float64) + rad).astype(np.float32)
    else:
        y, x = np.unravel_index(np.argmax(cosang), cosang.shape)
        scale = 2.0 * np.pi * (1.0 - np.cos(half_angle)) / texel_solid_angles(n)[y, x]
        a[y, x] = (a[y, x].astype(np.float64) + rad * scale).astype(np.float32)
    return _as_map(a, n)


def gradient_sky(zenith, horizon, ground, n):
    """horizon -> zenith with the height above the horizon, horizon -> ground below it (linear in y)"""
    zenith, horizon, ground = (np.asarray(c, np.float64) for c in (zenith, horizon, ground))

    def f(d):
        y = d[..., 1:2].astype(np.float64)
        return np.where(y >= 0, horizon + (zenith - horizon) * y, horizon + (ground - horizon) * -y)
    return from_function(f, n)
