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


def gradient_sky(zenith, horizon, ground, n):
    """horizon -> zenith with the height above the horizon, horizon -> ground below it (linear in y)"""
    zenith, horizon, ground = (np.asarray(c, np.float64) for c in (zenith, horizon, ground))

    def f(d):
        y = d[..., 1:2].astype(np.float64)
        return np.where(y >= 0, horizon + (zenith - horizon) * y, horizon + (ground - horizon) * -y)
    return from_function(f, n)
