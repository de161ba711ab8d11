"""numpy binary32 model of a textured mesh's albedo (include/raytrace_hip.h, rt_mesh_set_texture): the barycentrics of the smooth-normal branch, per-corner UV
interpolation, nearest / bilinear filtering with repeat / clamp wrap, and the product with the mesh albedo.  Every operation is one float32 rounding in the order
the device performs it, so the device's uv and albedo are reproduced bit for bit."""
import numpy as np

f32 = np.float32
NEAREST, BILINEAR = 0, 1
REPEAT, CLAMP = 0, 1
LIM = f32(2.0 ** 31)


def default_decode():
    """decode = NULL: byte / 255.0f"""
    return (np.arange(256, dtype=np.float32) / f32(255)).astype(np.float32)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def triangle_records(vertices, tri_vertex_idx):
    """A, e1 = B - A, e2 = C - A, N = e1 x e2 of each triangle, as the upload (and a refit) computes them"""
    v = np.asarray(vertices, np.float32)
    t = np.asarray(tri_vertex_idx, np.int64)
    A, B, Cc = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    e1, e2 = B - A, Cc - A
    return A, e1, e2, _cross(e1, e2)


def barycentrics(A, e1, e2, N, O, u):
    """alpha, beta, gamma of the smooth-normal branch: beta = dot(e2, cross(A - O, u)) / dot(u, N), gamma = -dot(e1, ...) / dot(u, N), alpha = 1 - beta - gamma"""
    O = np.asarray(O, np.float32)
    u = np.asarray(u, np.float32)
    with np.errstate(all="ignore"):
        c = _cross(A - O, u)
        det = _dot(u, N)
        beta = _dot(e2, c) / det
        gamma = -_dot(e1, c) / det
        alpha = (f32(1) - beta) - gamma
    return alpha, beta, gamma


def interpolate_uv(alpha, beta, gamma, uva, uvb, uvc):
    """(alpha uv_a + beta uv_b) + gamma uv_c per component"""
    a, b, g = (np.asarray(x, np.float32)[..., None] for x in (alpha, beta, gamma))
    return (a * uva + b * uvb) + g * uvc


def tex_floor(c):
    """(index, fraction): floor and c - floor(c); a coordinate that is NaN or outside [-2^31, 2^31) is index 0, fraction 0"""
    c = np.asarray(c, np.float32)
    with np.errstate(all="ignore"):
        ok = (c >= -LIM) & (c < LIM)
        f = np.floor(c)
        frac = np.where(ok, c - f, f32(0)).astype(np.float32)
        idx = np.where(ok, f, f32(0)).astype(np.int64)
    return idx, frac


def wrap(i, n, mode):
    i = np.asarray(i, np.int64)
    return np.clip(i, 0, n - 1) if mode == CLAMP else np.mod(i, n)


def texel(texels, decode, x, y):
    """decode[byte] of the first three channels of texel (x, y); row 0 is the top of the image"""
    return np.asarray(decode, np.float32)[np.asarray(texels)[y, x, :3]]


def sample(texels, decode, filt, mode, u, v):
    """the filtered texture at (u, v) -> [..., 3] float32"""
    texels = np.asarray(texels)
    H, W = texels.shape[:2]
    Wf, Hf = f32(W), f32(H)
    u = np.asarray(u, np.float32)
    v = np.asarray(v, np.float32)
    with np.errstate(all="ignore"):
        if filt == NEAREST:
            x, _ = tex_floor(u * Wf)
            y, _ = tex_floor((f32(1) - v) * Hf)
            return texel(texels, decode, wrap(x, W, mode), wrap(y, H, mode))
        x0, fx = tex_floor(u * Wf - f32(0.5))
        y0, fy = tex_floor((f32(1) - v) * Hf - f32(0.5))
        xa, xb = wrap(x0, W, mode), wrap(x0 + 1, W, mode)
        ya, yb = wrap(y0, H, mode), wrap(y0 + 1, H, mode)
        t00, t10, t01, t11 = (texel(texels, decode, x, y) for x, y in ((xa, ya), (xb, ya), (xa, yb), (xb, yb)))
        fx, fy = fx[..., None], fy[..., None]
        gx, gy = f32(1) - fx, f32(1) - fy
        return (t00 * gx + t10 * fx) * gy + (t01 * gx + t11 * fx) * fy


def surface(vertices, tri_vertex_idx, tri_uv_idx, uvs, texels, decode, filt, mode, albedo, tri, O, u):
    """uv [n, 2] and albedo [n, 3] of hits on triangles `tri` (indices into the per-triangle arrays) by rays (O, u) [n, 3]"""
    tri = np.asarray(tri, np.int64)
    A, e1, e2, N = (x[tri] for x in triangle_records(vertices, np.asarray(tri_vertex_idx)))
    a, b, g = barycentrics(A, e1, e2, N, O, u)
    uvs = np.asarray(uvs, np.float32)
    ti = np.asarray(tri_uv_idx, np.int64)[tri]
    uv = interpolate_uv(a, b, g, uvs[ti[:, 0]], uvs[ti[:, 1]], uvs[ti[:, 2]])
    s = sample(texels, decode, filt, mode, uv[:, 0], uv[:, 1])
    return uv, np.asarray(albedo, np.float32) * s
