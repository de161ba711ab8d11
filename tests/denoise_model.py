"""Reference model of rt_denoise and of the pixel-centre camera ray of rt_render_aov (test infrastructure, like tests/texture_model.py).

numpy binary32 throughout: every operation one rounding, in the order include/raytrace_hip.h states, so the device's frames are held to it bit for bit.  The 25
taps of a pass are vectorised over the image; the order in which they are accumulated (dy outer, dx inner) is the contract's.  max is maxNum (np.fmax), as the
header states; tests/scalar_filter_reference.py is the same contract as plain loops, and tests/test_synthetic_filters_model.py holds this model to it."""
import numpy as np

F = np.float32
H3 = np.array([0.375, 0.25, 0.0625], np.float32)


def _sqdiff(a, b):
    x, y, z = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (x * x + y * y) + z * z


def _term(d, k):
    """max(0, 1 - d k); a k of exactly 0 makes the term exactly 1 (no operation at all)"""
    k = F(k)
    if k == 0:
        return None
    return np.fmax(F(0), F(1) - d * k)                               # maxNum, as the kernel's fmaxf: a NaN distance gives a term of 0


DIV_LO, DIV_HI = F(2.0 ** -60), F(2.0 ** 60)                          # rt_div.h's kDivLo, kDivHi


def div_in_range(x):
    """rt_div.h's div_in_range: where the shared sequence is the quotient; False for NaN"""
    with np.errstate(all="ignore"):
        return (np.abs(x) >= DIV_LO) & (np.abs(x) <= DIV_HI)


class TapStats:
    """What the taps of one pass did, per pixel, for the stats= of the models: which far taps (2 s away along a row, along a column) were taken, whether a tap was dropped by its id,
    whether taps came from both sides of a seam of the kernel's 32 x 8 tiles of a sub-image."""
    TILE_W, TILE_H = 32, 8

    def __init__(self, Hh, W, s):
        self.s = s
        self.ys, self.xs = np.meshgrid(np.arange(Hh), np.arange(W), indexing="ij")
        self.far_x, self.far_y, self.dropped, self.own, self.other = (np.zeros((Hh, W), bool) for _ in range(5))

    def tap(self, dx, dy, inside, ok, take, qx, qy):
        if abs(dx) == 2 and dy == 0:
            self.far_x |= take
        if abs(dy) == 2 and dx == 0:
            self.far_y |= take
        self.dropped |= inside & ~ok
        same = (qx // self.s // self.TILE_W == self.xs // self.s // self.TILE_W) & (qy // self.s // self.TILE_H == self.ys // self.s // self.TILE_H)
        self.own |= take & same
        self.other |= take & ~same

    def counts(self, hit, fast):
        """fast: the pixels whose every quotient took the shared sequence"""
        n = lambda m: int((m & hit).sum())
        return dict(far_x=n(self.far_x), far_y=n(self.far_y), dropped_by_id=n(self.dropped), across_seam=n(self.own & self.other), shared=n(fast), literal=n(~fast))


def lum(c):
    """Rec. 709 luminance, in the kernel's order of operations"""
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def color_term(C, k_color):
    """The colour term of rt_denoise for atrous_pass: the squared colour difference against k_color (which already carries its 4^k)."""
    return lambda qy, qx: (_term(_sqdiff(C[..., :3], C[qy, qx, :3]), k_color), None)


def luminance_term(C, D):
    """The colour term of rt_denoise_var and rt_svgf_filter for atrous_pass: the squared luminance difference over the pixel's tolerance D [H, W]."""
    L = lum(C)

    def term(qy, qx):
        dl = L - L[qy, qx]
        dl2 = dl * dl
        # equal luminance: the term is exactly 1 and no quotient is formed; else the quotient is rt_div.h's shared sequence where D and dl2 are in its range
        return np.where(dl2 == 0, F(1), np.fmax(F(0), F(1) - dl2 / D)), (dl2 != 0) & ~(div_in_range(D) & div_in_range(dl2))
    return term


def atrous_pass(C, aov, s, k_normal, k_position, k_albedo, color, V=None, carry=None, stats=None):
    """One 5 x 5 pass with step s over the colour frame C [H, W, 4], guided by aov [3, H, W, 4]: the pass of all three filters.  color(qy, qx) -> (the colour
    term of the taps at [qy, qx], or None for exactly 1; the taps whose term formed a literal quotient, or None).  V [H, W]: the variance, filtered along from
    the values `carry` (V itself unless given) that the taps bring; then the result is (colour, variance), else the colour.  stats: an optional dict that
    receives, under the key s, TapStats.counts of this pass."""
    Hh, W = C.shape[:2]
    N, ID, P, A = aov[0, ..., :3], aov[0, ..., 3], aov[1, ..., :3], aov[2, ..., :3]
    ys, xs = np.meshgrid(np.arange(Hh), np.arange(W), indexing="ij")
    S = np.zeros((Hh, W, 3), np.float32)
    Wt = np.zeros((Hh, W), np.float32)
    Sv = np.zeros((Hh, W), np.float32)
    if V is not None and carry is None:
        carry = V
    ts = TapStats(Hh, W, s) if stats is not None else None
    fast = np.ones((Hh, W), bool)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + dy * s, xs + dx * s
                inside = (qy >= 0) & (qy < Hh) & (qx >= 0) & (qx < W)
                qy, qx = np.clip(qy, 0, Hh - 1), np.clip(qx, 0, W - 1)
                ok = inside & (ID[qy, qx] == ID)
                w = np.full((Hh, W), H3[abs(dy)] * H3[abs(dx)], np.float32)
                t = _term(_sqdiff(N, N[qy, qx]), k_normal)
                if t is not None:
                    w = w * t
                if F(k_position) != 0:
                    Pq = P[qy, qx]
                    e = (N[..., 0] * (Pq[..., 0] - P[..., 0]) + N[..., 1] * (Pq[..., 1] - P[..., 1])) + N[..., 2] * (Pq[..., 2] - P[..., 2])
                    w = w * _term(e * e, k_position)
                t = _term(_sqdiff(A, A[qy, qx]), k_albedo)
                if t is not None:
                    w = w * t
                t, literal = color(qy, qx)
                if t is not None:
                    w = w * t
                take = ok & (w > 0)                                    # False for a NaN weight
                if ts is not None:
                    ts.tap(dx, dy, inside, ok, take, qx, qy)
                    if literal is not None:
                        fast &= ~(ok & literal)
                Cq = C[qy, qx, :3]
                S = np.where(take[..., None], S + w[..., None] * Cq, S)
                Wt = np.where(take, Wt + w, Wt)
                if V is not None:
                    Sv = np.where(take, Sv + (w * w) * carry[qy, qx], Sv)
        rgb = S / Wt[..., None]
        vo = Sv / (Wt * Wt)
        fast &= div_in_range(Wt) & div_in_range(S).all(-1)
        if V is not None:
            fast &= div_in_range(Sv) & div_in_range(Wt * Wt)
    out = C.copy()
    hit = ID != F(-1)
    out[hit, :3] = rgb[hit]
    if ts is not None:
        stats[s] = ts.counts(hit, fast)
    assert out.dtype == np.float32
    if V is None:
        return out
    Vo = V.copy()
    Vo[hit] = vo[hit]
    assert Vo.dtype == np.float32
    return out, Vo


def denoise_pass(C, aov, s, k_normal, k_position, k_albedo, k_color, stats=None):
    """One pass with step s over the colour frame C [H, W, 4], guided by aov [3, H, W, 4]; k_color already carries its 4^k.  stats: an optional dict that receives,
    under the key s, TapStats.counts of this pass."""
    C = np.ascontiguousarray(C, np.float32)
    return atrous_pass(C, np.ascontiguousarray(aov, np.float32), s, k_normal, k_position, k_albedo, color_term(C, k_color), stats=stats)


def denoise(C, aov, n_passes, k_normal, k_position, k_albedo, k_color, stats=None, keep=None):
    """rt_denoise: pass k = 0 .. n_passes - 1 with step 2^k; the colour term's k is k_color 4^k.  stats: see denoise_pass.  keep: an optional dict that receives
    the output of every pass, keyed by the number of passes run (what a call with that n_passes gives)."""
    assert 1 <= n_passes <= 8
    out = np.ascontiguousarray(C, np.float32)
    for k in range(n_passes):
        out = denoise_pass(out, aov, 1 << k, k_normal, k_position, k_albedo, F(k_color) * F(4 ** k), stats=stats)
        if keep is not None:
            keep[k + 1] = out
    return out


# ---- the camera ray of rt_render_aov: the pixel centre, cpu_launcher.cpp:694-709 with sigma = 0 (or realtime_render.cu:1112-1115 for a pose) ----
def camera_rays(W, H, cam=(0.0, 0.0, 55.0), fov=None, rows=None, basis=None):
    """-> (O [3], u [n_rows, W, 3]) in binary32.  rows: image row indices (None = all); basis = (bx, by, bz) of a posed camera (the position is `cam`)."""
    fov = F(np.pi / 3) if fov is None else F(fov)
    z = -F(W) / (F(2) * F(np.tan(np.float64(fov / F(2)))))
    rows = np.arange(H) if rows is None else np.asarray(rows)
    j = np.arange(W, dtype=np.float32)[None, :]
    i = rows.astype(np.float32)[:, None]
    x = ((j - F(W) / F(2)).astype(np.float64) + 0.5).astype(np.float32) + np.zeros_like(i)
    y = ((F(H) / F(2) - i).astype(np.float64) - 0.5).astype(np.float32) + np.zeros_like(j)
    v = np.stack([x, y, np.full_like(x, z)], axis=-1)
    O = np.asarray(cam, np.float32)
    if basis is not None:
        bx, by, bz = (np.asarray(b, np.float32) for b in basis)
        v = ((O + bz * v[..., 2:3]) + bx * v[..., 0:1]) + by * v[..., 1:2]
    n = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    u = v / n[..., None]
    assert u.dtype == np.float32
    return O, u


def oracle_aov(scene, albedos, W, H, tri_tmin=1e-4, **camera):
    """The planes rt_render_aov writes, from the oracle's Scene::intersect_all: albedos[id] = the object's albedo.  -> [3, n_rows, W, 4]"""
    O, u = camera_rays(W, H, **camera)
    out = np.zeros((3,) + u.shape[:2] + (4,), np.float32)
    out[0, ..., 3] = -1
    for r in range(u.shape[0]):
        for c in range(W):
            hit, oid, P, N = scene.intersect_all(O, u[r, c], tri_tmin)
            if hit:
                out[0, r, c, :3], out[0, r, c, 3] = N, oid
                out[1, r, c, :3], out[1, r, c, 3] = P, 1
                out[2, r, c, :3] = albedos[oid]
    return out
