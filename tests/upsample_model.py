"""Reference model of rt_upsample (test infrastructure, like tests/denoise_model.py): numpy binary32 throughout, every operation one rounding, in the order
include/raytrace_hip.h states, so the device's frames are held to it bit for bit.  The four taps are vectorised over the full-resolution image; the order in which they
are accumulated is the contract's.  max is maxNum (np.fmax).  tests/test_upsample_model.py holds this model to a scalar, pixel-by-pixel reading of the header.

mutant=: one wrong reading of the header at a time (MUTANTS), for the tests that show the fixture tells them apart.  id_test=False with both k = 0 is plain bilinear."""
import numpy as np

from .denoise_model import _sqdiff, _term

F = np.float32
# ("b_is_by_bx" is NOT in the list: binary32 multiplication commutes, by bx is bx by bit for bit -- tests/test_upsample_model.py asserts that it changes nothing;
# what the order of the product does pin is its association, "b_not_formed_first": w = ((bx wn) wp) by)
MUTANTS = ("taps_reversed", "b_not_formed_first", "no_id_test", "plane_with_Nq", "fallback_nearest", "w_averaged", "no_half")


def coords(n_full, f, mutant=None):
    """-> (i [n] int64, fr [n] float32): floor and fraction of g = (x + 0.5) / f - 0.5"""
    x = np.arange(n_full, dtype=np.float32)
    g = (x + F(0.5)) / F(f)
    if mutant != "no_half":
        g = g - F(0.5)
    fl = np.floor(g)
    assert g.dtype == np.float32
    return fl.astype(np.int64), g - fl


def upsample(low, low_aov, aov, factor, k_normal, k_position, stats=None, mutant=None, id_test=True):
    """rt_upsample: low [h, w, 4] or [n, h, w, 4], low_aov [>= 2, h, w, 4], aov [>= 2, f h, f w, 4] -> [f h, f w, 4] or [n, f h, f w, 4].
    stats: an optional dict that receives, per full-resolution pixel, `counted` (the number of counted taps of the guided round, 0 .. 4), `fallback`, and per tap
    t = 0 .. 3 the [H, W] masks `outside`, `id`, `normal`, `plane` (the tap was inside the image and had the id but this term was not > 0; `normal` and `plane` are
    looked at independently of each other), and the totals of taps dropped for one reason ALONE."""
    low, low_aov, aov = (np.ascontiguousarray(a, np.float32) for a in (low, low_aov, aov))
    single = low.ndim == 3
    L = low[None] if single else low
    n_planes, h, w = L.shape[:3]
    f = int(factor)
    Hh, W = aov.shape[1:3]
    assert (Hh, W) == (h * f, w * f) and low_aov.shape[1:3] == (h, w)
    N, ID, P = aov[0, ..., :3], aov[0, ..., 3], aov[1, ..., :3]
    Nl, IDl, Pl = low_aov[0, ..., :3], low_aov[0, ..., 3], low_aov[1, ..., :3]
    ix, fx = coords(W, f, mutant)
    iy, fy = coords(Hh, f, mutant)
    IX, IY = np.meshgrid(ix, iy)
    FX, FY = np.meshgrid(fx, fy)
    order = (3, 2, 1, 0) if mutant == "taps_reversed" else (0, 1, 2, 3)
    taps = []
    with np.errstate(all="ignore"):
        for t in order:
            qx, qy = IX + (t & 1), IY + (t >> 1)
            inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            bx = FX if t & 1 else F(1) - FX
            by = FY if t >> 1 else F(1) - FY
            b = by * bx if mutant == "b_is_by_bx" else bx * by
            same = IDl[qy, qx] == ID if id_test and mutant != "no_id_test" else np.ones((Hh, W), bool)
            Nq, Pq = Nl[qy, qx], Pl[qy, qx]
            wt = bx if mutant == "b_not_formed_first" else b
            tn = _term(_sqdiff(N, Nq), k_normal)
            if tn is not None:
                wt = wt * tn
            tp = None
            if F(k_position) != 0:
                Ne = Nq if mutant == "plane_with_Nq" else N
                e = (Ne[..., 0] * (Pq[..., 0] - P[..., 0]) + Ne[..., 1] * (Pq[..., 1] - P[..., 1])) + Ne[..., 2] * (Pq[..., 2] - P[..., 2])
                tp = _term(e * e, k_position)
                wt = wt * tp
            if mutant == "b_not_formed_first":
                wt = wt * by
            taps.append(dict(t=t, qx=qx, qy=qy, inside=inside, same=same, b=b, w=wt, tn=tn, tp=tp))
        S = np.zeros((n_planes, Hh, W, 4), np.float32)
        Wt = np.zeros((Hh, W), np.float32)
        w0 = np.zeros((Hh, W), np.float32)
        have = np.zeros((Hh, W), bool)
        counted = np.zeros((Hh, W), np.int64)

        def take(tap, m, wt):
            nonlocal S, Wt, w0, have
            Lq = L[:, tap["qy"], tap["qx"]]
            S = np.where(m[None, ..., None], S + wt[None, ..., None] * Lq, S)
            Wt = np.where(m, Wt + wt, Wt)
            w0 = np.where(m & ~have, Lq[0, ..., 3], w0)
            have = have | m

        for tap in taps:
            m = tap["inside"] & tap["same"] & (tap["w"] > 0)           # False for a NaN weight
            take(tap, m, tap["w"])
            counted += m
        fallback = Wt == 0
        if mutant == "fallback_nearest":
            best = np.full((Hh, W), -1.0, np.float32)
            pick = np.zeros((Hh, W), np.int64)
            for i, tap in enumerate(taps):
                better = tap["inside"] & (tap["b"] > best)
                best, pick = np.where(better, tap["b"], best), np.where(better, i, pick)
            for i, tap in enumerate(taps):
                take(tap, fallback & (pick == i), np.ones((Hh, W), np.float32))
        else:
            for tap in taps:
                take(tap, fallback & tap["inside"], tap["b"])
        out = S / Wt[None, ..., None]
        if mutant != "w_averaged":
            out[0, ..., 3] = w0
    assert out.dtype == np.float32
    if stats is not None:
        stats["counted"], stats["fallback"] = counted, fallback
        alone = dict(outside=0, id=0, normal=0, plane=0)
        for tap in taps:
            one = np.ones((Hh, W), bool)
            n_bad = ~(tap["tn"] > 0) if tap["tn"] is not None else ~one
            p_bad = ~(tap["tp"] > 0) if tap["tp"] is not None else ~one
            live = tap["inside"] & tap["same"]
            d = dict(outside=~tap["inside"], id=tap["inside"] & ~tap["same"], normal=live & n_bad, plane=live & p_bad)
            stats[tap["t"]] = d
            alone["outside"] += int(d["outside"].sum())
            # by id alone: the tap's other two terms would have let it count
            alone["id"] += int((d["id"] & ~n_bad & ~p_bad).sum())
            alone["normal"] += int((d["normal"] & ~p_bad).sum())
            alone["plane"] += int((d["plane"] & ~n_bad).sum())
        stats["alone"] = alone
    return out[0] if single else out


def bilinear(low, low_aov, aov, factor):
    """plain bilinear: the model with both k = 0 and the id test off (every tap inside the image counts with w = b)"""
    return upsample(low, low_aov, aov, factor, 0.0, 0.0, id_test=False)
