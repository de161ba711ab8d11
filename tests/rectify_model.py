"""Reference model of rt_temporal_accumulate_fast and rt_history_rectify (test infrastructure, like tests/temporal_model.py), and a second, scalar reading of both.

numpy binary32 throughout, one rounding per operation in the order include/raytrace_hip.h states: the device's planes are held to the vectorised model bit for bit, and
the vectorised model to the scalar reading (plain loops, one pixel and one numpy.float32 operation at a time, `continue` where the header says "skipped").  min and max
are minNum and maxNum (np.fmin, np.fmax; the scalar reading's own fmin and fmax).  A correctly rounded quotient is `/` and a correctly rounded root np.sqrt.

The fast accumulation takes the tap from the accumulation's own model (tests/temporal_model.py with taps=): one reprojection, not a second search.

mutant= (the scalar reading only, tests only) changes one thing a broken kernel would plausibly change; tests/test_rectify_model.py proves the 96 x 64 case tells each
from the contract."""
import numpy as np

from . import temporal_model as tm
from .scalar_filter_reference import accumulate as scalar_accumulate
from .scalar_filter_reference import fmax, fmin, lum as scalar_lum

F = np.float32
ZERO, ONE = F(0), F(1)
RECTIFY_MUTANTS = ("radius_plus_1", "no_id_test", "copy_lt", "dx_outer", "n_kept", "moments_kept", "k_clamp_ignored")
FAST_MUTANTS = ("fast_max_history", "fast_tap0")


# ---------------------------------------------------------------- the vectorised model ----------------------------------------------------------------
def accumulate_fast(C, aov, prev_aov=None, prev_history=None, prev_fast=None, fast_history=4, alpha_min=0.0, **kw):
    """rt_temporal_accumulate_fast -> (the history [2, H, W, 4] of temporal_model.accumulate, the fast plane [H, W, 4]).  kw: accumulate's other keywords (stats= too)."""
    assert (prev_fast is None) == (prev_history is None) == (prev_aov is None) and fast_history >= 1
    C = np.ascontiguousarray(C, np.float32)
    taps = {}
    hist = tm.accumulate(C, aov, prev_aov, prev_history, alpha_min=alpha_min, taps=taps, **kw)
    hit = np.ascontiguousarray(aov, np.float32)[0, ..., 3] != F(-1)
    fast = np.zeros(C.shape, np.float32)
    fast[..., :3] = C[..., :3]
    fast[..., 3] = hit                                                  # n_f = 1 with a hit, 0 on a miss
    if prev_fast is not None:
        pf = np.ascontiguousarray(prev_fast, np.float32)
        q = taps["q"]
        took = q[..., 0] >= 0
        Fq = pf[np.maximum(q[..., 1], 0), np.maximum(q[..., 0], 0)]
        with np.errstate(all="ignore"):
            nf = np.fmin(Fq[..., 3] + ONE, F(fast_history))
            af = np.fmax(ONE / nf, F(alpha_min))
            blend = Fq[..., :3] + af[..., None] * (C[..., :3] - Fq[..., :3])
        fast[..., :3][took] = blend[took]
        fast[..., 3][took] = nf[took]
    assert fast.dtype == np.float32
    return hist, fast


def rectify(history, fast, aov, radius, k_clamp, stats=None):
    """rt_history_rectify -> the rectified history [2, H, W, 4].  aov: at least plane 0.  stats: an optional dict that receives pixel counts: copied_n (a hit copied
    because n <= n_f), lost_to_id (windows that skipped a tap inside the image for its id), clipped_left / right / top / bottom and corner_* (windows the image's edge
    cut), clamped_low / clamped_high (a channel raised to lo / lowered to hi), unmoved (inside the band on all three channels), moved_1 / 2 / 3 (channels moved)."""
    assert 1 <= radius <= 3 and k_clamp >= 0
    history = np.ascontiguousarray(history, np.float32)
    fast = np.ascontiguousarray(fast, np.float32)
    ID = np.ascontiguousarray(aov, np.float32)[0, ..., 3]
    Hh, W = ID.shape
    H0, H1 = history
    k = F(k_clamp)
    with np.errstate(all="ignore"):
        hit = ID != F(-1)
        work = hit & ~(H1[..., 2] <= fast[..., 3])
        ys, xs = np.meshgrid(np.arange(Hh), np.arange(W), indexing="ij")
        s1, s2 = np.zeros((Hh, W, 3), np.float32), np.zeros((Hh, W, 3), np.float32)
        cnt = np.zeros((Hh, W), np.float32)
        lost = np.zeros((Hh, W), bool)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                qy, qx = ys + dy, xs + dx
                inside = (qy >= 0) & (qy < Hh) & (qx >= 0) & (qx < W)
                qy, qx = np.clip(qy, 0, Hh - 1), np.clip(qx, 0, W - 1)
                same = (ID[qy, qx] == ID) | (dx == 0 and dy == 0)       # the pixel itself always counts
                ok = inside & same
                lost |= inside & ~same
                Fq = fast[qy, qx, :3]
                s1 = np.where(ok[..., None], s1 + Fq, s1)
                s2 = np.where(ok[..., None], s2 + Fq * Fq, s2)
                cnt = np.where(ok, cnt + ONE, cnt)
        mu, e2 = s1 / cnt[..., None], s2 / cnt[..., None]
        sg = np.sqrt(np.fmax(ZERO, e2 - mu * mu))
        lo, hi = mu - k * sg, mu + k * sg
        Hc = np.fmin(np.fmax(H0[..., :3], lo), hi)
        ch_moved = ~(Hc == H0[..., :3])
        moved = work & ch_moved.any(-1)
        new0 = np.concatenate([Hc, H0[..., 3:]], axis=-1)
        d = tm.lum(new0) - tm.lum(H0)
        m1 = H1[..., 0] + d
        m2 = H1[..., 1] + (m1 * m1 - H1[..., 0] * H1[..., 0])
        new1 = np.stack([m1, m2, fast[..., 3], H1[..., 3]], axis=-1)
    out = history.copy()
    out[0][moved] = new0[moved]
    out[1][moved] = new1[moved]
    if stats is not None:
        stats["copied_n"] = int((hit & ~work).sum())
        stats["lost_to_id"] = int((work & lost).sum())
        left, right, top, bottom = xs < radius, xs >= W - radius, ys < radius, ys >= Hh - radius
        for name, m in (("clipped_left", left), ("clipped_right", right), ("clipped_top", top), ("clipped_bottom", bottom), ("corner_tl", top & left),
                        ("corner_tr", top & right), ("corner_bl", bottom & left), ("corner_br", bottom & right)):
            stats[name] = int((work & m).sum())
        stats["clamped_low"] = int((work & (ch_moved & (Hc == lo)).any(-1)).sum())
        stats["clamped_high"] = int((work & (ch_moved & (Hc == hi) & ~(Hc == lo)).any(-1)).sum())
        stats["unmoved"] = int((work & ~moved).sum())
        for c in (1, 2, 3):
            stats[f"moved_{c}"] = int((work & (ch_moved.sum(-1) == c)).sum())
    assert out.dtype == np.float32
    return out


# ---------------------------------------------------------------- the header, read pixel by pixel ----------------------------------------------------------------
def scalar_accumulate_fast(C, aov, prev_aov=None, prev_history=None, prev_fast=None, fast_history=4, alpha_min=0.0, max_history=32, mutant=None, **kw):
    """rt_temporal_accumulate_fast from the header: the history and the accepted tap of scalar_filter_reference.accumulate, then the fast plane pixel by pixel"""
    assert mutant is None or mutant in FAST_MUTANTS
    C = np.ascontiguousarray(C, np.float32)
    aov = np.ascontiguousarray(aov, np.float32)
    Hh, W = C.shape[:2]
    taps = {}
    hist = scalar_accumulate(C, aov, prev_aov, prev_history, alpha_min=alpha_min, max_history=max_history, taps=taps, **kw)
    fast = np.zeros((Hh, W, 4), np.float32)
    limit = F(max_history) if mutant == "fast_max_history" else F(fast_history)
    if prev_fast is not None and mutant == "fast_tap0":                # the nearest previous pixel, accepted or not
        Pm, _ = tm.moved(aov, kw.get("motion"))
        _, gx, gy = tm.project(Pm, W, Hh, kw.get("camera"), kw.get("pose"))
    with np.errstate(all="ignore"):
        for y in range(Hh):
            for x in range(W):
                Cp = C[y, x]
                if aov[0, y, x, 3] == F(-1):
                    fast[y, x] = (Cp[0], Cp[1], Cp[2], ZERO)
                    continue
                qx, qy = taps["q"][y, x]
                if qx < 0:
                    fast[y, x] = (Cp[0], Cp[1], Cp[2], ONE)
                    continue
                if mutant == "fast_tap0":
                    qx, qy = min(max(int(np.floor(gx[y, x])), 0), W - 1), min(max(int(np.floor(gy[y, x])), 0), Hh - 1)
                Fq = prev_fast[qy, qx]
                nf = fmin(Fq[3] + ONE, limit)
                af = fmax(ONE / nf, F(alpha_min))
                fast[y, x] = (Fq[0] + af * (Cp[0] - Fq[0]), Fq[1] + af * (Cp[1] - Fq[1]), Fq[2] + af * (Cp[2] - Fq[2]), nf)
    return hist, fast


def scalar_rectify(history, fast, aov, radius, k_clamp, mutant=None, pixels=None):
    """rt_history_rectify from the header, for the pixels (x, y) given (None: all) -> the history [2, H, W, 4] (pixels not asked for are left 0)"""
    assert mutant is None or mutant in RECTIFY_MUTANTS
    history = np.ascontiguousarray(history, np.float32)
    fast = np.ascontiguousarray(fast, np.float32)
    ID = np.ascontiguousarray(aov, np.float32)[0, ..., 3]
    Hh, W = ID.shape
    out = np.zeros_like(history)
    k = ONE if mutant == "k_clamp_ignored" else F(k_clamp)
    r = radius + 1 if mutant == "radius_plus_1" else radius
    window = [(dx, dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1)]
    if mutant == "dx_outer":
        window = [(dx, dy) for dx in range(-r, r + 1) for dy in range(-r, r + 1)]
    if pixels is None:
        pixels = [(x, y) for y in range(Hh) for x in range(W)]
    with np.errstate(all="ignore"):
        for x, y in pixels:
            H0, H1, Fp, idp = history[0, y, x], history[1, y, x], fast[y, x], ID[y, x]
            out[0, y, x], out[1, y, x] = H0, H1
            if idp == F(-1):
                continue
            if (H1[2] < Fp[3]) if mutant == "copy_lt" else (H1[2] <= Fp[3]):
                continue
            s1, s2, cnt = [ZERO] * 3, [ZERO] * 3, ZERO
            for dx, dy in window:
                qx, qy = x + dx, y + dy
                if qx < 0 or qx >= W or qy < 0 or qy >= Hh:
                    continue
                if mutant != "no_id_test" and not (dx == 0 and dy == 0) and ID[qy, qx] != idp:
                    continue
                Fq = fast[qy, qx]
                for c in range(3):
                    s1[c] = s1[c] + Fq[c]
                    s2[c] = s2[c] + Fq[c] * Fq[c]
                cnt = cnt + ONE
            Hc = [ZERO] * 3
            for c in range(3):
                mu, e2 = s1[c] / cnt, s2[c] / cnt
                sg = np.sqrt(fmax(ZERO, e2 - mu * mu))
                lo, hi = mu - k * sg, mu + k * sg
                Hc[c] = fmin(fmax(H0[c], lo), hi)
            if all(Hc[c] == H0[c] for c in range(3)):
                continue
            d = scalar_lum(Hc) - scalar_lum(H0)
            m1 = H1[0] + d
            m2 = H1[1] + (m1 * m1 - H1[0] * H1[0])
            if mutant == "moments_kept":
                m1, m2 = H1[0], H1[1]
            out[0, y, x] = (Hc[0], Hc[1], Hc[2], H0[3])
            out[1, y, x] = (m1, m2, H1[2] if mutant == "n_kept" else Fp[3], H1[3])
    return out
