"""Reference model of rt_svgf_filter (test infrastructure, like tests/temporal_model.py, whose pass -- denoise_model.atrous_pass -- this one runs with the two switches).

numpy binary32 throughout: every operation one rounding, in the order include/raytrace_hip.h states (dy outer, dx inner, sums left to right; numpy's binary32 quotient is
the correctly rounded one).  `mutant` (tests only) names one wrong reading of the header that a kernel could plausibly implement; tests/test_svgf_model.py shows that each
changes the bits of the synthetic case."""
import numpy as np

from .denoise_model import atrous_pass, luminance_term

F = np.float32
G3 = (F(0.5), F(0.25))
MUTANTS = ("gauss_no_id", "gauss_step_1", "carry_vg", "feedback_earlier", "feedback_later", "plane1_filtered_variance", "w_from_plane1")


def gaussian_variance(V, ID, s, stats=None, mutant=None):
    """Vg [H, W]: the 3 x 3 Gaussian of V over the taps (x + dx s, y + dy s) inside the image with the pixel's own id.  stats: an optional dict that receives how many
    taps of hit pixels were skipped for each reason."""
    Hh, W = V.shape
    ys, xs = np.meshgrid(np.arange(Hh), np.arange(W), indexing="ij")
    SG, WG = np.zeros((Hh, W), np.float32), np.zeros((Hh, W), np.float32)
    hit = ID != F(-1)
    outside = other = 0
    step = 1 if mutant == "gauss_step_1" else s
    with np.errstate(all="ignore"):
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                qy, qx = ys + dy * step, xs + dx * step
                inside = (qy >= 0) & (qy < Hh) & (qx >= 0) & (qx < W)
                qy, qx = np.clip(qy, 0, Hh - 1), np.clip(qx, 0, W - 1)
                same = ID[qy, qx] == ID
                ok = inside & (same | (mutant == "gauss_no_id"))
                g = G3[abs(dy)] * G3[abs(dx)]
                SG = np.where(ok, SG + g * V[qy, qx], SG)
                WG = np.where(ok, WG + g, WG)
                outside += int((hit & ~inside).sum())
                other += int((hit & inside & ~same).sum())
        Vg = SG / WG
    if stats is not None:
        stats["gauss_outside"], stats["gauss_other_id"] = outside, other
    assert Vg.dtype == np.float32
    return Vg


def svgf_pass(C, V, aov, s, prefilter, k_normal, k_position, k_albedo, k_sigma, var_floor, stats=None, mutant=None):
    """One pass with step s over colour C [H, W, 4] and variance V [H, W] -> (colour, variance): temporal_model.denoise_var_pass with D from the Gaussian of V when
    prefilter is 1.  stats: an optional dict that receives, under s, the Gaussian's skipped taps and the hit pixels whose D the pre-filter changed."""
    C = np.ascontiguousarray(C, np.float32)
    V = np.ascontiguousarray(V, np.float32)
    aov = np.ascontiguousarray(aov, np.float32)
    ID = aov[0, ..., 3]
    with np.errstate(all="ignore"):
        Vd = V
        if prefilter:
            st = {} if stats is not None else None
            Vd = gaussian_variance(V, ID, s, stats=st, mutant=mutant)
            if stats is not None:
                D0, D1 = F(k_sigma) * V + F(var_floor), F(k_sigma) * Vd + F(var_floor)
                st["d_changed"] = int(((ID != F(-1)) & (D0.view(np.uint32) != D1.view(np.uint32))).sum())
                stats[s] = st
        D = F(k_sigma) * Vd + F(var_floor)
    # (the variance the taps carry on: the unfiltered one)
    return atrous_pass(C, aov, s, k_normal, k_position, k_albedo, luminance_term(C, D), V=V, carry=Vd if mutant == "carry_vg" else V)


def svgf_filter(history, aov, n_passes, feedback_pass, prefilter, k_normal, k_position, k_albedo, k_sigma, var_floor, stats=None, keep=None, mutant=None):
    """rt_svgf_filter -> (the filtered colour [H, W, 4], the fed-back history [2, H, W, 4] or None when feedback_pass is -1).  keep: an optional dict that
    receives every pass's colour under the number of passes run."""
    assert 1 <= n_passes <= 8 and -1 <= feedback_pass < n_passes and prefilter in (0, 1)
    history = np.ascontiguousarray(history, np.float32)
    out, V = history[0], history[1, ..., 3]
    fed = None
    take_at = feedback_pass + {"feedback_earlier": -1, "feedback_later": 1}.get(mutant, 0) if feedback_pass >= 0 else -1
    for k in range(n_passes):
        if feedback_pass >= 0 and take_at < 0 and k == 0:              # (the mutant that takes the pass before pass 0: the unfiltered colour)
            fed = history.copy()
        out, V = svgf_pass(out, V, aov, 1 << k, prefilter, k_normal, k_position, k_albedo, k_sigma, var_floor, stats=stats, mutant=mutant)
        if keep is not None:
            keep[k + 1] = out
        if k == min(take_at, n_passes - 1):
            fed = history.copy()                                       # plane 1: the input's, bit for bit
            fed[0, ..., :3] = out[..., :3]                             # plane 0: this pass's .rgb, the input history's .w
            if mutant == "plane1_filtered_variance":
                fed[1, ..., 3] = V
            if mutant == "w_from_plane1":
                fed[0, ..., 3] = history[1, ..., 3]
    return out, fed
