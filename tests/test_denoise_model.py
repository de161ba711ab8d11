"""The reference model of rt_denoise (tests/denoise_model.py) without a GPU: the properties the formula of include/raytrace_hip.h promises, and the quality the
committed defaults buy on the two scenes of DESIGN.md section 5.7 -- measured against the CPU oracle's many-sample frames."""
import numpy as np
import pytest

import raytracinggpu_amd as rt
from . import denoise_model as dm

F = np.float32


def _guides(h, w, ids=None, rng=None):
    """planes of a flat wall seen head-on (or random ones): [3, h, w, 4]"""
    aov = np.zeros((3, h, w, 4), np.float32)
    aov[0, ..., 2] = 1
    aov[0, ..., 3] = 0 if ids is None else ids
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    aov[1, ..., 0], aov[1, ..., 1], aov[1, ..., 3] = xs, ys, 1
    aov[2, ..., :3] = 0.5
    if rng is not None:
        n = rng.normal(size=(h, w, 3)).astype(np.float32)
        aov[0, ..., :3] = n / np.linalg.norm(n, axis=-1, keepdims=True).astype(np.float32)
        aov[1, ..., :3] += rng.normal(size=(h, w, 3)).astype(np.float32)
        aov[2, ..., :3] = rng.random((h, w, 3)).astype(np.float32)
    return aov


def _bits_equal(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def test_constant_power_of_two_image_comes_back_bit_for_bit():
    rng = np.random.default_rng(0)
    for c in (0.25, 2.0 ** 17, 2.0 ** -9):
        C = np.full((37, 53, 4), c, np.float32)
        C[..., 3] = rng.integers(1, 9, size=(37, 53))
        for aov in (_guides(37, 53), _guides(37, 53, rng=rng)):
            for n in (1, 3, 5):
                _bits_equal(dm.denoise(C, aov, n, 2.0, 0.25, 16.0, 0.5), C)
                _bits_equal(dm.denoise(C, aov, n, 0.0, 0.0, 0.0, 0.0), C)


def test_two_objects_never_mix_and_misses_are_copied():
    h, w = 40, 64
    ids = np.zeros((h, w), np.float32)
    ids[:, w // 2:] = 1
    C = np.zeros((h, w, 4), np.float32)
    C[:, w // 2:, :3] = 1
    C[..., 3] = 2
    out = dm.denoise(C, _guides(h, w, ids), 5, 0.0, 0.0, 0.0, 0.0)     # nothing but the ids keeps the halves apart: 5 passes reach 62 pixels
    _bits_equal(out, C)
    # a column of misses keeps its (noisy) values, and nobody reads them
    rng = np.random.default_rng(1)
    C = rng.random((h, w, 4)).astype(np.float32)
    ids[:, 10] = -1
    out = dm.denoise(C, _guides(h, w, ids), 3, 0.0, 0.0, 0.0, 0.0)
    _bits_equal(out[:, 10], C[:, 10])
    C2 = C.copy()
    C2[:, 10, :3] = 1e9
    out2 = dm.denoise(C2, _guides(h, w, ids), 3, 0.0, 0.0, 0.0, 0.0)
    keep = np.ones(w, bool)
    keep[10] = False
    _bits_equal(out2[:, keep], out[:, keep])


def _b3_pass_loops(C, s):
    """the plain a-trous B3-spline pass, pixel by pixel with scalar binary32 arithmetic: taps inside the image, renormalised"""
    h, w = C.shape[:2]
    H3 = [F(0.375), F(0.25), F(0.0625)]
    out = C.copy()
    for y in range(h):
        for x in range(w):
            S = [F(0), F(0), F(0)]
            Wt = F(0)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = y + dy * s, x + dx * s
                    if not (0 <= qy < h and 0 <= qx < w):
                        continue
                    wgt = H3[abs(dy)] * H3[abs(dx)]
                    for c in range(3):
                        S[c] = F(S[c] + F(wgt * C[qy, qx, c]))
                    Wt = F(Wt + wgt)
            for c in range(3):
                out[y, x, c] = F(S[c] / Wt)
    return out


def test_all_k_zero_is_the_b3_spline_pyramid():
    rng = np.random.default_rng(2)
    C = (rng.random((13, 17, 4)) * 100).astype(np.float32)
    aov = _guides(13, 17, rng=rng)                                    # random guides: with every k = 0 they must not matter
    exp = C
    for k in range(4):
        exp = _b3_pass_loops(exp, 1 << k)
        _bits_equal(dm.denoise(C, aov, k + 1, 0.0, 0.0, 0.0, 0.0), exp)
    # interior pixels of the first pass: the separable kernel (1, 4, 6, 4, 1) / 16, here in binary64
    k1 = np.array([1, 4, 6, 4, 1], np.float64) / 16
    one = dm.denoise(C, aov, 1, 0.0, 0.0, 0.0, 0.0)
    ref = sum(k1[a] * k1[b] * C[a:a + 9, b:b + 13, :3].astype(np.float64) for a in range(5) for b in range(5))
    np.testing.assert_allclose(one[2:-2, 2:-2, :3], ref, rtol=2e-6)


def test_w_channel_is_the_inputs():
    rng = np.random.default_rng(3)
    C = rng.random((21, 30, 4)).astype(np.float32)
    C[..., 3] = rng.integers(1, 50, size=(21, 30))
    ids = rng.integers(-1, 3, size=(21, 30)).astype(np.float32)
    out = dm.denoise(C, _guides(21, 30, ids, rng=rng), 4, 2.0, 0.25, 16.0, 0.5)
    _bits_equal(out[..., 3], C[..., 3])
    assert (out[..., :3] != C[..., :3]).any()


def test_edge_terms_stop_at_edges():
    """a step in one guide (normal, plane, albedo) or in the colour itself: with its k large the step survives exactly, with k = 0 it is smeared"""
    h, w = 16, 32
    C = np.zeros((h, w, 4), np.float32)
    C[:, w // 2:, :3] = 1
    for which in range(4):
        aov = _guides(h, w)
        if which == 0:
            aov[0, :, w // 2:, :3] = (1, 0, 0)
        elif which == 1:
            aov[1, :, w // 2:, 2] = 5                                 # the right half lies 5 units off the left half's plane
        elif which == 2:
            aov[2, :, w // 2:, :3] = 0.9
        k = [0.0, 0.0, 0.0, 0.0]
        k[which] = 100.0
        _bits_equal(dm.denoise(C, aov, 2, *k), C)
        assert (dm.denoise(C, aov, 2, 0.0, 0.0, 0.0, 0.0) != C).any()


def test_nan_guides_do_not_spread():
    rng = np.random.default_rng(4)
    C = rng.random((12, 12, 4)).astype(np.float32)
    aov = _guides(12, 12)
    aov[1, 5, 5, :3] = np.nan
    out = dm.denoise(C, aov, 2, 2.0, 0.25, 16.0, 0.0)
    bad = np.isnan(out[..., :3]).any(-1)
    assert bad[5, 5] and bad.sum() == 1                              # the pixel itself has no valid tap (0 / 0); its neighbours skip it


def _rmse(oracle, a, b):
    return float(np.sqrt(np.mean((oracle.gamma_unit(a[..., :3]) - oracle.gamma_unit(b[..., :3])) ** 2)))


@pytest.mark.parametrize("scene", ["cpu", "demo10"])
def test_defaults_reduce_the_error_of_a_one_sample_frame(oracle, oracle_cat, scene):
    """DESIGN.md section 5.7 at test size: 128 x 128, b = 3, the 1-sample frame and its denoised version against a 256-sample frame, RMSE in the tonemap's [0, 1]
    scale.  The committed defaults must make the error strictly smaller (at 256 x 256 against 1024 samples the ratios are 0.34 and 0.74)."""
    W = H = 128
    sc = oracle.Scene.preset(scene, oracle_cat if scene == "cpu" else None)
    albedos = [s[2] for s in rt.scenes.spheres(scene)] + ([rt.scenes.CAT_ALBEDO] if scene == "cpu" else [])
    noisy, _, _ = sc.render(W, H, 1, 3, want_rgb8=False)
    ref, _, _ = sc.render(W, H, 256, 3, want_rgb8=False, seed=99)
    aov = dm.oracle_aov(sc, albedos, W, H)
    d = rt.make_denoise_params()
    out = dm.denoise(noisy, aov, d.n_passes, d.k_normal, d.k_position, d.k_albedo, d.k_color)
    e_noisy, e_out = _rmse(oracle, noisy, ref), _rmse(oracle, out, ref)
    print(f"{scene}: rmse noisy {e_noisy:.4f}, denoised {e_out:.4f}, ratio {e_out / e_noisy:.3f}")
    assert e_out < e_noisy
