"""The dead-channel rule under an environment (raytracinggpu_amd/csrc/rt_wavefront.hip.h: the argument above wf_dead_channels, its "Z = E" case), by brute force on the CPU.

Without a map a path's fold starts from +0.  Under one it starts from E, what the path's last ray met beyond the scene: per channel finite, sign bit clear, below 2^98
(a bilinear mean of texels below 2^96).  The claim of tests/test_dead_channels.py must hold for that start too: wherever the guard admits the elision of a shadow ray the
pixel is the reference's, NaN for NaN.  The guard and the emission are that file's (they do not know the fold's start); the fold is restated here with its start Z, and
Z is drawn from +0 up to just below 2^96, and past it to 2^98, on the same chains of up to 17 segments."""
import numpy as np

from . import test_dead_channels as dc
from .test_dead_channels import MAX_SEG, PI_F, _bits, f32

TEXEL_END = f32(2.0 ** 96)


def fold_from(Z, diffuse, alb, l):
    """Back to front from ans = Z [n, 3]: fold_segment per diffuse segment"""
    n, S = diffuse.shape
    ans = np.asarray(Z, f32).copy()
    with np.errstate(all="ignore"):
        for k in range(S - 1, -1, -1):
            a, lk = alb[:, k], l[:, k, None]
            nxt = (((lk * a).astype(f32) / PI_F).astype(f32) + (a * ans).astype(f32)).astype(f32)
            ans = np.where(diffuse[:, k, None], nxt, ans)
    return ans


def both_worlds(Z, diffuse, alb, lvis, hidden):
    elided = dc.emit(diffuse, alb, lvis)
    l_ref = np.where(hidden, f32(0), lvis).astype(f32)
    l_ker = np.where(elided, lvis, l_ref).astype(f32)
    return fold_from(Z, diffuse, alb, l_ker), fold_from(Z, diffuse, alb, l_ref), elided


def _sky(rng, n, top):
    """E per chain: channels from +0, denormals, the usual range and up to just below `top`"""
    e = np.exp2(rng.uniform(-149, np.log2(float(top)), (n, 3))).astype(f32)
    pick = rng.random((n, 3))
    e = np.where(pick < 0.2, f32(0), e)
    e = np.where((pick >= 0.2) & (pick < 0.5), np.exp2(rng.uniform(-10, 10, (n, 3))).astype(f32), e)
    e = np.where((pick >= 0.5) & (pick < 0.6), np.nextafter(f32(top), f32(0)), e)
    return np.minimum(e, np.nextafter(f32(top), f32(0))).astype(f32)


def test_the_fold_from_zero_is_the_existing_fold():
    rng = np.random.default_rng(5)
    diffuse, alb, lvis, hidden = dc._chains(rng, 50_000, 0.05)
    l = np.where(hidden, f32(0), lvis).astype(f32)
    a, b = fold_from(np.zeros((50_000, 3), f32), diffuse, alb, l), dc.fold(diffuse, alb, l)[0]
    assert ((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all()


def test_elided_rays_cannot_change_a_bit_of_the_colour_under_a_sky():
    rng = np.random.default_rng(2096)
    n_use = n_changed = n_lit = 0
    for top in (TEXEL_END, f32(2.0 ** 98)):                           # a texel's range, and the bilinear sum's
        for odd in (0.0, 0.02, 0.1):
            diffuse, alb, lvis, hidden = dc._chains(rng, 200_000, odd)
            Z = _sky(rng, 200_000, top)
            assert (_bits(Z) < _bits(f32(top))).all()
            got, exp, elided = both_worlds(Z, diffuse, alb, lvis, hidden)
            use = dc._assert_same_where_elided(got, exp, elided)
            n_use += int(use.sum())
            n_changed += int((use & (elided & hidden & (lvis != 0)).any(1)).sum())
            n_lit += int((use & (exp != 0).any(1) & ~np.isnan(exp).any(1)).sum())
    print("chains with an elided ray:", n_use, "folded with an l the reference does not have:", n_changed, "whose pixel is not black:", n_lit)
    assert n_use > 50_000 and n_changed > 25_000, (n_use, n_changed)
    assert n_lit > 1000, n_lit                                        # the sky does reach pixels of such chains: the comparison is not of zeros alone


def test_a_sky_behind_pure_colour_walls():
    """the room with a wall removed: red kills green and blue, green kills the rest -- the ray of the third segment is elided, the path escapes, and E reaches no channel;
    with one kill missing it reaches exactly that channel, in both chains alike"""
    diffuse = np.ones((1, 3), bool)
    lvis = np.array([[3.0, 5.0, 7.0]], f32)
    hidden = np.array([[False, False, True]])
    E = np.array([[1.9 * 2.0 ** 95, 0.5, 2.0]], f32)
    red, green, grey = (1, 0, 0), (0, 1, 0), (0.25, 0.25, 0.25)
    got, exp, elided = both_worlds(E, diffuse, np.array([[red, green, grey]], f32), lvis, hidden)
    assert elided.tolist() == [[False, True, True]]
    assert (_bits(got) == _bits(exp)).all() and got[0, 1] == 0 and got[0, 2] == 0 and got[0, 0] == f32(f32(f32(3.0) * f32(1)) / PI_F)
    got, exp, elided = both_worlds(E, diffuse, np.array([[red, grey, grey]], f32), lvis, hidden)
    assert not elided.any() and (_bits(got) == _bits(exp)).all() and got[0, 0] > 2.0 ** 90        # red sees the sky through two grey bounces
    assert MAX_SEG == 17
