"""The dead-channel rule for shadow rays (raytracinggpu_amd/csrc/rt_wavefront.hip.h: wf_dead_channels, wf_fold_bounded), restated in numpy binary32 and checked by
brute force on the CPU.

The fold of a path is, per channel and back to front,  ans_k = fl(fl(fl(l_k alb_k) / pi) + fl(alb_k ans_{k+1}))  (fold_segment, cpu:624, 642-644).  A channel is dead
from the first diffuse segment whose albedo in it is +0; a diffuse segment whose three channels are dead does not trace its shadow ray and keeps l = lvis where the
reference has lvis or +0.  The claim: wherever the guard known at emission admits the elision (albedo components in [+0, 1] and a direct term in [+0, 2^96) from the kill
to the elided segment) the pixel is the reference's, NaN for NaN -- whatever the rest of the path holds.  That is a claim about IEEE arithmetic, so it is tested here
without a GPU, on chains of up to 17 segments with albedo components from {+0, -0, denormal, tiny, 0.25, 1, > 1, negative, inf, NaN} and direct terms from denormal to
2^127, inf, NaN and negative.  (The first version of the guard admitted every finite non-negative operand and held only while the kernel's own chain stayed below 2^126,
which the fold still checks as a statistic: `sure` below.)"""
import numpy as np

f32 = np.float32
PI_F = f32(3.14159265358979323846)
FINITE = np.uint32(0x7f800000)          # kFoldFinite: bits of +inf
ALBEDO_MAX = np.uint32(0x3f800000)      # kDeadAlbedoMax: bits of 1
DIRECT_END = np.uint32(0x6f800000)      # kDeadDirectEnd: bits of 2^96
BOUND = np.uint32(0x7e800000)           # kFoldBound: bits of 2^126
MAX_SEG = 17                            # RT_MAX_SEGMENTS + 1 launches: depth 0..16


def _bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def guard(alb, lvis):
    """the segment counts: albedo components in [+0, 1], direct term in [+0, 2^96)"""
    return (_bits(alb).max(-1) <= ALBEDO_MAX) & (_bits(lvis) < DIRECT_END)


def dead_channels(dead, alb, lvis):
    """wf_dead_channels: the mask after a diffuse segment (alb [n, 3], lvis [n]) given the mask before it"""
    good = guard(alb, lvis)
    kill = ((_bits(alb) == 0) * np.array([1, 2, 4])).sum(-1)
    return np.where(good, dead | kill, 0)


def emit(diffuse, alb, lvis):
    """Front to back, as wf_advance_path shades the segments: which shadow rays the rule elides.  diffuse [n, S] bool, alb [n, S, 3], lvis [n, S]."""
    n, S = diffuse.shape
    dead = np.zeros(n, np.int64)
    elided = np.zeros((n, S), bool)
    for k in range(S):
        now = dead_channels(dead, alb[:, k], lvis[:, k])
        moot = _bits(lvis[:, k]) == 0                         # the first kind of moot ray: direct term +0 either way
        elided[:, k] = diffuse[:, k] & (now == 7) & ~moot
        dead = np.where(diffuse[:, k], now, dead)             # mirror and glass segments change nothing
    return elided


def fold(diffuse, alb, l):
    """Back to front: the colour [n, 3] and whether every folded segment passed wf_fold_bounded"""
    n, S = diffuse.shape
    ans = np.zeros((n, 3), f32)
    sure = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for k in range(S - 1, -1, -1):
            a, lk = alb[:, k], l[:, k, None]
            nxt = (((lk * a).astype(f32) / PI_F).astype(f32) + (a * ans).astype(f32)).astype(f32)
            ok = (_bits(l[:, k]) < FINITE) & (_bits(a).max(-1) < FINITE) & (_bits(nxt).max(-1) < BOUND)
            d = diffuse[:, k]
            ans = np.where(d[:, None], nxt, ans)
            sure &= ok | ~d
    return ans, sure


def both_worlds(diffuse, alb, lvis, hidden):
    """(kernel's colour, reference's colour, elided, sure): the reference has l = +0 where the light is hidden, the kernel keeps lvis where the ray was elided"""
    elided = emit(diffuse, alb, lvis)
    l_ref = np.where(hidden, f32(0), lvis).astype(f32)
    l_ker = np.where(elided, lvis, l_ref).astype(f32)
    got, sure = fold(diffuse, alb, l_ker)
    exp, _ = fold(diffuse, alb, l_ref)
    return got, exp, elided, sure


TINY = np.array([1e-45, 1e-40, 1.1754944e-38, 1e-30], f32)         # denormals, the smallest normal, small


def _albedo(rng, shape, odd):
    """components from {+0, -0, tiny, 0.25, 1, > 1}; odd > 0: that share from {negative, inf, NaN} on top"""
    pick = rng.integers(0, 8, shape)
    a = np.select([pick <= 2, pick == 3, pick == 4, pick == 5, pick == 6],
                  [f32(0), f32(0.25), f32(1), rng.choice(TINY, shape), rng.choice(np.array([1.5, 2, 1e3, 1e30], f32), shape)], f32(0)).astype(f32)
    a = np.where((pick == 7) & (rng.random(shape) < 0.3), f32(-0.0), a).astype(f32)                 # -0 among the zeros
    if odd > 0:
        bad = rng.random(shape) < odd
        a = np.where(bad, rng.choice(np.array([-0.5, -1e-40, np.inf, -np.inf, np.nan], f32), shape), a).astype(f32)
    return a


def _direct(rng, shape, odd):
    """l from denormal to 2^127, +0 and inf; odd > 0: that share from {negative, -0, NaN}"""
    l = np.exp2(rng.uniform(-149, 127, shape)).astype(f32)
    pick = rng.random(shape)
    l = np.where(pick < 0.15, f32(0), l)
    l = np.where((pick >= 0.15) & (pick < 0.18), f32(np.inf), l)
    l = np.where((pick >= 0.18) & (pick < 0.4), np.exp2(rng.uniform(-10, 40, shape)).astype(f32), l)   # the usual range, more often
    if odd > 0:
        bad = rng.random(shape) < odd
        l = np.where(bad, rng.choice(np.array([-1.0, -0.0, np.nan, -np.inf], f32), shape), l)
    return l.astype(f32)


def _chains(rng, n, odd):
    S = MAX_SEG
    nseg = rng.integers(1, S + 1, n)
    live = np.arange(S)[None, :] < nseg[:, None]
    diffuse = live & (rng.random((n, S)) < 0.85)                     # the others: mirror / glass segments (SID 0xff)
    return diffuse, _albedo(rng, (n, S, 3), odd), _direct(rng, (n, S), odd), rng.random((n, S)) < 0.5


def _assert_same_where_elided(got, exp, elided):
    """every chain with an elided ray, inside the fold's old range or not: the same bits, or NaN in both"""
    use = elided.any(1)
    same = (_bits(got) == _bits(exp)) | (np.isnan(got) & np.isnan(exp))
    assert same[use].all(), (got[use & ~same.all(1)][:4], exp[use & ~same.all(1)][:4])
    return use


def test_elided_rays_cannot_change_a_bit_of_the_colour():
    rng = np.random.default_rng(624)
    n_use = n_changed = n_unsure = 0
    for odd in (0.0, 0.02, 0.1):
        for _ in range(2):
            diffuse, alb, lvis, hidden = _chains(rng, 200_000, odd)
            got, exp, elided, sure = both_worlds(diffuse, alb, lvis, hidden)
            use = _assert_same_where_elided(got, exp, elided)
            n_use += int(use.sum())
            n_changed += int((use & (elided & hidden & (lvis != 0)).any(1)).sum())      # the kernel folded an l the reference does not have
            n_unsure += int((elided.any(1) & ~sure).sum())
    print("chains with an elided ray:", n_use, "of them folded with an l the reference does not have:", n_changed, "outside the fold's old range:", n_unsure)
    assert n_use > 50_000 and n_changed > 25_000, (n_use, n_changed)
    assert n_unsure > 1000, n_unsure                                  # the generator reaches overflow, negative and non-finite operands beside an elided ray


def test_what_the_guard_refuses():
    """a segment with a negative, -0, inf or NaN albedo component or direct term, an albedo component above 1 or a direct term of 2^96 and more kills nothing and clears
    the mask; +0 alone kills"""
    one = np.ones(1, f32)
    z = f32(0)
    assert dead_channels(np.array([0]), np.array([[z, 1, z]], f32), one)[0] == 5
    assert dead_channels(np.array([2]), np.array([[z, 1, z]], f32), one)[0] == 7
    assert dead_channels(np.array([7]), np.array([[z, 7.5, z]], f32), one)[0] == 0
    assert dead_channels(np.array([7]), np.array([[z, np.nextafter(f32(1), f32(2)), z]], f32), one)[0] == 0
    assert dead_channels(np.array([2]), np.array([[z, 1, z]], f32), np.array([np.nextafter(f32(2.0 ** 96), f32(0))], f32))[0] == 7
    assert dead_channels(np.array([7]), np.array([[z, 1, z]], f32), np.array([2.0 ** 96], f32))[0] == 0
    assert dead_channels(np.array([2]), np.array([[z, 1e-45, z]], f32), one)[0] == 7           # a denormal kills nothing, but it is a good operand
    assert dead_channels(np.array([0]), np.array([[1e-45, 1e-45, 1e-45]], f32), one)[0] == 0
    for bad in (-0.0, -1.0, np.inf, -np.inf, np.nan):
        assert dead_channels(np.array([7]), np.array([[z, bad, z]], f32), one)[0] == 0, bad
        assert dead_channels(np.array([7]), np.array([[z, z, z]], f32), np.array([bad], f32))[0] == 0, bad
    assert dead_channels(np.array([0]), np.array([[z, z, z]], f32), np.array([0], f32))[0] == 7   # lvis = +0 is a good operand (and its ray moot already)
    # the rule never elides the ray of a segment whose own operands fail the guard, whatever came before
    rng = np.random.default_rng(7)
    diffuse, alb, lvis, _ = _chains(rng, 200_000, 0.2)
    elided = emit(diffuse, alb, lvis)
    assert elided.any() and not (elided & ~guard(alb, lvis)).any()


def test_every_channel_needs_its_own_kill():
    """two dead channels are not enough, and a kill is forgotten behind a segment that fails the guard"""
    S = 4
    diffuse = np.ones((1, S), bool)
    lvis = np.full((1, S), 3.0, f32)
    red, green, grey = (1, 0, 0), (0, 1, 0), (0.25, 0.25, 0.25)
    assert emit(diffuse, np.array([[red, grey, grey, red]], f32), lvis).tolist() == [[False] * 4]
    assert emit(diffuse, np.array([[red, grey, green, grey]], f32), lvis).tolist() == [[False, False, True, True]]
    assert emit(diffuse, np.array([[red, green, (-1, 1, 1), grey]], f32), lvis).tolist() == [[False, True, False, False]]
    mirror = np.array([[True, False, True, True]])
    assert emit(mirror, np.array([[red, green, green, grey]], f32), lvis).tolist() == [[False, False, True, True]]   # the mirror segment's albedo counts for nothing


def test_the_path_that_overflowed_under_the_first_guard_keeps_its_ray():
    """segment 0 kills every channel; what segments 2 and 3 hand up is 3.5 x 2^126, and segment 1's own direct term (1.9 x 2^127, the light hidden) would take the kernel's
    chain past 2^128 where the reference's stays finite: NaN against +0 at segment 0 under a guard that admits any finite operand.  Segment 1 fails the guard (a direct
    term of 2^96 and more), its ray is traced, and so are those behind it: the bits are the reference's."""
    diffuse = np.ones((1, 4), bool)
    alb = np.array([[(0, 0, 0), (1, 1, 1), (2, 2, 2), (1, 1, 1)]], f32)
    lvis = np.array([[1.0, 1.9 * 2.0 ** 127, 1.9 * 2.0 ** 126, 1.8 * 2.0 ** 127]], f32)
    hidden = np.array([[False, True, False, False]])
    got, exp, elided, sure = both_worlds(diffuse, alb, lvis, hidden)
    assert elided.tolist() == [[True, False, False, False]]
    assert (_bits(exp) == 0).all() and (_bits(got) == 0).all()
    # with every ray elided, as the first guard did: NaN, and the fold's range check says so
    got, _ = fold(diffuse, alb, lvis)
    assert np.isnan(got).all() and not fold(diffuse, alb, lvis)[1][0]
    # a huge chain BELOW a guarded run (albedo 1, direct terms below 2^96) changes nothing: the elided terms are less than half an ulp of it
    alb = np.array([[(0, 0, 0), (1, 1, 1), (1, 1, 1), (1, 1, 1)]], f32)
    lvis = np.array([[1.0, 1.9 * 2.0 ** 95, 1.9 * 2.0 ** 95, 1.99 * 2.0 ** 127]], f32)
    hidden = np.array([[False, True, True, False]])
    got, exp, elided, sure = both_worlds(diffuse, alb, lvis, hidden)
    assert elided.tolist() == [[True, True, True, False]] and not sure[0]
    assert (_bits(got) == _bits(exp)).all() and (_bits(got) == 0).all()


def test_the_guard_admits_the_benchmark_scene():
    """the benchmark's magnitudes: wall albedos of 0 and 1, the cat's 0.25, a light of 3e10 between 0.1 and 2000 units away (l = I / (4 pi r^2) max(cos, 0)), up to 17
    segments -- every segment passes the guard, every chain the fold's check, and the rule elides"""
    from raytracinggpu_amd import scenes
    rng = np.random.default_rng(3)
    n, S = 200_000, MAX_SEG
    palette = np.array([w[2] for w in scenes.WALLS] + [scenes.CAT_ALBEDO] * 3, f32)
    alb = palette[rng.integers(0, len(palette), (n, S))]
    r2 = np.exp2(rng.uniform(np.log2(0.1 ** 2), np.log2(2000.0 ** 2), (n, S)))
    lvis = (scenes.LIGHT[1] / (4 * np.pi * r2) * np.maximum(rng.uniform(-1, 1, (n, S)), 0)).astype(f32)
    diffuse = np.ones((n, S), bool)
    hidden = rng.random((n, S)) < 0.5
    assert guard(alb, lvis).all()
    got, exp, elided, sure = both_worlds(diffuse, alb, lvis, hidden)
    assert sure.all()
    assert float(np.abs(got).max()) < 2.0 ** 60                       # 66 binades below the bound
    assert elided.mean() > 0.3
    np.testing.assert_array_equal(_bits(got), _bits(exp))
