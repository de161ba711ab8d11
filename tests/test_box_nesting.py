"""The nesting claim behind the forest's union nodes and the fixed-point BOX steps, restated in numpy binary32 and checked by brute force on the CPU.

BoundingBox::intersect (cpu_launcher.cpp:146-157), literally:
    t0k = (mn[k] - O[k]) / u[k];  t1k = (mx[k] - O[k]) / u[k]            six binary32 divisions
    if (t0k > t1k) std::swap(t0k, t1k)                                    per axis
    return std::min({t1x, t1y, t1z}) > std::max({t0x, t0y, t0z})
The initializer-list min / max are min_element / max_element: the FIRST element is kept unless a later one compares '<' (max: the running value '<' the later one).
A NaN is never '<' anything and nothing is '<' a NaN, so a NaN in position 0 becomes the result (and the box is missed: NaN > x and x > NaN are false), while a NaN
in position 1 or 2 is skipped as if the axis were absent.  That asymmetry is the whole difference between an origin on a face with u = 0 on the first axis and on the others.

Two claims rest on "hit(inner) => hit(outer) in the computed values" for a box inside another (rt_host_scene.hip.h build_forest, rt_qnodes.hip.h):
  (1) rt_qnodes.hip.h: for rays without zero components the test is monotone along nested boxes -- per axis the outer box's two bounds bracket the inner box's.  The
      fixed-point BOX steps only ever see such rays (rays with a zero / denormal / huge component are walked serially with the literal test).
  (2) build_forest: a synthetic node above the meshes' roots must be hit whenever one of the roots below it is, for EVERY ray (all kernels walk those nodes).  Brute force
      finds that the exact union does not give this: an inner box FLAT on axis y or z (lo == hi), the origin exactly on that plane, u = -0.0 on that axis, and an outer box
      that shares the plane as one of its faces but is not flat there.  The inner box sees 0 / -0 = NaN for both bounds of the axis -- skipped in positions 1 and 2 -- while
      the outer box sees NaN and -inf (or +inf and NaN): a miss.  So the union nodes are the union of their children's boxes -- each child's box taken per axis as
      [min(lo, hi), max(lo, hi)], which is what the reference's swap makes of an inverted box -- widened by one float step on every face: then the origin can lie on no face of
      the union that some child also has, and the claim holds.
This test samples nested boxes with shared faces, flat boxes, unions of two boxes, coordinates from 1e-3 to 1e7, origins on faces / edges / corners and directions with
+-0, denormal, huge, tiny and axis-parallel components; it prints the first counterexamples of the exact union (the class described above, and only that class) and
asserts that the widened union has none."""
import time

import numpy as np

f32 = np.float32
N_CHUNKS, CHUNK = 32, 1 << 20                                           # 33.5 M (inner, outer, ray) samples


def hit(lo, hi, O, u):
    """BoundingBox::intersect on (n, 3) binary32 arrays; also the swapped lower / upper bounds (for the edge-class counts)."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        t0 = (lo - O) / u
        t1 = (hi - O) / u
    sw = t0 > t1                                                        # if (t0 > t1) std::swap(t0, t1)
    a = np.where(sw, t1, t0)
    b = np.where(sw, t0, t1)
    mn = b[:, 0].copy()                                                 # std::min({t1x, t1y, t1z}) = min_element: keep unless a later one is '<'
    for k in (1, 2):
        np.copyto(mn, b[:, k], where=b[:, k] < mn)
    mx = a[:, 0].copy()                                                 # std::max({t0x, t0y, t0z}) = max_element: replace when the running value is '<' the later one
    for k in (1, 2):
        np.copyto(mx, a[:, k], where=mx < a[:, k])
    return mn > mx, a, b


def widen(lo, hi):
    """build_forest's union node box around (lo, hi): one float step outwards on every face."""
    return np.nextafter(lo, f32(-np.inf)).astype(f32), np.nextafter(hi, f32(np.inf)).astype(f32)


def sample(rng, n):
    def U(a, b, shape):                                                 # uniform in binary32 (cheaper than binary64 draws)
        return (f32(a) + f32(b - a) * rng.random(shape, dtype=f32)).astype(f32)

    scale = (f32(10.0) ** U(-3, 7, (n, 1))).astype(f32)       # box size 1e-3 .. 1e7
    off = (rng.standard_normal((n, 3), dtype=f32) * (f32(10.0) ** U(-3, 7, (n, 1)))).astype(f32)   # box position 1e-3 .. 1e7 from the origin
    # inner box; some axes flat (lo == hi)
    ilo = (off + U(-1, 1, (n, 3)) * scale).astype(f32)
    ihi = (ilo + U(0, 1, (n, 3)) * scale).astype(f32)
    flat = rng.random((n, 3)) < 0.25
    ihi = np.where(flat, ilo, ihi)
    ihi = np.maximum(ihi, ilo)
    # outer box: contains the inner one, shares each face with probability 1/2
    share_lo, share_hi = rng.random((n, 3)) < 0.5, rng.random((n, 3)) < 0.5
    olo = np.where(share_lo, ilo, (ilo - U(0, 1, (n, 3)) * scale * (f32(10.0) ** U(-6, 0, (n, 1)))).astype(f32))
    ohi = np.where(share_hi, ihi, (ihi + U(0, 1, (n, 3)) * scale * (f32(10.0) ** U(-6, 0, (n, 1)))).astype(f32))
    olo, ohi = np.minimum(olo, ilo), np.maximum(ohi, ihi)
    # a quarter: the union of the inner box with a second random box (how forest nodes are made); some of those second boxes flat too
    un = rng.random(n) < 0.25
    slo = (off + U(-2, 2, (n, 3)) * scale).astype(f32)
    shi = np.where(rng.random((n, 3)) < 0.2, slo, (slo + U(0, 1, (n, 3)) * scale).astype(f32))
    olo = np.where(un[:, None], np.minimum(ilo, slo), olo)
    ohi = np.where(un[:, None], np.maximum(ihi, shi), ohi)
    # origins: random near the boxes; on a face plane of the inner and / or the outer box, on one, two or three axes (faces, edges, corners)
    O = (off + U(-3, 3, (n, 3)) * scale).astype(f32)
    placed = rng.random((n, 3)) < rng.choice([0.0, 0.34, 0.67, 1.0], (n, 1))
    which = rng.integers(0, 4, (n, 3))                                  # inner lo / inner hi / outer lo / outer hi
    face = np.choose(which, [ilo, ihi, olo, ohi])
    O = np.where(placed, face, O)
    # directions
    u = rng.standard_normal((n, 3), dtype=f32).astype(f32)
    kind = rng.integers(0, 8, n)
    z1 = rng.integers(0, 3, n)
    z2 = (z1 + rng.integers(1, 3, n)) % 3
    sgn = np.where(rng.random(n) < 0.5, f32(-0.0), f32(0.0))
    r = np.arange(n)
    m = kind == 1                                                       # one component +-0
    u[r[m], z1[m]] = sgn[m]
    m = kind == 2                                                       # two components +-0 (axis-parallel, sign of the rest random)
    u[r[m], z1[m]] = sgn[m]; u[r[m], z2[m]] = np.where(rng.random(m.sum()) < 0.5, f32(-0.0), f32(0.0))
    m = kind == 3                                                       # exactly axis-parallel, unit
    u[m] = 0.0; u[r[m], z1[m]] = rng.choice([-1.0, 1.0], m.sum())
    m = kind == 4                                                       # denormal components
    u[r[m], z1[m]] = rng.choice([f32(1e-42), f32(-1e-42)], m.sum())
    m = kind == 5
    u[m] *= f32(1e20)
    m = kind == 6
    u[m] *= f32(1e-20)
    m = kind == 7                                                       # one zero and one denormal
    u[r[m], z1[m]] = sgn[m]; u[r[m], z2[m]] = rng.choice([f32(1e-42), f32(-1e-42)], m.sum())
    return ilo, ihi, olo.astype(f32), ohi.astype(f32), O, u.astype(f32)


def explained(ilo, ihi, olo, ohi, O, u):
    """The class of counterexamples of the EXACT union described in the module docstring: some axis k in {y, z} with the inner box flat on it, the origin on that plane,
    u[k] = -0.0, and the outer box sharing that plane as a face without being flat there."""
    nz = (u == 0) & np.signbit(u)
    flat_on = (ilo == ihi) & (O == ilo)
    shares = ((olo == ilo) | (ohi == ihi)) & (olo < ohi)
    c = nz & flat_on & shares
    return c[:, 1] | c[:, 2]


def test_hit_inner_implies_hit_outer_brute_force():
    rng = np.random.default_rng(20261016)
    t_start = time.time()
    n_total = n_inner_hits = n_exact_bad = n_unexplained = n_wide_bad = n_bad_nonzero_u = 0
    nan_lo, nan_hi = np.zeros(3, np.int64), np.zeros(3, np.int64)      # NaN lower / upper bound of the INNER test per position of max / min
    on_shared_zero = 0
    examples = []
    for _ in range(N_CHUNKS):
        ilo, ihi, olo, ohi, O, u = sample(rng, CHUNK)
        assert (olo <= ilo).all() and (ihi <= ohi).all() and (ilo <= ihi).all()
        hi_in, a, b = hit(ilo, ihi, O, u)
        hi_out, _, _ = hit(olo, ohi, O, u)
        wlo, whi = widen(olo, ohi)
        hi_wide, _, _ = hit(wlo, whi, O, u)
        n_total += CHUNK
        n_inner_hits += int(hi_in.sum())
        nan_lo += np.isnan(a).sum(0)
        nan_hi += np.isnan(b).sum(0)
        on_shared_zero += int(((((O == ilo) & (O == olo)) | ((O == ihi) & (O == ohi))) & (u == 0)).any(1).sum())
        bad = hi_in & ~hi_out
        n_exact_bad += int(bad.sum())
        ex = explained(ilo, ihi, olo, ohi, O, u)
        n_unexplained += int((bad & ~ex).sum())
        n_bad_nonzero_u += int((bad & (u != 0).all(1)).sum())
        n_wide_bad += int((hi_in & ~hi_wide).sum())
        for i in np.flatnonzero(bad)[: max(0, 3 - len(examples))]:
            examples.append((ilo[i], ihi[i], olo[i], ohi[i], O[i], u[i]))
        for i in np.flatnonzero(hi_in & ~hi_wide)[:3]:
            print("COUNTEREXAMPLE of the widened union:", ilo[i], ihi[i], wlo[i], whi[i], O[i], u[i])
    dt = time.time() - t_start
    print(f"\n{n_total} samples in {dt:.1f} s, inner hits {n_inner_hits}; NaN lower bound of the inner test at max position 0/1/2: {nan_lo.tolist()}, NaN upper bound "
          f"at min position 0/1/2: {nan_hi.tolist()}; origin on a shared face with u = 0 on that axis: {on_shared_zero}")
    print(f"exact union: {n_exact_bad} counterexamples (all of the flat-plane / u = -0 class: {n_unexplained == 0}); union widened by one float step: {n_wide_bad}")
    for e in examples:
        print("counterexample of the exact union: inner lo %r hi %r, outer lo %r hi %r, O %r, u %r" % tuple(tuple(float(x) for x in v) for v in e))
    # the sampler reaches the edge classes
    assert n_total >= 30_000_000
    assert (nan_lo >= 2000).all() and (nan_hi >= 2000).all(), (nan_lo, nan_hi)
    assert on_shared_zero >= 2000
    assert n_inner_hits >= 1_000_000
    # claim (1): rays without a zero component are monotone along nested boxes
    assert n_bad_nonzero_u == 0
    # the exact union fails only in the class the module docstring describes (and the sampler does meet it)
    assert n_unexplained == 0
    assert n_exact_bad > 0
    # claim (2), what build_forest relies on: a widened union is hit whenever a box inside the exact union is
    assert n_wide_bad == 0
