"""TEST INFRASTRUCTURE -- the exact model of the two float -> byte conversions, in the standard library's `decimal` alone.

  byte_d(c)   the byte of the correctly rounded pow((double)c, 1./2.2):   (unsigned char)min(., 255.), NaN -> 0       (cpu:714-716, oracle/rt_oracle.c tonemap1)
  byte_f(c)   the byte of the correctly rounded powf(c, 1 / 2.2f):        v = (double)powf; if (!(v < 255.)) v = 255.  (realtime:1136-1147)

c is a binary32 value (any Python float that is one).  The power is exp(e * ln c) at PREC = 80 digits; e is the exponent as the C expression gives it, exactly.  "Correctly
rounded, then truncated" needs no rounding step of its own: with k = floor(power), the rounded value reaches k + 1 exactly when the power is at or above the midpoint between
k + 1 and the format's number just below it (a tie goes to k + 1, whose significand is even), and otherwise its integer part is k.  The power of a binary32 c != 1 is
irrational or, at the few exact cases (c = 2048, c = 177147 on the binary64 path), an integer that 1./2.2 != 1/2.2 keeps the power away from: no tie occurs.

thresholds_d() / thresholds_f(): for k = 1 ... 255 the bit pattern of the least binary32 T_k whose byte is >= k, by bisection over bit patterns (the byte does not fall as
c rises).  edge_values(), SPECIALS, log_uniform() are the input sets the CPU and the GPU tests share.
"""
import functools
import math
import struct
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np

PREC = 80
INF_BITS = 0x7f800000


def f32_of_bits(b):
    return struct.unpack("<f", struct.pack("<I", b))[0]


def bits_of_f32(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _round_to_binary32(q):
    """the binary32 nearest to the positive normal rational q, ties to even, in integer arithmetic"""
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1                                                         # 2^e <= q < 2^(e + 1)
    scaled = q / Fraction(2) ** (e - 23)                                # in [2^23, 2^24)
    n = scaled.numerator // scaled.denominator
    rest = scaled - n
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n & 1):
        n += 1
    return float(Fraction(n) * Fraction(2) ** (e - 23))


EXP_D = 1. / 2.2                                                       # the binary64 quotient of 1 and the binary64 2.2: Python's own arithmetic is C's
EXP_F = _round_to_binary32(1 / Fraction(f32_of_bits(bits_of_f32(2.2))))  # 1 / 2.2f: int 1 converted, one binary32 division of 1 by the binary32 2.2


def _half_gap_below(m, mant_bits):
    """half the distance between the integer m >= 1 and the format's number just below it"""
    e = m.bit_length() - 1
    if m == 1 << e:
        e -= 1
    return Fraction(1, 2) * Fraction(2) ** (e - mant_bits)


@functools.lru_cache(maxsize=None)
def _edges(mant_bits):
    """edge[m], m = 1 ... 255: the correctly rounded power is >= m exactly when the power is >= edge[m]"""
    with localcontext() as ctx:
        ctx.prec = PREC
        out = [None]
        for m in range(1, 256):
            f = Fraction(m) - _half_gap_below(m, mant_bits)
            out.append(Decimal(f.numerator) / Decimal(f.denominator))   # a dyadic rational of < 40 digits: exact at PREC
        return tuple(out)


def _byte_of_power(c, exponent, mant_bits):
    """c finite and > 0"""
    with localcontext() as ctx:
        ctx.prec = PREC
        p = (Decimal(exponent) * Decimal(c).ln()).exp()
        k = int(p)                                                     # towards zero; p > 0
        if k >= 255:
            return 255
        return k + 1 if p >= _edges(mant_bits)[k + 1] else k


def byte_d(c):
    c = float(c)
    if math.isinf(c):                                                  # pow(-inf, y) is +inf for a y > 0 that is no odd integer (C Annex F), as the oracle records
        return 255
    if math.isnan(c) or c < 0:                                         # pow of a finite negative base and a fraction is NaN; NaN -> 0 (rt_oracle.c tonemap1)
        return 0
    if c == 0:
        return 0
    return _byte_of_power(c, EXP_D, 52)


def byte_f(c):
    c = float(c)
    if math.isnan(c) or c < 0:                                         # NaN fails `v < 255.`: 255.  -1e-45 and -inf too
        return 255
    if c == 0:
        return 0
    if math.isinf(c):
        return 255
    return _byte_of_power(c, EXP_F, 23)


def bytes_of(fn, values):
    """fn (byte_d or byte_f) over an array of binary32 values -> uint8 of the same shape"""
    a = np.asarray(values, np.float32)
    return np.array([fn(float(v)) for v in a.ravel()], np.uint8).reshape(a.shape)


def _thresholds(fn):
    out = []
    for k in range(1, 256):
        lo, hi = 0, INF_BITS                                           # byte(+0) = 0 < k <= 255 = byte(+inf)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if fn(f32_of_bits(mid)) >= k:
                hi = mid
            else:
                lo = mid
        out.append(hi)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def thresholds_d():
    """bit patterns of T_1 ... T_255 of the binary64 path"""
    return _thresholds(byte_d)


@functools.lru_cache(maxsize=None)
def thresholds_f():
    """bit patterns of T_1 ... T_255 of the binary32 path"""
    return _thresholds(byte_f)


# ---- the shared input sets
SPECIALS = np.array([0.0, -0.0, 1e-45, 1e-39, 1.1754944e-38, 0.5, 1.0, 196964.0, 196965.0, 3e38, np.inf, np.nan, -1.0, -np.inf, -1e-45], np.float32)
EXACT_ROOTS = (2048.0, 177147.0)                                       # 32^2.2 and 243^2.2: the binary32 inputs other than 1 whose exact 2.2-th root is a code


def edge_values(thresholds):
    """T_k - 4 ... T_k + 3 (in floats) for every k -> float32 [255, 8]"""
    t = np.array(thresholds, np.int64)[:, None] + np.arange(-4, 4)[None, :]
    assert t.min() > 0 and t.max() < INF_BITS
    return t.astype(np.uint32).view(np.float32)


def exact_root_values():
    """2048 and 177147, each with its two neighbours on either side -> float32 [10]"""
    b = np.array([bits_of_f32(v) + d for v in EXACT_ROOTS for d in (-2, -1, 0, 1, 2)], np.uint32)
    return b.view(np.float32)


def log_uniform(n=4096, seed=20261021):
    rng = np.random.default_rng(seed)
    return np.exp(rng.uniform(np.log(1e-6), np.log(4e5), n)).astype(np.float32)


def edges_are_covered(values, expected, thresholds):
    """the two things a test says about its own inputs: all 256 codes occur, and for every k both k - 1 and k occur among T_k's eight neighbours"""
    v, e = np.asarray(values, np.float32).ravel().view(np.uint32), np.asarray(expected).ravel()
    if len(np.unique(e)) != 256:
        return False
    by_bits = dict(zip(v.tolist(), e.tolist()))
    for k, t in enumerate(thresholds, start=1):
        seen = {by_bits.get(t + d) for d in range(-4, 4)}
        if not {k - 1, k} <= seen:
            return False
    return True


def ulps_from_a_code(c, exponent=None):
    """how far the exact power of the positive finite binary32 c lies from the nearest integer code 1 ... 255, in binary32 ulps on the power's side of that code"""
    with localcontext() as ctx:
        ctx.prec = PREC
        p = (Decimal(EXP_F if exponent is None else exponent) * Decimal(float(c)).ln()).exp()
        m = min(max(int(p + Decimal("0.5")), 1), 255)
        gap = 2 * _half_gap_below(m, 23) if p < m else Fraction(2) ** (m.bit_length() - 1 - 23)
        return float(abs(p - m) / (Decimal(gap.numerator) / Decimal(gap.denominator)))
