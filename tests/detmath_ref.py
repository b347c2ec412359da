"""A multiprecision reference for the pinned elementary functions of include/rayn_detmath.h, and the stratified grids they are swept on.

The kernels and the CPU oracle compile the same header, so a wrong exp / sin / cos / tan / atan2 / pow / log there passes every GPU-vs-oracle
test.  This module states what those functions SHOULD return without sharing anything with the header: finite non-zero results come from mpmath
at PREC bits and are rounded ONCE to binary32 (ties to even, gradual underflow, overflow to +-inf) in integer arithmetic; zeros, infinities
and NaN come from a written-out table of the C Annex F rules (mpmath has no signed zero).  No GPU, no oracle.

    correctly_rounded(op, a, b=None) -> float32 array        the correctly rounded result
    hardness(op, a, b=None)          -> float64 array        relative distance of the TRUE value to the nearest binary32 rounding boundary
                                                              (the midpoint of two consecutive floats); inf where the table answers
    truth(op, a, b=None)             -> list of mpf / None   the PREC-bit values themselves (None where the table answers)
    grid_unary / grid_pairs / grid_pow (seed)                every binade, the mantissas where rounding goes wrong, seeded random ones

Ops are named as oracle_detmath numbers them: 0 exp, 1 sin, 2 cos, 3 tan, 4 atan2(a, b), 5 pow(a, b), 6 log.

pow follows the conventions the header's comment lists, which are libm's on the domain rayn uses (base >= 0): pow(x, 0) = 1 and pow(1, y) = 1
even for a NaN partner, pow(0, y > 0) = 0, pow(0, y < 0) = inf, and a NEGATIVE BASE IS NaN (Annex F would give -8 for pow(-2, 3) and -0 for
pow(-0, 3); the header documents that it does not, and no grid here holds a negative base)."""
import math

import mpmath
import numpy as np

PREC = 320  # bits; >= 300
OPS = {"exp": 0, "sin": 1, "cos": 2, "tan": 3, "atan2": 4, "pow": 5, "log": 6}
EDGE_MANTISSAS = (0, 1, 2, 0x3FFFFF, 0x400000, 0x400001, 0x7FFFFE, 0x7FFFFF)  # a power of two, one and two ulps above, around 1.5, just below the next
PAIR_MANTISSAS = (0, 1, 0x7FFFFF, 0x400000)

_INF, _NAN = float("inf"), float("nan")


def _op(op):
    return OPS[op] if isinstance(op, str) else int(op)


def round_to_binary32(v):
    """(the float nearest to the non-zero finite mpf v as a Python float, relative distance of v to the nearest rounding boundary).  One rounding, in integers:
    v = +-man 2^exp with an odd integer man; the binary32 quantum at v is 2^(e - 23) for a normal magnitude (e = floor(log2 |v|)) and 2^-149 below 2^-126."""
    sign, man, exp, bc = v._mpf_
    e = exp + bc - 1
    qe = (e if e >= -126 else -126) - 23
    s = qe - exp  # |v| / quantum = man / 2^s
    if s <= 0:    # a multiple of the quantum: exact, the boundaries are half a quantum away
        n = man << -s
        hard = 1.0 / float(n << 1)
    else:
        n, rem, half = man >> s, man & ((1 << s) - 1), 1 << (s - 1)
        d = rem - half
        if d > 0 or (d == 0 and (n & 1)):
            n += 1
        hard = float(mpmath.mpf(abs(d)) / man)  # |v - boundary| / |v|
    r = math.ldexp(n, qe) if qe + n.bit_length() <= 128 else _INF  # n <= 2^24: exact in binary64; 2^128 and above is the overflow
    return (-r if sign else r), hard


def _special_unary(op, x):
    """The table for one argument: the result as a Python float, or None where the multiprecision value decides."""
    if x != x:
        return _NAN
    if op == 0:    # exp
        return _INF if x == _INF else 0.0 if x == -_INF else None
    if op == 6:    # log
        if x == 0.0:
            return -_INF  # log(+-0) = -inf
        if x < 0.0:
            return _NAN
        return _INF if x == _INF else 0.0 if x == 1.0 else None  # log(1) = +0
    if abs(x) == _INF:
        return _NAN   # sin, cos, tan of an infinity
    if x == 0.0:
        return 1.0 if op == 2 else x  # sin(-0) = -0, tan(-0) = -0, cos(+-0) = 1
    return None


def _special_atan2(y, x):
    """atan2(y, x), Annex F.10.1.4, for NaN / zero / infinite arguments: a multiple of pi / 4 as (numerator, sign), a signed zero, NaN, or None."""
    if y != y or x != x:
        return _NAN
    sy = math.copysign(1.0, y)
    xneg = math.copysign(1.0, x) < 0
    if y == 0.0:
        return ("pi", 4, sy) if xneg else sy * 0.0       # atan2(+-0, -0 or x < 0) = +-pi; atan2(+-0, +0 or x > 0) = +-0
    if abs(y) == _INF:
        if abs(x) == _INF:
            return ("pi", 3 if xneg else 1, sy)           # atan2(+-inf, -inf) = +-3 pi / 4; atan2(+-inf, +inf) = +-pi / 4
        return ("pi", 2, sy)                              # atan2(+-inf, finite x) = +-pi / 2
    if x == 0.0:
        return ("pi", 2, sy)                              # atan2(y != 0, +-0) = +-pi / 2
    if abs(x) == _INF:
        return ("pi", 4, sy) if xneg else sy * 0.0        # atan2(finite y, -inf) = +-pi; atan2(finite y, +inf) = +-0
    return None


def _special_pow(x, y):
    if y == 0.0 or x == 1.0:
        return 1.0            # also for a NaN partner
    if x != x or y != y or x < 0.0:
        return _NAN           # the header's domain: a negative base is NaN
    if x == 0.0:
        return 0.0 if y > 0.0 else _INF
    if x == _INF:
        return _INF if y > 0.0 else 0.0
    if abs(y) == _INF:
        return _INF if (x > 1.0) == (y > 0.0) else 0.0
    return None


_cache = {}


def _evaluate(op, a, b):
    op = _op(op)
    a = np.ascontiguousarray(a, np.float32).ravel()
    b = np.zeros_like(a) if b is None else np.ascontiguousarray(b, np.float32).ravel()
    assert a.size == b.size
    key = (op, a.tobytes(), b.tobytes())
    if key in _cache:
        return _cache[key]
    out = np.zeros(a.size, np.float64)
    hard = np.full(a.size, np.inf)
    true = [None] * a.size
    mpf = mpmath.mpf
    fn1 = {0: mpmath.exp, 1: mpmath.sin, 2: mpmath.cos, 3: mpmath.tan, 6: mpmath.log}.get(op)
    with mpmath.workprec(PREC):
        pi4 = mpmath.pi / 4
        for i, (x, y) in enumerate(zip(a.tolist(), b.tolist())):  # tolist(): exact binary64 copies of the floats
            if op == 4:
                sp = _special_atan2(x, y)
                if isinstance(sp, tuple):
                    v = pi4 * sp[1] * sp[2]
                elif sp is None:
                    v = mpmath.atan2(mpf(x), mpf(y))
                else:
                    out[i] = sp
                    continue
            elif op == 5:
                sp = _special_pow(x, y)
                if sp is not None:
                    out[i] = sp
                    continue
                t = mpf(y) * mpmath.log(mpf(x))
                if t > 100 or t < -120:  # far past 2^128 / below 2^-150: no need to raise e to 10^13
                    out[i] = _INF if t > 0 else 0.0
                    continue
                v = mpmath.exp(t)
            else:
                sp = _special_unary(op, x)
                if sp is not None:
                    out[i] = sp
                    continue
                if op == 0 and (x > 100.0 or x < -120.0):
                    out[i] = _INF if x > 0 else 0.0
                    continue
                v = fn1(mpf(x))
            if not isinstance(sp, tuple):
                true[i] = v
            if v == 0:
                out[i] = 0.0  # (not reached by a finite non-zero argument outside the table: sin / tan / atan2 of one never vanish)
                continue
            r, h = round_to_binary32(v)
            out[i] = r
            if not isinstance(sp, tuple):
                hard[i] = h
    with np.errstate(over="ignore"):
        res = (out.astype(np.float32), hard, true)  # every entry is a binary32 value, an infinity or NaN already: the cast is exact
    _cache[key] = res
    return res


def correctly_rounded(op, a, b=None):
    return _evaluate(op, a, b)[0]


def hardness(op, a, b=None):
    return _evaluate(op, a, b)[1]


def truth(op, a, b=None):
    return _evaluate(op, a, b)[2]


def core_error(op, a, b, core):
    """|core - truth| / |truth| per point for the binary64 values `core` (NaN = no value); 0 where there is no multiprecision value to compare with."""
    t = truth(op, a, b)
    err = np.zeros(len(t))
    with mpmath.workprec(PREC):
        for i, (v, c) in enumerate(zip(t, np.asarray(core, np.float64).tolist())):
            if v is not None and c == c and v != 0:
                err[i] = float(abs((mpmath.mpf(c) - v) / v))
    return err


def _from_bits(u):
    return np.ascontiguousarray(u, np.uint32).view(np.float32)


def grid_unary(seed, fields=range(0, 255), random_per_field=56):
    """Every exponent field x both signs x (the 8 edge mantissas + random_per_field seeded random ones): 255 x 2 x 64 = 32640 floats, zero and the denormals included."""
    rng = np.random.default_rng(seed)
    fields = np.asarray(list(fields), np.uint32)
    man = np.concatenate([np.tile(np.array(EDGE_MANTISSAS, np.uint32), (fields.size, 1)),
                          rng.integers(0, 1 << 23, (fields.size, random_per_field), dtype=np.uint32)], axis=1)
    pos = ((fields[:, None] << np.uint32(23)) | man).ravel()
    return _from_bits(np.concatenate([pos, pos | np.uint32(0x80000000)]))


def grid_pairs(seed):
    """atan2: both arguments from every 6th exponent field x ({0, 1, 0x7FFFFF, 0x400000} + 4 random mantissas), all pairs, random signs: 344^2 = 118336 pairs."""
    rng = np.random.default_rng(seed)
    fields = np.arange(0, 255, 6, dtype=np.uint32)

    def axis():
        man = np.concatenate([np.tile(np.array(PAIR_MANTISSAS, np.uint32), (fields.size, 1)), rng.integers(0, 1 << 23, (fields.size, 4), dtype=np.uint32)], axis=1)
        return ((fields[:, None] << np.uint32(23)) | man).ravel()
    ya, xa = axis(), axis()
    y, x = [v.ravel().copy() for v in np.meshgrid(ya, xa, indexing="ij")]
    y |= rng.integers(0, 2, y.size, dtype=np.uint32) << np.uint32(31)
    x |= rng.integers(0, 2, x.size, dtype=np.uint32) << np.uint32(31)
    return _from_bits(y), _from_bits(x)


def grid_pow(seed):
    """pow: bases = every 5th exponent field x the 8 edge mantissas plus the 81 floats around 1.0 (489, all >= 0); exponents = fields 90..164 step 3
    (2^-37 .. 2^37) x {0, 1, 0x7FFFFF, 0x400000}, both signs (200): 97800 pairs.  Nothing is random; the seed is accepted for symmetry."""
    fields = np.arange(0, 255, 5, dtype=np.uint32)
    bases = ((fields[:, None] << np.uint32(23)) | np.array(EDGE_MANTISSAS, np.uint32)[None, :]).ravel()
    bases = np.unique(np.concatenate([bases, np.uint32(0x3F800000) + np.arange(-40, 41).astype(np.int64).astype(np.uint32)]))
    ef = np.arange(90, 165, 3, dtype=np.uint32)
    ex = ((ef[:, None] << np.uint32(23)) | np.array(PAIR_MANTISSAS, np.uint32)[None, :]).ravel()
    ex = np.concatenate([ex, ex | np.uint32(0x80000000)])
    x, y = [v.ravel().copy() for v in np.meshgrid(bases, ex, indexing="ij")]
    return _from_bits(x), _from_bits(y)
