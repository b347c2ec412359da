"""The kernels' elementary functions (rayn_hip_probe_detmath: include/rayn_detmath_fast.h with include/rayn_detmath.h behind it, built by hipcc for the
device) against the oracle's host build of include/rayn_detmath.h on EVERY binade: bit for bit, no tolerance.

test_detmath_bit_exact (test_gpu_parity.py) draws uniform arguments from moderate intervals (sin up to 2e4, a dozen special values); this file is the
device half of the stratified sweep of tests/test_detmath.py: every exponent field, both signs, the mantissas next to the powers of two plus seeded
random ones - zero, the denormals, the fast windows' edges, the thresholds of exp and, for sin / cos / tan, every argument from 2^20 to the largest
float, where the reduction is dm_sincos_large's integer Payne-Hanek step (no float-to-integer conversion of an out-of-range value is involved on
either side).  mpmath is not used here: that the oracle's values are the correctly rounded ones is tests/test_detmath.py's statement."""
import ctypes as C

import numpy as np
import pytest

import detmath_ref as R

pytestmark = pytest.mark.gpu

SEED = 11
ORACLE_OP = {0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 14: 6}  # probe op -> oracle_detmath op (14 = dmf_logf, the Mandelbulb estimator's logarithm)


def _binade_pairs(fields_a, fields_b, rng, signs_a, signs_b):
    """64 x 64 binades x 64 mantissa pairs: the 16 pairs of {0, 1, 0x7FFFFF, 0x400000} and 48 seeded random pairs per pair of binades."""
    fa, fb = np.asarray(fields_a, np.uint32), np.asarray(fields_b, np.uint32)
    assert fa.size == 64 and fb.size == 64
    edge = np.array(R.PAIR_MANTISSAS, np.uint32)
    shape = (64, 64, 64)
    ma = rng.integers(0, 1 << 23, shape, dtype=np.uint32)
    mb = rng.integers(0, 1 << 23, shape, dtype=np.uint32)
    ma[:, :, :16] = np.repeat(edge, 4)[None, None, :]
    mb[:, :, :16] = np.tile(edge, 4)[None, None, :]
    a = (fa[:, None, None] << np.uint32(23)) | ma
    b = (fb[None, :, None] << np.uint32(23)) | mb
    if signs_a:
        a |= rng.integers(0, 2, shape, dtype=np.uint32) << np.uint32(31)
    if signs_b:
        b |= rng.integers(0, 2, shape, dtype=np.uint32) << np.uint32(31)
    return a.ravel().view(np.float32), b.ravel().view(np.float32)


def _arguments(op):
    rng = np.random.default_rng(SEED + op)
    if op == 4:    # atan2: both arguments over every 4th exponent field, random signs - ratios from 2^-276 to 2^276
        f = np.arange(0, 256, 4)
        return _binade_pairs(f, f, rng, True, True)
    if op == 5:    # pow: bases >= 0 over every 4th exponent field (126 and 127, the binades around 1, in place of 120 and 132), exponents 2^-32 .. 2^32 of both signs
        fb = np.array(sorted((set(range(0, 256, 4)) - {120, 132}) | {126, 127}))
        return _binade_pairs(fb, np.arange(95, 159), rng, False, True)
    a = R.grid_unary(SEED + op, random_per_field=1016)  # 255 fields x 2 signs x 1024 mantissas = 522240
    return a, np.zeros_like(a)


@pytest.mark.parametrize("op", sorted(ORACLE_OP))
def test_device_functions_equal_the_oracle_on_every_binade(gpu_ctx, oracle, op):
    from rayn_amd._lib import lib
    a, b = _arguments(op)
    assert a.size == (262144 if op in (4, 5) else 522240)
    out = np.zeros_like(a)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    assert lib().rayn_hip_probe_detmath(gpu_ctx.h, op, fp(a), fp(b), fp(out), a.size) == 0
    ref = oracle.detmath(ORACLE_OP[op], a, b)
    same = out.view(np.uint32) == ref.view(np.uint32)  # a NaN too: both sides return the header's one quiet NaN
    bad = np.flatnonzero(~same)[:4]
    assert same.all(), (int((~same).sum()), a[bad], b[bad], out[bad], ref[bad])
