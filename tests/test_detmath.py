"""include/rayn_detmath.h (host side, through the oracle's probe): within 1 ulp of a double-precision
reference and identical under both FMA policies (the pinned functions never use mul_add)."""
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ulp_diff(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("op,fn,lo,hi", [
    (0, np.exp, -40.0, 10.0), (1, np.sin, -20.0, 20.0), (2, np.cos, -20.0, 20.0), (3, np.tan, -1.55, 1.55), (6, np.log, 1.0e-3, 300.0)])
def test_unary(oracle, op, fn, lo, hi):
    x = np.random.default_rng(op).uniform(lo, hi, 100000).astype(np.float32)
    got = oracle.detmath(op, x)
    want = fn(x.astype(np.float64)).astype(np.float32)
    assert _ulp_diff(got, want).max() <= 1
    assert np.array_equal(got, oracle.detmath(op, x, fma=True))


def test_atan2_pow(oracle):
    rng = np.random.default_rng(9)
    y, x = rng.uniform(-5, 5, 100000).astype(np.float32), rng.uniform(-5, 5, 100000).astype(np.float32)
    assert _ulp_diff(oracle.detmath(4, y, x), np.arctan2(y.astype(np.float64), x).astype(np.float32)).max() <= 1
    b, e = rng.uniform(0, 1, 100000).astype(np.float32), rng.uniform(0.05, 12, 100000).astype(np.float32)
    assert _ulp_diff(oracle.detmath(5, b, e), np.power(b.astype(np.float64), e).astype(np.float32)).max() <= 1


def test_special_values(oracle):
    f = lambda op, a, b=0.0: float(oracle.detmath(op, np.array([a], np.float32), np.array([b], np.float32))[0])
    assert f(0, 0.0) == 1.0 and f(0, -200.0) == 0.0 and math.isinf(f(0, 100.0)) and math.isnan(f(0, float("nan")))
    assert f(1, 0.0) == 0.0 and f(2, 0.0) == 1.0 and math.isnan(f(1, float("inf")))
    assert f(4, 0.0, -1.0) == np.float32(math.pi) and f(4, -0.0, -1.0) == -np.float32(math.pi) and f(4, 1.0, 0.0) == np.float32(math.pi / 2)
    assert f(5, 0.0, 2.0) == 0.0 and f(5, 1.0, 7.0) == 1.0 and f(5, 0.5, 0.0) == 1.0 and math.isnan(f(5, -1.0, 0.5))
    bits = lambda op, a: int(oracle.detmath(op, np.array([a], np.float32)).view(np.uint32)[0])
    assert [bits(op, z) for op in (1, 3) for z in (0.0, -0.0)] == [0, 0x80000000] * 2  # sin and tan keep the sign of a zero argument


# ---- include/rayn_detmath_fast.h: what the KERNELS evaluate (host build of the same header, through oracle_detmath_fast) ----
FAST_CASES = [  # op, a range, b range, EPS the header's rounding test assumes
    (0, (-82.0, 87.0), None, 1.0e-12), (1, (-9000.0, 9000.0), None, 2.0e-12), (2, (-8.0, 8.0), None, 2.0e-12), (3, (-1.6, 1.6), None, 4.0e-12),
    (4, None, None, 1.0e-12), (5, (0.0, 1.0), (0.05, 310.0), 2.0e-12), (5, (0.5, 40.0), (-12.0, 12.0), 2.0e-12),
    (6, (0.0, 300.0), None, 1.0e-13), (6, (0.98, 1.02), None, 1.0e-13), (6, "log-uniform", None, 1.0e-13)]  # r6: ln (Mandelbulb extension): |w|^2 up to the bailout, around 1, all magnitudes


@pytest.mark.parametrize("op,ra,rb,eps", FAST_CASES)
def test_fast_functions_return_the_reference_bits(oracle, op, ra, rb, eps):
    """Bit equality with the reference evaluation on 8 M arguments per case, the measured |d_fast - d_ref| / |d_ref| at most a
    third of the EPS the rounding-safety test assumes, and a fallback rate that shows the fast path is the one that runs."""
    import ctypes as C
    rng = np.random.default_rng(100 + op)
    n = 8_000_000
    if op == 4:
        a = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 4, n)).astype(np.float32)
        b = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 4, n)).astype(np.float32)
    elif ra == "log-uniform":
        a = (10.0 ** rng.uniform(-29.9, 29.9, n)).astype(np.float32)
        b = np.zeros(n, np.float32)
    else:
        a = rng.uniform(ra[0], ra[1], n).astype(np.float32)
        b = rng.uniform(rb[0], rb[1], n).astype(np.float32) if rb else np.zeros(n, np.float32)
    L = oracle.lib()
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    out = np.zeros_like(a)
    st = (C.c_double * 2)()
    L.oracle_detmath_fast(C.c_uint32(op), fp(a), fp(b), fp(out), C.c_uint64(n), st)
    ref = oracle.detmath(op, a, b)
    same = (out.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(out) & np.isnan(ref))
    assert same.all(), (int((~same).sum()), a[~same][:4], b[~same][:4])
    assert st[1] < eps / 3.0, st[1]
    if op != 5:
        assert st[0] / n < 1e-3, st[0] / n  # pow: many results underflow below the normal floats and take the reference path by design


def test_fast_functions_special_values(oracle):
    import ctypes as C
    L = oracle.lib()
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    sp = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 3e38, -3e38, 88.5, -87.5, 1e4, -1e4, 1e-30, 1e30, 0.5, 2.0, 300.0], np.float32)
    a, b = [x.ravel().copy() for x in np.meshgrid(sp, sp)]
    st = (C.c_double * 2)()
    for op in range(7):
        out = np.zeros_like(a)
        L.oracle_detmath_fast(C.c_uint32(op), fp(a), fp(b), fp(out), C.c_uint64(a.size), st)
        ref = oracle.detmath(op, a, b)
        assert (((out.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(out) & np.isnan(ref)))).all(), op


# ---- r6: dmf_round_safe decides on the BITS of the binary64 result - its soundness claim, tested directly ----
_ROUND_SAFE_SRC = r"""
#include <cstdint>
#include <cstring>
#include "rayn_detmath_fast.h"
extern "C" void round_safe_batch(const double* d, double eps, uint64_t n, uint8_t* safe, float* out) {
    for (uint64_t i = 0; i < n; i++) { float o = 0.0f; safe[i] = dmf_round_safe(d[i], eps, &o) ? 1 : 0; out[i] = o; }
}
"""


@pytest.fixture(scope="module")
def round_safe_lib(tmp_path_factory):
    import ctypes as C
    import subprocess
    d = tmp_path_factory.mktemp("round_safe")
    src, so = str(d / "rs.cpp"), str(d / "librs.so")
    open(src, "w").write(_ROUND_SAFE_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), src, "-o", so])
    return C.CDLL(so)


@pytest.mark.parametrize("eps", [1.0e-13, 1.0e-12, 2.0e-12, 4.0e-12])
def test_round_safe_is_sound_and_not_wasteful(round_safe_lib, eps):
    """If dmf_round_safe says `safe`, EVERY double within eps |d| of d rounds to the same float (checked at both ends of the interval - rounding is monotonic),
    and the float it returns is that one.  Doubles are drawn uniformly AND packed around the rounding boundaries (midpoints of consecutive floats), where a wrong
    margin would show; the share of uniformly drawn doubles that is refused stays below 2^-11 (the fallback stays rare)."""
    import ctypes as C
    rng = np.random.default_rng(int(eps * 1e15))
    n = 2_000_000
    f = (rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(-100, 100, n).astype(np.float64))).astype(np.float32)
    f[: n // 8] = np.float32(1.0) + rng.integers(0, 64, n // 8).astype(np.float32) * np.float32(2.0 ** -23)  # binade edges too
    mid = (f.astype(np.float64) + np.nextafter(f, np.float32(np.inf)).astype(np.float64)) * 0.5              # exact in binary64
    near = mid * (1.0 + rng.uniform(-3.0, 3.0, n) * eps) * np.where(rng.integers(0, 2, n) == 0, 1.0, -1.0)
    uni = rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(-120, 120, n).astype(np.float64)) * np.where(rng.integers(0, 2, n) == 0, 1.0, -1.0)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-300, 1e300, 2.0 ** -127, 2.0 ** 127, 2.0 ** 128, 3.4e38, 1.17e-38, -1.17e-38], np.float64)
    for d, uniform in ((near, False), (uni, True), (special, False)):
        d = np.ascontiguousarray(d)
        safe = np.zeros(d.size, np.uint8)
        out = np.zeros(d.size, np.float32)
        round_safe_lib.round_safe_batch(d.ctypes.data_as(C.POINTER(C.c_double)), C.c_double(eps), C.c_uint64(d.size), safe.ctypes.data_as(C.POINTER(C.c_uint8)),
                                        out.ctypes.data_as(C.POINTER(C.c_float)))
        s = safe.astype(bool)
        with np.errstate(over="ignore", invalid="ignore"):
            lo, hi, me = (d * (1.0 - eps)).astype(np.float32), (d * (1.0 + eps)).astype(np.float32), d.astype(np.float32)
        assert np.array_equal(out[s].view(np.uint32), me[s].view(np.uint32))
        assert np.array_equal(lo[s].view(np.uint32), hi[s].view(np.uint32)) and np.array_equal(lo[s].view(np.uint32), me[s].view(np.uint32))
        assert np.isfinite(out[s]).all() and (np.abs(out[s]) >= np.float32(2.0 ** -126)).all()
        if uniform:
            inside = (np.abs(d) >= 2.0 ** -126) & (np.abs(d) < 2.0 ** 127)
            assert 0 < (~s[inside]).mean() < 2.0 ** -11, (~s[inside]).mean()  # 2 MARGIN / 2^29: 2^-18 .. 2^-12 for the four EPS in use
        elif d is near:
            assert 0.05 < s.mean() < 0.95  # the sample straddles the margin: both answers occur
    assert not safe.any()  # (the last batch: zeros, infinities, NaN, denormal and overflowing magnitudes all take the reference path)


# ---- r6: "within 1 ulp of float64" sharpened - correctly rounded wherever binary64 decides, and how often that equals THIS host's libm ----
_LIBM_SRC = r"""
#include <cmath>
#include <cstdint>
extern "C" void libm_f32(uint32_t op, const float* a, const float* b, float* out, uint64_t n) {
    for (uint64_t i = 0; i < n; i++) {
        switch (op) {
        case 0: out[i] = expf(a[i]); break;
        case 1: out[i] = sinf(a[i]); break;
        case 2: out[i] = cosf(a[i]); break;
        case 3: out[i] = tanf(a[i]); break;
        case 4: out[i] = atan2f(a[i], b[i]); break;
        case 5: out[i] = powf(a[i], b[i]); break;
        default: out[i] = logf(a[i]); break;
        }
    }
}
"""


@pytest.fixture(scope="module")
def libm_lib(tmp_path_factory):
    import ctypes as C
    import subprocess
    d = tmp_path_factory.mktemp("libm_f32")
    src, so = str(d / "lm.cpp"), str(d / "liblm.so")
    open(src, "w").write(_LIBM_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fno-builtin", "-shared", "-fPIC", src, "-o", so, "-lm"])
    return C.CDLL(so)


@pytest.mark.parametrize("op,fn2,ra,rb", [
    (0, lambda a, b: np.exp(a), (-80.0, 80.0), None), (1, lambda a, b: np.sin(a), (-50.0, 50.0), None), (2, lambda a, b: np.cos(a), (-50.0, 50.0), None),
    (3, lambda a, b: np.tan(a), (-1.56, 1.56), None), (4, lambda a, b: np.arctan2(a, b), (-8.0, 8.0), (-8.0, 8.0)), (5, lambda a, b: np.power(a, b), (0.001, 4.0), (0.05, 60.0)),
    (6, lambda a, b: np.log(a), (1.0e-6, 1.0e4), None)])
def test_pinned_functions_are_correctly_rounded_where_binary64_decides(oracle, libm_lib, op, fn2, ra, rb):
    """rayn_detmath.h claims correctly rounded binary32 results.  numpy's binary64 function is within 1 ulp(binary64) of the true value, so wherever its result is
    more than 4 ulp(binary64) away from a binary32 rounding boundary it DECIDES the correctly rounded float: there the pinned function must return exactly that float
    (1 M arguments per function; the undecided rest - about 2^-26 of them - must still be within 1 ulp).  Next to it, informational but bounded: how many of the same
    arguments THIS host's libm (glibc's expf / sinf / .., what a rayn built here would call: assumption A3, oracle/SENSITIVITY.md) answers differently - glibc's float
    functions are not correctly rounded in every case, so the pinned functions can only match a particular libm where that libm is right."""
    import ctypes as C
    rng = np.random.default_rng(40 + op)
    n = 1_000_000
    a = rng.uniform(ra[0], ra[1], n).astype(np.float32)
    b = rng.uniform(rb[0], rb[1], n).astype(np.float32) if rb else np.zeros(n, np.float32)
    got = oracle.detmath(op, a, b)
    with np.errstate(all="ignore"):
        d = fn2(a.astype(np.float64), b.astype(np.float64))
    u = d.view(np.uint64)
    low = (u & np.uint64(0x1FFFFFFF)).astype(np.int64)
    ex = ((u >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)
    decided = (np.abs(low - 0x10000000) > 4) & (ex >= 897) & (ex < 1150) & np.isfinite(d)
    want = d.astype(np.float32)
    assert decided.mean() > 0.95  # (pow: 2 % of the results leave the binary32-normal range)
    assert np.array_equal(got[decided].view(np.uint32), want[decided].view(np.uint32)), int((got[decided].view(np.uint32) != want[decided].view(np.uint32)).sum())
    rest = ~decided & np.isfinite(d) & (ex >= 897) & (ex < 1150)
    if rest.any():
        assert _ulp_diff(got[rest], want[rest]).max() <= 1
    lm = np.zeros(n, np.float32)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    libm_lib.libm_f32(C.c_uint32(op), fp(a), fp(b), fp(lm), C.c_uint64(n))
    differ = (lm.view(np.uint32) != got.view(np.uint32)) & ~(np.isnan(lm) & np.isnan(got))
    print(f"op {op}: host libm differs from rayn_detmath.h on {int(differ.sum())} of {n} arguments ({differ.mean():.2e}); max {int(_ulp_diff(lm[differ], got[differ]).max()) if differ.any() else 0} ulp")
    # measured here (glibc 2.35, x86-64): exp 6.4e-4, log 2.1e-4, pow 1.0e-3 of the arguments, but sin / cos 1.3 % (arguments up to +-50), tan 3.7 % and atan2 16 % -
    # always by ONE ulp: glibc's sinf / cosf / tanf / atan2f are not correctly rounded, so on THIS libm a rayn build would draw equi-angular distances (src/light.rs:75-102) that differ in the last bit on
    # one call in six; what that does to a frame is oracle/SENSITIVITY.md's row A3.  Bounded only in size: a difference beyond 2 ulp would be a bug on either side.
    assert not differ.any() or _ulp_diff(lm[differ], got[differ]).max() <= 2


# ---- every binade, against a multiprecision reference that shares nothing with the header (tests/detmath_ref.py) ----
SWEEP_OPS = ["exp", "sin", "cos", "tan", "atan2", "pow", "log"]
SWEEP_SEED = 7
HARD_BOUND = 2.0 ** -49  # exp, log, sin, cos, tan, atan2: see _sweep
_sweeps = {}


def _sweep(name):
    """The grid of one function, its correctly rounded results, and which points are HARD.

    rayn_detmath.h evaluates every function in binary64 and converts once to float.  If the binary64 value is within a relative distance E of the true
    value, the float can differ from the correctly rounded one only where the true value lies within E of a binary32 rounding boundary (the midpoint of two
    consecutive floats), and then by one ulp.  A point is hard when its true value is that close; `hardness` is computed from mpmath alone.
      exp, log, sin, cos, tan, atan2: E = 2^-49.  The cores are a reduction of a few binary64 roundings, a polynomial whose truncation is below 2^-56 and
        at most a division, a few 2^-53 in all (test_cores_are_as_accurate_as_the_hard_bound_assumes measures 2^-51.1 .. 2^-52.8); 2^-49 leaves a factor 4.
      pow: E = (4 |y ln x| + 8) 2^-53.  x^y = e^a with a = fl(y * L), L = dm_log_core(x) = ln x (1 + e1), |e1| <= 2.5 x 2^-53 (the roundings of 2 s p and of the two sums; measured
        2^-52.1 on the unary grid), and the product's rounding e2, |e2| <= 2^-53: a = y ln x (1 + e1)(1 + e2), an ABSOLUTE error of at most 3.51 |y ln x| 2^-53 in the exponent, which is the
        RELATIVE error of e^a.  dm_exp_core adds its own error on a binary64 argument (measured 2^-52.8 on floats; the reduction of a 53-bit argument costs
        another |a| 2^-53 through a * LOG2E's k) - (4 |a| + 8) 2^-53 covers the sum.  |y ln x| reaches 104 before the result leaves the floats, so a pow
        result carries up to 2^-44.3 of relative error: pow is NOT correctly rounded next to a tie, and this test pins where it may differ, not that it never does."""
    if name not in _sweeps:
        import detmath_ref as R
        a, b = R.grid_pairs(SWEEP_SEED) if name == "atan2" else R.grid_pow(SWEEP_SEED) if name == "pow" else (R.grid_unary(SWEEP_SEED), None)
        want, hardness = R.correctly_rounded(name, a, b), R.hardness(name, a, b)
        if name == "pow":
            import mpmath
            ylnx = np.array([abs(float(mpmath.log(v))) if v is not None else 0.0 for v in R.truth(name, a, b)])  # |ln(x^y)|, from the reference alone
            bound = (4.0 * ylnx + 8.0) * 2.0 ** -53
        else:
            bound = np.full(a.size, HARD_BOUND)
        _sweeps[name] = (a, np.zeros_like(a) if b is None else b, want, hardness < bound, bound)
    return _sweeps[name]


def _same_bits(x, y):
    return (x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))


@pytest.mark.parametrize("fma", [False, True])
@pytest.mark.parametrize("name", SWEEP_OPS)
def test_pinned_functions_are_correctly_rounded_on_every_binade(oracle, name, fma):
    """Every exponent field, both signs, the mantissas where rounding goes wrong (a power of two, one and two ulps above it, around 1.5, one and two ulps
    below the next power) and seeded random ones - uniform draws from moderate intervals never visit most of these.  The result equals the correctly rounded
    float bit for bit (NaN = NaN, the sign of zero compared) under both mul_add policies, except at a HARD point (_sweep), where it may be one ulp off; hard
    points are at most 0.5 % of a grid.  sin, cos and tan run over ALL binades: the two-piece reduction of dm_sincos_core is exact only below 2^20, and until
    dm_sincos_large existed this test failed from tan(8388610) on (|sin| > 1 from 4.1e16, inf and NaN from 5.3e18)."""
    import detmath_ref as R
    a, b, want, hard, _ = _sweep(name)
    got = oracle.detmath(R.OPS[name], a, b, fma=fma)
    off = ~_same_bits(got, want)
    print(f"{name} (fma={fma}): {int(off.sum())} of {a.size} points differ from the correctly rounded float; {int(hard.sum())} points are hard")
    first = np.flatnonzero(off & ~hard)[:4]
    assert not (off & ~hard).any(), (int((off & ~hard).sum()), a[first], b[first], got[first], want[first])
    assert hard.mean() <= 0.005, hard.mean()
    if off.any():
        assert not (np.isnan(got[off]) | np.isnan(want[off])).any() and _ulp_diff(got[off], want[off]).max() <= 1
    if name in ("sin", "cos", "tan"):
        fin = np.isfinite(a)
        assert np.isfinite(got[fin]).all()  # (tan: no float is close enough to an odd multiple of pi / 2 to overflow)
        if name != "tan":
            assert (np.abs(got[fin]) <= 1.0).all()


@pytest.mark.parametrize("name", SWEEP_OPS)
def test_fast_functions_return_the_reference_bits_on_every_binade(oracle, name):
    """include/rayn_detmath_fast.h (host build) on the same grids: the bits of rayn_detmath.h everywhere.  Most of a grid lies outside the fast windows by
    design, so nothing is claimed about the fallback rate here (test_fast_functions_return_the_reference_bits does that on its own inputs)."""
    import ctypes as C
    import detmath_ref as R
    a, b, _, _, _ = _sweep(name)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    out = np.zeros_like(a)
    st = (C.c_double * 2)()
    oracle.lib().oracle_detmath_fast(C.c_uint32(R.OPS[name]), fp(a), fp(b), fp(out), C.c_uint64(a.size), st)
    same = _same_bits(out, oracle.detmath(R.OPS[name], a, b))
    assert same.all(), (int((~same).sum()), a[~same][:4], b[~same][:4])


@pytest.mark.parametrize("name", SWEEP_OPS)
def test_cores_are_as_accurate_as_the_hard_bound_assumes(oracle, name):
    """Measured, not assumed: the binary64 value each dm_* function hands to its final conversion (oracle_detmath_core) against the multiprecision value,
    max |core - truth| / |truth| over the grid, below the bound that defines a hard point.  The header's opening comment quotes these figures
    (seed 7: exp 2^-52.8, sin 2^-51.8, cos 2^-51.8, tan 2^-51.1, atan2 2^-51.7, log 2^-52.1; pow 2^-45.2, at most 0.78 of its |y ln x| bound)."""
    import detmath_ref as R
    a, b, _, _, bound = _sweep(name)
    core = oracle.detmath_core(R.OPS[name], a, b)
    assert np.isfinite(core).sum() > a.size // 3  # the export covers the grid, not a corner of it
    err = R.core_error(name, a, b, core)
    print(f"{name}: max |core - truth| / |truth| = 2^{np.log2(err.max()):.2f}; largest share of the hard bound {float((err / bound).max()):.3f}")
    assert (err < bound).all(), (float(err.max()), a[np.argmax(err / bound)], b[np.argmax(err / bound)])
