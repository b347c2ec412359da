/* rayn_detmath.h — pinned elementary functions + the FMA policy for the rayn hot path.
 *
 * WHY THIS EXISTS
 * rayn's arithmetic runs through `wide` 0.4.6 / `ultraviolet` 0.4.6 (Cargo.lock:641-669), whose
 * transcendentals (exp, sin_cos, tan, atan2, powf; call sites: src/integrator.rs:65,123,234,272,
 * src/math.rs:89,108,111,217, src/light.rs:61,93-97, src/material.rs:199,236) fall through to the
 * platform libm lane by lane.  A path tracer is chaotic: one ulp of difference in a transcendental
 * can flip a hit/miss three bounces later.  To make "GPU == CPU oracle" a testable statement, both
 * sides evaluate these functions with THIS header: only IEEE-754 correctly-rounded +,-,*,/,sqrt,
 * fusedMultiplyAdd, floor and int<->float conversions in binary64, no implicit contraction, no libm.
 * The polynomial (Horner) steps are EXPLICIT fused multiply-adds (__builtin_fma: one rounding, defined by
 * IEEE 754, the same result from an x86-64 FMA unit, from glibc's software fma and from gfx950's
 * v_fma_f64) - half the binary64 instructions of the mul + add form r1 used, which matters on the GPU
 * (k_shade_setup spends about a third of its cycles here).  The same source
 * compiled by g++ (oracle) and by hipcc for gfx950 (kernels) therefore yields bit-identical floats.
 * Internally everything is evaluated in binary64 and converted once to float.  HOW CLOSE the binary64 value is to the true one is
 * measured, not assumed (tests/test_detmath.py against mpmath at 320 bits, tests/detmath_ref.py: every exponent field, both signs, the
 * mantissas next to the powers of two + seeded random ones; oracle_detmath_core exports the value before the conversion).
 * max |core - truth| / |truth| over those grids:
 *     exp 2^-52.8   log 2^-52.1   sin 2^-51.8   cos 2^-51.8   tan 2^-51.1   atan2 2^-51.7          (all below 2^-49)
 *     pow 2^-45.2: x^y = e^a with a = y * ln x, and the error of ln x and of the product is scaled by |a| - up to 104 before the
 *     result leaves the floats.  Bound (4 |y ln x| + 8) 2^-53, reached to 0.78 of it.
 * THE RULE FOR HARD POINTS: the float returned is the correctly rounded one unless the TRUE value lies within that bound (relative) of a
 * binary32 rounding boundary, the midpoint of two consecutive floats; such a point is hard and may be one ulp off.  On the grids:
 *     exp 3 hard of 32640, 0 off    sin, tan, log 0 hard    cos 2 hard of 32640, 0 off    atan2 33 hard of 118336, 1 off
 *     pow 102 hard of 97800, 15 off by one ulp (bases 2^k (1 - 2^-24) and the like with y = 0.5, 1.5): pow is NOT correctly rounded
 *     next to a tie; that is a stated limit, pinned by the test.
 * sin, cos and tan hold this for EVERY finite float (dm_sincos_large above 2^20), |sin|, |cos| <= 1 included.  Next to a good libm
 * (glibc's sinf / expf / powf are themselves double-evaluated) the results agree wherever that libm is correctly rounded.
 *
 * Both compilers MUST be run with -ffp-contract=off (hipcc defaults to 'fast').
 *
 * FMA POLICY: the reference ships no RUSTFLAGS, so `f32x4::mul_add` in wide 0.4.6
 * compiles to an unfused multiply then add on the default x86-64 target.  RAYN_MULADD is therefore
 * unfused unless RAYN_FMA_POLICY=1 is defined (equivalent to building rayn with +fma).
 */
#ifndef RAYN_DETMATH_H
#define RAYN_DETMATH_H

#include <stdint.h>

#if defined(__HIPCC__)
#define RAYN_HD static __host__ __device__ inline
#else
#define RAYN_HD inline
#endif
#if defined(__HIPCC__) && defined(RAYN_DM_NOINLINE)
#define RAYN_HD_CORE static __host__ __device__ __attribute__((noinline))
#else
#define RAYN_HD_CORE RAYN_HD
#endif
/* A rarely taken arm (dm_sincosf_large, dm_tanf_large): one float in, the results by value, behind an unlikely branch, and whether a
 * call site inlines it is left to the compiler.  k_shade_setup runs at its register cap, and what this arm costs there is decided by what
 * the allocator evicts around it, not by the arm's own instructions (it runs for no argument a shipped scene produces).  Measured on
 * the c3 frame (k_shade_setup 1134 ms): this form +5 ms, the benchmark's headline inside its run-to-run spread; the same with a
 * select per funnel shift in dm_sincos_large +8 ms; forced out of line (noinline, with or without `cold`) +23 ms; the reduction
 * inlined in front of the shared dm_sincos_core +18 ms; the reduction alone out of line +29 ms. */
#if defined(__HIPCC__)
#define RAYN_HD_COLD static __host__ __device__ inline
#else
#define RAYN_HD_COLD inline
#endif

#ifndef RAYN_FMA_POLICY
#define RAYN_FMA_POLICY 0
#endif

/* a*b + c with the policy's rounding: two roundings (policy 0) or one (policy 1). */
RAYN_HD float rayn_muladd(float a, float b, float c) {
#if RAYN_FMA_POLICY
    return __builtin_fmaf(a, b, c);
#else
    return a * b + c;
#endif
}

RAYN_HD double dm_u2d(uint64_t u) { double d; __builtin_memcpy(&d, &u, 8); return d; }
RAYN_HD uint64_t dm_d2u(double d) { uint64_t u; __builtin_memcpy(&u, &d, 8); return u; }
RAYN_HD float dm_u2f(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
RAYN_HD uint32_t dm_f2u(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }

RAYN_HD float dm_nanf() { return dm_u2f(0x7fc00000u); }
RAYN_HD float dm_inff() { return dm_u2f(0x7f800000u); }
RAYN_HD bool dm_isnan(float x) { return x != x; }
RAYN_HD bool dm_isnand(double x) { return x != x; }

/* 2^k as a double, k in [-1022, 1023]. */
/* A polynomial coefficient.  On the GPU it is pinned to a scalar register pair right where it is used: left alone, the
 * compiler keeps all ~60 coefficients of the inlined functions live in vector registers across the whole kernel
 * (k_shade_setup then needs 161 VGPRs instead of 80).  The value is the same on both sides. */
#if defined(__HIP_DEVICE_COMPILE__)
static __device__ inline double dm_k(double c) { asm volatile("" : "+s"(c)); return c; }
#define DM_K(c) dm_k(c)
#else
#define DM_K(c) (c)
#endif

RAYN_HD double dm_pow2i(int k) { return dm_u2d((uint64_t)(k + 1023) << 52); }

/* e^a for a double argument, returned as double; caller guarantees -745 < a < 709. */
RAYN_HD_CORE double dm_exp_core(double a) {
    const double LOG2E = 1.44269504088896338700e+00;
    const double LN2_HI = 6.93147180369123816490e-01; /* 33 significant bits: k*LN2_HI exact */
    const double LN2_LO = 1.90821492927058770002e-10;
    double kf = __builtin_floor(a * LOG2E + 0.5);
    double r = (a - kf * LN2_HI) - kf * LN2_LO; /* |r| <= ~0.347 */
    /* Taylor through r^14/14!  (0.347^14/14! ~ 4e-18) */
    double p = 1.0 / 87178291200.0;
    p = __builtin_fma(p, r, DM_K(1.0 / 6227020800.0));
    p = __builtin_fma(p, r, DM_K(1.0 / 479001600.0));
    p = __builtin_fma(p, r, DM_K(1.0 / 39916800.0));
    p = __builtin_fma(p, r, DM_K(1.0 / 3628800.0));
    p = __builtin_fma(p, r, DM_K(1.0 / 362880.0));
    p = __builtin_fma(p, r, DM_K(1.0 / 40320.0));
    p = __builtin_fma(p, r, DM_K(1.0 / 5040.0));
    p = __builtin_fma(p, r, DM_K(1.0 / 720.0));
    p = __builtin_fma(p, r, DM_K(1.0 / 120.0));
    p = __builtin_fma(p, r, DM_K(1.0 / 24.0));
    p = __builtin_fma(p, r, DM_K(1.0 / 6.0));
    p = __builtin_fma(p, r, DM_K(0.5));
    p = __builtin_fma(p, r, DM_K(1.0));
    p = __builtin_fma(p, r, DM_K(1.0));
    int k = (int)kf;
    /* split the scale so that 2^k never leaves the normal double range */
    int k1 = k / 2, k2 = k - k1;
    return (p * dm_pow2i(k1)) * dm_pow2i(k2);
}

/* expf: wide f32x4::exp stand-in. */
RAYN_HD float dm_expf(float xf) {
    if (dm_isnan(xf)) return xf;
    double x = (double)xf;
    if (x > 89.0) return dm_inff();
    if (x < -104.0) return 0.0f;
    return (float)dm_exp_core(x);
}

/* natural log of a positive, finite double that came from a float (always a normal double). */
RAYN_HD_CORE double dm_log_core(double x) {
    const double LN2_HI = 6.93147180369123816490e-01;
    const double LN2_LO = 1.90821492927058770002e-10;
    uint64_t u = dm_d2u(x);
    int e = (int)((u >> 52) & 0x7ff) - 1023;
    double m = dm_u2d((u & 0x000fffffffffffffULL) | 0x3ff0000000000000ULL); /* [1,2) */
    if (m > 1.41421356237309514547) { m = m * 0.5; e += 1; }
    double s = (m - 1.0) / (m + 1.0); /* |s| <= 0.1716 */
    double z = s * s;
    /* 2*atanh(s) = 2s(1 + z/3 + z^2/5 + ... + z^12/25) */
    double p = 1.0 / 25.0;
    p = __builtin_fma(p, z, DM_K(1.0 / 23.0));
    p = __builtin_fma(p, z, DM_K(1.0 / 21.0));
    p = __builtin_fma(p, z, DM_K(1.0 / 19.0));
    p = __builtin_fma(p, z, DM_K(1.0 / 17.0));
    p = __builtin_fma(p, z, DM_K(1.0 / 15.0));
    p = __builtin_fma(p, z, DM_K(1.0 / 13.0));
    p = __builtin_fma(p, z, DM_K(1.0 / 11.0));
    p = __builtin_fma(p, z, DM_K(1.0 / 9.0));
    p = __builtin_fma(p, z, DM_K(1.0 / 7.0));
    p = __builtin_fma(p, z, DM_K(1.0 / 5.0));
    p = __builtin_fma(p, z, DM_K(1.0 / 3.0));
    p = __builtin_fma(p, z, DM_K(1.0));
    double logm = 2.0 * s * p;
    double ef = (double)e;
    return ef * LN2_HI + (ef * LN2_LO + logm);
}

/* natural log of a float (used by the Mandelbulb distance estimator, an extension outside the reference). */
RAYN_HD float dm_logf(float xf) {
    if (dm_isnan(xf) || xf < 0.0f) return dm_nanf();
    if (xf == 0.0f) return -dm_inff();
    if (xf == dm_inff()) return xf;
    return (float)dm_log_core((double)xf);
}

/* powf for the domain rayn uses (x >= 0 or NaN; src/material.rs:199,236, src/math.rs:108).
 * libm conventions kept: pow(x,0)=1, pow(1,y)=1, pow(0,y>0)=0, negative base -> NaN. */
RAYN_HD float dm_powf(float xf, float yf) {
    if (yf == 0.0f) return 1.0f;
    if (xf == 1.0f) return 1.0f;
    if (dm_isnan(xf) || dm_isnan(yf)) return dm_nanf();
    if (xf < 0.0f) return dm_nanf();
    if (xf == 0.0f) return yf > 0.0f ? 0.0f : dm_inff();
    if (xf == dm_inff()) return yf > 0.0f ? dm_inff() : 0.0f;
    double a = (double)yf * dm_log_core((double)xf);
    if (dm_isnand(a)) return dm_nanf();
    if (a > 89.0) return dm_inff();
    if (a < -104.0) return 0.0f;
    return (float)dm_exp_core(a);
}

/* sin and cos of q * pi/2 + r for a reduced argument |r| <= ~pi/4 and a quadrant q in 0..3. */
RAYN_HD void dm_sincos_poly(double r, int q, double* sn, double* cs) {
    double z = r * r;
    /* sin r = r + r z (s1 + z(s2 + ...)), through r^17/17! */
    double ps = 1.0 / 355687428096000.0;
    ps = __builtin_fma(ps, z, DM_K(-1.0 / 1307674368000.0));
    ps = __builtin_fma(ps, z, DM_K(1.0 / 6227020800.0));
    ps = __builtin_fma(ps, z, DM_K(-1.0 / 39916800.0));
    ps = __builtin_fma(ps, z, DM_K(1.0 / 362880.0));
    ps = __builtin_fma(ps, z, DM_K(-1.0 / 5040.0));
    ps = __builtin_fma(ps, z, DM_K(1.0 / 120.0));
    ps = __builtin_fma(ps, z, DM_K(-1.0 / 6.0));
    double S = r + r * (z * ps);
    /* cos r = 1 + z (c1 + z(c2 + ...)), through r^18/18! */
    double pc = -1.0 / 6402373705728000.0;
    pc = __builtin_fma(pc, z, DM_K(1.0 / 20922789888000.0));
    pc = __builtin_fma(pc, z, DM_K(-1.0 / 87178291200.0));
    pc = __builtin_fma(pc, z, DM_K(1.0 / 479001600.0));
    pc = __builtin_fma(pc, z, DM_K(-1.0 / 3628800.0));
    pc = __builtin_fma(pc, z, DM_K(1.0 / 40320.0));
    pc = __builtin_fma(pc, z, DM_K(-1.0 / 720.0));
    pc = __builtin_fma(pc, z, DM_K(1.0 / 24.0));
    pc = __builtin_fma(pc, z, DM_K(-0.5));
    double C = 1.0 + z * pc;
    if (q == 0) { *sn = S; *cs = C; }
    else if (q == 1) { *sn = C; *cs = -S; }
    else if (q == 2) { *sn = -S; *cs = -C; }
    else { *sn = -C; *cs = S; }
}

/* sin and cos of a double, |x| < 2^20 (rayn's arguments are < 7): k = round(x * 2/pi) stays below 2^20, so k * PIO2_1 (33 bits) is
 * exact and r carries about 2^-53 * |x| of absolute error.  dm_sincosf / dm_tanf send larger arguments to dm_sincos_large. */
RAYN_HD_CORE void dm_sincos_core(double x, double* sn, double* cs) {
    const double TWO_OVER_PI = 6.36619772367581382433e-01;
    const double PIO2_1 = 1.57079632673412561417e+00;  /* first 33 bits of pi/2 */
    const double PIO2_1T = 6.07710050650619224932e-11; /* pi/2 - PIO2_1 */
    double kf = __builtin_floor(x * TWO_OVER_PI + 0.5);
    double r = (x - kf * PIO2_1) - kf * PIO2_1T; /* |r| <= ~pi/4 */
    long long k = (long long)kf;                 /* |kf| < 2^20 */
    dm_sincos_poly(r, (int)(k & 3), sn, cs);
}

/* sin and cos of a finite float with |x| >= 2^20: a Payne-Hanek reduction in integers.  x = +-m 2^e with the 24-bit significand m
 * and e in -3..104.  2/pi = 0.b1 b2 b3.. in binary; the bits b_i with i <= e - 2 contribute multiples of 4 to x * 2/pi and are dropped, the
 * 128 bits W = b_(e-1) .. b_(e+126) are kept (256 bits of 2/pi cover every e), and m * W mod 2^128 is x * 2/pi mod 4 in units of 2^-126:
 * two quadrant bits and a 126-bit fraction, short of the true product by less than m 2^-126 < 2^-102.  The fraction is taken to the nearest
 * quadrant (|f| <= 1/2), its leading 63 bits converted to binary64 (one rounding; the 2^-102 would only show for |f| < 2^-49, and the closest
 * a binary32 comes to a multiple of pi/2 is about 2^-30 of a quadrant: Muller et al., Handbook of Floating-Point Arithmetic, "Range
 * Reduction") and r = f * pi/2 formed with a two-piece pi/2 and one fused step: |r - true| < 2^-52 |r|.
 * Integer operations, one int64 -> binary64 conversion, an exact scaling and one fma: the same bits from g++ and hipcc, and no
 * conversion of an out-of-range value.  Reached only through dm_sincosf_large / dm_tanf_large below. */
RAYN_HD void dm_sincos_large(float xf, double* sn, double* cs) {
    const uint64_t TOP1 = 0xA2F9836E4E441529ULL, TOP2 = 0xFC2757D1F534DDC0ULL; /* floor(2/pi * 2^256), most significant word first */
    const uint64_t TOP3 = 0xDB6295993C439041ULL, TOP4 = 0xFE5163ABDEBBC561ULL;
    const double PIO2_H = 1.57079632679489655800e+00; /* pi/2 rounded to binary64 */
    const double PIO2_L = 6.12323399573676603587e-17; /* pi/2 - PIO2_H */
    const uint32_t u = dm_f2u(xf);
    const uint64_t m = (uint64_t)((u & 0x007fffffu) | 0x00800000u);
    const int g = (int)((u >> 23) & 0xffu) - 150 - 1 + 63; /* position of b_(e-1) in the string {64 zero bits, TOP1, TOP2, TOP3, TOP4}: 59..166 */
    const int w = g >> 6, sh = g & 63;
    const uint64_t w0 = w == 0 ? 0ULL : (w == 1 ? TOP1 : TOP2);
    const uint64_t w1 = w == 0 ? TOP1 : (w == 1 ? TOP2 : TOP3);
    const uint64_t w2 = w == 0 ? TOP2 : (w == 1 ? TOP3 : TOP4);
    const uint64_t whi = (w0 << sh) | ((w1 >> 1) >> (63 - sh)); /* (w1 >> 1) >> (63 - sh): w1 >> (64 - sh), and 0 for sh = 0 */
    const uint64_t wlo = (w1 << sh) | ((w2 >> 1) >> (63 - sh));
    /* m * W mod 2^128 from 24 x 32 -> 56-bit partial products */
    const uint64_t p0 = m * (wlo & 0xffffffffULL), p1 = m * (wlo >> 32);
    uint64_t lo = p0 + (p1 << 32);
    uint64_t hi = m * whi + (p1 >> 32) + (lo < p0 ? 1ULL : 0ULL);
    int q = (int)(hi >> 62);
    hi &= 0x3fffffffffffffffULL;
    const bool up = (hi >> 61) != 0; /* fraction >= 1/2: the next quadrant, f = fraction - 1 < 0 */
    if (up) {
        q += 1;
        hi = 0x4000000000000000ULL - hi - (lo != 0 ? 1ULL : 0ULL); /* 2^126 - (hi 2^64 + lo) */
        lo = 0ULL - lo;
    }
    double f = 0.0; /* |fraction| as a binary64 */
    if (hi != 0) {
        const int lz = __builtin_clzll(hi); /* 2..63 */
        const uint64_t t = (hi << (lz - 1)) | (lo >> (65 - lz)); /* leading 63 bits */
        f = (double)(int64_t)t * dm_pow2i(-61 - lz);
    } else if (lo != 0) {
        const int lz = __builtin_clzll(lo);
        f = (double)(int64_t)((lo << lz) >> 1) * dm_pow2i(-125 - lz);
    }
    double r = __builtin_fma(f, PIO2_H, f * PIO2_L);
    if (up) r = -r;
    double s, c;
    dm_sincos_poly(r, q & 3, &s, &c);
    *sn = (u >> 31) ? -s : s; /* sin is odd, cos even */
    *cs = c;
}

/* The large-argument arm as dm_sincosf / dm_tanf reach it (RAYN_HD_COLD above): an early exit, the code for |x| < 2^20 stays as it was. */
struct dm_sincos_pair { float sn, cs; };
RAYN_HD_COLD dm_sincos_pair dm_sincosf_large(float xf) {
    double s, c;
    dm_sincos_large(xf, &s, &c);
    dm_sincos_pair p;
    p.sn = (float)s;
    p.cs = (float)c;
    return p;
}
RAYN_HD_COLD float dm_tanf_large(float xf) {
    double s, c;
    dm_sincos_large(xf, &s, &c);
    return (float)(s / c);
}

/* f32x4::sin_cos stand-in: every finite float (|x| < 2^20: dm_sincos_core; above: dm_sincos_large). */
RAYN_HD void dm_sincosf(float xf, float* sn, float* cs) {
    float ax = xf < 0.0f ? -xf : xf;
    if (dm_isnan(xf) || ax == dm_inff()) { *sn = dm_nanf(); *cs = dm_nanf(); return; }
    if (__builtin_expect(ax >= 1048576.0f, 0)) { const dm_sincos_pair p = dm_sincosf_large(xf); *sn = p.sn; *cs = p.cs; return; }
    double s, c;
    dm_sincos_core((double)xf, &s, &c);
    *sn = xf == 0.0f ? xf : (float)s; /* sin(-0) = -0: the core's r + r * (z * ps) is +0 for r = -0 */
    *cs = (float)c;
}

RAYN_HD float dm_cosf(float xf) { float s, c; dm_sincosf(xf, &s, &c); return c; }
RAYN_HD float dm_sinf(float xf) { float s, c; dm_sincosf(xf, &s, &c); return s; }

/* f32x4::tan stand-in (src/light.rs:97; host: src/camera.rs:61). */
RAYN_HD float dm_tanf(float xf) {
    float ax = xf < 0.0f ? -xf : xf;
    if (dm_isnan(xf) || ax == dm_inff()) return dm_nanf();
    if (__builtin_expect(ax >= 1048576.0f, 0)) return dm_tanf_large(xf);
    double s, c;
    dm_sincos_core((double)xf, &s, &c);
    return xf == 0.0f ? xf : (float)(s / c); /* tan(-0) = -0 (see dm_sincosf) */
}

/* atan of t in [0,1]. */
RAYN_HD_CORE double dm_atan_core(double t) {
    const double PI_4 = 7.85398163397448278999e-01;
    double base = 0.0, u = t;
    if (t > 0.41421356237309503) { u = (t - 1.0) / (t + 1.0); base = PI_4; }
    double z = u * u; /* z <= 0.1716 */
    /* u(1 - z/3 + z^2/5 - ... ) through z^23/47 */
    double p = -1.0 / 47.0;
    p = __builtin_fma(p, z, DM_K(1.0 / 45.0));
    p = __builtin_fma(p, z, DM_K(-1.0 / 43.0));
    p = __builtin_fma(p, z, DM_K(1.0 / 41.0));
    p = __builtin_fma(p, z, DM_K(-1.0 / 39.0));
    p = __builtin_fma(p, z, DM_K(1.0 / 37.0));
    p = __builtin_fma(p, z, DM_K(-1.0 / 35.0));
    p = __builtin_fma(p, z, DM_K(1.0 / 33.0));
    p = __builtin_fma(p, z, DM_K(-1.0 / 31.0));
    p = __builtin_fma(p, z, DM_K(1.0 / 29.0));
    p = __builtin_fma(p, z, DM_K(-1.0 / 27.0));
    p = __builtin_fma(p, z, DM_K(1.0 / 25.0));
    p = __builtin_fma(p, z, DM_K(-1.0 / 23.0));
    p = __builtin_fma(p, z, DM_K(1.0 / 21.0));
    p = __builtin_fma(p, z, DM_K(-1.0 / 19.0));
    p = __builtin_fma(p, z, DM_K(1.0 / 17.0));
    p = __builtin_fma(p, z, DM_K(-1.0 / 15.0));
    p = __builtin_fma(p, z, DM_K(1.0 / 13.0));
    p = __builtin_fma(p, z, DM_K(-1.0 / 11.0));
    p = __builtin_fma(p, z, DM_K(1.0 / 9.0));
    p = __builtin_fma(p, z, DM_K(-1.0 / 7.0));
    p = __builtin_fma(p, z, DM_K(1.0 / 5.0));
    p = __builtin_fma(p, z, DM_K(-1.0 / 3.0));
    p = __builtin_fma(p, z, DM_K(1.0));
    return base + u * p;
}

/* f32x4::atan2 stand-in: dm_atan2f(y, x) == y.atan2(x) (src/light.rs:93-94). */
RAYN_HD float dm_atan2f(float yf, float xf) {
    const double PI = 3.14159265358979311600e+00;
    const double PI_2 = 1.57079632679489655800e+00;
    if (dm_isnan(xf) || dm_isnan(yf)) return dm_nanf();
    bool xneg = (dm_f2u(xf) >> 31) != 0;
    bool yneg = (dm_f2u(yf) >> 31) != 0;
    double ax = (double)(xneg ? -xf : xf);
    double ay = (double)(yneg ? -yf : yf);
    double a;
    double inf = (double)dm_inff();
    if (ax == 0.0 && ay == 0.0) a = 0.0;
    else if (ax == inf && ay == inf) a = 0.78539816339744827900;
    else if (ay == inf) a = PI_2;
    else if (ax == inf) a = 0.0;
    else if (ay > ax) a = PI_2 - dm_atan_core(ax / ay);
    else a = dm_atan_core(ay / ax);
    if (xneg) a = PI - a;
    float r = (float)a;
    return yneg ? -r : r;
}

/* f32::fract as Rust defines it: x - trunc(x) (src/sampler.rs:63,92; src/filter.rs:231). */
RAYN_HD float dm_fractf(float x) { return x - __builtin_truncf(x); }

#endif /* RAYN_DETMATH_H */
