"""CPU twin of tests/test_div3_device.py: div3_by (rayn_amd/csrc/device_core.h, a device-only function built on v_rcp_f32) restated in
numpy on the same operands.  binary32 fma is emulated exactly through binary64 (the product of two binary32 numbers is exact in binary64;
the one rounding of the sum is repaired where it lands on a binary32 tie).  The hardware reciprocal is accurate to 1 ulp and otherwise
unspecified: the restatement starts from the correctly rounded reciprocal moved by -1, 0 and +1 ulp and must return the IEEE quotient from
each - the sequence does not depend on which of them the hardware delivers."""
import numpy as np

import div3_cases as D


def fma32(a, b, c):
    """fl32(a * b + c) for float32 arrays, exactly"""
    p = a.astype(np.float64) * b.astype(np.float64)  # exact: 48 significant bits
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)  # TwoSum: p + c == s + err exactly
    r = s.astype(np.float32)
    d = s - r.astype(np.float64)  # exact
    up = np.nextafter(r, np.float32(np.inf), dtype=np.float32).astype(np.float64) - r.astype(np.float64)
    dn = r.astype(np.float64) - np.nextafter(r, np.float32(-np.inf), dtype=np.float32).astype(np.float64)
    # r was chosen by ties-to-even on s; where s sat exactly on a binary32 tie and err != 0, the true sum lies on err's side of it
    r = np.where((d == 0.5 * up) & (err > 0), np.nextafter(r, np.float32(np.inf), dtype=np.float32), r)
    r = np.where((d == -0.5 * dn) & (err < 0), np.nextafter(r, np.float32(-np.inf), dtype=np.float32), r)
    return r


def div3_by_np(v, m, ulp):
    """div3_by with rcp(m) = the correctly rounded reciprocal moved by `ulp` units in the last place"""
    win = D.in_window(v, m)
    out = D.ieee(v, m)
    vw, mw = v[win], m[win]
    r = (np.float64(1.0) / mw.astype(np.float64)).astype(np.float32)
    for _ in range(abs(ulp)):
        r = np.nextafter(r, np.float32(np.inf if ulp > 0 else -np.inf), dtype=np.float32)
    one = np.ones_like(mw)
    r = fma32(fma32(-mw, r, one), r, r)
    q = np.empty_like(vw)
    for c in range(3):
        a = vw[:, c]
        qc = a * r
        qc = fma32(fma32(-mw, qc, a), r, qc)
        qc = fma32(fma32(-mw, qc, a), r, qc)
        q[:, c] = qc
    out[win] = q
    return out


def test_fma32_rounds_once():
    a = np.array([1.0 + 2.0 ** -23, 3.0, 1.5, 2.0 ** -30], np.float32)
    b = np.array([1.0 + 2.0 ** -23, 1.0 / 3.0, 2.0 ** -24, 2.0 ** -30], np.float32)
    c = np.array([-1.0, -1.0, 1.0, 1.0], np.float32)
    from fractions import Fraction
    got = fma32(a, b, c)
    for i in range(a.size):  # the result is a nearest binary32 neighbour of the exact rational value
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        near = np.float32(float(exact))
        cands = [np.nextafter(near, np.float32(-np.inf), dtype=np.float32), near, np.nextafter(near, np.float32(np.inf), dtype=np.float32)]
        best = min(abs(Fraction(float(x)) - exact) for x in cands)
        assert abs(Fraction(float(got[i])) - exact) == best, (i, float(got[i]), float(exact))


def test_div3_by_restated_is_ieee():
    v, m = D.operands()
    ref = D.ieee(v, m)
    win = D.in_window(v, m)
    assert 0.5 < win.mean() < 0.9
    bad = D.mismatches(div3_by_np(v, m, 0), ref)
    assert bad.size == 0, (bad.size, [(v[i].tolist(), float(m[i])) for i in bad[:5, 0]])
    # the hardware reciprocal's 1-ulp freedom: the edge cases and the first 2^19 bulk triples
    k = m.size - (1 << 22) + (1 << 19)
    for ulp in (-1, 1):
        bad = D.mismatches(div3_by_np(v[:k], m[:k], ulp), ref[:k])
        assert bad.size == 0, (ulp, bad.size, [(v[i].tolist(), float(m[i])) for i in bad[:5, 0]])
