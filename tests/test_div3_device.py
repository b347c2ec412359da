"""div3_by on the device (probe ops 17 / 18 / 19 of rayn_hip_probe_detmath) against IEEE division: every bit of every quotient, inside the
window (shared refined reciprocal) and outside it (literal divisions).  Operands: tests/div3_cases.py."""
import ctypes as C

import numpy as np
import pytest

import div3_cases as D

pytestmark = pytest.mark.gpu


def test_div3_by_is_ieee(gpu_ctx):
    from rayn_amd._lib import lib
    v, m = D.operands()
    n = m.size
    assert n >= 1 << 22
    win = D.in_window(v, m)
    assert 0.5 < win.mean() < 0.9 and (~win).sum() > 100000  # both paths are exercised
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    ref = D.ieee(v, m)
    for c, op in enumerate((17, 18, 19)):
        out = np.zeros(n, np.float32)
        assert lib().rayn_hip_probe_detmath(gpu_ctx.h, op, fp(v), fp(m), fp(out), n) == 0
        bad = D.mismatches(out, ref[:, c])
        assert bad.size == 0, (c, bad.size, [(v[i].tolist(), float(m[i]), float(out[i]), float(ref[i, c])) for i in bad[:5, 0]])
