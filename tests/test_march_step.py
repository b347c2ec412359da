"""The per-step bookkeeping of the single-SDF march kernels (k_shadow1 / k_extend1): the straight-line march test in which 'first' is data (wave masks),
on the corners of TracedSDF::occluded / TracedSDF::hit - NaN first and later distances, exhausted and zero march budgets, signed zeros.

Mode: about 30 000 entries per launch, far below ENDGAME_ENTRIES (rayn_amd/csrc/kernels.h), so every launch here runs the kernels' ENDGAME - one ray per lane, fetched
when the lane is idle, no spare rays - and k_shadow_bulb is not run at all.  The same corner classes in the STEADY STATE (spares, K rays per lane), spread
through queues sized from the library's thresholds, are in tests/test_march_steady_device.py (inputs: tests/march_cases.py)."""
import ctypes as C

import numpy as np
import pytest

def _fp(x):
    return x.ctypes.data_as(C.POINTER(C.c_float))


def _world(name, **kw):
    import rayn_amd as R
    from rayn_amd import params as P
    from rayn_amd import setup as S
    cam, world = S.SCENES[name]((64, 64))
    sdf_only = kw.pop("sdf_only", False)
    if sdf_only:
        world.hitables[:] = [h for h in world.hitables if isinstance(h, R.TracedSDF)]
    return world.to_desc(cam), P.frame_params(64, 64, 1, 3, **kw)


def _segments(n, seed):
    """Shadow segments that reach the corners of the march test: ordinary ones, NaN / infinite starts (a NaN FIRST distance), starts far outside (the first
    distance exceeds the segment), zero-length segments (NaN direction: NaN LATER distances), ends inside the set, signed zeros."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32)
    b = rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32)
    a[0:200, 0] = np.nan
    a[200:300, 1] = np.inf
    a[300:600] *= np.float32(40.0)
    b[600:900] = a[600:900]
    b[900:1500] *= np.float32(0.05)
    a[1500:1600] = np.float32(-0.0); b[1600:1700] = np.float32(-0.0)
    b[1700:1800, 2] = np.nan
    a[1800:2000] = b[1800:2000] + rng.uniform(-1e-5, 1e-5, (200, 3)).astype(np.float32)
    return a, b


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", [("s1", {}), ("s1", {"max_vis_marches": 0}), ("s1", {"max_vis_marches": 1}), ("s1", {"max_vis_marches": 5}),
                                     ("s1", {"sdf_detail_scale": 2.0}), ("s0", {}), ("s0", {"max_vis_marches": 0}), ("s0", {"max_vis_marches": 3})])
def test_occluded_march_test_cases(gpu_ctx, oracle, name, kw):
    """k_shadow1 (MandelBox in its shipped-shape instantiation, sphere SDF in the generic one) against TracedSDF::occluded of the oracle on the segments above."""
    from rayn_amd._lib import lib
    wd, p = _world(name, sdf_only=True, **kw)
    gpu_ctx.upload_world(wd)
    n = 30000 + 37
    a, b = _segments(n, 31)
    out = np.zeros(n, np.float32)
    assert lib().rayn_hip_probe_shadow(gpu_ctx.h, C.byref(p), _fp(a), _fp(b), _fp(out), n) == 0, gpu_ctx.last_error()
    ref = oracle.test_occluded(wd, p, a, b)
    print(name, kw, "mismatches:", int((out != ref).sum()), "occluded share:", float(ref.mean()))
    assert np.array_equal(out, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name,depth,kw", [("s1", 0, {}), ("s1", 2, {"max_marches": 0}), ("s1", 0, {"max_marches": 1}), ("s1", 2, {"max_marches": 12}),
                                           ("s0", 0, {"max_marches": 0}), ("s0", 2, {"max_marches": 7}), ("bulb", 0, {"max_marches": 9})])
def test_closest_hit_march_test_cases(gpu_ctx, oracle, name, depth, kw):
    """k_extend1 against HitableStore::add_hits of the oracle on rays that include NaN / infinite origins and directions (a NaN first distance, NaN later
    distances), origins far outside and exhausted march budgets."""
    from rayn_amd._lib import lib
    wd, p = _world(name, **kw)
    gpu_ctx.upload_world(wd)
    n = 30000 - 5
    rng = np.random.default_rng(41)
    org = rng.uniform(-3.0, 3.0, (n, 3)).astype(np.float32)
    d = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    org[0:200, 0] = np.nan
    org[200:300, 2] = np.inf
    d[300:500, 1] = np.nan
    org[500:800] *= np.float32(30.0)
    d[800:900] = np.float32(0.0)
    org[900:1000] = np.float32(-0.0)
    t = np.zeros(n, np.float32)
    obj = np.zeros(n, np.uint32)
    assert lib().rayn_hip_probe_extend(gpu_ctx.h, C.byref(p), depth, _fp(org), _fp(d), _fp(t), obj.ctypes.data_as(C.POINTER(C.c_uint32)), n) == 0, gpu_ctx.last_error()
    rt, robj = oracle.closest_hit(wd, p, depth, org, d)
    same_t = (t.view(np.uint32) == rt.view(np.uint32)) | (np.isnan(t) & np.isnan(rt))
    print(name, depth, kw, "object mismatches:", int((obj != robj).sum()), "t mismatches:", int((~same_t).sum()))
    assert np.array_equal(obj, robj)
    assert same_t.all()
