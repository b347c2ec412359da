"""The analytic Sphere on the device against the CPU oracle, bit for bit under both mul_add policies, on the families of tests/sphere_cases.py (what each family
pins is checked without a GPU in tests/test_sphere_cases.py): sphere_hit and sphere_occluded_dir per lane (rayn_hip_probe_shading ops 13 and 14, on every
family, sphere and lane time), and the hitable fold of the PRODUCT extend kernels (rayn_hip_probe_extend at depths 0 and 2) on three worlds - spheres only
(the generic k_extend), spheres before and after one SDF with duplicates and a one-ulp-larger twin (k_extend1, whose candidates are computed at fetch time),
two SDFs (the generic k_extend) - including the rays on which a sphere and the SDF change order.  Nothing here has a tolerance."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import sphere_cases as SC
from common import bits_equal

pytestmark = pytest.mark.gpu
f32 = np.float32
fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))


@contextlib.contextmanager
def _policy(ctx, fma):
    ctx.set_fma_policy(1 if fma else 0)
    try:
        yield
    finally:
        ctx.set_fma_policy(0)


@pytest.fixture(scope="module")
def world():
    return SC.probe_world()


def _per_sphere(groups):
    """the records of a case list per sphere index, with the family of every lane"""
    out = {}
    for fam, idx, rec in groups:
        out.setdefault(idx, ([], []))
        out[idx][0].append(rec)
        out[idx][1].extend([fam] * len(rec))
    return {idx: (np.ascontiguousarray(np.concatenate(recs)), np.array(fams)) for idx, (recs, fams) in out.items()}


def _probe(gpu_ctx, p, op, index, rec):
    from rayn_amd._lib import lib
    out = np.full((len(rec), 1), f32(-7.25), f32)
    rc = lib().rayn_hip_probe_shading(gpu_ctx.h, C.byref(p), op, index, fp(rec), fp(out), None, len(rec))
    assert rc == 0, gpu_ctx.last_error()
    return out[:, 0]


def _report(op, idx, rec, fams, got, ref):
    bad = ~((got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref)))
    i = int(np.nonzero(bad)[0][0])
    per = {f: int(bad[fams == f].sum()) for f in np.unique(fams[bad])}
    return f"op {op} sphere {idx}: {int(bad.sum())} of {len(got)} lanes differ {per}; first lane {i} ({fams[i]})\n  in  {rec[i].tolist()}\n  dev {got[i]!r}  ref {ref[i]!r}"


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("op", [13, 14])
def test_sphere_ops_bit_exact(gpu_ctx, oracle, world, op, fma):
    wd, p = world
    groups = SC.hit_cases(wd, bool(fma)) if op == 13 else SC.occ_cases(wd, bool(fma))
    lanes = 0
    gpu_ctx.upload_world(wd)
    assert gpu_ctx.probe_scene_dispatch(p)["anim_spheres"] == 1
    with _policy(gpu_ctx, fma):
        for idx, (rec, fams) in sorted(_per_sphere(groups).items()):
            got = _probe(gpu_ctx, p, op, idx, rec)
            ref = oracle.probe_shading(wd, op, idx, rec, fma=bool(fma))[:, 0]
            assert bits_equal(got, ref), _report(op, idx, rec, fams, got, ref)
            nan_t = np.isnan(rec[:, 7 if op == 13 else 6])
            if idx == SC.MOVING:
                assert nan_t.any() and (got[nan_t] == (SC.F32_MAX if op == 13 else 1.0)).all()  # the time of a packet without a lane 0: miss / not occluded
            lanes += len(rec)
    print(f"op {op} fma {fma}: {lanes} lanes")
    assert lanes >= 250000


def test_sphere_ops_reject_what_is_no_sphere(gpu_ctx, oracle, world):
    from rayn_amd._lib import lib
    wd, p = world
    buf, mark = np.zeros(8, f32), np.full(1, f32(7.25), f32)
    gpu_ctx.upload_world(wd)
    for op in (13, 14):
        for idx in (wd.n_hitables, 16, 0xFFFFFFFF):
            assert lib().rayn_hip_probe_shading(gpu_ctx.h, C.byref(p), op, idx, fp(buf), fp(mark), None, 1) == -1 and len(gpu_ctx.last_error()) > 10, (op, idx)
            with pytest.raises(ValueError):
                oracle.probe_shading(wd, op, idx, buf[: 8 if op == 13 else 7])
    wd2, p2, sdf = SC.fold_world("F2")
    gpu_ctx.upload_world(wd2)
    for op in (13, 14):
        assert lib().rayn_hip_probe_shading(gpu_ctx.h, C.byref(p2), op, sdf, fp(buf), fp(mark), None, 1) == -1 and "Sphere" in gpu_ctx.last_error()
        assert lib().rayn_hip_probe_shading(gpu_ctx.h, C.byref(p2), op, sdf + 1, fp(buf), fp(mark), None, 1) == 0
    assert mark[0] != f32(7.25)  # (only the accepted call wrote)


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("name", ["F1", "F2", "F3"])
def test_fold_bit_exact(gpu_ctx, oracle, name, fma):
    from rayn_amd._lib import lib
    wd, p, single = SC.fold_world(name)
    gpu_ctx.upload_world(wd)
    d = gpu_ctx.probe_scene_dispatch(p)
    assert d["single_sdf"] == single and d["anim_spheres"] == 0, d  # F2: k_extend1; F1 and F3: the generic k_extend
    assert d["sdf_kind"] == (0 if name == "F2" else -1), d
    org, dirs = SC.fold_rays(wd, bool(fma))
    with _policy(gpu_ctx, fma):
        for depth in (0, 2):
            o, dd = org, dirs
            if name == "F2":  # + the rays on which the SDF and a sphere before / after it change order
                ties = [SC.sdf_tie_rays(oracle, bool(fma), depth, which) for which in ("pre", "post")]
                o, dd = np.concatenate([org] + [t[0] for t in ties]), np.concatenate([dirs] + [t[1] for t in ties])
                print(f"F2 depth {depth} fma {fma}: exact sphere-against-SDF ties sent: pre {ties[0][3]}, post {ties[1][3]}")
            n = len(o) - (1 if len(o) % 64 == 0 else 0)
            o, dd = np.ascontiguousarray(o[:n]), np.ascontiguousarray(dd[:n])
            assert n % 64 != 0 and n >= SC.N_FOLD - 1
            t, obj = np.zeros(n, f32), np.zeros(n, np.uint32)
            rc = lib().rayn_hip_probe_extend(gpu_ctx.h, C.byref(p), depth, fp(o), fp(dd), fp(t), obj.ctypes.data_as(C.POINTER(C.c_uint32)), n)
            assert rc == 0, gpu_ctx.last_error()
            rt, robj = oracle.closest_hit(wd, p, depth, o, dd, fma=bool(fma))
            bad = obj != robj
            assert not bad.any(), (name, fma, depth, int(bad.sum()), int(np.nonzero(bad)[0][0]), obj[bad][:4].tolist(), robj[bad][:4].tolist(), t[bad][:4].tolist(), rt[bad][:4].tolist())
            assert bits_equal(t, rt), (name, fma, depth, int((t.view(np.uint32) != rt.view(np.uint32)).sum()))
