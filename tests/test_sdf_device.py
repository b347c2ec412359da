"""What the VALUES of an uploaded scene select - DHitable::fast_div (build_scene), the march kernels and their instantiation (scene_march_kernels), the arm of
sdf_dist (device_core.h) - on the rows of tests/sdf_cases.py: the dispatch each row gets (rayn_hip_probe_scene_dispatch), the distance function in every
admissible instantiation and division arm (rayn_hip_probe_sdf_dist_as), the PRODUCT march kernels the dispatch names (rayn_hip_probe_extend /
rayn_hip_probe_shadow) and a whole film, each against the CPU oracle bit for bit under both mul_add policies; plus div_nr at the corners of the exponent
window that enables it.

On the parent of the commit that added this file the rows side_m1 and side_nan disagreed with the oracle in every arm (4356 and 4405 of 4407 points: the box
fold was the median of (p, -l, l) for every box side); build_scene now sends a negative, -0 or NaN box side to the fast_div == 0 arm, which clamps in the
reference's order.  test_film[bulb_it0] lost whole groups of depth-1 rays there (a register copy of k_shade_setup made under an empty exec mask; its docstring)."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import sdf_cases as SC
from common import bits_equal, film_equal_bits

pytestmark = pytest.mark.gpu
INVALID_ARG = -1  # RAYN_ERR_INVALID_ARG (include/rayn_hip.h)


@contextlib.contextmanager
def _policy(ctx, fma):
    ctx.set_fma_policy(1 if fma else 0)
    try:
        yield
    finally:
        ctx.set_fma_policy(0)


def _scene(name, sdf_only=False):
    row = SC.BY_NAME[name]
    wd, p, idx = SC.scene(row, sdf_only=sdf_only)
    return row, wd, p, idx


def _expected_kind(row, h, fd):
    if not row["expect"]["single"]:
        return -1
    if h.sdf_kind == 1 and fd == 2 and h.iterations == 12:
        return 100
    return int(h.sdf_kind)


@pytest.mark.parametrize("name", SC.ROW_NAMES)
def test_dispatch(gpu_ctx, name):
    row, wd, p, idx = _scene(name)
    gpu_ctx.upload_world(wd)
    d = gpu_ctx.probe_scene_dispatch(p)
    e, h = row["expect"], wd.hitables[idx]
    fd = d["fast_div"]
    assert len(fd) == wd.n_hitables
    assert (fd[idx] == 0) if e["fd0"] else (fd[idx] in (1, 2)), fd
    if row["kind"] == "box" and not e["fd0"] and not h.min_radius < h.fixed_radius:
        assert fd[idx] == 1  # short_div_is_exact: nothing to verify when no denominator lies in [min^2, fixed^2)
    assert all(v == 0 for i, v in enumerate(fd) if i != idx), fd  # analytic spheres and the sphere SDF carry no fold constants
    assert d["single_sdf"] == (idx if e["single"] else -1)
    assert d["sdf_kind"] == _expected_kind(row, h, fd[idx]), d
    assert (d["sdf_kind"] == 100) == (e["single"] and h.sdf_kind == 1 and fd[idx] == 2 and h.iterations == 12)
    assert d["bulb"] == int(e["bulb"]) and d["anim_spheres"] == int(e["anim"]), d
    gpu_ctx.set_fma_policy(1)  # the decisions do not depend on the mul_add policy
    try:
        assert gpu_ctx.probe_scene_dispatch(p) == d
    finally:
        gpu_ctx.set_fma_policy(0)


def test_verdict_of_every_listed_pair(gpu_ctx):
    """k_verify_short_div's verdict for every (min_radius, fixed_radius) of SC.VERDICT_PAIRS: an in-window MandelBox gets 1 (div_nr) or 2 (div_short).  Measured on
    gfx950: all 34 pairs get 2; div_nr is what the probe's lowering and the rows mr_gt_fr / mr_eq_fr run."""
    got = {}
    for mr, fr in SC.VERDICT_PAIRS:
        wd, p, idx = SC.scene(SC.verdict_row(mr, fr))
        gpu_ctx.upload_world(wd)
        got[(mr, fr)] = gpu_ctx.probe_scene_dispatch(p)["fast_div"][idx]
    print("verdicts:", {v: sum(1 for x in got.values() if x == v) for v in (0, 1, 2)}, "div_nr pairs:", [k for k, v in got.items() if v == 1])
    assert all(v in (1, 2) for v in got.values()), got


def _group_report(groups, bad):
    return {k: int(bad[s].sum()) for k, s in groups.items() if bad[s].any()}


@pytest.mark.parametrize("name", SC.ROW_NAMES)
def test_distance_in_every_admissible_arm(gpu_ctx, oracle, name):
    row, wd, p, idx = _scene(name)
    pts, groups = SC.points(row)
    h = wd.hitables[idx]
    gpu_ctx.upload_world(wd)
    own = gpu_ctx.probe_scene_dispatch(p)["fast_div"][idx]
    arms = SC.admissible_arms(int(h.sdf_kind), int(h.iterations), own)
    for fma in (False, True):
        with _policy(gpu_ctx, fma):
            for t0 in row["t0s"]:
                ref = oracle.sdf_dist(h, pts, fma=fma, t0=t0)
                for sdfk, fd in arms:
                    _, got = gpu_ctx.probe_sdf_dist_as(p, idx, sdfk, fd, pts, t0=t0)
                    bad = ~((got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref)))
                    assert not bad.any(), (name, fma, t0, sdfk, fd, int(h.iterations), _group_report(groups, bad))
                if t0 == 0.0:  # the unnamed probe is the generic instantiation in the object's own arm
                    got = np.zeros(len(pts), np.float32)
                    from rayn_amd._lib import lib
                    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
                    assert lib().rayn_hip_probe_sdf_dist(gpu_ctx.h, C.byref(p), idx, fp(pts), fp(got), len(pts)) == 0
                    assert bits_equal(got, oracle.sdf_dist(h, pts, fma=fma))


def test_invalid_arm_requests_are_refused(gpu_ctx):
    pts = SC.points(SC.BY_NAME["it12"])[0][:256]
    mark = np.float32(7.25)

    def refused(name, sdfk, fd):
        _, wd, p, idx = _scene(name)
        gpu_ctx.upload_world(wd)
        own = gpu_ctx.probe_scene_dispatch(p)["fast_div"][idx]
        out = np.full(len(pts), mark, np.float32)
        rc, _ = gpu_ctx.probe_sdf_dist_as(p, idx, sdfk, fd(own) if callable(fd) else fd, pts, out=out, check=False)
        assert rc == INVALID_ARG and len(gpu_ctx.last_error()) > 10 and (out == mark).all(), (name, sdfk, rc, gpu_ctx.last_error())
        return gpu_ctx.last_error()

    texts = [refused("it12", 2, 0), refused("it12", 0, 0), refused("bulb_it8", 1, 0), refused("sphere_sdf", 2, 0),  # an sdfk that is not the object's kind
             refused("it12", 7, 0), refused("it12", -2, 0),
             refused("it5", 100, 2), refused("mr_2m31", 100, 2), refused("mr_eq_fr", 100, 2), refused("bulb_it8", 100, 2),  # 100 without 12 iterations / fast_div 2
             refused("it12", 100, 1),
             refused("it12", -1, lambda own: own + 1), refused("mr_2m31", 1, 1), refused("mr_eq_fr", -1, 2), refused("sphere_sdf", 0, 1)]  # above the object's own
    assert len(set(texts)) >= 4
    _, wd, p, idx = _scene("it12")  # and the accepted neighbours of those calls
    gpu_ctx.upload_world(wd)
    for sdfk, fd in ((1, 0), (-1, 0)):
        rc, out = gpu_ctx.probe_sdf_dist_as(p, idx, sdfk, fd, pts)
        assert rc == 0 and np.isfinite(out).all()


@pytest.mark.parametrize("name", SC.ROW_NAMES)
def test_march_kernels_the_dispatch_names(gpu_ctx, oracle, name):
    from rayn_amd._lib import lib
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    row, wd, p, idx = _scene(name)
    org, d = SC.rays()
    a, b = SC.segments()
    n = len(org)
    assert n == 8192 - 13
    _, wd_s, p_s, _ = _scene(name, sdf_only=True)
    for fma in (False, True):
        with _policy(gpu_ctx, fma):
            gpu_ctx.upload_world(wd)
            for depth in (0, 2):
                t, obj = np.zeros(n, np.float32), np.zeros(n, np.uint32)
                assert lib().rayn_hip_probe_extend(gpu_ctx.h, C.byref(p), depth, fp(org), fp(d), fp(t), obj.ctypes.data_as(C.POINTER(C.c_uint32)), n) == 0, gpu_ctx.last_error()
                rt, robj = oracle.closest_hit(wd, p, depth, org, d, fma=fma)
                assert np.array_equal(obj, robj), (name, fma, depth, int((obj != robj).sum()))
                assert bits_equal(t, rt), (name, fma, depth)
                ids = set(np.unique(obj).tolist())  # the sky and the SDF (two rows have no surface to meet: a NaN distance, a distance never near zero)
                assert 0 in ids and (idx in ids) == row["hits_sdf"], (name, sorted(ids))
            gpu_ctx.upload_world(wd_s)
            out = np.zeros(n, np.float32)
            assert lib().rayn_hip_probe_shadow(gpu_ctx.h, C.byref(p_s), fp(a), fp(b), fp(out), n) == 0, gpu_ctx.last_error()
            ref = oracle.test_occluded(wd_s, p_s, a, b, fma=fma)
            assert np.array_equal(out, ref), (name, fma, int((out != ref).sum()))


@pytest.mark.parametrize("name", SC.ROW_NAMES)
def test_film(gpu_ctx, oracle, name):
    """A 40x32 film at 8 spp and 3 bounces per row against the oracle: every bit, and the path and segment counts.

    The row bulb_it0 (a Mandelbulb with 0 iterations, d = 0.25 ln|p|^2 |p|: the unit sphere) found a miscompiled k_shade_setup: 12251 to 12700 segments
    against the oracle's 13341, whole 64-slot groups of depth-0 hits spawning no depth-1 ray.  The kernel took its lane number from threadIdx.x at its very
    end, and the compiler's copy that keeps that register across the out-of-line bulb_logf call ran under an empty exec mask when no lane of a wave entered
    the orbit loop; the kernel now takes thread and lane number from its slot index (finding 2)."""
    row, wd, p, idx = _scene(name)
    tabs = oracle.build_tables(4 * p.samples, p.max_bounces, p.volume_marches, p.frame, p.width, p.height)
    gpu_ctx.upload_world(wd)
    for fma in (False, True):
        ref, ctr = oracle.render(wd, p, tabs, fma=fma)
        with _policy(gpu_ctx, fma):
            out = gpu_ctx.render_host(p, tabs)
            st = gpu_ctx.stats()
        assert st["paths"] == ctr.paths and st["segments"] == ctr.segments, (name, fma)
        assert film_equal_bits(out, ref), (name, fma)


def test_div_nr_at_the_corners_of_its_window(gpu_ctx):
    """div_nr == IEEE division in every bit where the window that enables it ends: numerators 2^60 (the largest fixed_radius^2) and its neighbours below,
    denominators every float of [2^-60, 2^-60 + 2^16 ulp) and of (2^60 - 2^16 ulp, 2^60] - the quotients reach 2^120 and 1 - plus seeded ones across the
    window.  test_gpu_parity.test_fast_division_is_ieee keeps |log2 q| < 100."""
    from rayn_amd._lib import lib
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    lo_bits, hi_bits = int(np.float32(2.0 ** -60).view(np.uint32)), int(np.float32(2.0 ** 60).view(np.uint32))
    k = np.arange(1 << 16, dtype=np.uint32)
    rng = np.random.default_rng(6)
    seeded = (rng.uniform(1.0, 2.0, 1 << 16) * np.exp2(rng.integers(-60, 60, 1 << 16).astype(np.float64))).astype(np.float32)
    den = np.concatenate([(lo_bits + k).view(np.float32), (hi_bits - k).view(np.float32), seeded])
    assert den.min() == np.float32(2.0 ** -60) and den.max() == np.float32(2.0 ** 60)
    nums = (np.uint32(hi_bits) - np.array([0, 1, 2, 3, 1 << 22, (1 << 23) - 1], np.uint32)).view(np.float32)
    num = np.repeat(nums, den.size)
    den = np.tile(den, nums.size)
    out = np.zeros_like(num)
    assert lib().rayn_hip_probe_detmath(gpu_ctx.h, 6, fp(num), fp(den), fp(out), num.size) == 0
    want = num / den
    assert np.isfinite(want).all() and want.max() == np.float32(2.0 ** 120)
    bad = out.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (int(bad.sum()), num[bad][:4], den[bad][:4])
