"""The reprojection kernels at their decision edges on the GPU: every case of tests/reproject_cases.py (what each pins, and which wrong
reading it tells from the statement, is checked without a GPU in tests/test_reproject_cases.py) through every entry it applies to, bit for
bit against the numpy restatements - k_temporal_accumulate<MOMENTS, RESAMPLE> in its four instantiations (Context.temporal_accumulate
plain and with moments, the resample entry with resample 0 and 1), k_temporal_upscale at factor 1 (where it must equal the accumulate)
and at factor 2 on the upscale families with the confidence off and on, k_upscale and k_interpolate - under both mul_add policies where
the entry's older device test runs under both.  The hand-written outcomes are asserted on the device's own output too.  Images are at
most 32x16; nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

import device_io as IO
import reproject_cases as RC
import scenes
import temporal_cases as TC
import temporal_np as T
from device_io import module_context as ctx  # noqa: F401

pytestmark = pytest.mark.gpu

f32 = np.float32
CASES = RC.all_cases()
ACC = [c for c in CASES if c.entry in ("accumulate", "tiny", "resample")]  # a Catmull-Rom case is an accumulate input like any other
UPSCALE = [c for c in CASES if c.entry == "upscale"]
INTERP = [c for c in CASES if c.entry == "interpolate"]
KEYS = (("color", 3), ("alpha", 1), ("background", 3), ("normal", 3))
GUARD = 64
ids = lambda cs: [c.name for c in cs]


@pytest.fixture(scope="module")
def still(ctx):
    """the module's context with a world that has no animated hitable uploaded: Pp = P"""
    wd, _, _ = scenes.scene("s0", (16, 8))
    assert not any(a for a, _ in T.world_hitables(wd))
    ctx.upload_world(wd)
    return ctx


def _policy(ctx, fma, body):
    ctx.set_fma_policy(fma)
    try:
        body()
    finally:
        ctx.set_fma_policy(0)


def _params(c, ts=0.0):
    import rayn_amd as R
    return R.frame_params(c.w, c.h, 1, 1, time_range=(float(ts), float(ts) + 0.05))


def _same_accumulate(got, want, what):
    IO.assert_bits_equal(got[0], want[0], (what, "colour"))
    TC.assert_history_equal(got[1], want[1], what)
    if len(want) > 2 and want[2] is not None:
        IO.assert_bits_equal(got[2], want[2], (what, "moments"))


def _outcome_holds(c, out, hist, what):
    """the case's hand-written n' and blended, on the device's output"""
    n1 = np.ascontiguousarray(hist[0][:, 3])
    bad = ~(np.isnan(c.n1) | (n1.view(np.uint32) == c.n1.view(np.uint32)))
    assert not bad.any(), (c.name, what, "n'", np.nonzero(bad)[0][:8], n1[bad][:8], c.n1[bad][:8])
    blended = (np.ascontiguousarray(out, f32).view(np.uint32) != c.color.view(np.uint32)).any(axis=1)
    bad = (c.blended != RC.UNKNOWN) & (blended != (c.blended == 1))
    assert not bad.any(), (c.name, what, "blended", np.nonzero(bad)[0][:8])


# ---- k_temporal_accumulate -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", ACC, ids=ids(ACC))
def test_temporal_accumulate_plain_and_with_moments(still, c):
    import rayn_amd as R
    tp = R.Temporal(*c.tp)
    want = RC.run_accumulate(c)
    got = TC.gpu_accumulate(still, _params(c), tp, c.color, c.normal, c.rec, c.obj, c.prev, None, c.prev_cam, 0.0, moments=False)
    _same_accumulate(got, want, (c.name, "plain"))
    if c.entry != "resample":
        _outcome_holds(c, got[0], got[1], "plain")
    want = RC.run_resample(c, 0, moments=True)
    got = TC.gpu_accumulate(still, _params(c), tp, c.color, c.normal, c.rec, c.obj, c.prev, c.mom, c.prev_cam, 0.0, moments=True)
    _same_accumulate(got, want, (c.name, "moments"))
    if hasattr(c, "moments_overflow"):  # the colour blended, y * y overflowed: (y, y2) is stored
        p = c.moments_overflow
        assert got[1][0][p, 3] == 3 and got[2][p, 0] > 1e38 and np.isposinf(got[2][p, 1])


def _resample_entry(ctx, c, resample, moments):
    """rayn_hip_temporal_accumulate_resample_device on the case's host arrays, with temporal_cases' guard and input checks"""
    import rayn_amd as R
    from rayn_amd import _abi
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    p, tp = _params(c), R.Temporal(*c.tp)
    t_abi, rp = tp.to_abi(), _abi.TemporalResampleParams(resample)

    def call(film, g, d_prev, d_new, d_out, d_pm, d_nm):
        rc = ctx._L.rayn_hip_temporal_accumulate_resample_device(
            ctx.h, C.byref(p), C.byref(t_abi), C.byref(rp), C.byref(c.prev_cam), 0.0, vp(film["color"]), vp(film["normal"]), vp(g["records"]), vp(g["object"]),
            vp(d_prev), vp(d_new), d_new.numel(), vp(d_pm), vp(d_nm), 0 if d_nm is None else d_nm.numel(), vp(d_out), None)
        assert rc == 0, ctx.last_error()

    return TC.gpu_accumulate(ctx, p, tp, c.color, c.normal, c.rec, c.obj, c.prev, c.mom, c.prev_cam, 0.0, moments, call)


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("c", ACC, ids=ids(ACC))
def test_resample_entry_bilinear_and_catmull_rom(still, c, fma):
    def body():
        for resample in (0, 1):
            for moments in (False, True):
                want = RC.run_resample(c, resample, moments)
                got = _resample_entry(still, c, resample, moments)
                _same_accumulate(got, want[:3], (c.name, resample, moments, fma))
                if resample == 0 and c.entry != "resample":
                    _outcome_holds(c, got[0], got[1], (resample, moments))
                if resample == 1 and c.entry == "resample":
                    # the kernel writes no arm: the one written on the case holds on the restatement (tests/test_reproject_cases.py), and
                    # the bit equality above carries it to the device - a cubic pixel's colour is not the bilinear arm's
                    _outcome_holds(c, got[0], got[1], (resample, moments))
    _policy(still, fma, body)


# ---- k_temporal_upscale --------------------------------------------------------------------------------------------------------------------

def _gpu_temporal_upscale(ctx, c, factor, sigmas, tp, confidence, film, low_g, high_g, prev, prev_cam):
    """Context.temporal_upscale without a low camera on host arrays: (planes, weight, (A, B, N, O)); guards behind every output, inputs
    and the previous history left alone"""
    import torch
    import rayn_amd as R
    from rayn_amd import film as F
    N = c.w * c.h * factor * factor
    d_film = IO.upload_film(film, [k for k, _ in KEYS])
    gl, gh = IO.upload_gbuffer(*low_g), IO.upload_gbuffer(*high_g)
    full = {k: IO.guarded(n * N, torch.float32, 7.0, GUARD) for k, n in KEYS if k in film}
    d_out = {k: v[1] for k, v in full.items()}
    full_wt, d_wt = IO.guarded(N, torch.float32, 7.0, GUARD)
    nb = F.temporal_history_bytes(c.w * factor, c.h * factor)
    d_prev = IO.upload_bytes(T.join_history(*prev))
    keep = IO.snapshot([d_prev])
    full_new, d_new = IO.guarded(nb, torch.uint8, 0xA5, GUARD)
    ctx.temporal_upscale(_params(c), R.Upscale(factor, *sigmas), R.Temporal(*tp), R.Supersample(jitter=False, confidence=confidence), d_film, gl, gh,
                         d_prev, prev_cam, 0.0, d_new, d_out, None, d_wt)
    torch.cuda.synchronize()
    for k, n in KEYS:
        if k in film:
            IO.assert_guards(full[k][0], n * N, 7.0, k)
    IO.assert_guards(full_wt, N, 7.0, "weight")
    IO.assert_guards(full_new, nb, 0xA5, "new history")
    IO.assert_unchanged([d_prev], keep, "the previous history")
    for k in d_film:
        IO.assert_is_host(d_film[k], film[k], k)
    IO.assert_gbuffer_is_host(gl, *low_g, "low G-buffer")
    IO.assert_gbuffer_is_host(gh, *high_g, "high G-buffer")
    out = {k: d_out[k].cpu().numpy().reshape((N, n) if n == 3 else (N,)) for k, n in KEYS if k in film}
    return out, d_wt.cpu().numpy(), T.split_history(d_new.cpu().numpy(), N)


def _same_upscaled(got, want, what):
    IO.assert_planes_equal(got[0], want[0], what)
    IO.assert_bits_equal(got[1], want[1], (what, "weight"))
    if len(got) > 2:
        TC.assert_history_equal(got[2], want[2], (what, "history"))


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("c", ACC, ids=ids(ACC))
def test_temporal_upscale_at_factor_1_is_the_accumulate(still, c, fma):
    """no low camera, confidence off: the restatement of the supersampling, and through it temporal_np.accumulate's colour and history"""
    def body():
        want = RC.run_temporal_upscale_1(c)
        acc = RC.run_accumulate(c)
        got = _gpu_temporal_upscale(still, c, 1, (0.0, 0.0), c.tp, False, {"color": c.color, "normal": c.normal}, (c.rec, c.obj), (c.rec, c.obj), c.prev, c.prev_cam)
        _same_upscaled(got, want, (c.name, fma))
        _same_accumulate((got[0]["color"], got[2]), acc, (c.name, fma, "the accumulate"))
        if c.entry != "resample":
            _outcome_holds(c, got[0]["color"], got[2], "factor 1")
    _policy(still, fma, body)


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("c", UPSCALE, ids=ids(UPSCALE))
def test_temporal_upscale_on_the_upscale_families(still, c, fma):
    """the tiers under a history (length 2, max_history 8), confidence off and on: n' = nh + conf shows which tier's b the kernel took"""
    def body():
        prev, cam = RC.upscale_history(c)
        for confidence in (False, True):
            want = RC.run_temporal_upscale(c, confidence)
            got = _gpu_temporal_upscale(still, c, c.factor, c.sigmas, (8, 0.25, -1.0), confidence, c.film, c.low_g, c.high_g, prev, cam)
            _same_upscaled(got, want, (c.name, confidence, fma))
            if confidence and hasattr(c, "conf"):
                assert (got[2][0][c.test, 3] == f32(2.0) + f32(c.conf)).all()
    _policy(still, fma, body)


# ---- k_upscale -----------------------------------------------------------------------------------------------------------------------------

def _gpu_upscale(ctx, c):
    """Context.upscale on the case's host arrays: (planes, weight); guards behind every output, inputs left alone"""
    import torch
    import rayn_amd as R
    N = c.w * c.h * c.factor * c.factor
    d_film = IO.upload_film(c.film, [k for k, _ in KEYS])
    gl, gh = IO.upload_gbuffer(*c.low_g), IO.upload_gbuffer(*c.high_g)
    full = {k: IO.guarded(n * N, torch.float32, 7.0, GUARD) for k, n in KEYS}
    d_out = {k: v[1] for k, v in full.items()}
    full_wt, d_wt = IO.guarded(N, torch.float32, 7.0, GUARD)
    ctx.upscale(_params(c), R.Upscale(c.factor, *c.sigmas), d_film, gl, gh, d_out, d_wt)
    torch.cuda.synchronize()
    for k, n in KEYS:
        IO.assert_guards(full[k][0], n * N, 7.0, k)
        IO.assert_is_host(d_film[k], c.film[k], k)
    IO.assert_guards(full_wt, N, 7.0, "weight")
    IO.assert_gbuffer_is_host(gl, *c.low_g, "low G-buffer")
    IO.assert_gbuffer_is_host(gh, *c.high_g, "high G-buffer")
    return {k: d_out[k].cpu().numpy().reshape((N, n) if n == 3 else (N,)) for k, n in KEYS}, d_wt.cpu().numpy()


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("c", UPSCALE, ids=ids(UPSCALE))
def test_upscale_tiers(still, c, fma):
    def body():
        want = RC.run_upscale(c)
        got = _gpu_upscale(still, c)
        _same_upscaled(got, want, (c.name, fma))
        # the tier as written, read off the device's own output: tier 1 has a weight > 0, tier 3 is the low pixel verbatim
        planes, weight = got
        t1 = c.test & (c.tier == 1)
        assert (weight[t1] > 0).all() and (weight[c.test & (c.tier != 1)] == 0).all()
        if getattr(c, "denormal", False):
            assert (weight < np.finfo(f32).tiny).all()
        t3 = np.nonzero(c.test & (c.tier == 3))[0]
        if t3.size:
            W = c.w * c.factor
            low = (t3 % W) // c.factor + (t3 // W) // c.factor * c.w
            assert IO.same_bits(planes["alpha"][t3], np.asarray(c.film["alpha"], f32)[low])
    _policy(still, fma, body)


# ---- k_interpolate -------------------------------------------------------------------------------------------------------------------------

def _gpu_interpolate(ctx, c):
    """Context.interpolate on the case's host arrays -> ({plane: (n, k)}, source); guards behind every output, inputs left alone"""
    import torch
    import rayn_amd as R
    n = c.w * c.h
    dev = [(IO.upload_film(k.film), IO.upload_gbuffer(k.rec, k.obj)) for k in (c.ka, c.kb)]
    g = IO.upload_gbuffer(c.rec, c.obj)
    ins = [t for f, gk in dev + [({}, g)] for t in (*f.values(), *gk.values())]
    keep = IO.snapshot(ins)
    full = {k: IO.guarded(k_n * n, torch.float32, 7.0, GUARD) for k, k_n in KEYS}
    d_out = {k: full[k][1] for k in dev[0][0]}
    full_src, d_src = IO.guarded(n, torch.int32, -3, GUARD)
    ctx.interpolate(_params(c, c.ts), R.Interpolate(2, c.tol), (dev[0][0], dev[0][1], c.ka.camera, c.ka.time), (dev[1][0], dev[1][1], c.kb.camera, c.kb.time),
                    g, d_out, d_src)
    torch.cuda.synchronize()
    for k, k_n in KEYS:
        IO.assert_guards(full[k][0], k_n * n, 7.0, k)
    IO.assert_guards(full_src, n, -3, "d_out_source")
    IO.assert_unchanged(ins, keep, "a key or the G-buffer")
    return {k: d_out[k].cpu().numpy().reshape(n, dict(KEYS)[k]) for k in d_out}, d_src.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("c", INTERP, ids=ids(INTERP))
def test_interpolate_sources(still, c, fma):
    def body():
        want = RC.run_interpolate(c)
        planes, source = _gpu_interpolate(still, c)
        assert np.array_equal(source, c.source), (c.name, np.nonzero(source != c.source)[0][:8], source[source != c.source][:8])
        assert np.array_equal(source, want[1])
        IO.assert_planes_equal(planes, want[0], (c.name, fma))
    _policy(still, fma, body)
