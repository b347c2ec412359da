"""rayn_hip_temporal_accumulate_moments_device (rayn_amd/csrc/temporal.hip) and rayn_hip_denoise_temporal_variance_device
(rayn_amd/csrc/denoise_temporal.hip) on the GPU: the moments entry writes the colour and history of the plain entry bit for bit; moments,
variance estimate and passes equal the numpy restatement (tests/temporal_variance_np.py) bit for bit on adversarial synthetic inputs
and on a rendered sequence; Film.render_sequence(temporal=, denoise=VarianceDenoise()) writes the bytes of the plain loop of the entries;
input hygiene and error texts; rayn_hip_denoise_variance_device keeps its bits; and the benefit on the shipped scene."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import denoise_variance_np as VN
import device_io as IO
import scenes
import temporal_cases as TC
import temporal_np as T
import temporal_variance_np as TV
from common import bits_equal
from device_io import module_context as ctx, same_bits  # noqa: F401
from temporal_cases import GUARD, SPECIAL

pytestmark = pytest.mark.gpu

f32 = np.float32
W0, H0 = 37, 23  # no multiple of 16: edge blocks, and 7x7 windows that cross block and image borders
SIGMAS = list(itertools.product((0.0, 4.0), (0.0, 0.4), (0.0, 0.3)))  # every on/off combination of luminance / normal / alpha


def _adversarial_accumulate_inputs(w, h, seed, cam_kind):
    """test_temporal_device's adversarial frame + history, and previous moments with the same special values scattered over them"""
    cur, prev_cam, color, normal, rec, obj, prev = TC.random_inputs(w, h, seed, cam_kind, True)
    rng = np.random.default_rng(seed + 500)
    pm = np.stack([rng.gamma(0.6, 0.5, w * h), rng.gamma(0.6, 0.8, w * h)], axis=1).astype(f32)
    flat = pm.reshape(-1)
    idx = rng.choice(flat.size, min(flat.size, 4 * SPECIAL.size), replace=False)
    flat[idx] = np.resize(SPECIAL, idx.size)
    color[rng.choice(w * h, min(w * h, 6), replace=False)] = (3.0e38, 3.0e38, 3.0e38)  # a finite colour whose luminance overflows
    return prev_cam, color, normal, rec, obj, prev, pm


# ---- 1. the moments entry is a superset of the plain one ---------------------------------------------------------------------------------

@pytest.mark.parametrize("cam_kind", [0, 2])
def test_moments_entry_writes_the_colour_and_history_of_the_plain_entry(ctx, cam_kind):
    import rayn_amd as R
    wd, _, _ = scenes.scene("s1", (40, 24), moving=True)
    ctx.upload_world(wd)
    for si, (w, h) in enumerate([(W0, H0), (48, 32), (1, 1)]):
        prev_cam, color, normal, rec, obj, prev, pm = _adversarial_accumulate_inputs(w, h, 20 + si, cam_kind)
        p = R.frame_params(w, h, 1, 1, time_range=(0.75, 0.8))
        for tp in (R.Temporal(4, 0.05, -1.0), R.Temporal(1, 0.05, 0.9), R.Temporal(65536, 1e30, 0.5)):
            out_p, hist_p, _ = TC.gpu_accumulate(ctx, p, tp, color, normal, rec, obj, prev, pm, prev_cam, 0.25, moments=False)
            out_m, hist_m, mom = TC.gpu_accumulate(ctx, p, tp, color, normal, rec, obj, prev, pm, prev_cam, 0.25)
            assert same_bits(out_p, out_m), (w, h, tp, "colour")
            for name, a, b in zip("ABNO", hist_p, hist_m):
                assert same_bits(a, b), (w, h, tp, name)
        out_p, hist_p, _ = TC.gpu_accumulate(ctx, p, tp, color, normal, rec, obj, None, None, None, 0.0, moments=False)
        out_m, hist_m, mom = TC.gpu_accumulate(ctx, p, tp, color, normal, rec, obj, None, None, None, 0.0)
        assert same_bits(out_p, out_m) and all(same_bits(a, b) for a, b in zip(hist_p, hist_m))


# ---- 2. the kernels against the restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cam_kind", [0, 1, 2])
def test_moments_match_the_restatement_on_adversarial_inputs(ctx, cam_kind):
    """NaN / inf / 3e38 colours, histories and moments, misses, taps rejected by depth, object and normal, history lengths 0 .. 8 with a
    fractional one, cameras that have moved so that taps straddle every border; max_history 1, 4 and a large one."""
    import rayn_amd as R
    wd, _, _ = scenes.scene("s1", (40, 24), moving=True)
    ctx.upload_world(wd)
    hit = T.world_hitables(wd)
    w, h = W0, H0
    prev_cam, color, normal, rec, obj, prev, pm = _adversarial_accumulate_inputs(w, h, 30 + cam_kind, cam_kind)
    p = R.frame_params(w, h, 1, 1, time_range=(0.75, 0.8))
    for tp in (R.Temporal(4, 0.05, -1.0), R.Temporal(1, 0.25, 0.9), R.Temporal(8, 1e30, 0.5), R.Temporal(65536, 0.25, -1.0)):
        want = TV.accumulate(w, h, color, normal, rec, obj, prev, pm, prev_cam, 0.25, 0.75, hit, tp.max_history, tp.depth_tolerance, tp.normal_min)
        got = TC.gpu_accumulate(ctx, p, tp, color, normal, rec, obj, prev, pm, prev_cam, 0.25)
        assert bits_equal(got[0], want[0]), (tp, "colour")
        assert all(bits_equal(a, b) for a, b in zip(got[1][:3], want[1][:3])) and np.array_equal(got[1][3], want[1][3]), (tp, "history")
        assert bits_equal(got[2], want[2]), (tp, "moments", int((got[2].view(np.uint32) != want[2].view(np.uint32)).sum()))
        n1 = want[1][0][:, 3]
        assert (n1 > 1).any() or tp.max_history == 1
    want = TV.accumulate(w, h, color, normal, rec, obj, None, None, None, 0.0, 0.75, hit, 4, 0.05, -1.0)
    got = TC.gpu_accumulate(ctx, p, R.Temporal(), color, normal, rec, obj, None, None, None, 0.0)
    assert bits_equal(got[0], want[0]) and bits_equal(got[2], want[2])
    assert np.all(got[2][~np.isfinite(color).all(axis=1)] == 0.0)


def _denoise(ctx, w, h, inp, L, sigmas, variance=True):
    """The entry through Context.denoise_temporal_variance; a guide whose sigma is 0 is passed as a null pointer."""
    import torch
    from rayn_amd import VarianceDenoise
    n = w * h
    d = IO.upload_film(inp, ("color",) + (("normal",) if sigmas[1] else ()) + (("alpha",) if sigmas[2] else ()))
    g = {"object": IO.upload(inp["obj"].view(np.int32), np.int32)}
    d_hist, d_mom = IO.upload_bytes(inp["hist"]), IO.upload_bytes(inp["mom"])
    ins = dict(d, object=g["object"], hist=d_hist, mom=d_mom)
    keep = IO.snapshot(ins)
    full_out, out = IO.guarded(3 * n, torch.float32, 7.0, GUARD)
    full_var, var = IO.guarded(n, torch.float32, 7.0, GUARD)
    ctx.denoise_temporal_variance(w, h, d, g, d_hist, d_mom, out, VarianceDenoise(L, *sigmas), var if variance else None)
    torch.cuda.synchronize()
    IO.assert_guards(full_out, 3 * n, 7.0, "colour")
    IO.assert_guards(full_var, n if variance else 0, 7.0, "variance")
    IO.assert_unchanged(ins, keep, "an input")
    return out.cpu().numpy().reshape(n, 3), var.cpu().numpy() if variance else None


def test_variance_estimate_and_passes_match_the_restatement(ctx, oracle):
    """All eight term combinations at 1 and 3 passes, with and without the variance output, at 37x23 and at 1x1."""
    w, h = W0, H0
    inp = TC.pack_inputs(w, h, 7)
    v0, k = TV.initial_variance(w, h, inp["color"], inp["obj"], inp["n1"], inp["mom"])
    n1, guided = inp["n1"], ~np.isnan(v0)
    # the case has substance: both arms, windows cut by objects and borders, pixels that are not guided for each reason
    assert (guided & (n1 >= 4)).sum() > 50 and (guided & (n1 < 4)).sum() > 50 and (~guided).sum() > 50
    assert len(np.unique(k[guided & (n1 < 4)])) > 10 and (v0[guided & (n1 >= 4)] == 0).any()
    for L, sigmas in itertools.product((1, 3), SIGMAS):
        want_c, want_v = TV.denoise(w, h, inp["color"], inp["alpha"], inp["normal"], inp["obj"], inp["n1"], inp["mom"], L, *sigmas)
        got_c, got_v = _denoise(ctx, w, h, inp, L, sigmas)
        assert bits_equal(got_c, want_c), (L, sigmas, "colour", int((got_c.view(np.uint32) != want_c.view(np.uint32)).sum()))
        assert bits_equal(got_v, want_v) and np.array_equal(np.isnan(got_v), np.isnan(want_v)), (L, sigmas, "variance")
        got_c2, none = _denoise(ctx, w, h, inp, L, sigmas, variance=False)
        assert none is None and same_bits(got_c2, got_c), (L, sigmas, "without the variance output")
    one = TC.pack_inputs(1, 1, 3)
    one["color"][:], one["normal"][:], one["alpha"][:], one["obj"][:], one["mom"][:] = (0.5, 0.25, 0.75), (0.0, 0.6, 0.8), 1.0, 1, (0.5, 0.3)
    for n_hist in (1.0, 4.0):
        one["n1"][:] = n_hist
        one["hist"] = T.join_history(np.array([[0.0, 0.0, 0.0, n_hist]], f32), np.zeros((1, 4), f32), np.zeros((1, 4), f32), one["obj"])
        want_c, want_v = TV.denoise(1, 1, one["color"], one["alpha"], one["normal"], one["obj"], one["n1"], one["mom"], 2, 4.0, 0.4, 0.3)
        got_c, got_v = _denoise(ctx, 1, 1, one, 2, (4.0, 0.4, 0.3))
        assert bits_equal(got_c, want_c) and bits_equal(got_v, want_v) and np.isfinite(want_v).all()


# ---- 3. a rendered sequence ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fma", [0, 1])
def test_render_sequence_is_the_plain_loop_of_the_entries_and_the_restatement(tmp_path, oracle, fma):
    """48x32, samples=1, 5 frames of the moving-camera scene, so that n' reaches 4 and both estimates run: render_sequence(temporal=,
    denoise=VarianceDenoise()) writes the bytes of a loop over render_device, gbuffer, temporal_accumulate (moments) and
    denoise_temporal_variance, and every frame's kernel outputs equal the restatement's bit for bit.  Under both mul_add policies: the
    G-buffer pass depends on the policy, the accumulate and the filter do not."""
    import torch
    import rayn_amd as R
    from rayn_amd import film as F
    from rayn_amd import image
    from rayn_amd import setup as S
    K = R.ChannelKind
    w, h, frames, samples, bounces = 48, 32, [1, 2, 3, 4, 5], 1, 2
    world, cam = scenes.moving_scene(w, h)
    integ = R.PathTracingIntegrator(max_bounces=bounces, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE)
    filt = R.BlackmanHarrisFilter(S.FILTER_RADIUS)
    tp, dn = R.Temporal(), R.VarianceDenoise(2, 4.0, 0.4, 0.3)
    film = R.Film([K.Color, K.Alpha, K.Background, K.WorldNormal], (w, h))
    ctx = film.ctx
    ctx.set_fma_policy(fma)
    film.render_sequence(world, cam, integ, filt, S.TILE_SIZE, frames, 24, 1.0 / 24.0, samples, [K.Color, K.Alpha], str(tmp_path / "seq"), "a",
                         denoise=dn, temporal=tp)
    got = IO.read_folder(tmp_path / "seq")
    assert sorted(got) == sorted(f"a_{f:04d}_{s}.png" for f in frames for s in ("color_temporal_denoised", "alpha"))
    desc = world.to_desc(cam)
    ctx.upload_world(desc)
    hit = T.world_hitables(desc)
    n = w * h
    hist = [torch.empty(F.temporal_history_bytes(w, h), dtype=torch.uint8, device="cuda") for _ in range(2)]
    mom = [torch.empty(F.temporal_moments_bytes(w, h), dtype=torch.uint8, device="cuda") for _ in range(2)]
    g, acc, shown = F.alloc_gbuffer(w, h, "cuda"), torch.empty(n, 3, dtype=torch.float32, device="cuda"), torch.empty(n, 3, dtype=torch.float32, device="cuda")
    var = torch.empty(n, dtype=torch.float32, device="cuda")
    img = torch.empty(n * 3, dtype=torch.uint8, device="cuda")
    prev_start, prev_host, arms = None, (None, None), set()
    for i, frame in enumerate(frames):
        p, out = IO.render_sequence_frame(ctx, w, h, frame, samples, bounces, filt)
        ctx.gbuffer(p, g)
        first = i == 0
        ctx.temporal_accumulate(p, tp, out, g, None if first else hist[(i + 1) % 2], None if first else desc.camera, 0.0 if first else prev_start,
                                hist[i % 2], acc, None, None if first else mom[(i + 1) % 2], mom[i % 2])
        ctx.denoise_temporal_variance(w, h, dict(out, color=acc), g, hist[i % 2], mom[i % 2], shown, dn, var)
        ctx.save_to_pixels(K.Color, film.have_mask(), False, w, h, dict(out, color=shown), img)
        image.save(str(tmp_path / "one.png"), img.cpu().numpy().reshape(h, w, 3))
        assert open(tmp_path / "one.png", "rb").read() == got[f"a_{frame:04d}_color_temporal_denoised.png"], frame
        # the restatement on the same film and G-buffer, fed the kernels' previous history and moments
        color, normal, alpha = out["color"].cpu().numpy(), out["normal"].cpu().numpy(), out["alpha"].cpu().numpy()
        rec, obj = g["records"].cpu().numpy().reshape(n, 4), g["object"].cpu().numpy().view(np.uint32)
        w_out, w_hist, w_mom = TV.accumulate(w, h, color, normal, rec, obj, prev_host[0], prev_host[1], desc.camera, 0.0 if first else prev_start, p.time_start,
                                             hit, tp.max_history, tp.depth_tolerance, tp.normal_min)
        g_hist, g_mom = T.split_history(hist[i % 2].cpu().numpy(), n), mom[i % 2].cpu().numpy().view(f32).reshape(n, 2)
        assert bits_equal(acc.cpu().numpy(), w_out) and bits_equal(g_hist[0], w_hist[0]) and bits_equal(g_mom, w_mom), frame
        w_c, w_v = TV.denoise(w, h, w_out, alpha, normal, obj, w_hist[0][:, 3], w_mom, dn.iterations, dn.sigma_luminance, dn.sigma_normal, dn.sigma_alpha)
        assert bits_equal(shown.cpu().numpy(), w_c) and bits_equal(var.cpu().numpy(), w_v), frame
        n1 = w_hist[0][:, 3]
        arms |= {"spatial"} if ((n1 >= 1) & (n1 < 4) & ~np.isnan(w_v)).any() else set()
        arms |= {"temporal"} if ((n1 >= 4) & ~np.isnan(w_v)).any() else set()
        prev_start, prev_host = p.time_start, (g_hist, g_mom)
    assert arms == {"spatial", "temporal"} and n1.max() == 4.0
    # Alpha's files are those of the plain sequence, and the film needs its Alpha channel for the alpha term
    if fma == 0:
        plain = R.Film([K.Color, K.Alpha, K.Background, K.WorldNormal], (w, h))
        plain.render_sequence(world, cam, integ, filt, S.TILE_SIZE, frames[:2], 24, 1.0 / 24.0, samples, [K.Color, K.Alpha], str(tmp_path / "plain"), "a", temporal=tp)
        base = IO.read_folder(tmp_path / "plain")
        assert all(got[f"a_{f:04d}_alpha.png"] == base[f"a_{f:04d}_alpha.png"] for f in frames[:2])
        assert got["a_0002_color_temporal_denoised.png"] != base["a_0002_color_temporal.png"]
        no_alpha = R.Film([K.Color, K.Background, K.WorldNormal], (w, h))
        with pytest.raises(ValueError, match="Alpha channel"):
            no_alpha.render_sequence(world, cam, integ, filt, S.TILE_SIZE, frames, 24, 1.0 / 24.0, samples, [K.Color], str(tmp_path / "x"), "a", denoise=dn, temporal=tp)
        with pytest.raises(ValueError, match="progressive render"):
            plain.render_sequence(world, cam, integ, filt, S.TILE_SIZE, frames, 24, 1.0 / 24.0, samples, [K.Color], str(tmp_path / "x"), "a", denoise=dn)
        assert not os.path.exists(tmp_path / "x")
        no_alpha.render_sequence(world, cam, integ, filt, S.TILE_SIZE, frames[:1], 24, 1.0 / 24.0, samples, [K.Color], str(tmp_path / "y"), "a",
                                 denoise=R.VarianceDenoise(1, 4.0, 0.4, 0.0), temporal=tp)
        assert sorted(IO.read_folder(tmp_path / "y")) == ["a_0001_color_temporal_denoised.png"]


# ---- 4. input hygiene ------------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_invalid_arg_with_a_text_and_leave_the_outputs_untouched(ctx):
    import torch
    import rayn_amd as R
    from rayn_amd import film as F
    L = ctx._L
    w, h, n = 40, 24, 40 * 24
    wd, _, _ = scenes.scene("s0", (w, h))
    ctx.upload_world(wd)
    p = R.frame_params(w, h, 1, 1)
    zero, huge = R.frame_params(0, h, 1, 1), R.frame_params(65536, 32768, 1, 1)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    hb, mb, sb = F.temporal_history_bytes(w, h), F.temporal_moments_bytes(w, h), F.denoise_variance_scratch_bytes(w, h)
    # every buffer in a slot of its own in one arena, each slot larger than any buffer: a deliberately misplaced pointer overlaps only
    # what the case names
    SLOT = 1 << 16
    assert max(hb + 16, sb + 16, 16 * n + 16) <= SLOT
    arena = torch.zeros(12 * SLOT, dtype=torch.uint8, device="cuda")
    slot = lambda i, nbytes: arena[i * SLOT: i * SLOT + nbytes]
    fl = lambda i, k: slot(i, 4 * k).view(torch.float32)
    color, normal, alpha, rec, obj = fl(0, 3 * n), fl(1, 3 * n), fl(2, n), fl(3, 4 * n + 4), slot(4, 4 * n).view(torch.int32)
    obj.fill_(1)
    h0, h1, m0, m1, scratch = slot(5, hb + 16), slot(6, hb + 16), slot(7, mb + 16), slot(8, mb + 16), slot(9, sb + 16)
    h1.fill_(0x5A)
    m1.fill_(0x5A)
    out, var = fl(10, 3 * n), fl(11, n)
    out.fill_(7.0)
    var.fill_(7.0)
    cam = wd.camera

    def untouched():
        torch.cuda.synchronize()
        return bool(torch.all(out == 7.0) and torch.all(var == 7.0) and torch.all(h1 == 0x5A) and torch.all(m1 == 0x5A))

    def acc(p=p, tp=R.Temporal().to_abi(), cam=cam, color=vp(color), rec=vp(rec), prev=vp(h0), new=vp(h1), hb=hb, pm=vp(m0), nm=vp(m1), mb=mb, out=vp(out)):
        rc = L.rayn_hip_temporal_accumulate_moments_device(ctx.h, None if p is None else C.byref(p), None if tp is None else C.byref(tp),
                                                           None if cam is None else C.byref(cam), 0.0, color, vp(normal), rec, vp(obj), prev, new, hb, pm, nm, mb,
                                                           out, None)
        return rc, ctx.last_error()

    for kw, text in ((dict(p=None), "null frame params"), (dict(p=zero), "zero-sized"), (dict(p=huge), "2^31"), (dict(tp=None), "null temporal params"),
                     (dict(color=None), "null buffer"), (dict(new=None), "null buffer"), (dict(nm=None), "null buffer"), (dict(out=None), "null buffer"),
                     (dict(cam=None), "previous camera"), (dict(hb=hb - 1), "history smaller"), (dict(mb=mb - 1), "moments smaller"), (dict(mb=0), "moments smaller"),
                     (dict(prev=None, cam=None), "previous moments without a previous history"), (dict(pm=None), "needs the previous moments"),
                     (dict(nm=vp(m1, 8)), "moments not 16-byte aligned"), (dict(pm=vp(m0, 4)), "moments not 16-byte aligned"),
                     (dict(new=vp(h1, 4)), "history not 16-byte aligned"), (dict(rec=vp(rec, 4)), "16-byte aligned"),
                     (dict(nm=vp(m0)), "alias the previous"), (dict(nm=vp(m0, 16)), "alias the previous"), (dict(new=vp(h0)), "alias the previous"),
                     (dict(nm=vp(color)), "alias an input"), (dict(nm=vp(rec)), "alias an input"), (dict(nm=vp(h0)), "alias an input"),
                     (dict(out=vp(m0)), "alias an input"), (dict(new=vp(m0), hb=0), "history smaller"), (dict(out=vp(color)), "alias an input"),
                     (dict(nm=vp(h1)), "alias another output"), (dict(nm=vp(out), mb=0), "moments smaller"), (dict(out=vp(m1)), "alias another output")):
        rc, err = acc(**kw)
        assert rc == -1 and text in err, (kw, rc, err)
        assert untouched(), kw
    fresh = R.Context(0)
    try:
        rc = L.rayn_hip_temporal_accumulate_moments_device(fresh.h, C.byref(p), C.byref(R.Temporal().to_abi()), None, 0.0, vp(color), vp(normal), vp(rec), vp(obj), None,
                                                           vp(h1), hb, None, vp(m1), mb, vp(out), None)
        assert (rc, fresh.last_error()) == (-1, "rayn_hip_upload_world has not been called")
    finally:
        fresh.close()
    assert untouched()

    def dn(w=w, h=h, L_=2, sl=4.0, sn=0.4, sa=0.3, color=vp(color), alpha=vp(alpha), normal=vp(normal), obj=vp(obj), hist=vp(h0), hb=hb, mom=vp(m0), mb=mb,
           out=vp(out), var=vp(var), scratch=vp(scratch), sb=sb):
        rc = L.rayn_hip_denoise_temporal_variance_device(ctx.h, w, h, L_, sl, sn, sa, color, alpha, normal, obj, hist, hb, mom, mb, out, var, scratch, sb, None)
        return rc, ctx.last_error()

    nan, inf = float("nan"), float("inf")
    for kw, text in ((dict(w=0), "zero-sized"), (dict(w=65536, h=32768), "2^31"), (dict(L_=0), "iterations"), (dict(L_=9), "iterations"),
                     (dict(sl=-1.0), "sigma_luminance"), (dict(sl=nan), "sigma_luminance"), (dict(sl=2.0 ** 31), "sigma_luminance"), (dict(sn=inf), "sigma_normal"),
                     (dict(sn=2.0 ** -31), "sigma_normal"), (dict(sa=-0.3), "sigma_alpha"), (dict(color=None), "null buffer"), (dict(obj=None), "null buffer"),
                     (dict(hist=None), "null buffer"), (dict(mom=None), "null buffer"), (dict(out=None), "null buffer"), (dict(scratch=None), "null buffer"),
                     (dict(normal=None), "null normal guide"), (dict(alpha=None), "null alpha guide"), (dict(hb=hb - 1), "history smaller"),
                     (dict(mb=mb - 1), "moments smaller"), (dict(sb=sb - 1), "scratch smaller"), (dict(scratch=vp(scratch, 4)), "scratch not 16-byte aligned"),
                     (dict(hist=vp(h0, 8)), "history not 16-byte aligned"), (dict(mom=vp(m0, 8)), "moments not 16-byte aligned"),
                     (dict(obj=vp(obj, 2)), "4-byte aligned"), (dict(out=vp(color)), "alias an input"), (dict(out=vp(h0)), "alias an input"),
                     (dict(var=vp(m0)), "alias an input"), (dict(var=vp(alpha)), "alias an input"), (dict(var=vp(out)), "d_out_variance must not alias d_out_color"),
                     (dict(scratch=vp(h0), sb=hb), "scratch must not alias an input"), (dict(scratch=vp(color)), "scratch must not alias an input"),
                     (dict(out=vp(scratch)), "scratch must not alias an output"), (dict(var=vp(scratch, 64)), "scratch must not alias an output")):
        rc, err = dn(**kw)
        assert rc == -1 and text in err, (kw, rc, err)
        assert untouched(), kw
    # the valid calls, last: null guides with their sigma at 0, no variance output, no previous history
    assert dn()[0] == 0 and dn(normal=None, sn=0.0, alpha=None, sa=0.0, var=None)[0] == 0
    assert acc()[0] == 0 and acc(prev=None, cam=None, pm=None)[0] == 0
    torch.cuda.synchronize()
    assert not untouched()
    # the Python wrapper's own checks
    with pytest.raises(ValueError, match="d_new_moments"):
        ctx.temporal_accumulate(p, R.Temporal(), {"color": color, "normal": normal}, {"records": rec[: 4 * n], "object": obj}, None, None, 0.0, h1[:hb], out,
                                None, m0[:mb], None)
    with pytest.raises(ValueError, match="d_moments"):
        ctx.denoise_temporal_variance(w, h, {"color": color}, {"object": obj}, h0[:hb], None, out, R.VarianceDenoise(1, 4.0, 0.0, 0.0))


# ---- 5. the pass-loop refactor left rayn_hip_denoise_variance_device alone ---------------------------------------------------------------------

def test_the_progressive_variance_denoiser_keeps_its_bits(oracle):
    import rayn_amd as R
    from rayn_amd import setup as S
    K = R.ChannelKind
    w, h = 32, 32
    cam, world = S.SCENES["s3"]((w, h))
    film = R.Film([K.Color, K.Alpha, K.Background, K.WorldNormal], (w, h))
    film.render_progressive(world, cam, R.PathTracingIntegrator(max_bounces=3, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE), R.BlackmanHarrisFilter(1.5), (16, 16), 1, None, 1,
                            R.Progressive(min_epochs=2, max_epochs=2, adaptive=False))
    arrays, pr = film._progressive_arrays()
    assert set(arrays["epochs"].tolist()) == {2}
    for params in (R.VarianceDenoise(), R.VarianceDenoise(3, 4.0, 0.4, 0.3), R.VarianceDenoise(2, 2.0, 0.0, 0.0)):
        want_c, want_v = VN.denoise(film.channel(K.Color), film.channel(K.Alpha), film.channel(K.WorldNormal), arrays["m2"], arrays["epochs"], w, h, (16, 16),
                                    params.iterations, params.sigma_luminance, params.sigma_normal, params.sigma_alpha)
        assert bits_equal(film.denoised_color(params).cpu().numpy(), want_c), params
        assert bits_equal(film.denoised_variance(params).reshape(-1), want_v), params
        assert np.isfinite(want_v).all()


# ---- 6. does it do its job -----------------------------------------------------------------------------------------------------------------------

# MSE of the last frame relative to the raw last frame's, computed with the CPU oracle and the numpy restatements
# (tools/temporal_variance_defaults.py --recommended) - the path the tests above hold the GPU to bit for bit
MEASURED_TEMPORAL, MEASURED_RATIO = 0.4940, 0.4571
RECOMMENDED = (1, 4.0, 0.4, 0.3)


def test_the_recommended_setting_lowers_the_error_of_the_accumulated_sequence():
    """temporal_np.DefaultsCase (shipped scene, 160x96, moving camera, 8 frames of 8 spp, against samples=256): Temporal() followed by
    VarianceDenoise(1, 4.0, 0.4, 0.3) reaches the ratio measured on the CPU path (times 1.05, the project's margin for this kind of test:
    the GPU path is bit-identical to it), which is below Temporal() alone."""
    import rayn_amd as R
    raw, temporal, both = TC.defaults_case_errors(R.Temporal(), R.VarianceDenoise(*RECOMMENDED))
    print(f"MSE raw {raw:.4e}, temporal {temporal / raw:.4f}x (CPU path: {MEASURED_TEMPORAL}x), temporal + variance denoise {both / raw:.4f}x (CPU path: {MEASURED_RATIO}x)")
    assert both / raw < MEASURED_RATIO * 1.05, (raw, temporal, both)
    assert both < temporal
