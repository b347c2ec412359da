"""rayn_hip_denoise_temporal_variance_feedback_device (rayn_amd/csrc/denoise_temporal.hip, pass 0 of k_vatrous in denoise_variance.hip) on
the GPU: the history after the call equals the numpy restatement (tests/temporal_feedback_np.py) bit for bit on adversarial inputs, the
planar outputs are the existing entry's bits, a strength of 0 writes nothing; Film.render_sequence(temporal=Temporal(feedback=)) writes
the bytes of the plain loop of the entries and of the restatement driven by the oracle; bad arguments; and what the feedback does to the
error of the shipped sequence."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import device_io as IO
import scenes
import temporal_feedback_np as TF
import temporal_np as T
import temporal_variance_np as TV
from device_io import module_context as ctx, same_bits  # noqa: F401
from temporal_cases import GUARD, defaults_case_errors
from temporal_feedback_cases import H0, SIGMAS, W0, adversarial_inputs, restate

pytestmark = pytest.mark.gpu

f32 = np.float32
BETAS = (0.0, 0.5, 1.0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the kernels against the restatement ------------------------------------------------------------------------------------------------

def _call(ctx, w, h, d, g, hist_bytes, d_mom, L, sigmas, beta):
    """Context.denoise_temporal_variance with the history between guard bytes: (colour, variance, history bytes after the call)"""
    import torch
    from rayn_amd import VarianceDenoise
    n, hb = w * h, len(hist_bytes)
    arena = torch.full((hb + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    d_hist = arena[GUARD: GUARD + hb]
    d_hist.copy_(torch.from_numpy(hist_bytes))
    full_out, out = IO.guarded(3 * n, torch.float32, 7.0, GUARD)
    full_var, var = IO.guarded(n, torch.float32, 7.0, GUARD)
    ctx.denoise_temporal_variance(w, h, d, g, d_hist, d_mom, out, VarianceDenoise(L, *sigmas), var, feedback=beta)
    torch.cuda.synchronize()
    assert torch.all(arena[:GUARD] == 0xA5), "a kernel wrote in front of the history"
    IO.assert_guards(arena, GUARD + hb, 0xA5, "history")
    IO.assert_guards(full_out, 3 * n, 7.0, "colour")
    IO.assert_guards(full_var, n, 7.0, "variance")
    return out.cpu().numpy().reshape(n, 3), var.cpu().numpy(), d_hist.cpu().numpy()


def test_history_matches_the_restatement_and_the_outputs_are_the_existing_entrys(ctx, oracle):
    """37x29 (partial edge blocks), every on/off combination of the three terms, 1 and 3 passes, strengths 0, 0.5 and 1."""
    w, h = W0, H0
    n = w * h
    inp = adversarial_inputs(w, h, 11)
    hist_bytes = np.ascontiguousarray(inp["hist"])
    before = T.split_history(hist_bytes, n)
    d = {"color": IO.upload(inp["color"]), "normal": IO.upload(inp["normal"]), "alpha": IO.upload(inp["alpha"])}
    g = {"object": IO.upload(inp["obj"].view(np.int32), np.int32)}
    d_mom = IO.upload_bytes(inp["mom"])
    ins = dict(d, object=g["object"], mom=d_mom)
    keep = IO.snapshot(ins)
    for sigmas in SIGMAS:
        want = {beta: restate(w, h, inp, 1, sigmas, beta)[2] for beta in BETAS}  # the write-back is pass 0's: the same for every L
        changed = (_bits(want[1.0][0]) != _bits(before[0])).any(axis=1)
        assert changed.sum() > 200, sigmas
        for L in (1, 3):
            plain_c, plain_v, plain_h = _call(ctx, w, h, d, g, hist_bytes, d_mom, L, sigmas, 0.0)  # feedback == 0: the existing entry
            assert np.array_equal(plain_h, hist_bytes), (L, sigmas, "a strength of 0 changed the history")
            for beta in BETAS[1:]:
                got_c, got_v, got_h = _call(ctx, w, h, d, g, hist_bytes, d_mom, L, sigmas, beta)
                assert same_bits(got_c, plain_c) and same_bits(got_v, plain_v), (L, sigmas, beta, "outputs")
                for name, a, b in zip("ABNO", T.split_history(got_h, n), want[beta]):
                    assert same_bits(a, b), (L, sigmas, beta, name, int((_bits(a) != _bits(b)).sum()))
    IO.assert_unchanged(ins, keep, "an input")  # as bits: the inputs hold NaNs


def test_the_new_entry_with_a_strength_of_zero_writes_nothing(ctx):
    """Straight through the C entry (the Python wrapper routes 0 to the existing one): outputs of the existing entry, history untouched."""
    import torch
    from rayn_amd import film as F
    w, h = W0, H0
    n = w * h
    inp = adversarial_inputs(w, h, 12)
    vp = lambda t: C.c_void_p(t.data_ptr())
    color, normal, alpha, obj = IO.upload(inp["color"]), IO.upload(inp["normal"]), IO.upload(inp["alpha"]), IO.upload(inp["obj"].view(np.int32), np.int32)
    d_hist, d_mom = IO.upload_bytes(inp["hist"]), IO.upload_bytes(inp["mom"])
    scratch = torch.empty(F.denoise_variance_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
    res = []
    for entry, extra in ((ctx._L.rayn_hip_denoise_temporal_variance_device, ()), (ctx._L.rayn_hip_denoise_temporal_variance_feedback_device, (0.0,)),
                         (ctx._L.rayn_hip_denoise_temporal_variance_feedback_device, (-0.0,))):
        out, var = torch.full((3 * n,), 7.0, device="cuda"), torch.full((n,), 7.0, device="cuda")
        rc = entry(ctx.h, w, h, 2, 4.0, 0.4, 0.3, vp(color), vp(alpha), vp(normal), vp(obj), vp(d_hist), d_hist.numel(), vp(d_mom), d_mom.numel(), vp(out), vp(var),
                   vp(scratch), scratch.numel(), *extra, None)
        torch.cuda.synchronize()
        assert rc == 0, ctx.last_error()
        assert np.array_equal(d_hist.cpu().numpy(), inp["hist"])
        res.append((out.cpu().numpy(), var.cpu().numpy()))
    for c, v in res[1:]:
        assert same_bits(c, res[0][0]) and same_bits(v, res[0][1])


# ---- 2. a rendered sequence ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fma", [0, 1])
def test_render_sequence_with_feedback_is_the_plain_loop_of_the_entries_and_the_restatement(tmp_path, oracle, fma):
    """48x32, samples=1, 3 frames of the moving-camera scene: render_sequence(temporal=Temporal(feedback=0.5), denoise=VarianceDenoise(2,
    4.0, 0.4, 0.3)) writes the bytes of a loop over render_device, gbuffer, temporal_accumulate (moments) and denoise_temporal_variance
    (feedback=0.5), and the bytes of the restatements run on the oracle's renders and closest hits.  With feedback=0 it writes the bytes
    of a call without the field, which differ."""
    import torch
    import rayn_amd as R
    from rayn_amd import film as F
    from rayn_amd import image
    from rayn_amd import setup as S
    K = R.ChannelKind
    w, h, frames, samples, bounces, beta = 48, 32, [1, 2, 3], 1, 2, 0.5
    n = w * h
    world, cam = scenes.moving_scene(w, h)
    integ = R.PathTracingIntegrator(max_bounces=bounces, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE)
    filt = R.BlackmanHarrisFilter(S.FILTER_RADIUS)
    dn = R.VarianceDenoise(2, 4.0, 0.4, 0.3)
    film = R.Film([K.Color, K.Alpha, K.Background, K.WorldNormal], (w, h))
    ctx = film.ctx
    ctx.set_fma_policy(fma)

    def sequence(name, temporal):
        film.render_sequence(world, cam, integ, filt, S.TILE_SIZE, frames, 24, 1.0 / 24.0, samples, [K.Color], str(tmp_path / name), "a", denoise=dn, temporal=temporal)
        return IO.read_folder(tmp_path / name)

    got = sequence("fed", R.Temporal(feedback=beta))
    names = [f"a_{f:04d}_color_temporal_denoised.png" for f in frames]
    assert sorted(got) == names
    without, zero = sequence("without", R.Temporal()), sequence("zero", R.Temporal(feedback=0.0))
    assert zero == without
    assert got[names[0]] == without[names[0]] and got[names[1]] != without[names[1]]  # the first frame's history feeds the second

    desc = world.to_desc(cam)
    ctx.upload_world(desc)
    hit = T.world_hitables(desc)
    tp = R.Temporal(feedback=beta)
    hist = [torch.empty(F.temporal_history_bytes(w, h), dtype=torch.uint8, device="cuda") for _ in range(2)]
    mom = [torch.empty(F.temporal_moments_bytes(w, h), dtype=torch.uint8, device="cuda") for _ in range(2)]
    g, acc, shown = F.alloc_gbuffer(w, h, "cuda"), torch.empty(n, 3, dtype=torch.float32, device="cuda"), torch.empty(n, 3, dtype=torch.float32, device="cuda")
    img = torch.empty(n * 3, dtype=torch.uint8, device="cuda")
    prev_start, prev_host, fed = None, (None, None), 0
    for i, frame in enumerate(frames):
        first = i == 0
        # the plain loop of the entries
        p, out = IO.render_sequence_frame(ctx, w, h, frame, samples, bounces, filt)
        ctx.gbuffer(p, g)
        ctx.temporal_accumulate(p, tp, out, g, None if first else hist[(i + 1) % 2], None if first else desc.camera, 0.0 if first else prev_start,
                                hist[i % 2], acc, None, None if first else mom[(i + 1) % 2], mom[i % 2])
        ctx.denoise_temporal_variance(w, h, dict(out, color=acc), g, hist[i % 2], mom[i % 2], shown, dn, feedback=beta)
        ctx.save_to_pixels(K.Color, film.have_mask(), False, w, h, dict(out, color=shown), img)
        image.save(str(tmp_path / "one.png"), img.cpu().numpy().reshape(h, w, 3))
        assert open(tmp_path / "one.png", "rb").read() == got[names[i]], frame
        # the restatements on the oracle's render and closest hits, fed their own previous history and moments
        o_film, _ = oracle.render(desc, p, oracle.build_tables(4 * samples, bounces, p.volume_marches, frame, w, h, 0, S.FILTER_RADIUS, fma=bool(fma)), fma=bool(fma))
        rec, obj = T.gbuffer_oracle(oracle, desc, p, fma=bool(fma))
        w_out, w_hist, w_mom = TV.accumulate(w, h, o_film["color"], o_film["normal"], rec, obj, prev_host[0], prev_host[1], desc.camera,
                                             0.0 if first else prev_start, p.time_start, hit, tp.max_history, tp.depth_tolerance, tp.normal_min)
        w_c, _, w_fed = TF.denoise(w, h, w_out, o_film["alpha"], o_film["normal"], obj, w_hist, w_mom, dn.iterations, dn.sigma_luminance, dn.sigma_normal,
                                   dn.sigma_alpha, beta)
        image.save(str(tmp_path / "np.png"), image.color_image(np.asarray(w_c, f32).reshape(h, w, 3), background=o_film["background"].reshape(h, w, 3)))
        assert open(tmp_path / "np.png", "rb").read() == got[names[i]], (frame, "the restatement on the oracle's frames")
        g_hist = T.split_history(hist[i % 2].cpu().numpy(), n)
        for name, a, b in zip("ABNO", g_hist, w_fed):
            assert same_bits(a, b), (frame, name)
        fed += int((_bits(w_fed[0]) != _bits(w_hist[0])).any(axis=1).sum())
        prev_start, prev_host = p.time_start, (w_fed, w_mom)
    assert fed > n // 2  # the write-back changed the history of the surfaces' pixels in every frame


# ---- 3. input hygiene ------------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_invalid_arg_with_a_text_and_leave_the_outputs_and_the_history_untouched(ctx):
    import torch
    from rayn_amd import film as F
    L = ctx._L
    w, h, n = 40, 24, 40 * 24
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    hb, mb, sb = F.temporal_history_bytes(w, h), F.temporal_moments_bytes(w, h), F.denoise_variance_scratch_bytes(w, h)
    # every buffer in a slot of its own in one arena, each slot larger than any buffer: a misplaced pointer overlaps only what the case names
    SLOT = 1 << 16
    assert max(hb + 16, sb + 16, 16 * n + 16) <= SLOT
    arena = torch.zeros(10 * SLOT, dtype=torch.uint8, device="cuda")
    slot = lambda i, nbytes: arena[i * SLOT: i * SLOT + nbytes]
    fl = lambda i, k: slot(i, 4 * k).view(torch.float32)
    color, normal, alpha, obj = fl(0, 3 * n), fl(1, 3 * n), fl(2, n), slot(3, 4 * n).view(torch.int32)
    color.fill_(0.5)
    obj.fill_(1)
    hist, mom, scratch = slot(4, hb + 16), slot(5, mb + 16), slot(6, sb + 16)
    hist[: 16 * n].view(torch.float32).fill_(4.0)  # plane A: colour 4, n' = 4 - a guided pixel everywhere, so a valid call writes
    out, var = fl(7, 3 * n), fl(8, n)
    out.fill_(7.0)
    var.fill_(7.0)
    keep = arena.clone()

    def untouched():
        torch.cuda.synchronize()
        return bool(torch.equal(arena[: 6 * SLOT], keep[: 6 * SLOT]) and torch.equal(arena[7 * SLOT:], keep[7 * SLOT:]))  # everything but the scratch

    def dn(w=w, h=h, L_=2, sl=4.0, sn=0.4, sa=0.3, color=vp(color), alpha=vp(alpha), normal=vp(normal), obj=vp(obj), hist=vp(hist), hb=hb, mom=vp(mom), mb=mb,
           out=vp(out), var=vp(var), scratch=vp(scratch), sb=sb, beta=0.5):
        rc = L.rayn_hip_denoise_temporal_variance_feedback_device(ctx.h, w, h, L_, sl, sn, sa, color, alpha, normal, obj, hist, hb, mom, mb, out, var, scratch, sb,
                                                                  beta, None)
        return rc, ctx.last_error()

    nan, inf = float("nan"), float("inf")
    cases = (
        # the strength
        (dict(beta=nan), "feedback must be finite and in [0, 1]"), (dict(beta=-0.25), "feedback must be finite"), (dict(beta=1.5), "feedback must be finite"),
        (dict(beta=inf), "feedback must be finite"), (dict(beta=-inf), "feedback must be finite"), (dict(beta=float(np.nextafter(f32(1.0), f32(2.0)))), "feedback must be finite"),
        # the history is an output: it may overlap nothing else
        (dict(hist=vp(color), hb=SLOT), "alias"), (dict(hist=vp(alpha), hb=SLOT), "alias"), (dict(hist=vp(normal), hb=SLOT), "alias"),
        (dict(hist=vp(obj), hb=SLOT), "alias"), (dict(hist=vp(mom), hb=SLOT), "alias"), (dict(hist=vp(mom, 16), hb=SLOT), "alias"),
        (dict(hist=vp(out), hb=SLOT), "alias"), (dict(out=vp(hist)), "alias"), (dict(out=vp(hist, 48 * n)), "alias"), (dict(var=vp(hist, 16)), "alias"),
        (dict(hist=vp(scratch), hb=SLOT), "alias"), (dict(scratch=vp(hist), sb=hb), "alias"),
        # the existing entry's cases against the new entry
        (dict(w=0), "zero-sized"), (dict(w=65536, h=32768), "2^31"), (dict(L_=0), "iterations"), (dict(L_=9), "iterations"),
        (dict(sl=-1.0), "sigma_luminance"), (dict(sl=nan), "sigma_luminance"), (dict(sl=2.0 ** 31), "sigma_luminance"), (dict(sn=inf), "sigma_normal"),
        (dict(sn=2.0 ** -31), "sigma_normal"), (dict(sa=-0.3), "sigma_alpha"), (dict(color=None), "null buffer"), (dict(obj=None), "null buffer"),
        (dict(hist=None), "null buffer"), (dict(mom=None), "null buffer"), (dict(out=None), "null buffer"), (dict(scratch=None), "null buffer"),
        (dict(normal=None), "null normal guide"), (dict(alpha=None), "null alpha guide"), (dict(hb=hb - 1), "history smaller"),
        (dict(mb=mb - 1), "moments smaller"), (dict(sb=sb - 1), "scratch smaller"), (dict(scratch=vp(scratch, 4)), "scratch not 16-byte aligned"),
        (dict(hist=vp(hist, 8)), "history not 16-byte aligned"), (dict(mom=vp(mom, 8)), "moments not 16-byte aligned"),
        (dict(obj=vp(obj, 2)), "4-byte aligned"), (dict(out=vp(color)), "alias an input"), (dict(var=vp(mom)), "alias an input"),
        (dict(var=vp(alpha)), "alias an input"), (dict(var=vp(out)), "d_out_variance must not alias d_out_color"),
        (dict(scratch=vp(color)), "scratch must not alias an input"), (dict(out=vp(scratch)), "scratch must not alias an output"),
        (dict(var=vp(scratch, 64)), "scratch must not alias an output"))
    for kw, text in cases:
        rc, err = dn(**kw)
        assert rc == -1 and text in err, (kw, rc, err)
        assert untouched(), kw
    # the valid calls, last: a strength of 0 writes the outputs and leaves the history, 1 writes the history too
    assert dn(beta=0.0)[0] == 0
    torch.cuda.synchronize()
    assert torch.equal(slot(4, hb + 16), keep[4 * SLOT: 4 * SLOT + hb + 16]) and not torch.any(out == 7.0)
    assert dn(beta=1.0, normal=None, sn=0.0, alpha=None, sa=0.0, var=None)[0] == 0
    torch.cuda.synchronize()
    assert torch.equal(hist[16 * n:], keep[4 * SLOT + 16 * n: 4 * SLOT + hb + 16]) and torch.all(hist[: 16 * n].view(torch.float32).view(n, 4)[:, 3] == 4.0)
    assert torch.all(hist[: 16 * n].view(torch.float32).view(n, 4)[:, :3] == 0.5)  # a constant colour filters to itself: fb = c + 1 * (c - c)
    # the Python wrapper's own check
    import rayn_amd as R
    for bad in (nan, -0.5, 2.0):
        with pytest.raises(ValueError, match="feedback must be finite and in"):
            ctx.denoise_temporal_variance(w, h, {"color": color}, {"object": obj}, hist[:hb], mom[:mb], out, R.VarianceDenoise(1, 4.0, 0.0, 0.0), feedback=bad)


# ---- 4. what it does to the error ----------------------------------------------------------------------------------------------------------------

# MSE of the last frame relative to the raw last frame's, computed with the CPU oracle and the numpy restatements
# (tools/temporal_feedback_defaults.py) - the path the tests above hold the GPU to bit for bit.  No strength above 0
# beat the 0.4571x of no feedback on this sequence; BEST is the best point of the grid that has one.
BEST_FEEDBACK, BEST_DENOISE, MEASURED_RATIO = 0.25, (1, 2.0, 0.4, 0.3), 0.4675
WITHOUT_FEEDBACK = 0.4571  # Temporal() + VarianceDenoise(1, 4.0, 0.4, 0.3), the recommended setting


def test_the_best_feedback_point_reaches_the_ratio_measured_on_the_cpu_path():
    """temporal_np.DefaultsCase (shipped scene, 160x96, moving camera, 8 frames of 8 spp, against samples=256): Temporal(feedback=0.25)
    with VarianceDenoise(1, 2.0, 0.4, 0.3), every frame's filter feeding the next frame's history, reaches the ratio measured on the CPU
    path (times 1.05, the project's margin for this kind of test: the GPU path is bit-identical to it).  That ratio is above the one
    without feedback: on this sequence the feedback does not pay, and nothing here claims it does."""
    import rayn_amd as R
    raw, _, both = defaults_case_errors(R.Temporal(feedback=BEST_FEEDBACK), R.VarianceDenoise(*BEST_DENOISE), feedback=True)
    print(f"MSE raw {raw:.4e}, Temporal(feedback={BEST_FEEDBACK}) + VarianceDenoise{BEST_DENOISE} {both / raw:.4f}x (CPU path: {MEASURED_RATIO}x; "
          f"without feedback at the recommended setting: {WITHOUT_FEEDBACK}x)")
    assert both / raw < MEASURED_RATIO * 1.05, (raw, both)
