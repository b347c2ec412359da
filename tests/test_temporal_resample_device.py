"""rayn_hip_temporal_accumulate_resample_device (k_temporal_accumulate<*, 1>, rayn_amd/csrc/temporal.hip) on the GPU: bit for bit against its
numpy restatement (tests/temporal_resample_np.py) on adversarial inputs that reach all three arms, on exactly integral reprojections, at
the borders and on tiny images, and on a rendered sequence; resample = 0 against the two older entries; render_sequence(temporal=
Temporal(resample="catmull_rom")) against the plain loop of the entries; error texts; and the measured figure of the best Catmull-Rom
point on the shipped scene."""
import ctypes as C
import os

import numpy as np
import pytest

import device_io as IO
import scenes
import temporal_cases as TC
import temporal_np as T
import temporal_resample_cases as K
import temporal_resample_np as TR
from common import bits_equal
from device_io import module_context as ctx  # noqa: F401

pytestmark = pytest.mark.gpu

f32 = np.float32


def _entry(ctx, p, tp, resample, color, normal, rec, obj, prev, prev_mom, prev_cam, prev_time, moments):
    """The new entry, called directly, on host arrays: (out (n, 3), (A, B, N, O), moments (n, 2) or None), with temporal_cases' checks"""
    from rayn_amd import _abi
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    t_abi, rp = tp.to_abi(), _abi.TemporalResampleParams(resample)

    def call(film, g, d_prev, d_new, d_out, d_pm, d_nm):
        rc = ctx._L.rayn_hip_temporal_accumulate_resample_device(
            ctx.h, C.byref(p), C.byref(t_abi), C.byref(rp), None if prev_cam is None else C.byref(prev_cam), float(prev_time), vp(film["color"]), vp(film["normal"]),
            vp(g["records"]), vp(g["object"]), vp(d_prev), vp(d_new), d_new.numel(), vp(d_pm), vp(d_nm), 0 if d_nm is None else d_nm.numel(), vp(d_out), None)
        assert rc == 0, ctx.last_error()

    return TC.gpu_accumulate(ctx, p, tp, color, normal, rec, obj, prev, prev_mom, prev_cam, prev_time, moments, call)


def _same(got, want, what):
    """colour, planes A, B, N and the moments bit for bit (NaN payloads aside), the objects equal"""
    IO.assert_bits_equal(got[0], want[0], (what, "colour"))
    TC.assert_history_equal(got[1], want[1], what)
    assert (got[2] is None) == (want[2] is None) and (got[2] is None or bits_equal(got[2], want[2])), (what, "moments")


def _upload_moving_world(ctx):
    wd, hit = K.moving_world()  # hitable 1 (the fractal) and one sphere are animated: object motion is exercised too
    ctx.upload_world(wd)
    return wd, hit


# ---- 1. the kernel against the restatement ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("cam_kind", [0, 1, 2])
def test_catmull_rom_matches_the_restatement_on_adversarial_inputs(ctx, cam_kind, fma):
    """37x29 under the three camera kinds and both mul_add policies, with and without moments, the normal test on and off.  Before it
    compares, the test asserts that the restatement alone sends >= 25 % of the pixels down the cubic arm, >= 15 % down the bilinear
    fallback and >= 5 % into a reset, so that no arm can hide."""
    import rayn_amd as R
    _, hit = _upload_moving_world(ctx)
    ctx.set_fma_policy(fma)
    try:
        pc, c, nr, rec, obj, prev, M = K.adversarial_inputs(5 + cam_kind, cam_kind)
        p = R.frame_params(K.W, K.H, 1, 1, time_range=(K.CUR_TIME, 0.8))
        for normal_min, moments, mh in ((-1.0, True, 8), (0.8, False, 8), (0.8, True, 3), (-1.0, False, 65536)):
            tp = R.Temporal(mh, 0.05, normal_min)
            want = TR.accumulate(K.W, K.H, c, nr, rec, obj, prev, M if moments else None, pc, K.PREV_TIME, K.CUR_TIME, hit, mh, 0.05, normal_min, 1)
            shares = K.arm_shares(want[3])
            print(cam_kind, fma, normal_min, moments, mh, shares)
            assert all(shares[code] >= least for code, least in K.MIN_SHARE.items()), shares
            got = _entry(ctx, p, tp, 1, c, nr, rec, obj, prev, M, pc, K.PREV_TIME, moments)
            _same(got, want[:3], (cam_kind, fma, normal_min, moments, mh))
    finally:
        ctx.set_fma_policy(0)


@pytest.mark.parametrize("cam_kind", [0, 1, 2])
def test_resample_0_through_the_new_entry_is_the_two_older_entries(ctx, cam_kind):
    import rayn_amd as R
    _, hit = _upload_moving_world(ctx)
    pc, c, nr, rec, obj, prev, M = K.adversarial_inputs(5 + cam_kind, cam_kind)
    p = R.frame_params(K.W, K.H, 1, 1, time_range=(K.CUR_TIME, 0.8))
    for normal_min, moments in ((-1.0, False), (0.8, True)):
        tp = R.Temporal(8, 0.05, normal_min)
        old = TC.gpu_accumulate(ctx, p, tp, c, nr, rec, obj, prev, M, pc, K.PREV_TIME, moments=moments)
        new = _entry(ctx, p, tp, 0, c, nr, rec, obj, prev, M, pc, K.PREV_TIME, moments)
        _same(new, old, (cam_kind, moments))
        cubic = _entry(ctx, p, tp, 1, c, nr, rec, obj, prev, M, pc, K.PREV_TIME, moments)
        assert not bits_equal(cubic[0], old[0])  # and the option does something
    # Context.temporal_accumulate routes "catmull_rom" to the new entry
    via_ctx = TC.gpu_accumulate(ctx, p, R.Temporal(8, 0.05, 0.8, resample="catmull_rom"), c, nr, rec, obj, prev, M, pc, K.PREV_TIME, moments=True)
    _same(via_ctx, cubic, "Context.temporal_accumulate")


def test_catmull_rom_on_exactly_integral_reprojections(ctx):
    """The exact orthographic case of test_accumulate_on_exactly_integral_reprojections: camera shifts by whole and quarter pixels across
    all four borders; at whole pixels t = 0 and the footprint's weights are (-0, 1, 0, +-0)."""
    import rayn_amd as R
    wd, _, _ = scenes.scene("s0", (16, 8))
    ctx.upload_world(wd)
    w, h = 16, 8
    rec, obj, normal = T.ortho_plane_gbuffer(w, h)
    rng = np.random.default_rng(3)
    p = R.frame_params(w, h, 1, 1, time_range=(0.0, 0.1))
    tp = R.Temporal(3, 0.05, 0.9)
    for sx, sy in ((0.0, 0.0), (3.0, 0.0), (-2.25, 0.0), (0.0, 2.0), (0.5, -1.75), (-20.0, 0.0)):
        prev_cam = T.ortho_camera(w, h, origin_x=-sx * 0.125)
        prev_cam.origin.y = prev_cam.at.y = -sy * 0.125
        prev_rec, _, _ = T.ortho_plane_gbuffer(w, h, origin_x=-sx * 0.125)
        prev_rec[:, 1] -= f32(sy * 0.125)
        A = np.concatenate([rng.random((w * h, 3)), np.full((w * h, 1), 3.0)], axis=1).astype(f32)  # at the cap
        prev = (A, prev_rec, np.concatenate([normal, np.zeros((w * h, 1), f32)], axis=1), obj)
        color, M = rng.random((w * h, 3)).astype(f32), rng.random((w * h, 2)).astype(f32)
        want = TR.accumulate(w, h, color, normal, rec, obj, prev, M, prev_cam, 0.0, 0.0, [], 3, 0.05, 0.9, 1)
        _same(_entry(ctx, p, tp, 1, color, normal, rec, obj, prev, M, prev_cam, 0.0, True), want[:3], (sx, sy))
        assert (want[3] == TR.ARM_CUBIC).any() or abs(sx) >= w


def test_catmull_rom_at_the_borders_and_on_tiny_images(ctx):
    """3x2 (never the cubic arm) and 4x4 (the one footprint that fits) bit for bit, and an 8x6 image whose reprojection puts x0 - 1 < 0 on
    the left columns and x0 + 2 >= width on the right ones, y likewise."""
    import rayn_amd as R
    wd, _, _ = scenes.scene("s0", (16, 8))
    ctx.upload_world(wd)
    rng = np.random.default_rng(11)
    seen = {}
    for (w, h), (sx, sy) in (((3, 2), (0.25, 0.5)), ((4, 4), (0.25, 0.5)), ((4, 4), (-0.5, -0.25)), ((8, 6), (0.5, 0.25)), ((8, 6), (-1.5, 1.75))):
        n = w * h
        rec, obj, normal = T.ortho_plane_gbuffer(w, h)
        prev_cam = T.ortho_camera(w, h, origin_x=-sx * 0.125)
        prev_cam.origin.y = prev_cam.at.y = -sy * 0.125
        prev_rec, _, _ = T.ortho_plane_gbuffer(w, h, origin_x=-sx * 0.125)
        prev_rec[:, 1] -= f32(sy * 0.125)
        A = np.concatenate([rng.random((n, 3)), rng.choice(np.array([1.0, 2.0, 5.0]), n)[:, None]], axis=1).astype(f32)
        prev = (A, prev_rec, np.concatenate([normal, np.zeros((n, 1), f32)], axis=1), obj)
        color, M = rng.random((n, 3)).astype(f32), rng.random((n, 2)).astype(f32)
        p = R.frame_params(w, h, 1, 1, time_range=(0.0, 0.1))
        for moments in (False, True):
            want = TR.accumulate(w, h, color, normal, rec, obj, prev, M if moments else None, prev_cam, 0.0, 0.0, [], 8, 0.05, -1.0, 1)
            _same(_entry(ctx, p, R.Temporal(8, 0.05, -1.0), 1, color, normal, rec, obj, prev, M, prev_cam, 0.0, moments), want[:3], (w, h, sx, sy, moments))
        seen[(w, h, sx)] = K.arm_shares(want[3])
    assert seen[(3, 2, 0.25)][2] == 0.0 and seen[(3, 2, 0.25)][1] > 0.0
    assert seen[(4, 4, 0.25)][2] == 1.0 / 16.0 and seen[(4, 4, -0.5)][2] == 1.0 / 16.0  # the one pixel whose footprint is the image
    assert 0.0 < seen[(8, 6, 0.5)][2] < 1.0 and seen[(8, 6, 0.5)][1] > 0.0 and seen[(8, 6, -1.5)][0] > 0.0


def test_catmull_rom_with_non_finite_history_inside_full_footprints(ctx):
    """temporal_resample_cases.non_finite_history_case - a single inf, a single NaN, a 2x2 block of inf and an inf moment inside whole
    footprints: the clamp's handling of NaN and infinite sums and the reset behind it, bit for bit (tests/test_temporal_resample.py
    asserts on the CPU that the restatement takes each of those paths here)."""
    import rayn_amd as R
    wd, _, _ = scenes.scene("s0", (16, 8))
    ctx.upload_world(wd)
    w, h = 12, 10
    pc, c, nr, rec, obj, prev, M, _, _ = K.non_finite_history_case(w, h)
    p = R.frame_params(w, h, 1, 1, time_range=(0.0, 0.1))
    for moments in (True, False):
        want = TR.accumulate(w, h, c, nr, rec, obj, prev, M if moments else None, pc, 0.0, 0.0, [], 8, 0.05, -1.0, 1)
        _same(_entry(ctx, p, R.Temporal(8, 0.05, -1.0), 1, c, nr, rec, obj, prev, M, pc, 0.0, moments), want[:3], moments)
        assert (want[3] == TR.ARM_CUBIC).sum() == (w - 3) * (h - 3) - 5  # the five pixels whose h stays +inf reset


def test_catmull_rom_on_a_rendered_sequence_with_a_moving_camera_and_a_moving_sphere(ctx):
    """48x32, 3 frames of 4 spp (GPU film, GPU G-buffer) of a scene whose camera, fractal and one sphere move: the entry chained by hand,
    with moments, equals the restatement frame by frame, each fed the kernel's previous history and moments."""
    import rayn_amd as R
    w, h = 48, 32
    wd, _, _ = scenes.scene("s1", (w, h), moving=True)
    ps = [R.frame_params(w, h, 1, 2, frame=f) for f in (1, 2, 4)]
    frames = IO.render_frames(ctx, wd, ps, 2)
    hit = T.world_hitables(wd)
    gbufs = [IO.gpu_gbuffer(ctx, p)[1:] for p in ps]
    for tp in (R.Temporal(8, 0.05, 0.3), R.Temporal(8, 0.05, -1.0)):  # the existing test's setting (its normal test leaves few whole footprints), and without it
        prev, mom, prev_time, cubic = None, None, 0.0, 0
        for p, film, (rec, obj) in zip(ps, frames, gbufs):
            color, normal = film["color"].cpu().numpy(), film["normal"].cpu().numpy()
            if prev is None:
                want = TR.accumulate_first(w, h, color, normal, rec, obj, True)
            else:
                want = TR.accumulate(w, h, color, normal, rec, obj, prev, mom, wd.camera, prev_time, p.time_start, hit, tp.max_history, tp.depth_tolerance,
                                     tp.normal_min, 1)
            got = _entry(ctx, p, tp, 1, color, normal, rec, obj, prev, mom, None if prev is None else wd.camera, prev_time, True)
            _same(got, want[:3], (tp.normal_min, p.frame))
            prev, mom, prev_time = got[1], got[2], p.time_start
            cubic = int((want[3] == TR.ARM_CUBIC).sum())
        print(f"normal_min {tp.normal_min}: {cubic} of {w * h} pixels of the last frame took the cubic arm, {K.arm_shares(want[3])}")
        assert cubic > 0 and (want[3] == TR.ARM_BILINEAR).any() and (want[3] == TR.ARM_RESET).any() and prev[0][:, 3].max() == 3.0


# ---- 2. the sequence wiring ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_variance", [False, True])
def test_render_sequence_with_catmull_rom_is_the_plain_loop_of_the_entries(tmp_path, with_variance):
    """render_sequence(temporal=Temporal(resample="catmull_rom")) writes the bytes of a loop over render_device, gbuffer, the resample entry
    (and denoise_temporal_variance), save_to_pixels; resample="bilinear" writes the files of a Temporal() without the argument."""
    import torch
    import rayn_amd as R
    from rayn_amd import _abi, image
    from rayn_amd import film as F
    from rayn_amd import setup as S
    Kd = R.ChannelKind
    w, h, frames, samples = 48, 32, [2, 3, 5], 1
    _, world, cam = scenes.scene("s1", (w, h), moving=True)
    integ = R.PathTracingIntegrator(max_bounces=2, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE)
    filt = R.BlackmanHarrisFilter(S.FILTER_RADIUS)
    kinds = [Kd.Color, Kd.Alpha, Kd.Background, Kd.WorldNormal]
    dn = R.VarianceDenoise(1, 4.0, 0.4, 0.3) if with_variance else None
    suffix = "color_temporal_denoised" if with_variance else "color_temporal"

    def sequence(tp, name):
        film = R.Film(kinds, (w, h))
        film.render_sequence(world, cam, integ, filt, S.TILE_SIZE, frames, 24, 1.0 / 24.0, samples, [Kd.Color], str(tmp_path / name), "a", denoise=dn, temporal=tp)
        return film, IO.read_folder(tmp_path / name)

    film, got = sequence(R.Temporal(resample="catmull_rom"), "cubic")
    _, default = sequence(R.Temporal(), "default")
    _, named = sequence(R.Temporal(resample="bilinear"), "bilinear")
    assert sorted(got) == sorted(default) == sorted(f"a_{f:04d}_{suffix}.png" for f in frames)
    assert named == default and got[f"a_0002_{suffix}.png"] == default[f"a_0002_{suffix}.png"] and got[f"a_0005_{suffix}.png"] != default[f"a_0005_{suffix}.png"]
    # the loop
    ctx = film.ctx
    desc = world.to_desc(cam)
    ctx.upload_world(desc)
    n = w * h
    hist = [torch.empty(F.temporal_history_bytes(w, h), dtype=torch.uint8, device="cuda") for _ in range(2)]
    mom = [torch.empty(F.temporal_moments_bytes(w, h), dtype=torch.uint8, device="cuda") for _ in range(2)]
    g, acc, shown = F.alloc_gbuffer(w, h, "cuda"), torch.empty(n, 3, dtype=torch.float32, device="cuda"), torch.empty(n, 3, dtype=torch.float32, device="cuda")
    img = torch.empty(n * 3, dtype=torch.uint8, device="cuda")
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    t_abi, rp, prev_start = R.Temporal().to_abi(), _abi.TemporalResampleParams(1), None
    for i, frame in enumerate(frames):
        p, out = IO.render_sequence_frame(ctx, w, h, frame, samples, 2, filt)
        ctx.gbuffer(p, g)
        first = i == 0
        rc = ctx._L.rayn_hip_temporal_accumulate_resample_device(
            ctx.h, C.byref(p), C.byref(t_abi), C.byref(rp), None if first else C.byref(desc.camera), 0.0 if first else prev_start, vp(out["color"]), vp(out["normal"]),
            vp(g["records"]), vp(g["object"]), None if first else vp(hist[(i + 1) % 2]), vp(hist[i % 2]), hist[0].numel(),
            None if first or not with_variance else vp(mom[(i + 1) % 2]), vp(mom[i % 2]) if with_variance else None, mom[0].numel(), vp(acc),
            C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, ctx.last_error()
        prev_start = p.time_start
        pic = acc
        if with_variance:
            ctx.denoise_temporal_variance(w, h, dict(out, color=acc), g, hist[i % 2], mom[i % 2], shown, dn)
            pic = shown
        ctx.save_to_pixels(Kd.Color, film.have_mask(), False, w, h, dict(out, color=pic), img)
        image.save(str(tmp_path / "one.png"), img.cpu().numpy().reshape(h, w, 3))
        assert open(tmp_path / "one.png", "rb").read() == got[f"a_{frame:04d}_{suffix}.png"], frame


def test_render_sequence_with_catmull_rom_denoise_and_feedback(tmp_path):
    """The option works with the other combinations too: a plain Denoise, and VarianceDenoise with feedback > 0."""
    import rayn_amd as R
    from rayn_amd import setup as S
    Kd = R.ChannelKind
    w, h, frames = 48, 32, [1, 2, 3]
    _, world, cam = scenes.scene("s1", (w, h), moving=True)
    integ = R.PathTracingIntegrator(max_bounces=2, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE)
    filt = R.BlackmanHarrisFilter(S.FILTER_RADIUS)
    film = R.Film([Kd.Color, Kd.Alpha, Kd.Background, Kd.WorldNormal], (w, h))
    out = {}
    for name, tp, dn in (("d_lin", R.Temporal(), R.Denoise()), ("d_cub", R.Temporal(resample="catmull_rom"), R.Denoise()),
                         ("f_lin", R.Temporal(feedback=0.5), R.VarianceDenoise(1, 4.0, 0.4, 0.3)),
                         ("f_cub", R.Temporal(feedback=0.5, resample="catmull_rom"), R.VarianceDenoise(1, 4.0, 0.4, 0.3))):
        film.render_sequence(world, cam, integ, filt, S.TILE_SIZE, frames, 24, 1.0 / 24.0, 1, [Kd.Color], str(tmp_path / name), "a", denoise=dn, temporal=tp)
        out[name] = IO.read_folder(tmp_path / name)
        assert sorted(out[name]) == [f"a_{f:04d}_color_temporal_denoised.png" for f in frames]
    for lin, cub in (("d_lin", "d_cub"), ("f_lin", "f_cub")):
        assert out[lin]["a_0001_color_temporal_denoised.png"] == out[cub]["a_0001_color_temporal_denoised.png"]  # no history yet
        assert out[lin]["a_0003_color_temporal_denoised.png"] != out[cub]["a_0003_color_temporal_denoised.png"]


# ---- 3. input hygiene ----------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_invalid_arg_with_a_text(ctx):
    import torch
    import rayn_amd as R
    from rayn_amd import _abi
    from rayn_amd import film as F
    L = ctx._L
    w, h, n = 40, 24, 40 * 24
    wd, _, _ = scenes.scene("s0", (w, h))
    ctx.upload_world(wd)
    p = R.frame_params(w, h, 1, 1)
    vp = lambda t: C.c_void_p(t.data_ptr())
    z = lambda k: torch.zeros(k, dtype=torch.float32, device="cuda")
    color, normal, out, rec, obj = z(3 * n), z(3 * n), z(3 * n), z(4 * n + 4), torch.zeros(n, dtype=torch.int32, device="cuda")
    hb, mb = F.temporal_history_bytes(w, h), F.temporal_moments_bytes(w, h)
    h0, h1 = (torch.zeros(hb + 16, dtype=torch.uint8, device="cuda") for _ in range(2))
    m0, m1 = (torch.zeros(mb + 16, dtype=torch.uint8, device="cuda") for _ in range(2))
    cam = wd.camera
    bad_cam = _abi.Camera.from_buffer_copy(cam)
    bad_cam.kind = 9
    RP, T_ = _abi.TemporalResampleParams, _abi.TemporalParams

    def acc(p=p, tp=R.Temporal().to_abi(), rp=RP(1), cam=cam, color=vp(color), new=vp(h1), prev=vp(h0), hb=hb, pm=vp(m0), nm=vp(m1), mb=mb, out=vp(out)):
        rc = L.rayn_hip_temporal_accumulate_resample_device(ctx.h, None if p is None else C.byref(p), None if tp is None else C.byref(tp),
                                                            None if rp is None else C.byref(rp), None if cam is None else C.byref(cam), 0.0, color, vp(normal),
                                                            vp(rec), vp(obj), prev, new, hb, pm, nm, mb, out, None)
        return rc, ctx.last_error()

    assert acc()[0] == 0 and acc(rp=RP(0))[0] == 0 and acc(pm=None, nm=None, mb=0)[0] == 0 and acc(prev=None, cam=None, pm=None)[0] == 0
    for kw, text in ((dict(rp=None), "null resample params"), (dict(rp=RP(2)), "resample must be 0"), (dict(rp=RP(0xFFFFFFFF)), "resample must be 0"),
                     (dict(nm=None), "null buffer"), (dict(pm=None), "needs the previous moments"), (dict(prev=None, cam=None), "previous moments without"),
                     (dict(p=None), "null frame params"), (dict(p=R.frame_params(0, h, 1, 1)), "zero-sized"), (dict(tp=None), "null temporal params"),
                     (dict(tp=T_(0, 0.05, 0.9)), "max_history"), (dict(tp=T_(4, -0.1, 0.9)), "depth_tolerance"), (dict(tp=T_(4, 0.05, 1.5)), "normal_min"),
                     (dict(color=None), "null buffer"), (dict(cam=None), "previous camera"), (dict(cam=bad_cam), "unknown camera kind"),
                     (dict(hb=hb - 1), "history smaller"), (dict(new=C.c_void_p(h1.data_ptr() + 4)), "16-byte aligned"), (dict(new=vp(h0)), "alias the previous"),
                     (dict(out=vp(color)), "alias an input"), (dict(out=vp(h1)), "alias the new history"), (dict(mb=mb - 1), "moments smaller"),
                     (dict(nm=C.c_void_p(m1.data_ptr() + 8)), "16-byte aligned"), (dict(nm=vp(m0)), "alias the previous"), (dict(nm=vp(h1)), "alias another output")):
        rc, err = acc(**kw)
        assert rc == -1 and err and text in err, (kw, rc, err)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="resample"):
        R.Temporal(resample="nearest")


# ---- 4. does it do its job -------------------------------------------------------------------------------------------------------------------

# The best Catmull-Rom point of the CPU grid (tools/temporal_resample_defaults.py: the oracle and the numpy restatements):
# Temporal(max_history=4, resample="catmull_rom") + VarianceDenoise(1, 4.0, 0.4, 0.3), MSE of the last frame relative to the raw last frame's.
# It does NOT beat the bilinear 0.4571x: the test pins the measured figure, it does not claim a gain.
BEST_MAX_HISTORY, MEASURED_RATIO, MEASURED_ALONE = 4, 0.4583, 0.4994
RECOMMENDED = (1, 4.0, 0.4, 0.3)


def test_the_best_catmull_rom_point_reaches_the_measured_ratio():
    """temporal_np.DefaultsCase (shipped scene, 160x96, moving camera, 8 frames of 8 spp, against samples=256) at the best Catmull-Rom point
    of the CPU grid reaches the ratio the CPU tool printed, times 1.05 - the margin of the three sibling tests; the GPU film is the oracle's
    bits and the kernels are the restatement's, so the GPU figure is the CPU one."""
    import rayn_amd as R
    raw, temporal, both = TC.defaults_case_errors(R.Temporal(max_history=BEST_MAX_HISTORY, resample="catmull_rom"), R.VarianceDenoise(*RECOMMENDED))
    print(f"MSE raw {raw:.4e}, catmull_rom alone {temporal / raw:.4f}x (CPU path: {MEASURED_ALONE}x), + variance denoise {both / raw:.4f}x (CPU path: {MEASURED_RATIO}x)")
    assert both / raw < MEASURED_RATIO * 1.05, (raw, temporal, both)
    assert temporal / raw < MEASURED_ALONE * 1.05, (raw, temporal, both)
