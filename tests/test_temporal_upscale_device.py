"""rayn_hip_temporal_upscale_device (rayn_amd/csrc/temporal_upscale.hip) on the GPU: the kernel bit for bit against its numpy restatement
(tests/temporal_upscale_np.py) on synthetic, adversarial and rendered inputs under both mul_add policies - every sigma pair, absent planes,
no low camera and an orthographic, a pinhole and an animated one, confidence off and on, chained frames - against the product's own
upscale and accumulate kernels where the definition says they agree, guard floats and untouched inputs, every INVALID_ARG text with
nothing written, and Film.render_sequence(upscale=, temporal=, supersample=) against a step-by-step loop of Context calls."""
import ctypes as C

import numpy as np
import pytest

import device_io as IO
import temporal_cases as TC
import temporal_np as T
import temporal_upscale_np as TU
from device_io import module_context as ctx  # noqa: F401
from temporal_upscale_cases import FACTORS, SIGMAS, SIZES, sequence

pytestmark = pytest.mark.gpu

f32 = np.float32
KEYS = (("color", 3), ("alpha", 1), ("background", 3), ("normal", 3))


@pytest.fixture(scope="module")
def moving_world():
    """The MandelBox scene with a moving fractal (hitable 1) and a moving sphere: the accumulate's object motion is exercised.  Not
    scenes.scene's moving s1: the fractal's velocity is a tenth of that one's, and the camera is left as the scene has it."""
    import rayn_amd as R
    from rayn_amd import setup as S
    from rayn_amd.scene import Linear, TracedSDF
    cam, world = S.SCENES["s1"]((24, 16))
    for h in world.hitables:
        if isinstance(h, TracedSDF) and h.transform_seq is None:
            h.transform_seq = Linear(R.vec3(0.0, 0.0, 0.0), R.vec3(-0.06, 0.045, 0.03))
    wd = world.to_desc(cam)
    assert wd.hitables[1].animated
    return wd


def _gpu(ctx, w, h, up, tp, sup, film, low_g, high_g, prev, prev_cam, prev_time, low_cam, ts, guard=64):
    """The entry through Context.temporal_upscale on host arrays: (planes, weight, (A, B, N, O)).  Checks the guard floats behind every
    output and the new history, and that no input and not the previous history changed."""
    import torch
    import rayn_amd as R
    from rayn_amd import film as F
    s = up.factor
    N = w * h * s * s
    d_film = IO.upload_film(film, [k for k, _ in KEYS])
    gl, gh = IO.upload_gbuffer(*low_g), IO.upload_gbuffer(*high_g)
    full = {k: IO.guarded(c * N, torch.float32, 7.0, guard) for k, c in KEYS if k in film}
    d_out = {k: v[1] for k, v in full.items()}
    full_wt, d_wt = IO.guarded(N, torch.float32, 7.0, guard)
    nb = F.temporal_history_bytes(w * s, h * s)
    d_prev = None if prev is None else IO.upload_bytes(T.join_history(*prev))
    keep = IO.snapshot([d_prev])
    full_new, d_new = IO.guarded(nb, torch.uint8, 0xA5, guard)
    p = R.frame_params(w, h, 1, 1, time_range=(float(ts), float(ts) + 0.05))
    ctx.temporal_upscale(p, up, tp, sup, d_film, gl, gh, d_prev, prev_cam, prev_time, d_new, d_out, low_cam, d_wt)
    torch.cuda.synchronize()
    for k, c in KEYS:
        if k in film:
            IO.assert_guards(full[k][0], c * N, 7.0, k)
    IO.assert_guards(full_wt, N, 7.0, "weight")
    IO.assert_guards(full_new, nb, 0xA5, "new history")
    IO.assert_unchanged([d_prev], keep, "the previous history")
    for k in d_film:
        IO.assert_is_host(d_film[k], film[k], k)
    IO.assert_gbuffer_is_host(gl, *low_g, "low G-buffer")
    IO.assert_gbuffer_is_host(gh, *high_g, "high G-buffer")
    out = {k: d_out[k].cpu().numpy().reshape((N, c) if c == 3 else (N,)) for k, c in KEYS if k in film}
    return out, d_wt.cpu().numpy(), T.split_history(d_new.cpu().numpy(), N)


def _same(got, want, what):
    IO.assert_planes_equal(got[0], want[0], what)
    IO.assert_bits_equal(got[1], want[1], (what, "weight"))
    TC.assert_history_equal(got[2], want[2], (what, "history"))


def _low_camera(which, w, h, s, shift, ts):
    """None, or a camera over the synthetic plane that stands for the jittered low camera: orthographic (offset by a fraction of a low
    pixel in x and y), a pinhole that sees the whole plane from z = 4, or the orthographic one with its offset as a closure of time."""
    from rayn_amd import _abi
    if which == "none":
        return None
    pixel = 4.0 / h
    c = T.ortho_camera(w, h, origin_x=shift + 0.25 * pixel, pixel=pixel)
    c.origin.y = c.at.y = -0.25 * pixel
    if which == "pinhole":
        c.kind, c.vfov_or_size = _abi.CAM_PINHOLE, 55.0
        c.at.x += 0.2
    elif which == "animated":
        c.animated = 1 | 2 | 4
        for v in (c.origin_vel, c.at_vel):
            v.x, v.y = 0.4 * pixel, -0.3 * pixel
        c.up_vel.x = 0.05
    return c


LOW_CAMERAS = ["none", "ortho", "pinhole", "animated"]


@pytest.mark.parametrize("fma", [0, 1])
def test_kernel_matches_the_restatement_on_synthetic_and_adversarial_inputs(ctx, moving_world, fma):
    """Every low size x every factor, random and adversarial, three chained frames each (the kernel's own history goes into the next
    frame, ping-pong), the sigma pairs, the films that lack Alpha / Background, the four low cameras and confidence off / on in turn.
    The kernel holds no mul_add: both policies of the context give the restatement's bits."""
    import rayn_amd as R
    ctx.set_fma_policy(fma)
    ctx.upload_world(moving_world)
    hit = T.world_hitables(moving_world)
    try:
        seen = {"tiers": set(), "projected": False, "conf": False, "blend": False, "reset": False}
        ci = 0
        for si, (w, h) in enumerate(SIZES):
            for s in FACTORS:
                for adversarial in (False, True):
                    sp, ss = SIGMAS[ci % 4]
                    lack = [(), ("alpha", "background"), ("background",)][ci % 3]
                    tp = [R.Temporal(2, 0.05, -1.0), R.Temporal(8, 0.01, 0.5), R.Temporal(32, 0.05, 0.9)][ci % 3]
                    which, conf = LOW_CAMERAS[(ci // 2) % 4], bool((ci // 2 + ci // 8) % 2)
                    ci += 1
                    up, sup = R.Upscale(s, sp, ss), R.Supersample(jitter=which != "none", confidence=conf)
                    prev, prev_cam, prev_time = None, None, 0.0
                    for k, (film, low_g, high_g, cam, ts) in enumerate(sequence(w, h, s, 100 * si + 10 * s + adversarial, adversarial)):
                        part = {key: v for key, v in film.items() if key not in lack}
                        low_cam = _low_camera(which, w, h, s, 0.3 * k * 4.0 / (h * s), ts)
                        want = TU.temporal_upscale(part, low_g, high_g, w, h, s, sp, ss, low_cam, ts, conf, prev, prev_cam, prev_time, hit,
                                                   tp.max_history, tp.depth_tolerance, tp.normal_min)
                        got = _gpu(ctx, w, h, up, tp, sup, part, low_g, high_g, prev, prev_cam, prev_time, low_cam, ts)
                        _same(got, want, (w, h, s, adversarial, sp, ss, lack, which, conf, k))
                        info = want[3]
                        seen["tiers"] |= set(np.unique(info["tier"]).tolist())
                        seen["projected"] |= bool(info["projected"].any())
                        seen["conf"] |= bool((info["conf"] < 1.0).any())
                        if prev is not None:
                            seen["blend"] |= bool((info["taps"] > 0).any())
                            seen["reset"] |= bool(((info["n"] == 1.0) & (high_g[1] != T.MISS)).any())
                        prev, prev_cam, prev_time = got[2], cam, ts
        assert seen == {"tiers": {1, 2, 3}, "projected": True, "conf": True, "blend": True, "reset": True}, seen
    finally:
        ctx.set_fma_policy(0)


def test_without_low_camera_and_confidence_it_is_the_products_two_kernels(ctx, moving_world):
    """low_camera NULL and confidence 0: every output and the whole new history equal, bit for bit, Context.upscale followed by
    Context.temporal_accumulate at the high size on the device - the product's own kernels as the yardstick - over three chained frames."""
    import torch
    import rayn_amd as R
    from rayn_amd import film as F
    ctx.upload_world(moving_world)
    for ci, ((w, h), s, adversarial) in enumerate([((24, 16), 2, False), ((20, 12), 3, True), ((25, 19), 4, False), ((25, 19), 1, True)]):
        sp, ss = SIGMAS[ci % 4]
        up, tp, sup = R.Upscale(s, sp, ss), R.Temporal(3, 0.05, 0.5 if ci % 2 else -1.0), R.Supersample(jitter=False, confidence=False)
        W, H, N = w * s, h * s, w * h * s * s
        prev, prev_cam, prev_time = None, None, 0.0
        for film, low_g, high_g, cam, ts in sequence(w, h, s, 500 + ci, adversarial):
            got = _gpu(ctx, w, h, up, tp, sup, film, low_g, high_g, prev, prev_cam, prev_time, None, ts)
            p = R.frame_params(w, h, 1, 1, time_range=(float(ts), float(ts) + 0.05))
            d_film = IO.upload_film(film, [k for k, _ in KEYS])
            gl, gh = IO.upload_gbuffer(*low_g), IO.upload_gbuffer(*high_g)
            d_up = F.alloc_device_film(W, H, "cuda")
            d_wt = torch.empty(N, dtype=torch.float32, device="cuda")
            ctx.upscale(p, up, d_film, gl, gh, d_up, d_wt)
            d_prev = None if prev is None else IO.upload_bytes(T.join_history(*prev))
            d_new = torch.empty(F.temporal_history_bytes(W, H), dtype=torch.uint8, device="cuda")
            d_acc = torch.empty(N * 3, dtype=torch.float32, device="cuda")
            ctx.temporal_accumulate(F._scaled_params(p, s), tp, d_up, gh, d_prev, prev_cam, prev_time, d_new, d_acc)
            torch.cuda.synchronize()
            want_planes = {"color": d_acc.cpu().numpy().reshape(N, 3), "alpha": d_up["alpha"].cpu().numpy().reshape(N),
                           "background": d_up["background"].cpu().numpy().reshape(N, 3), "normal": d_up["normal"].cpu().numpy().reshape(N, 3)}
            _same(got, (want_planes, d_wt.cpu().numpy(), T.split_history(d_new.cpu().numpy(), N)), (w, h, s, adversarial, ts))
            prev, prev_cam, prev_time = got[2], cam, ts
        assert (prev[0][:, 3] > 1).any()


def _gbuffer_host(ctx, p):
    return IO.gpu_gbuffer(ctx, p)[1:]


@pytest.mark.parametrize("scene,fma", [("s0", 0), ("ship", 1), ("s0", 1), ("ship", 0)])
def test_kernel_matches_the_restatement_on_rendered_inputs(ctx, scene, fma):
    """The sphere scene and the shipped scene at 24 x 16, factor 2: three frames under a camera whose origin moves, each rendered through
    the jittered camera of its phase, with the product's G-buffers - the low one through the jittered camera, the high one through the
    frame's own - and the kernel's own history chained."""
    import torch
    import rayn_amd as R
    from rayn_amd import film as F
    from rayn_amd import setup as S
    from rayn_amd.scene import Linear
    w, h, s = 24, 16, 2
    cam, world = S.SCENES[scene]((w, h))
    c = world.cameras.get(cam)
    c.origin = Linear(c.origin, R.vec3(0.9, -0.3, 0.15))
    wd = world.to_desc(cam)
    up, tp, sup = R.Upscale(s, 0.02, 0.3), R.Temporal(4, 0.05, -1.0), R.Supersample(jitter=True, confidence=True)
    ctx.set_fma_policy(fma)
    try:
        prev, prev_time, blended = None, 0.0, 0
        for i, frame in enumerate((1, 2, 4)):
            p = R.frame_params(w, h, 1, 2, frame=frame)
            low = type(wd).from_buffer_copy(wd)
            low.camera = F.jittered_camera(wd.camera, *sup.offset(s, i), p.time_start)
            ctx.upload_world(low)
            d_film = F.alloc_device_film(w, h, "cuda")
            ctx.render_device(p, [torch.from_numpy(t).cuda() for t in R.build_tables(4, 2, p.volume_marches, frame, w, h)], d_film)
            low_g = _gbuffer_host(ctx, p)
            ctx.upload_world(wd)
            high_g = _gbuffer_host(ctx, F._scaled_params(p, s))
            film = {k: d_film[k].cpu().numpy() for k, _ in KEYS}
            want = TU.temporal_upscale(film, low_g, high_g, w, h, s, up.sigma_plane, up.sigma_position, low.camera, p.time_start, True, prev,
                                       wd.camera, prev_time, T.world_hitables(wd), tp.max_history, tp.depth_tolerance, tp.normal_min)
            got = _gpu(ctx, w, h, up, tp, sup, film, low_g, high_g, prev, None if prev is None else wd.camera, prev_time, low.camera, p.time_start)
            _same(got, want, (scene, fma, frame))
            assert want[3]["projected"].mean() > 0.5 and (want[3]["tier"] == 1).mean() > 0.8
            prev, prev_time = got[2], p.time_start
            blended = int((prev[0][:, 3] > 1).sum())
        assert blended > w * h * s * s // 4
    finally:
        ctx.set_fma_policy(0)


def test_invalid_arguments_return_their_texts_and_write_nothing(ctx, moving_world):
    import torch
    import rayn_amd as R
    from rayn_amd import _abi
    from rayn_amd import film as F
    L = ctx._L
    w, h, s = 8, 4, 2
    n, N = w * h, w * h * s * s
    hb = F.temporal_history_bytes(w * s, h * s)
    z = lambda k: torch.zeros(k, dtype=torch.float32, device="cuda")
    base = {"color": z(3 * n), "alpha": z(n), "background": z(3 * n), "normal": z(3 * n), "lrec": z(4 * n + 4), "lobj": z(n), "hrec": z(4 * N + 4), "hobj": z(N),
            "prev": torch.zeros(hb + 16, dtype=torch.uint8, device="cuda"), "new": torch.full((hb + 16,), 0xA5, dtype=torch.uint8, device="cuda"),
            "ocolor": z(3 * N) + 7, "oalpha": z(N) + 7, "obackground": z(3 * N) + 7, "onormal": z(3 * N) + 7, "oweight": z(N) + 7}
    order = ["color", "alpha", "background", "normal", "lrec", "lobj", "hrec", "hobj", "prev", "new", "hb", "ocolor", "oalpha", "obackground", "onormal", "oweight"]
    cam = moving_world.camera
    bad_cam = _abi.Camera.from_buffer_copy(cam)
    bad_cam.kind = 9
    p0 = R.frame_params(w, h, 1, 1)
    fresh = R.Context(0)

    def call(c=ctx, p=p0, up=(s, 0.02, 0.05), tp=(4, 0.05, -1.0), sp=(1,), low=cam, prev_cam=cam, hb=hb, **over):
        args = []
        for k in order:
            if k == "hb":
                args.append(hb)
                continue
            v = over.get(k, base[k])
            args.append(None if v is None else C.c_void_p(v if isinstance(v, int) else v.data_ptr()))
        rc = L.rayn_hip_temporal_upscale_device(c.h, None if p is None else C.byref(p), None if up is None else C.byref(_abi.UpscaleParams(*up)),
                                                None if tp is None else C.byref(_abi.TemporalParams(*tp)),
                                                None if sp is None else C.byref(_abi.TemporalUpscaleParams(*sp)), None if low is None else C.byref(low),
                                                None if prev_cam is None else C.byref(prev_cam), 0.0, *args, None)
        return rc, c.last_error()

    try:
        rc, err = call(c=fresh)
        assert rc == -1 and "rayn_hip_upload_world has not been called" in err
    finally:
        fresh.close()
    ctx.upload_world(moving_world)
    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(p=None), "null frame params"),
        # what rayn_hip_upscale_device rejects
        (dict(up=None), "null upscale params"), (dict(up=(0, 0.02, 0.05)), "factor must be in 1..8"), (dict(up=(9, 0.02, 0.05)), "factor must be in 1..8"),
        (dict(p=R.frame_params(0, h, 1, 1)), "zero-sized image"), (dict(p=R.frame_params(w, 0, 1, 1)), "zero-sized image"),
        (dict(p=R.frame_params(1 << 15, 1 << 14, 1, 1)), "upscaled image larger than 2^31 pixels"),
        (dict(p=R.frame_params(1 << 22, 1, 1, 1), up=(4, 0.0, 0.0)), "wider or taller than 2^23"),
        (dict(up=(s, -1.0, 0.05)), "sigma_plane must be 0 (off) or in [2^-30, 2^30]"), (dict(up=(s, nan, 0.05)), "sigma_plane must be 0 (off) or in [2^-30, 2^30]"),
        (dict(up=(s, 0.02, inf)), "sigma_position must be 0 (off) or in [2^-30, 2^30]"), (dict(up=(s, 0.02, 2.0 ** -31)), "sigma_position must be 0 (off) or in [2^-30, 2^30]"),
        (dict(color=None), "null Color buffer"), (dict(ocolor=None), "null Color buffer"),
        (dict(lrec=None), "null G-buffer"), (dict(lobj=None), "null G-buffer"), (dict(hrec=None), "null G-buffer"), (dict(hobj=None), "null G-buffer"),
        (dict(oalpha=None), "null output for a present input plane"), (dict(obackground=None), "null output for a present input plane"),
        (dict(onormal=None), "null output for a present input plane"), (dict(alpha=None), "null input for a present output plane"),
        (dict(normal=None, onormal=None), "null normal guide with sigma_plane != 0"),
        (dict(lrec=base["lrec"].data_ptr() + 4), "G-buffer records not 16-byte aligned"), (dict(hrec=base["hrec"].data_ptr() + 8), "G-buffer records not 16-byte aligned"),
        (dict(hobj=base["hobj"].data_ptr() + 2), "G-buffer objects not 4-byte aligned"),
        (dict(ocolor=base["hrec"]), "an output must not alias an input"), (dict(oweight=base["color"]), "an output must not alias an input"),
        (dict(oalpha=base["hobj"]), "an output must not alias an input"),
        (dict(oweight=base["ocolor"].data_ptr() + 12 * N - 4), "the outputs must not alias each other"), (dict(obackground=base["onormal"]), "the outputs must not alias each other"),
        # what rayn_hip_temporal_accumulate_device rejects, at the high size
        (dict(tp=None), "null temporal params"), (dict(tp=(0, 0.05, 0.9)), "max_history must be in 1..65536"), (dict(tp=(65537, 0.05, 0.9)), "max_history must be in 1..65536"),
        (dict(tp=(4, -0.1, 0.9)), "depth_tolerance must be finite and >= 0"), (dict(tp=(4, inf, 0.9)), "depth_tolerance must be finite and >= 0"),
        (dict(tp=(4, nan, 0.9)), "depth_tolerance must be finite and >= 0"), (dict(tp=(4, 0.05, -1.5)), "normal_min must be in [-1, 1]"),
        (dict(tp=(4, 0.05, nan)), "normal_min must be in [-1, 1]"),
        (dict(up=(s, 0.0, 0.05), normal=None, onormal=None), "null buffer"), (dict(new=None), "null buffer"),
        (dict(prev_cam=None), "a previous history needs the previous camera"), (dict(prev_cam=bad_cam), "unknown camera kind"),
        # this entry's own
        (dict(sp=None), "null temporal upscale params"), (dict(sp=(2,)), "confidence must be 0 (off) or 1 (on)"), (dict(low=bad_cam), "unknown camera kind"),
        (dict(hb=hb - 1), "history smaller than rayn_temporal_history_bytes(width, height)"),
        (dict(hb=F.temporal_history_bytes(w, h)), "history smaller than rayn_temporal_history_bytes(width, height)"),  # the LOW size is not enough
        (dict(new=base["new"].data_ptr() + 4), "history not 16-byte aligned"), (dict(prev=base["prev"].data_ptr() + 8), "history not 16-byte aligned"),
        (dict(new=base["prev"]), "the new history must not alias the previous one"), (dict(new=base["prev"].data_ptr() + 16), "the new history must not alias the previous one"),
        (dict(new=base["color"]), "an output must not alias an input"),
        (dict(hrec=base["new"].data_ptr() + 16), "an output must not alias an input"), (dict(lobj=base["new"].data_ptr() + hb - 4 * n), "an output must not alias an input"),
        (dict(ocolor=base["prev"]), "an output must not alias an input"), (dict(oweight=base["prev"].data_ptr() + hb - 4), "an output must not alias an input"),
        (dict(ocolor=base["new"]), "d_out_color must not alias the new history"), (dict(onormal=base["new"].data_ptr() + 16), "the outputs must not alias each other"),
    ]
    for over, text in cases:
        rc, err = call(**over)
        assert rc == -1 and text in err, (list(over), rc, err)
    torch.cuda.synchronize()
    # nothing was written by any of them
    assert torch.all(base["new"] == 0xA5) and all(torch.all(base[k] == 7.0) for k in ("ocolor", "oalpha", "obackground", "onormal", "oweight"))
    assert all(not torch.any(base[k]) for k in ("color", "alpha", "background", "normal", "lrec", "lobj", "hrec", "hobj", "prev"))
    # what is allowed: no low camera, no previous history (then no previous camera), planes absent on both sides, no weight
    assert call()[0] == 0 and call(low=None)[0] == 0 and call(prev=None, prev_cam=None)[0] == 0 and call(sp=(0,))[0] == 0
    assert call(alpha=None, oalpha=None, background=None, obackground=None, oweight=None)[0] == 0
    torch.cuda.synchronize()
    assert torch.all(base["new"][hb:] == 0xA5)


def _kinds():
    import rayn_amd as R
    K = R.ChannelKind
    return [K.Color, K.Alpha, K.Background, K.WorldNormal]


def test_render_sequence_supersample_is_the_step_by_step_loop(tmp_path):
    """Three frames at 24 x 16, factor 2, under setup_s3 (camera origin and fractal move): the files are byte for byte those of a loop of
    upload_world(jittered), render_device, gbuffer, upload_world, gbuffer, temporal_upscale and save_to_pixels; denoise=Denoise() and
    display= compose on the high film; without supersample= the old ValueError still comes."""
    import torch
    import rayn_amd as R
    from rayn_amd import film as F
    from rayn_amd import image
    from rayn_amd import setup as S
    K = R.ChannelKind
    w, h, s = 24, 16, 2
    W, H = w * s, h * s
    frames, rate, shutter = [3, 4, 7], 24, 1.0 / 24.0
    cam, world = S.setup_s3((w, h))
    integ, filt = R.PathTracingIntegrator(max_bounces=2, volume_marches=2), R.BlackmanHarrisFilter(1.5)
    up, tp, sup = R.Upscale(s, 0.02, 0.05), R.Temporal(), R.Supersample(jitter=True, confidence=True)
    disp, dn = R.Display(exposure=0.5, tone="reinhard"), R.Denoise()
    film = R.Film(_kinds(), (w, h))
    with pytest.raises(ValueError, match="temporal= together with upscale= is not built: the temporal histories live at one resolution"):
        film.render_sequence(world, cam, integ, filt, (16, 16), frames, rate, shutter, 1, _kinds(), str(tmp_path / "no"), "anim", upscale=up, temporal=tp)
    assert not (tmp_path / "no").exists()
    stats = film.render_sequence(world, cam, integ, filt, (16, 16), frames, rate, shutter, 1, _kinds(), str(tmp_path / "seq"), "anim", upscale=up, temporal=tp,
                                 supersample=sup)
    film.render_sequence(world, cam, integ, filt, (16, 16), frames, rate, shutter, 1, [K.Color], str(tmp_path / "seq2"), "anim", upscale=up, temporal=tp,
                         supersample=sup, denoise=dn, display=disp)
    assert [st["frame"] for st in stats] == frames and film.res == (w, h) and film.channels["color"].numel() == 3 * w * h
    got, got2 = IO.read_folder(tmp_path / "seq"), IO.read_folder(tmp_path / "seq2")
    assert sorted(got) == sorted(f"anim_{f:04d}_{sfx}_x2.png" for f in frames for sfx in ("color_temporal", "alpha", "background", "normal"))
    assert sorted(got2) == sorted(f"anim_{f:04d}_color_temporal_denoised_display_x2.png" for f in frames)
    # the loop
    ctx, desc, mask = film.ctx, world.to_desc(cam), film.have_mask()
    hist = [torch.empty(F.temporal_history_bytes(W, H), dtype=torch.uint8, device="cuda") for _ in range(2)]
    g_low, g_high = F.alloc_gbuffer(w, h, "cuda"), F.alloc_gbuffer(W, H, "cuda")
    d_state, prev_start, shown_start = ctx.display_state() if disp.auto else None, None, None
    for i, frame in enumerate(frames):
        start = f32(frame) * (f32(1.0) / f32(rate))
        p = R.frame_params(w, h, 1, 2, 2, frame, (float(start), float(f32(start + f32(shutter)))), (16, 16))
        low = type(desc).from_buffer_copy(desc)
        low.camera = F.jittered_camera(desc.camera, *sup.offset(s, i), p.time_start)
        ctx.upload_world(low)
        d_film = F.alloc_device_film(w, h, "cuda")
        ctx.render_device(p, [torch.from_numpy(t).cuda() for t in R.build_tables(4, 2, 2, frame, w, h, filt)], d_film)
        ctx.gbuffer(p, g_low)
        ctx.upload_world(desc)
        ctx.gbuffer(F._scaled_params(p, s), g_high)
        d_out = F.alloc_device_film(W, H, "cuda")
        ctx.temporal_upscale(p, up, tp, sup, d_film, g_low, g_high, None if i == 0 else hist[(i + 1) % 2], None if i == 0 else desc.camera,
                             0.0 if i == 0 else prev_start, hist[i % 2], d_out, low.camera)
        prev_start = p.time_start
        for kind, sfx in zip(_kinds(), ("color_temporal", "alpha", "background", "normal")):
            img = torch.empty(H * W * F.save_to_bpp(kind, mask), dtype=torch.uint8, device="cuda")
            ctx.save_to_pixels(kind, mask, False, W, H, d_out, img)
            image.save(str(tmp_path / "one.png"), img.cpu().numpy().reshape(H, W, -1))
            assert open(tmp_path / "one.png", "rb").read() == got[f"anim_{frame:04d}_{sfx}_x2.png"], (frame, sfx)
        d_dn = torch.empty(W * H, 3, dtype=torch.float32, device="cuda")
        ctx.denoise(W, H, d_out, d_dn, dn)
        img = torch.empty(H * W * 3, dtype=torch.uint8, device="cuda")
        ctx.display(disp, mask, False, W, H, dict(d_out, color=d_dn), img, d_state, None, 1.0 if shown_start is None else disp.adapt(float(start) - float(shown_start)))
        shown_start = start
        image.save(str(tmp_path / "one.png"), img.cpu().numpy().reshape(H, W, 3))
        assert open(tmp_path / "one.png", "rb").read() == got2[f"anim_{frame:04d}_color_temporal_denoised_display_x2.png"], frame
    # the uploaded world is the frame's own again
    assert bytes(memoryview(desc).cast("B")) == bytes(memoryview(world.to_desc(cam)).cast("B"))


def test_render_sequence_without_jitter_and_confidence_is_the_composition(tmp_path):
    """Supersample(jitter=False, confidence=False): the images equal Film.upscaled -> Context.temporal_accumulate at the high size ->
    save_to, frame by frame; and they differ from the jittered default's from the second frame on."""
    import torch
    import rayn_amd as R
    from rayn_amd import film as F
    from rayn_amd import setup as S
    K = R.ChannelKind
    w, h, s = 24, 16, 2
    W, H = w * s, h * s
    frames, rate, shutter = [3, 4, 7], 24, 1.0 / 24.0
    cam, world = S.setup_s3((w, h))
    integ, filt = R.PathTracingIntegrator(max_bounces=2, volume_marches=2), R.BlackmanHarrisFilter(1.5)
    up, tp = R.Upscale(s, 0.02, 0.05), R.Temporal()
    film = R.Film(_kinds(), (w, h))
    film.render_sequence(world, cam, integ, filt, (16, 16), frames, rate, shutter, 1, _kinds(), str(tmp_path / "seq"), "anim", upscale=up, temporal=tp,
                         supersample=R.Supersample(jitter=False, confidence=False))
    film.render_sequence(world, cam, integ, filt, (16, 16), frames, rate, shutter, 1, [K.Color], str(tmp_path / "jit"), "anim", upscale=up, temporal=tp,
                         supersample=R.Supersample(jitter=True, confidence=True))
    got, jit = IO.read_folder(tmp_path / "seq"), IO.read_folder(tmp_path / "jit")
    plain = R.Film(_kinds(), (w, h))
    desc = world.to_desc(cam)
    hist = [torch.empty(F.temporal_history_bytes(W, H), dtype=torch.uint8, device="cuda") for _ in range(2)]
    prev_start = None
    for i, frame in enumerate(frames):
        plain.render_frame_into(world, cam, integ, filt, (16, 16), frame, IO.shutter_range(frame, rate, shutter), 1)
        hi = plain.upscaled(up)
        g = F.alloc_gbuffer(W, H, "cuda")
        hi.ctx.gbuffer(hi._last_params, g)
        acc = torch.empty(W * H, 3, dtype=torch.float32, device="cuda")
        hi.ctx.temporal_accumulate(hi._last_params, tp, hi.channels, g, None if i == 0 else hist[(i + 1) % 2], None if i == 0 else desc.camera,
                                   0.0 if i == 0 else prev_start, hist[i % 2], acc)
        prev_start = hi._last_params.time_start
        hi.channels = dict(hi.channels, color=acc)
        hi.save_to(_kinds(), str(tmp_path / "loop"), f"anim_{frame:04d}")
        for sfx, name in (("color", "color_temporal"), ("alpha", "alpha"), ("background", "background"), ("normal", "normal")):
            assert (tmp_path / "loop" / f"anim_{frame:04d}_{sfx}.png").read_bytes() == got[f"anim_{frame:04d}_{name}_x2.png"], (frame, sfx)
    assert jit["anim_0007_color_temporal_x2.png"] != got["anim_0007_color_temporal_x2.png"]
