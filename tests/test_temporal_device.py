"""rayn_hip_gbuffer_device and rayn_hip_temporal_accumulate_device (rayn_amd/csrc/temporal.hip) on the GPU: the G-buffer bit for bit against
the CPU oracle's camera and closest hit, the accumulate kernel bit for bit against its numpy restatement (tests/temporal_np.py) on synthetic,
adversarial and rendered inputs, Film.render_sequence(temporal=...) against the plain loop of the same entries, input hygiene and error
texts, and the benefit of the defaults on the shipped scene under a moving camera."""
import ctypes as C
import os

import numpy as np
import pytest

import device_io as IO
import scenes
import temporal_cases as TC
import temporal_np as T
from common import bits_equal
from device_io import module_context as ctx  # noqa: F401
from temporal_cases import SIZES

pytestmark = pytest.mark.gpu

f32 = np.float32


def _gpu_accumulate(ctx, p, temporal, color, normal, rec, obj, prev, prev_cam, prev_time):
    """The plain entry through Context.temporal_accumulate on host arrays: (out colour (n, 3), (A, B, N, O)), with temporal_cases' checks"""
    return TC.gpu_accumulate(ctx, p, temporal, color, normal, rec, obj, prev, None, prev_cam, prev_time, moments=False)[:2]


def _same(got, want, what):
    out_g, hist_g = got
    out_w, hist_w = want
    IO.assert_bits_equal(out_g, out_w, (what, "colour"))
    TC.assert_history_equal(hist_g, hist_w, what)


# ---- 1. the G-buffer against the oracle --------------------------------------------------------------------------------------------------

def _check_gbuffer(ctx, oracle, wd, p, fma, what):
    ctx.upload_world(wd)
    _, rec, obj = IO.gpu_gbuffer(ctx, p)
    want_rec, want_obj = T.gbuffer_oracle(oracle, wd, p, fma=fma)
    assert np.array_equal(obj, want_obj), (what, int((obj != want_obj).sum()))
    assert bits_equal(rec, want_rec), (what, int((rec.view(np.uint32) != want_rec.view(np.uint32)).sum()))
    hit = want_obj != T.MISS
    assert hit.any() and np.all(np.isposinf(rec[~hit, 3])) and not np.any(rec[~hit, :3])
    return want_obj


@pytest.mark.parametrize("fma", [0, 1])
def test_gbuffer_is_the_oracles_closest_hit_at_the_pixel_centres(ctx, oracle, fma):
    """Three camera kinds x four scenes over the three film sizes, under both mul_add policies; the shipped world radius makes the sky dome
    a hit, so a smaller one supplies the misses."""
    import rayn_amd as R
    ctx.set_fma_policy(fma)
    try:
        seen = set()
        for i, (scene, camera) in enumerate([("s0", "pinhole"), ("s1", "thin"), ("bulb", "ortho"), ("multi", "pinhole"), ("s1", "ortho"), ("bulb", "thin")]):
            w, h = SIZES[i % 3]
            wd, _, _ = scenes.scene(scene, (w, h), camera)
            p = R.frame_params(w, h, 2, 3)
            seen |= set(_check_gbuffer(ctx, oracle, wd, p, bool(fma), (scene, camera, w, h)).tolist())
        assert len(seen) >= 4
        # misses: without the sky dome (hitable 0 swapped for a small sphere far away) most centre rays hit nothing
        wd, _, _ = scenes.scene("s1", (40, 24))
        wd.hitables[0].radius = 0.05
        wd.hitables[0].center.x = 50.0
        objs = _check_gbuffer(ctx, oracle, wd, R.frame_params(40, 24, 2, 3), bool(fma), "misses")
        assert (objs == T.MISS).sum() > 100
    finally:
        ctx.set_fma_policy(0)


def test_gbuffer_evaluates_animated_hitables_at_time_start(ctx, oracle):
    """A moving camera, a moving fractal and a moving sphere: at time_start = 0 the oracle's probe (ray time 0) is the reference directly; at
    time_start != 0 it is the oracle on the world frozen at that time in f32 (temporal_np.frozen_world)."""
    import rayn_amd as R
    wd, _, _ = scenes.scene("s1", (40, 24), moving=True)
    assert sum(wd.hitables[i].animated for i in range(wd.n_hitables)) == 2 and wd.camera.animated == 3
    for time_range in ((0.0, 1.0 / 24.0), (0.375, 0.4), (-1.25, -1.0)):
        p = R.frame_params(40, 24, 2, 3, time_range=time_range)
        _check_gbuffer(ctx, oracle, wd, p, False, time_range)
    p0 = R.frame_params(40, 24, 2, 3, time_range=(0.0, 0.1))
    org, dirs = T.pixel_centre_rays(oracle, wd, p0)
    t, obj = oracle.closest_hit(wd, p0, 0, org, dirs)  # the unfrozen world
    want_rec, want_obj = T.gbuffer_assemble(org, dirs, t, obj)
    ctx.upload_world(wd)
    _, rec, got_obj = IO.gpu_gbuffer(ctx, p0)
    assert np.array_equal(got_obj, want_obj) and bits_equal(rec, want_rec)


def test_film_gbuffer_after_a_render(oracle):
    import rayn_amd as R
    from rayn_amd import setup as S
    K = R.ChannelKind
    w, h = 40, 24
    _, world, cam = scenes.scene("s1", (w, h))
    film = R.Film([K.Color, K.Alpha, K.Background, K.WorldNormal], (w, h))
    with pytest.raises(ValueError, match="no rendered frame"):
        film.gbuffer()
    film.render_frame_into(world, cam, R.PathTracingIntegrator(max_bounces=2, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE), R.BlackmanHarrisFilter(S.FILTER_RADIUS),
                           S.TILE_SIZE, 3, None, 1)
    g = film.gbuffer()
    rec, obj = T.gbuffer_oracle(oracle, world.to_desc(cam), R.frame_params(w, h, 1, 2, frame=3))
    assert g["position"].shape == (h, w, 3) and g["t"].shape == (h, w) and g["object"].dtype == np.uint32
    assert bits_equal(g["position"], rec[:, :3].reshape(h, w, 3)) and bits_equal(g["t"], rec[:, 3].reshape(h, w)) and np.array_equal(g["object"].reshape(-1), obj)


# ---- 2. the accumulate kernel against the restatement ------------------------------------------------------------------------------------

@pytest.mark.parametrize("cam_kind", [0, 1, 2])
def test_accumulate_matches_the_restatement_on_adversarial_inputs(ctx, cam_kind):
    """Random and adversarial frames and histories (NaN and inf colours, positions, depths and history lengths, t = +inf, misses) under
    cameras that have translated and rotated so that taps straddle every image border, for every film size, with max_history 1, a history at
    the cap, and each test on and off."""
    # temporal_cases.older_accumulate_calls copies this loop (what these inputs can see is measured in tests/test_reproject_cases.py): change both
    import rayn_amd as R
    wd, _, _ = scenes.scene("s1", (40, 24), moving=True)  # hitables 1 (the fractal) and one sphere are animated: object motion is exercised too
    ctx.upload_world(wd)
    hit = T.world_hitables(wd)
    params = [R.Temporal(4, 0.05, -1.0), R.Temporal(1, 0.05, 0.9), R.Temporal(8, 0.0, 0.5), R.Temporal(3, 1e30, 1.0), R.Temporal(65536, 0.25, -1.0)]
    for si, (w, h) in enumerate(SIZES + [(1, 1), (17, 13)]):
        for adversarial in (False, True):
            cur, prev_cam, color, normal, rec, obj, prev = TC.random_inputs(w, h, 10 * si + adversarial, cam_kind, adversarial)
            p = R.frame_params(w, h, 1, 1, time_range=(0.75, 0.8))
            for tp in params[(si + adversarial) % 2::2] if w > 17 else params:
                want = T.accumulate(w, h, color, normal, rec, obj, prev, prev_cam, 0.25, 0.75, hit, tp.max_history, tp.depth_tolerance, tp.normal_min)
                got = _gpu_accumulate(ctx, p, tp, color, normal, rec, obj, prev, prev_cam, 0.25)
                _same(got, want, (w, h, adversarial, tp))
            if not adversarial and w > 17:  # the case has substance: pixels that blend and pixels that reset
                n1 = T.accumulate(w, h, color, normal, rec, obj, prev, prev_cam, 0.25, 0.75, hit, 4, 0.25, -1.0)[1][0][:, 3]
                assert (n1 > 1).sum() > w * h // 20 and (n1 == 1).sum() > w * h // 20
            # no previous history: every pixel passes through
            want = T.accumulate(w, h, color, normal, rec, obj, None, None, 0.0, 0.75, hit, 4, 0.05, -1.0)
            _same(_gpu_accumulate(ctx, p, params[0], color, normal, rec, obj, None, None, 0.0), want, (w, h, "no history"))


def test_accumulate_on_exactly_integral_reprojections(ctx):
    """The exact orthographic case: fx and fy are integers, so one tap has weight 1 and three have weight 0 (they still count: 0 * c_tap);
    camera shifts by whole and quarter pixels across all four borders; a history that has reached the cap stays there."""
    # temporal_cases.older_accumulate_calls copies this loop as well: change both
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
        color = rng.random((w * h, 3)).astype(f32)
        want = T.accumulate(w, h, color, normal, rec, obj, prev, prev_cam, 0.0, 0.0, [], 3, 0.05, 0.9)
        _same(_gpu_accumulate(ctx, p, tp, color, normal, rec, obj, prev, prev_cam, 0.0), want, (sx, sy))
        n1 = want[1][0][:, 3].reshape(h, w)
        assert set(np.unique(n1).tolist()) <= {1.0, 3.0} and ((n1 == 3.0).any() or abs(sx) >= w)


def test_accumulate_on_a_rendered_sequence_with_a_moving_camera_and_a_moving_sphere(ctx):
    """Three rendered frames (GPU film, GPU G-buffer) of a scene whose camera, fractal and one sphere move: the kernel's histories and
    colours equal the restatement's, frame by frame, each fed the other's previous history."""
    import rayn_amd as R
    w, h = 40, 24
    wd, _, _ = scenes.scene("s1", (w, h), moving=True)
    ps = [R.frame_params(w, h, 1, 2, frame=f) for f in (1, 2, 4)]
    frames = IO.render_frames(ctx, wd, ps, 2)
    tp = R.Temporal(8, 0.05, 0.3)
    prev, prev_time, blended = None, 0.0, 0
    for p, film in zip(ps, frames):
        _, rec, obj = IO.gpu_gbuffer(ctx, p)
        color, normal = film["color"].cpu().numpy(), film["normal"].cpu().numpy()
        want = T.accumulate(w, h, color, normal, rec, obj, prev, wd.camera, prev_time, p.time_start, T.world_hitables(wd), tp.max_history, tp.depth_tolerance, tp.normal_min)
        got = _gpu_accumulate(ctx, p, tp, color, normal, rec, obj, prev, None if prev is None else wd.camera, prev_time)
        _same(got, want, p.frame)
        prev, prev_time = got[1], p.time_start
        blended = int((prev[0][:, 3] > 1).sum())
    assert blended > w * h // 4 and prev[0][:, 3].max() == 3.0


# ---- 3. the sequence wiring -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_denoise", [False, True])
def test_render_sequence_with_temporal_is_the_plain_loop_of_the_entries(tmp_path, with_denoise):
    """render_sequence(temporal=...) writes the bytes a Python loop of render_device, gbuffer, temporal_accumulate (and denoise),
    save_to_pixels produces - frames that are not consecutive included; the other channels' files are those of the plain sequence."""
    import torch
    import rayn_amd as R
    from rayn_amd import film as F
    from rayn_amd import image
    from rayn_amd import setup as S
    K = R.ChannelKind
    w, h, frames, samples = 50, 37, [2, 3, 7], 1
    _, world, cam = scenes.scene("s1", (w, h), moving=True)
    integ = R.PathTracingIntegrator(max_bounces=2, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE)
    filt = R.BlackmanHarrisFilter(S.FILTER_RADIUS)
    kinds = [K.Color, K.Alpha, K.Background, K.WorldNormal]
    tp, dn = R.Temporal(), (R.Denoise(2, 0.5, 0.4, 0.3) if with_denoise else None)
    film = R.Film(kinds, (w, h))
    film.render_sequence(world, cam, integ, filt, S.TILE_SIZE, frames, 24, 1.0 / 24.0, samples, [K.Color, K.WorldNormal], str(tmp_path / "seq"), "a",
                         denoise=dn, temporal=tp)
    got = IO.read_folder(tmp_path / "seq")
    suffix = "color_temporal_denoised" if with_denoise else "color_temporal"
    assert sorted(got) == sorted(f"a_{f:04d}_{s}.png" for f in frames for s in (suffix, "normal"))
    # the loop
    ctx = film.ctx
    desc = world.to_desc(cam)
    ctx.upload_world(desc)
    mask = film.have_mask()
    hist = [torch.empty(F.temporal_history_bytes(w, h), dtype=torch.uint8, device="cuda") for _ in range(2)]
    g, acc, prev_start = F.alloc_gbuffer(w, h, "cuda"), torch.empty(w * h, 3, dtype=torch.float32, device="cuda"), None
    img = torch.empty(h * w * 3, dtype=torch.uint8, device="cuda")
    for i, frame in enumerate(frames):
        p, out = IO.render_sequence_frame(ctx, w, h, frame, samples, 2, filt)
        ctx.gbuffer(p, g)
        ctx.temporal_accumulate(p, tp, out, g, None if i == 0 else hist[(i + 1) % 2], None if i == 0 else desc.camera, 0.0 if i == 0 else prev_start,
                                hist[i % 2], acc)
        prev_start = p.time_start
        shown = acc
        if with_denoise:
            shown = torch.empty_like(acc)
            ctx.denoise(w, h, dict(out, color=acc), shown, dn)
        ctx.save_to_pixels(K.Color, mask, False, w, h, dict(out, color=shown), img)
        image.save(str(tmp_path / "one.png"), img.cpu().numpy().reshape(h, w, 3))
        assert open(tmp_path / "one.png", "rb").read() == got[f"a_{frame:04d}_{suffix}.png"], frame
    # the accumulation changed the picture, and only the Color one
    plain = R.Film(kinds, (w, h))
    plain.render_sequence(world, cam, integ, filt, S.TILE_SIZE, frames, 24, 1.0 / 24.0, samples, [K.Color, K.WorldNormal], str(tmp_path / "plain"), "a", denoise=dn)
    base = IO.read_folder(tmp_path / "plain")
    plain_suffix = "color_denoised" if with_denoise else "color"
    assert got[f"a_0002_{suffix}.png"] == base[f"a_0002_{plain_suffix}.png"]  # the first frame has no history
    assert got[f"a_0007_{suffix}.png"] != base[f"a_0007_{plain_suffix}.png"]
    assert all(got[f"a_{f:04d}_normal.png"] == base[f"a_{f:04d}_normal.png"] for f in frames)


def test_render_sequence_without_temporal_is_unchanged(tmp_path):
    """temporal=None (and a sequence that does not write Color) writes the files and bytes of render_frame_into + save_to, frame by frame."""
    import rayn_amd as R
    from rayn_amd import setup as S
    K = R.ChannelKind
    w, h, frames = 40, 24, [1, 2]
    _, world, cam = scenes.scene("s1", (w, h), moving=True)
    integ = R.PathTracingIntegrator(max_bounces=2, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE)
    filt = R.BlackmanHarrisFilter(S.FILTER_RADIUS)
    kinds = [K.Color, K.Alpha, K.Background, K.WorldNormal]
    film = R.Film(kinds, (w, h))
    film.render_sequence(world, cam, integ, filt, S.TILE_SIZE, frames, 24, 1.0 / 24.0, 1, [K.Color, K.Alpha], str(tmp_path / "none"), "a", temporal=None)
    film.render_sequence(world, cam, integ, filt, S.TILE_SIZE, frames, 24, 1.0 / 24.0, 1, [K.Alpha], str(tmp_path / "alpha"), "a", temporal=R.Temporal())
    one = R.Film(kinds, (w, h))
    for frame in frames:
        one.render_frame_into(world, cam, integ, filt, S.TILE_SIZE, frame, IO.shutter_range(frame), 1)
        one.save_to([K.Color, K.Alpha], str(tmp_path / "loop"), f"a_{frame:04d}")
    want = IO.read_folder(tmp_path / "loop")
    assert IO.read_folder(tmp_path / "none") == want
    assert IO.read_folder(tmp_path / "alpha") == {k: v for k, v in want.items() if k.endswith("_alpha.png")}
    no_normal = R.Film([K.Color, K.Alpha, K.Background], (w, h))
    with pytest.raises(ValueError, match="WorldNormal"):
        no_normal.render_sequence(world, cam, integ, filt, S.TILE_SIZE, frames, 24, 1.0 / 24.0, 1, [K.Color], str(tmp_path / "x"), "a", temporal=R.Temporal())
    with pytest.raises(ValueError, match="Temporal"):
        film.render_sequence(world, cam, integ, filt, S.TILE_SIZE, frames, 24, 1.0 / 24.0, 1, [K.Color], str(tmp_path / "x"), "a", temporal=4)
    assert not os.path.exists(tmp_path / "x")


# ---- 4. input hygiene ------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_invalid_arg_with_a_text(ctx):
    import torch
    import rayn_amd as R
    from rayn_amd import _abi
    from rayn_amd import film as F
    L = ctx._L
    w, h, n = 40, 24, 40 * 24
    wd, _, _ = scenes.scene("s0", (w, h))
    fresh = R.Context(0)
    p = R.frame_params(w, h, 1, 1)
    vp = lambda t: C.c_void_p(t.data_ptr())
    rec, obj = torch.zeros(4 * n + 4, dtype=torch.float32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(F.gbuffer_scratch_bytes(w, h) + 16, dtype=torch.uint8, device="cuda")
    sb = F.gbuffer_scratch_bytes(w, h)

    def gb(c=ctx, p=p, rec=vp(rec), obj=vp(obj), scratch=vp(scratch), sb=sb):
        rc = L.rayn_hip_gbuffer_device(c.h, None if p is None else C.byref(p), rec, obj, scratch, sb, None)
        return rc, c.last_error()

    try:
        assert gb(c=fresh) == (-1, "rayn_hip_upload_world has not been called")
    finally:
        fresh.close()
    ctx.upload_world(wd)
    assert gb()[0] == 0
    zero, huge = R.frame_params(0, h, 1, 1), R.frame_params(65536, 32768, 1, 1)
    for kw, text in ((dict(p=None), "null frame params"), (dict(p=zero), "zero-sized"), (dict(p=huge), "2^31"), (dict(rec=None), "null buffer"),
                     (dict(obj=None), "null buffer"), (dict(scratch=None), "null buffer"), (dict(sb=sb - 1), "scratch smaller"),
                     (dict(scratch=C.c_void_p(scratch.data_ptr() + 4)), "16-byte aligned"), (dict(rec=C.c_void_p(rec.data_ptr() + 4)), "16-byte aligned"),
                     (dict(rec=vp(scratch)), "overlap")):
        rc, err = gb(**kw)
        assert rc == -1 and text in err, (kw, rc, err)

    color, normal = torch.zeros(3 * n, dtype=torch.float32, device="cuda"), torch.zeros(3 * n, dtype=torch.float32, device="cuda")
    out = torch.zeros(3 * n, dtype=torch.float32, device="cuda")
    hb = F.temporal_history_bytes(w, h)
    h0, h1 = torch.zeros(hb + 16, dtype=torch.uint8, device="cuda"), torch.zeros(hb + 16, dtype=torch.uint8, device="cuda")
    cam = wd.camera
    bad_cam = _abi.Camera.from_buffer_copy(cam)
    bad_cam.kind = 9

    def acc(p=p, tp=R.Temporal().to_abi(), cam=cam, color=vp(color), normal=vp(normal), rec=vp(rec), obj=vp(obj), prev=vp(h0), new=vp(h1), hb=hb, out=vp(out)):
        rc = L.rayn_hip_temporal_accumulate_device(ctx.h, None if p is None else C.byref(p), None if tp is None else C.byref(tp), None if cam is None else C.byref(cam),
                                                   0.0, color, normal, rec, obj, prev, new, hb, out, None)
        return rc, ctx.last_error()

    assert acc()[0] == 0 and acc(prev=None, cam=None)[0] == 0
    T_ = _abi.TemporalParams
    nan, inf = float("nan"), float("inf")
    for kw, text in ((dict(p=None), "null frame params"), (dict(p=zero), "zero-sized"), (dict(p=huge), "2^31"), (dict(tp=None), "null temporal params"),
                     (dict(tp=T_(0, 0.05, 0.9)), "max_history"), (dict(tp=T_(65537, 0.05, 0.9)), "max_history"), (dict(tp=T_(4, -0.1, 0.9)), "depth_tolerance"),
                     (dict(tp=T_(4, inf, 0.9)), "depth_tolerance"), (dict(tp=T_(4, nan, 0.9)), "depth_tolerance"), (dict(tp=T_(4, 0.05, -1.5)), "normal_min"),
                     (dict(tp=T_(4, 0.05, 1.5)), "normal_min"), (dict(tp=T_(4, 0.05, nan)), "normal_min"), (dict(color=None), "null buffer"),
                     (dict(normal=None), "null buffer"), (dict(rec=None), "null buffer"), (dict(obj=None), "null buffer"), (dict(new=None), "null buffer"),
                     (dict(out=None), "null buffer"), (dict(cam=None), "previous camera"), (dict(cam=bad_cam), "unknown camera kind"), (dict(hb=hb - 1), "history smaller"),
                     (dict(new=C.c_void_p(h1.data_ptr() + 4)), "16-byte aligned"), (dict(prev=C.c_void_p(h0.data_ptr() + 8)), "16-byte aligned"),
                     (dict(rec=C.c_void_p(rec.data_ptr() + 4)), "16-byte aligned"), (dict(new=vp(h0)), "alias the previous"),
                     (dict(new=C.c_void_p(h0.data_ptr() + 16)), "alias the previous"), (dict(out=vp(color)), "alias an input"), (dict(out=vp(normal)), "alias an input"),
                     (dict(out=vp(rec)), "alias an input"), (dict(out=vp(h0)), "alias an input"), (dict(new=vp(color), hb=0), "history smaller"),
                     (dict(out=vp(h1)), "alias the new history")):
        rc, err = acc(**kw)
        assert rc == -1 and text in err, (kw, rc, err)
    torch.cuda.synchronize()


# ---- 5. does it do its job ---------------------------------------------------------------------------------------------------------------

# temporal / raw MSE of the last frame with Temporal()'s defaults, computed with the CPU oracle and the numpy restatement
# (tools/temporal_defaults.py --defaults) - the path the tests above hold the GPU to bit for bit
MEASURED_RATIO = 0.4940


def test_temporal_accumulation_lowers_the_error_of_a_moving_camera_sequence(tmp_path):
    """The shipped scene at 160x96 under a camera whose origin moves, 8 frames at samples=2: the MSE of the saturated Color + Background of
    the temporally accumulated last frame against a samples=256 render of it, relative to the raw last frame's, is below 1 and reaches the
    ratio measured on the CPU path (times 1.05: the GPU path is bit-identical to it; the 5 % only absorbs a later change of defaults)."""
    import rayn_amd as R
    raw, temporal, _ = TC.defaults_case_errors(R.Temporal(), moments=False)
    print(f"MSE raw {raw:.4e}, temporal {temporal:.4e}, ratio {temporal / raw:.4f}x (CPU path: {MEASURED_RATIO}x)")
    assert temporal / raw < 1.0
    assert temporal / raw < MEASURED_RATIO * 1.05, (raw, temporal)
