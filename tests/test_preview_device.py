"""rayn_hip_preview_device (rayn_amd/csrc/preview.hip) on the GPU: colour, alpha, normal, ao, records and objects bit for bit against the numpy
restatement (tests/preview_np.py) over the scenes of the G-buffer tests - spheres only (no march), the shipped MandelBox (k_shadow1), a
Mandelbulb (k_shadow_bulb), two SDFs (the generic k_shadow), moving hitables at time_start != 0 - the three cameras, both mul_add policies,
K in {1, 4, 8, 64}, a size that is no multiple of 64, and without scramble and optional outputs; the records and objects against
rayn_hip_gbuffer_device; Film.render_preview and render_sequence(preview=...) against a loop of the entries; error texts."""
import ctypes as C
import os

import numpy as np
import pytest

import device_io as IO
import preview_np as PN
from common import bits_equal
from device_io import module_context as ctx  # noqa: F401

pytestmark = pytest.mark.gpu

f32 = np.float32
GUARD = 64


def _gpu_preview(ctx, wd, p, preview, samples, scramble, optional):
    """The entry through Context.preview with guard elements behind every output -> dict of host arrays (ao, records, object: None without
    the optional outputs)."""
    import torch
    from rayn_amd import film as F
    n = p.width * p.height
    ctx.upload_world(wd)
    sizes = {"color": 3 * n, "alpha": n, "normal": 3 * n}
    full = {k: IO.guarded(size, torch.float32, 7.0, GUARD) for k, size in sizes.items()}
    if optional:
        full.update(ao=IO.guarded(n, torch.float32, 7.0, GUARD), records=IO.guarded(4 * n, torch.float32, 7.0, GUARD), object=IO.guarded(n, torch.int32, 7, GUARD))
    # the entry is handed the whole buffers: it takes their sizes from the frame parameters
    d_out = {k: full[k][0] for k in sizes}
    d_ao = full["ao"][0] if optional else None
    g = {"records": full["records"][0], "object": full["object"][0]} if optional else None
    nb = F.preview_scratch_bytes(p.width, p.height, preview.samples)
    full_scratch, d_scratch = IO.guarded(nb, torch.uint8, 0xA5, GUARD)
    d_samples = torch.from_numpy(np.ascontiguousarray(samples, f32)).cuda()
    d_scramble = None if scramble is None else torch.from_numpy(np.ascontiguousarray(scramble, f32)).cuda()
    ctx.preview(p, preview, d_samples, d_out, d_scramble, d_ao, g, d_scratch)
    torch.cuda.synchronize()
    for k, (whole, view) in full.items():
        IO.assert_guards(whole, view.numel(), 7 if k == "object" else 7.0, k)
    IO.assert_guards(full_scratch, nb, 0xA5, "scratch")
    got = {k: full[k][1].cpu().numpy() if k in full else None for k in ("color", "alpha", "normal", "ao", "records", "object")}
    got["color"], got["normal"] = got["color"].reshape(n, 3), got["normal"].reshape(n, 3)
    if optional:
        got["records"], got["object"] = got["records"].reshape(n, 4), got["object"].view(np.uint32)
    return got


def _compare(got, ref, what):
    for k in ("color", "alpha", "normal", "ao", "records"):
        if got[k] is not None:
            IO.assert_bits_equal(got[k], ref[k], (what, k))
    if got["object"] is not None:
        assert np.array_equal(got["object"], ref["object"]), (what, "object")


@pytest.mark.parametrize("case", PN.CASES, ids=[c[0] for c in PN.CASES])
def test_preview_is_the_restatement_bit_for_bit(ctx, oracle, case):
    """Every output of the entry against tests/preview_np.py, after the coverage conditions have been checked on the restatement alone; with
    the optional outputs, the records and objects also against rayn_hip_gbuffer_device on the same frame parameters."""
    import torch
    import rayn_amd as R
    from rayn_amd import film as F
    name, scene, _, _, (w, h), K, fma, radius, _, _, optional = case
    ref = PN.case_reference(oracle, case)
    PN.check_coverage(ref, scene != "spheres")  # the spheres-only scene has no TracedSDF: the two conditions about SDF scenes do not apply
    wd, p, samples, scramble = PN.case_inputs(case)
    ctx.set_fma_policy(fma)
    try:
        got = _gpu_preview(ctx, wd, p, R.Preview(K, radius, PN.AMBIENT), samples, scramble, optional)
        _compare(got, ref, name)
        if optional:
            g = F.alloc_gbuffer(w, h, "cuda")
            ctx.gbuffer(p, g)
            torch.cuda.synchronize()
            assert bits_equal(g["records"].cpu().numpy().reshape(-1, 4), got["records"]) and np.array_equal(g["object"].cpu().numpy().view(np.uint32), got["object"]), name
    finally:
        ctx.set_fma_policy(0)


def test_rounds_do_not_change_the_count(ctx, oracle):
    """K = 64 runs in eight rounds of eight rays: a second call repeats the first bit for bit (the job list's order, which differs from run
    to run, does not reach the result), and K = 8 on the first eight pairs of the same table - its first round alone - is the restatement's."""
    import rayn_amd as R
    case = next(c for c in PN.CASES if c[5] == 64)
    wd, p, samples, scramble = PN.case_inputs(case)
    a = _gpu_preview(ctx, wd, p, R.Preview(64, case[7], PN.AMBIENT), samples, scramble, True)
    b = _gpu_preview(ctx, wd, p, R.Preview(64, case[7], PN.AMBIENT), samples, scramble, True)
    _compare(a, b, "repeat")
    first = PN.preview(oracle, wd, p, samples[:8], scramble, case[7], PN.AMBIENT)
    _compare(_gpu_preview(ctx, wd, p, R.Preview(8, case[7], PN.AMBIENT), samples[:8], scramble, True), first, "first round")


def _host_pixels(ref, kind, w, h):
    """save_to's host arm (rayn_amd.image) on the restatement's planes of a [Color, Alpha, WorldNormal] film"""
    import rayn_amd as R
    from rayn_amd import image
    K = R.ChannelKind
    if kind == K.Color:
        return image.color_image(ref["color"].reshape(h, w, 3))
    if kind == K.Alpha:
        return image.alpha_image(ref["alpha"].reshape(h, w))
    return image.normal_image(ref["normal"].reshape(h, w, 3))


def test_film_render_preview(oracle, tmp_path):
    """Film.render_preview(...).pixels() is save_to's host arm on the restatement's planes; the new film's gbuffer() is the preview's own,
    save_to, save_hdr, denoise= and display= run on it, and a preview of the last rendered frame needs no world."""
    import rayn_amd as R
    from rayn_amd import film as F
    from rayn_amd import image
    K = R.ChannelKind
    w, h, frame = 40, 24, 5
    wd, world, cam = PN.scene("s1", (w, h))
    pv = R.Preview(4, 0.3, 0.25)
    film = R.Film([K.Color, K.Alpha, K.Background, K.WorldNormal], (w, h))
    with pytest.raises(ValueError, match="no rendered frame"):
        film.render_preview(pv)
    out = film.render_preview(pv, frame=frame, world=world, camera=cam)
    p = R.frame_params(w, h, 1, 0, frame=frame)
    samples, scramble = F.preview_tables(4, frame, w, h)
    ref = PN.preview(oracle, wd, p, samples, scramble, 0.3, 0.25)
    PN.check_coverage(ref, True)
    assert out.res == (w, h) and out.channel_kinds == [K.Color, K.Alpha, K.WorldNormal] and film.channels is None
    for kind in out.channel_kinds:
        assert np.array_equal(out.pixels(kind), _host_pixels(ref, kind, w, h)), kind
    assert bits_equal(out.ao.cpu().numpy(), ref["ao"])
    g = out.gbuffer()
    assert bits_equal(g["position"].reshape(-1, 3), ref["records"][:, :3]) and bits_equal(g["t"].reshape(-1), ref["records"][:, 3])
    assert np.array_equal(g["object"].reshape(-1), ref["object"])
    out.save_to([K.Color, K.Alpha, K.WorldNormal], str(tmp_path), "pv")
    out.save_to([K.Color], str(tmp_path), "pv", denoise=R.Denoise(1, 0.5, 0.4, 0.3), display=R.Display(exposure=0.0, tone="linear"))
    out.save_hdr(str(tmp_path / "pv.pfm"))
    assert sorted(os.listdir(tmp_path)) == ["pv.pfm", "pv_alpha.png", "pv_color.png", "pv_color_denoised_display.png", "pv_normal.png"]
    image.save(str(tmp_path / "want.png"), _host_pixels(ref, K.Color, w, h))
    assert open(tmp_path / "want.png", "rb").read() == open(tmp_path / "pv_color.png", "rb").read()
    assert bits_equal(image.load_pfm(str(tmp_path / "pv.pfm")), ref["color"].reshape(h, w, 3))
    # the identity display on the film itself is save_to's image
    assert np.array_equal(out.pixels(K.Color, display=R.Display(exposure=0.0, tone="linear")), _host_pixels(ref, K.Color, w, h))
    # a preview of a rendered frame: its world, its parameters; another frame number gives other directions
    film.render_frame_into(world, cam, R.PathTracingIntegrator(max_bounces=1, volume_marches=2), R.BlackmanHarrisFilter(1.5), (16, 16), frame, None, 1)
    again = film.render_preview(pv)
    assert np.array_equal(again.pixels(K.Color), out.pixels(K.Color)) and film.channels is not None
    assert not np.array_equal(film.render_preview(pv, frame=frame + 1).pixels(K.Color), out.pixels(K.Color))


def test_render_sequence_with_preview_is_the_plain_loop_of_the_entries(tmp_path):
    """render_sequence(preview=...) over 3 frames with temporal=, denoise= and display= writes the bytes of a loop of Context.preview (into
    the temporal stage's G-buffer), temporal_accumulate, denoise, display and save_to_pixels; the other channels' files are the preview's."""
    import torch
    import rayn_amd as R
    from rayn_amd import film as F
    from rayn_amd import image
    K = R.ChannelKind
    w, h, frames = 37, 23, [2, 3, 7]
    _, world, cam = PN.scene("s1", (w, h), moving=True)
    pv, tp, dn, dsp = R.Preview(4, 0.3, 0.3), R.Temporal(), R.Denoise(2, 0.5, 0.4, 0.3), R.Display(exposure=0.5, tone="reinhard")
    kinds = [K.Color, K.Alpha, K.Background, K.WorldNormal]
    film = R.Film(kinds, (w, h))
    stats = film.render_sequence(world, cam, None, None, (16, 16), frames, 24, 1.0 / 24.0, 1, [K.Color, K.Alpha, K.WorldNormal], str(tmp_path / "seq"), "a",
                                 denoise=dn, display=dsp, preview=pv, temporal=tp)
    film.render_sequence(world, cam, None, None, (16, 16), frames, 24, 1.0 / 24.0, 1, [K.Color], str(tmp_path / "bare"), "a", preview=pv)
    assert stats == [{"frame": f} for f in frames]
    got, bare = IO.read_folder(tmp_path / "seq"), IO.read_folder(tmp_path / "bare")
    suffix = "color_preview_temporal_denoised_display"
    assert sorted(got) == sorted(f"a_{f:04d}_{s}.png" for f in frames for s in (suffix, "alpha", "normal"))
    assert sorted(bare) == [f"a_{f:04d}_color_preview.png" for f in frames]
    ctx = film.ctx
    desc = world.to_desc(cam)
    ctx.upload_world(desc)
    mask = film.have_mask()
    hist = [torch.empty(F.temporal_history_bytes(w, h), dtype=torch.uint8, device="cuda") for _ in range(2)]
    g, acc, den, prev_start = F.alloc_gbuffer(w, h, "cuda"), torch.empty(w * h, 3, dtype=torch.float32, device="cuda"), torch.empty(w * h, 3, dtype=torch.float32, device="cuda"), None
    img = {3: torch.empty(h * w * 3, dtype=torch.uint8, device="cuda"), 1: torch.empty(h * w, dtype=torch.uint8, device="cuda")}

    def same(t, bpp, name):
        image.save(str(tmp_path / "one.png"), t.cpu().numpy().reshape(h, w, bpp))
        assert open(tmp_path / "one.png", "rb").read() == name, bpp

    for i, frame in enumerate(frames):
        start = f32(frame) * (f32(1.0) / f32(24))
        p = R.frame_params(w, h, 1, 0, 2, frame=frame, time_range=(float(start), float(f32(start + f32(1.0 / 24.0)))))
        out = F.alloc_device_film(w, h, "cuda")
        samples, scramble = F.preview_tables(pv.samples, frame, w, h)
        ctx.preview(p, pv, torch.from_numpy(samples).cuda(), out, torch.from_numpy(scramble).cuda(), None, g)
        ctx.save_to_pixels(K.Color, mask, False, w, h, out, img[3])
        same(img[3], 3, bare[f"a_{frame:04d}_color_preview.png"])
        ctx.temporal_accumulate(p, tp, out, g, None if i == 0 else hist[(i + 1) % 2], None if i == 0 else desc.camera, 0.0 if i == 0 else prev_start, hist[i % 2], acc)
        prev_start = p.time_start
        ctx.denoise(w, h, dict(out, color=acc), den, dn)
        ctx.display(dsp, mask, False, w, h, dict(out, color=den), img[3])
        same(img[3], 3, got[f"a_{frame:04d}_{suffix}.png"])
        ctx.save_to_pixels(K.Alpha, mask, False, w, h, out, img[1])
        same(img[1], 1, got[f"a_{frame:04d}_alpha.png"])
        ctx.save_to_pixels(K.WorldNormal, mask, False, w, h, out, img[3])
        same(img[3], 3, got[f"a_{frame:04d}_normal.png"])
    assert bare["a_0002_color_preview.png"] != bare["a_0007_color_preview.png"]


def test_render_sequence_without_preview_is_unchanged(tmp_path):
    """preview=None writes the files and bytes of render_frame_into + save_to, frame by frame, as before."""
    import rayn_amd as R
    from rayn_amd import setup as S
    K = R.ChannelKind
    w, h, frames = 40, 24, [1, 2]
    _, world, cam = PN.scene("s1", (w, h), moving=True)
    integ = R.PathTracingIntegrator(max_bounces=2, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE)
    filt = R.BlackmanHarrisFilter(S.FILTER_RADIUS)
    kinds = [K.Color, K.Alpha, K.Background, K.WorldNormal]
    film = R.Film(kinds, (w, h))
    film.render_sequence(world, cam, integ, filt, S.TILE_SIZE, frames, 24, 1.0 / 24.0, 1, [K.Color, K.Alpha], str(tmp_path / "none"), "a", preview=None)
    one = R.Film(kinds, (w, h))
    for frame in frames:
        one.render_frame_into(world, cam, integ, filt, S.TILE_SIZE, frame, IO.shutter_range(frame), 1)
        one.save_to([K.Color, K.Alpha], str(tmp_path / "loop"), f"a_{frame:04d}")
    assert IO.read_folder(tmp_path / "none") == IO.read_folder(tmp_path / "loop")


def test_bad_arguments_are_invalid_arg_with_a_text(ctx):
    import torch
    import rayn_amd as R
    from rayn_amd import _abi
    from rayn_amd import film as F
    L = ctx._L
    w, h, n, K = 40, 24, 40 * 24, 4
    wd, _, _ = PN.scene("spheres", (w, h))
    fresh = R.Context(0)
    p = R.frame_params(w, h, 1, 0)
    vp = lambda t: C.c_void_p(t.data_ptr())
    fl = lambda k: torch.zeros(k, dtype=torch.float32, device="cuda")
    color, alpha, normal, ao, rec, obj = fl(3 * n), fl(n), fl(3 * n), fl(n), fl(4 * n + 4), torch.zeros(n, dtype=torch.int32, device="cuda")
    samples, scramble = fl(2 * K + 2), fl(n)
    sb = F.preview_scratch_bytes(w, h, K)
    scratch = torch.zeros(sb + 16, dtype=torch.uint8, device="cuda")
    PP = _abi.PreviewParams

    def pv(c=ctx, p=p, pp=PP(K, 0.5, 0.3), samples=vp(samples), scramble=vp(scramble), color=vp(color), alpha=vp(alpha), normal=vp(normal), ao=vp(ao),
           rec=vp(rec), obj=vp(obj), scratch=vp(scratch), sb=sb):
        rc = L.rayn_hip_preview_device(c.h, None if p is None else C.byref(p), None if pp is None else C.byref(pp), samples, scramble, color, alpha, normal, ao, rec,
                                       obj, scratch, sb, None)
        return rc, c.last_error()

    try:
        assert pv(c=fresh) == (-1, "rayn_hip_upload_world has not been called")
    finally:
        fresh.close()
    ctx.upload_world(wd)
    assert pv()[0] == 0 and pv(scramble=None, ao=None, rec=None, obj=None)[0] == 0
    zero, huge = R.frame_params(0, h, 1, 0), R.frame_params(65536, 32768, 1, 0)
    nan, inf = float("nan"), float("inf")
    off = lambda t, k: C.c_void_p(t.data_ptr() + k)
    for kw, text in ((dict(p=None), "null frame params"), (dict(pp=None), "null preview params"), (dict(p=zero), "zero-sized"), (dict(p=huge), "2^31"),
                     (dict(pp=PP(0, 0.5, 0.3)), "samples must be in 1..64"), (dict(pp=PP(65, 0.5, 0.3)), "samples must be in 1..64"),
                     (dict(pp=PP(K, 0.0, 0.3)), "radius"), (dict(pp=PP(K, -1.0, 0.3)), "radius"), (dict(pp=PP(K, inf, 0.3)), "radius"), (dict(pp=PP(K, nan, 0.3)), "radius"),
                     (dict(pp=PP(K, 0.5, -0.1)), "ambient"), (dict(pp=PP(K, 0.5, 1.5)), "ambient"), (dict(pp=PP(K, 0.5, nan)), "ambient"),
                     (dict(samples=None), "null buffer"), (dict(color=None), "null buffer"), (dict(alpha=None), "null buffer"), (dict(normal=None), "null buffer"),
                     (dict(scratch=None), "null buffer"), (dict(sb=sb - 1), "scratch smaller"), (dict(pp=PP(8, 0.5, 0.3)), "scratch smaller"),
                     (dict(scratch=off(scratch, 4)), "16-byte aligned"), (dict(rec=off(rec, 4)), "16-byte aligned"), (dict(samples=off(samples, 4)), "8-byte aligned"),
                     (dict(color=off(color, 2)), "4-byte aligned"), (dict(scramble=off(scramble, 1)), "4-byte aligned"), (dict(obj=off(obj, 2)), "4-byte aligned"),
                     (dict(color=vp(scratch)), "overlap"), (dict(normal=vp(color)), "overlap"), (dict(ao=vp(alpha)), "overlap"), (dict(rec=vp(normal)), "overlap"),
                     (dict(obj=off(scratch, 64)), "overlap"), (dict(alpha=vp(samples)), "alias an input"), (dict(ao=vp(scramble)), "alias an input"),
                     (dict(scramble=off(scratch, 128)), "alias an input")):
        rc, err = pv(**kw)
        assert rc == -1 and text in err, (kw, rc, err)
    # a refused call writes nothing
    color.fill_(7.0)
    assert pv(sb=sb - 1)[0] == -1
    torch.cuda.synchronize()
    assert torch.all(color == 7.0)
