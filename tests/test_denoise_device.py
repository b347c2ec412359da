"""rayn_hip_denoise_device (rayn_amd/csrc/denoise.hip): the edge-avoiding a-trous denoiser of the Color channel on the GPU, bit for bit
against the numpy restatement (tests/denoise_np.py; NaN payloads aside) on random, adversarial, oracle-rendered and GPU-rendered films,
for every film shape, pass count and on/off combination of the three terms; the inputs stay untouched; stream order; the multi-device
context; error codes and texts; Film.save_to / Film.render_sequence with denoise=; and the denoiser's effect on the shipped scene."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import denoise_np
import device_io as IO
from common import case
from denoise_cases import random_film
from rayn_amd import image

pytestmark = pytest.mark.gpu

SIGMAS = list(itertools.product((0.0, 0.5), (0.0, 0.4), (0.0, 0.3)))  # every on/off combination of colour / normal / alpha
SHAPES = [(1, 1), (1, 7), (7, 1), (17, 13), (33, 65), (300, 200)]  # (width, height)


def _scratch_bytes(w, h):
    from rayn_amd import film as F
    return F.denoise_scratch_bytes(w, h)


def _adversarial(w, h, seed):
    f = random_film(w, h, seed)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 3.0e38, -3.0e38, 1e-45, -np.nan, 1e30], np.float32)
    rng = np.random.default_rng(seed + 100)
    for key in ("color", "normal", "alpha"):
        flat = f[key].reshape(-1)
        idx = rng.choice(flat.size, min(flat.size, 4 * special.size), replace=False)
        flat[idx] = np.resize(special, idx.size)
    f["normal"][rng.choice(w * h, max(1, w * h // 10), replace=False)] = 0.0  # zero normals
    return f


def _run(ctx, film_d, w, h, L, sigmas, stream=None):
    """the entry through Context.denoise; a guide whose sigma is 0 is passed as a null pointer.  Returns the colour (n, 3) on the host."""
    import torch
    from rayn_amd import Denoise
    d = {"color": film_d["color"]}
    if sigmas[1]:
        d["normal"] = film_d["normal"]
    if sigmas[2]:
        d["alpha"] = film_d["alpha"]
    full, out = IO.guarded(w * h * 3, torch.float32, 7.0, 16)  # 16 guard floats after the image
    ctx.denoise(w, h, d, out, Denoise(L, *sigmas), stream=stream)
    torch.cuda.synchronize()
    IO.assert_guards(full, w * h * 3, 7.0, "the output")
    return out.cpu().numpy().reshape(-1, 3)


def _restated(film, w, h, L, sigmas):
    return denoise_np.atrous(film["color"], film["alpha"], film["normal"], w, h, L, *sigmas)


def test_every_shape_pass_count_and_term_combination(gpu_ctx, oracle):
    for si, (w, h) in enumerate(SHAPES):
        film = random_film(w, h, si)
        d = IO.upload_film(film)
        runs = [(L, SIGMAS[(L + si) % 8]) for L in range(1, 9)] + [(3, s) for s in SIGMAS]  # steps up to 128: larger than every image
        for L, sigmas in runs:
            IO.assert_bits_equal(_run(gpu_ctx, d, w, h, L, sigmas), _restated(film, w, h, L, sigmas), (w, h, L, sigmas))


def test_adversarial_films(gpu_ctx, oracle):
    for seed, (w, h) in enumerate([(1, 1), (7, 1), (17, 13), (33, 65)]):
        film = _adversarial(w, h, seed)
        d = IO.upload_film(film)
        for L, sigmas in [(1, (0.5, 0.4, 0.3)), (4, (0.5, 0.4, 0.3)), (2, (2.0 ** -30, 2.0 ** 30, 0.3)), (3, (2.0 ** 30, 0.0, 2.0 ** -30)),
                          (5, (0.0, 0.0, 0.0)), (8, (0.5, 0.0, 0.3))]:
            IO.assert_bits_equal(_run(gpu_ctx, d, w, h, L, sigmas), _restated(film, w, h, L, sigmas), (w, h, L, sigmas))
    # the inputs are not modified
    film = _adversarial(33, 65, 9)
    d = IO.upload_film(film)
    _run(gpu_ctx, d, 33, 65, 5, (0.5, 0.4, 0.3))
    for k, v in film.items():
        IO.assert_is_host(d[k], v, k)


def test_oracle_and_gpu_rendered_films(gpu_ctx, oracle):
    import torch
    import rayn_amd
    wd, p = case("s2", 40, 24, 2, 3)
    tabs = oracle.build_tables(8, 3, p.volume_marches, p.frame, 40, 24)
    rendered, _ = oracle.render(wd, p, tabs)
    gpu_ctx.upload_world(wd)
    out = rayn_amd.film.alloc_device_film(40, 24, "cuda")
    gpu_ctx.render_device(p, [torch.from_numpy(t).cuda() for t in tabs], out)
    torch.cuda.synchronize()
    on_gpu = {k: v.cpu().numpy() for k, v in out.items()}
    for name, film in (("oracle", rendered), ("gpu", on_gpu)):
        film = {"color": np.asarray(film["color"], np.float32).reshape(-1, 3), "alpha": np.asarray(film["alpha"], np.float32).reshape(-1),
                "normal": np.asarray(film["normal"], np.float32).reshape(-1, 3)}
        d = IO.upload_film(film)
        for L, sigmas in [(5, (0.5, 0.4, 0.3)), (2, (1.0, 0.1, 0.0)), (3, (0.0, 0.4, 0.3))]:
            got = _run(gpu_ctx, d, 40, 24, L, sigmas)
            IO.assert_bits_equal(got, _restated(film, 40, 24, L, sigmas), (name, L, sigmas))
            assert not np.array_equal(got, film["color"])


def test_entry_is_stream_ordered(gpu_ctx, oracle):
    """The entry and the post-process run on the side stream they are given, after the copies queued there, with no sync in between."""
    import torch
    from rayn_amd import Denoise
    w, h = 640, 360
    film = random_film(w, h, 5)
    film["background"] = np.zeros((w * h, 3), np.float32)
    want = image.color_image(_restated(film, w, h, 3, (0.5, 0.4, 0.3)).reshape(h, w, 3), background=film["background"].reshape(h, w, 3))
    src = IO.upload_film(film)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dst = {k: torch.zeros_like(v) for k, v in src.items()}
        for k in dst:
            dst[k].copy_(src[k])  # queued on s before the denoiser: it must see the copied film, not zeros
        den = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
        scratch = torch.empty(_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
        gpu_ctx.denoise(w, h, dst, den, Denoise(3, 0.5, 0.4, 0.3), scratch, s.cuda_stream)
        img = torch.zeros(w * h * 3, dtype=torch.uint8, device="cuda")
        gpu_ctx.save_to_pixels(0, 15, False, w, h, dict(dst, color=den), img, s.cuda_stream)
        host = torch.empty(w * h * 3, dtype=torch.uint8, pin_memory=True)
        host.copy_(img, non_blocking=True)
    s.synchronize()
    assert np.array_equal(host.numpy().reshape(h, w, 3), want)


def test_multi_device_context_runs_on_the_first_device(oracle):
    import rayn_amd
    film = random_film(33, 17, 2)
    ctx = rayn_amd.Context([0, 0])
    try:
        got = _run(ctx, IO.upload_film(film), 33, 17, 4, (0.5, 0.4, 0.3))
    finally:
        ctx.close()
    IO.assert_bits_equal(got, _restated(film, 33, 17, 4, (0.5, 0.4, 0.3)), "multi-device")


def test_bad_arguments_return_invalid_arg_with_a_text(gpu_ctx):
    import torch
    from rayn_amd import _lib
    L = _lib.lib()
    w, h = 5, 3
    d = IO.upload_film(random_film(w, h, 1))
    out = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
    need = _scratch_bytes(w, h)
    scratch = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(w=w, h=h, L=5, sc=0.5, sn=0.4, sa=0.3, color=d["color"], alpha=d["alpha"], normal=d["normal"], dst=out, scr=p(scratch), nbytes=need):
        return L_(w, h, L, sc, sn, sa, p(color), p(alpha), p(normal), p(dst), scr, nbytes)

    def L_(*args):
        return L.rayn_hip_denoise_device(gpu_ctx.h, *args, s)

    nan, inf = float("nan"), float("inf")
    cases = [(dict(w=0), "zero-sized image"), (dict(h=0), "zero-sized image"),
             (dict(w=1 << 16, h=1 << 15), "image larger than 2^31 pixels unsupported (32-bit pixel indices)"),
             (dict(L=0), "iterations must be in 1..8"), (dict(L=9), "iterations must be in 1..8")]
    for name, arg in (("sigma_color", "sc"), ("sigma_normal", "sn"), ("sigma_alpha", "sa")):
        for v in (nan, inf, -inf, -0.5, 2.0 ** 31, 2.0 ** -31):
            cases.append(({arg: v}, f"{name} must be 0 (off) or in [2^-30, 2^30]"))
    cases += [(dict(color=None), "null buffer"), (dict(dst=None), "null buffer"), (dict(scr=None), "null buffer"),
              (dict(normal=None), "null normal guide with sigma_normal != 0"), (dict(alpha=None), "null alpha guide with sigma_alpha != 0"),
              (dict(nbytes=need - 1), "scratch smaller than rayn_denoise_scratch_bytes(width, height)"),
              (dict(scr=C.c_void_p(scratch.data_ptr() + 4)), "scratch not 16-byte aligned"),
              (dict(dst=d["color"]), "d_out_color must not be d_color")]
    for kwargs, text in cases:
        assert call(**kwargs) == -1, kwargs  # RAYN_ERR_INVALID_ARG
        assert gpu_ctx.last_error() == text, kwargs
    assert L.rayn_hip_denoise_device(None, w, h, 5, 0.5, 0.4, 0.3, p(d["color"]), p(d["alpha"]), p(d["normal"]), p(out), p(scratch), need, s) == -1
    # good calls after the bad ones: null guides whose sigma is 0, -0 switching a term off
    assert call(sn=0.0, normal=None, sa=-0.0, alpha=None) == 0
    assert call(sc=2.0 ** 30, sn=2.0 ** -30) == 0
    torch.cuda.synchronize()
    # the Python wrapper refuses buffers too small for the image before anything is enqueued
    from rayn_amd import Denoise
    with pytest.raises(ValueError):
        gpu_ctx.denoise(w, h, d, torch.zeros(w * h * 3 - 1, dtype=torch.float32, device="cuda"), Denoise())
    with pytest.raises(ValueError):
        gpu_ctx.denoise(w + 1, h, d, torch.zeros(3 * (w + 1) * h, dtype=torch.float32, device="cuda"), Denoise())


# ---- Film.save_to / Film.render_sequence with denoise= --------------------------------------------------------------------------

def _small_scene(w, h):
    import rayn_amd as R
    from rayn_amd import setup as S
    cam, world = S.setup_s3((w, h))
    return R, cam, world, R.PathTracingIntegrator(max_bounces=3, volume_marches=2), R.BlackmanHarrisFilter(1.5)


def test_save_to_with_denoise(tmp_path, oracle):
    W, H = 48, 32
    R, cam, world, integ, filt = _small_scene(W, H)
    K = R.ChannelKind
    params = R.Denoise(4, 0.5, 0.4, 0.3)
    film = R.Film([K.Color, K.Alpha, K.Background, K.WorldNormal], (W, H))
    film.render_frame_into(world, cam, integ, filt, (16, 16), 2, None, 2)
    host = IO.host_film(film)
    restated = denoise_np.atrous(host["color"], host["alpha"], host["normal"], W, H, 4, 0.5, 0.4, 0.3).reshape(H, W, 3)
    IO.assert_bits_equal(film.denoised_color(params).cpu().numpy().reshape(H, W, 3), restated, "denoised_color")
    for transparent in (False, True):
        out = tmp_path / f"t{int(transparent)}"
        film.save_to([K.Color, K.Alpha, K.WorldNormal], str(out), "x", transparent, denoise=params)
        assert sorted(os.listdir(out)) == ["x_alpha.png", "x_color_denoised.png", "x_normal.png"]
        want = (image.color_image(restated, alpha=host["alpha"], transparent_background=True) if transparent
                else image.color_image(restated, background=host["background"]))
        assert (out / "x_color_denoised.png").read_bytes() == IO.png_bytes(tmp_path, want)
        assert (out / "x_alpha.png").read_bytes() == IO.png_bytes(tmp_path, image.alpha_image(host["alpha"]))
        assert (out / "x_normal.png").read_bytes() == IO.png_bytes(tmp_path, image.normal_image(host["normal"]))
        assert np.array_equal(film.pixels(K.Color, transparent, denoise=params), want)
    # denoise=None is save_to as before
    film.save_to([K.Color], str(tmp_path / "plain"), "x")
    assert os.listdir(tmp_path / "plain") == ["x_color.png"]
    assert (tmp_path / "plain" / "x_color.png").read_bytes() == IO.png_bytes(tmp_path, image.color_image(host["color"], background=host["background"]))
    # a guide the film lacks is switched off; a film without Color cannot be denoised
    no_normal = R.Film([K.Color, K.Alpha, K.Background], (W, H))
    no_normal.render_frame_into(world, cam, integ, filt, (16, 16), 2, None, 2)
    restated = denoise_np.atrous(no_normal.channel(K.Color), no_normal.channel(K.Alpha), None, W, H, 4, 0.5, 0.0, 0.3)
    IO.assert_bits_equal(no_normal.denoised_color(params).cpu().numpy(), restated, "no WorldNormal")
    no_color = R.Film([K.Alpha, K.WorldNormal], (W, H))
    no_color.render_frame_into(world, cam, integ, filt, (16, 16), 2, None, 2)
    with pytest.raises(ValueError, match="Color"):
        no_color.denoised_color(params)
    no_color.save_to([K.Alpha], str(tmp_path / "nc"), "x", denoise=params)  # Alpha alone needs no Color
    assert os.listdir(tmp_path / "nc") == ["x_alpha.png"]


def test_sequence_with_denoise_equals_the_plain_loop(tmp_path, oracle):
    W, H = 48, 32
    FRAMES, RATE, SHUTTER = [3, 5], 24, 1.0 / 24.0
    R, cam, world, integ, filt = _small_scene(W, H)
    K = R.ChannelKind
    kinds = [K.Color, K.Alpha, K.Background, K.WorldNormal]
    params = R.Denoise()
    film = R.Film(kinds, (W, H))
    seq = tmp_path / "seq"
    film.render_sequence(world, cam, integ, filt, (16, 16), FRAMES, RATE, SHUTTER, 2, [K.Alpha, K.WorldNormal, K.Color], str(seq), "a",
                         denoise=params)
    assert sorted(os.listdir(seq)) == sorted(f"a_{f:04d}_{s}.png" for f in FRAMES for s in ("alpha", "normal", "color_denoised"))
    plain = R.Film(kinds, (W, H))
    loop = tmp_path / "loop"
    f32 = np.float32
    for frame in FRAMES:
        plain.render_frame_into(world, cam, integ, filt, (16, 16), frame, IO.shutter_range(frame, RATE, SHUTTER), 2)
        plain.save_to([K.Alpha, K.WorldNormal, K.Color], str(loop), f"a_{frame:04d}", denoise=params)
    assert sorted(os.listdir(loop)) == sorted(os.listdir(seq))
    for name in os.listdir(loop):
        assert (loop / name).read_bytes() == (seq / name).read_bytes(), name


def test_denoiser_lowers_the_error_of_the_shipped_scene_at_8_spp():
    """The shipped scene at 160x96, 8 spp and 1024 spp: the default Denoise brings the MSE of the saturated linear Color + Background
    against the 1024-spp film down to the measured ratio, and one pass with the colour term off to half."""
    import rayn_amd as R
    from rayn_amd import setup as S
    W, H = 160, 96
    cam, world = S.setup((W, H))
    integ = R.PathTracingIntegrator(max_bounces=3, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE)
    filt = R.BlackmanHarrisFilter(S.FILTER_RADIUS)
    K = R.ChannelKind
    films = {}
    for samples in (2, 256):
        films[samples] = R.Film([K.Color, K.Alpha, K.Background, K.WorldNormal], (W, H))
        films[samples].render_frame_into(world, cam, integ, filt, S.TILE_SIZE, 1, None, samples)
    ref = IO.host_film(films[256])
    noisy = IO.host_film(films[2])
    sat = lambda c: np.clip(c.astype(np.float64) + noisy["background"], 0.0, 1.0)
    want = np.clip(ref["color"].astype(np.float64) + ref["background"], 0.0, 1.0)
    mse = lambda c: float(np.mean((sat(c) - want) ** 2))
    base = mse(noisy["color"])
    ratios = {}
    for name, params in (("default", R.Denoise()), ("one pass", R.Denoise(1, 0.0, 0.7, 0.3))):
        ratios[name] = mse(films[2].denoised_color(params).cpu().numpy().reshape(H, W, 3)) / base
    print(f"MSE ratio denoised / noisy: {ratios}")
    assert ratios["default"] <= 0.8, ratios
    assert ratios["one pass"] <= 0.52, ratios
