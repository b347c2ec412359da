"""rayn_hip_denoise_variance_device (rayn_amd/csrc/denoise_variance.hip): the variance-guided a-trous denoiser of a progressive render's
Color channel on the GPU, bit for bit against the numpy restatement (tests/denoise_variance_np.py; NaN payloads aside) on synthetic films
and states - every film shape, tile sizes that divide, do not divide and under-cover the film, per-tile epoch counts from {0, 1, 2, 5,
64}, every pass count and on/off combination of the three terms, adversarial values - and on real progressive renders, fresh and resumed;
the inputs and the state stay untouched; stream order; the multi-device context; error codes and texts; Film.save_to / pixels /
denoised_variance with a VarianceDenoise; and the denoiser's effect on the shipped scene."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import denoise_np
import denoise_variance_np as VN
import device_io as IO
import progressive_np as PN
from denoise_cases import random_film
from rayn_amd import image

pytestmark = pytest.mark.gpu

SIGMAS = list(itertools.product((0.0, 4.0), (0.0, 0.4), (0.0, 0.3)))  # every on/off combination of luminance / normal / alpha
# (width, height), tile size: dividing, covering without dividing, and under-covering grids (50x37 in 16x16 tiles: 3x2 tiles, 48x32 pixels)
SHAPES = [((1, 1), (1, 1)), ((1, 7), (1, 2)), ((7, 1), (3, 1)), ((17, 13), (16, 16)), ((33, 65), (8, 8)), ((33, 65), (11, 13)),
          ((50, 37), (16, 16)), ((300, 200), (16, 16))]
GUARD = 16


def _params(w, h, tile):
    import rayn_amd as R
    return R.frame_params(w, h, 1, 3, tile_size=tile)


def _random_state(w, h, tile, seed):
    """the arrays of a progressive state (rayn_amd.progressive.split_state): per-tile epochs from {0, 1, 2, 5, 64}, m2 >= 0 with zeros"""
    rng = np.random.default_rng(seed + 1000)
    n, t = w * h, len(PN.tile_rects(w, h, *tile))
    m2 = rng.gamma(1.0, 0.05, n).astype(np.float32)
    m2[rng.choice(n, max(1, n // 16), replace=False)] = 0.0
    epochs = rng.choice(np.array([0, 1, 2, 5, 64], np.uint32), t)
    if t >= 2:
        epochs[rng.choice(t, 2, replace=False)] = (2, 64)  # something is always guided
    else:
        epochs[0] = 5
    return {"sum_color": rng.normal(size=(n, 3)).astype(np.float32), "sum_alpha": rng.normal(size=n).astype(np.float32),
            "sum_background": rng.normal(size=(n, 3)).astype(np.float32), "sum_normal": rng.normal(size=(n, 3)).astype(np.float32),
            "mean_y": rng.normal(size=n).astype(np.float32), "m2": m2, "epochs": epochs.astype(np.uint32), "retired": np.zeros(t, np.uint32),
            "outliers": np.zeros(t, np.uint32), "max_e": np.zeros(t, np.float32)}


SPECIAL = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 3.0e38, -3.0e38, 1e-45, -np.nan, 1e30], np.float32)


def _adversarial(w, h, tile, seed):
    film, state = random_film(w, h, seed), _random_state(w, h, tile, seed)
    rng = np.random.default_rng(seed + 100)
    for arr in (film["color"], film["normal"], film["alpha"], state["m2"]):
        flat = arr.reshape(-1)
        idx = rng.choice(flat.size, min(flat.size, 4 * SPECIAL.size), replace=False)
        flat[idx] = np.resize(SPECIAL, idx.size)
    film["normal"][rng.choice(w * h, max(1, w * h // 10), replace=False)] = 0.0  # zero normals
    return film, state


def _device_state(state, w, h, tile):
    import torch
    from rayn_amd import progressive as P
    raw = P.join_state(state, w, h, tile)
    d, view = IO.guarded(raw.size, torch.uint8, 0xA5, 64)
    view.copy_(torch.from_numpy(raw))
    return d


def _run(ctx, film_d, d_state, w, h, tile, L, sigmas, stream=None, variance=True):
    """the entry through Context.denoise_variance; a guide whose sigma is 0 is passed as a null pointer.  Returns the colour (n, 3) and
    the variance (n) (None without a variance buffer) on the host."""
    import torch
    from rayn_amd import VarianceDenoise
    d = {"color": film_d["color"]}
    if sigmas[1]:
        d["normal"] = film_d["normal"]
    if sigmas[2]:
        d["alpha"] = film_d["alpha"]
    n = w * h
    full_out, out = IO.guarded(n * 3, torch.float32, 7.0, GUARD)  # guard floats after the image
    full_var, var = IO.guarded(n, torch.float32, 7.0, GUARD) if variance else (None, None)
    ctx.denoise_variance(_params(w, h, tile), d, d_state, out, VarianceDenoise(L, *sigmas), var, stream=stream)
    torch.cuda.synchronize()
    IO.assert_guards(full_out, n * 3, 7.0, "the colour output")
    if variance:
        IO.assert_guards(full_var, n, 7.0, "the variance output")
    return out.cpu().numpy().reshape(-1, 3), var.cpu().numpy() if variance else None


def _restated(film, state, w, h, tile, L, sigmas):
    return VN.denoise(film["color"], film["alpha"], film["normal"], state["m2"], state["epochs"], w, h, tile, L, *sigmas)


def _check(ctx, film, state, d, d_state, w, h, tile, L, sigmas, what=None):
    what = (w, h, tile, L, sigmas) if what is None else what
    got_c, got_v = _run(ctx, d, d_state, w, h, tile, L, sigmas)
    want_c, want_v = _restated(film, state, w, h, tile, L, sigmas)
    IO.assert_bits_equal(got_c, want_c, (what, "colour"))
    IO.assert_bits_equal(got_v, want_v, (what, "variance"))
    return got_c, got_v


def test_every_shape_tile_size_pass_count_and_term_combination(gpu_ctx, oracle):
    for si, ((w, h), tile) in enumerate(SHAPES):
        film, state = random_film(w, h, si), _random_state(w, h, tile, si)
        d, d_state = IO.upload_film(film), _device_state(state, w, h, tile)
        runs = [(L, SIGMAS[(L + si) % 8]) for L in range(1, 9)] + [(3, s) for s in SIGMAS]  # steps up to 128: larger than every image
        for L, sigmas in runs:
            _check(gpu_ctx, film, state, d, d_state, w, h, tile, L, sigmas)
    # without a variance buffer the colour is the same
    (w, h), tile = SHAPES[4]
    film, state = random_film(w, h, 4), _random_state(w, h, tile, 4)
    got_c, none = _run(gpu_ctx, IO.upload_film(film), _device_state(state, w, h, tile), w, h, tile, 4, (4.0, 0.4, 0.3), variance=False)
    assert none is None
    IO.assert_bits_equal(got_c, _restated(film, state, w, h, tile, 4, (4.0, 0.4, 0.3))[0], "no variance buffer")


def test_adversarial_films_and_states(gpu_ctx, oracle):
    from rayn_amd import progressive as P
    for seed, ((w, h), tile) in enumerate([((1, 1), (1, 1)), ((7, 1), (3, 1)), ((17, 13), (16, 16)), ((33, 65), (8, 8)), ((50, 37), (16, 16))]):
        film, state = _adversarial(w, h, tile, seed)
        d, d_state = IO.upload_film(film), _device_state(state, w, h, tile)
        for L, sigmas in [(1, (4.0, 0.4, 0.3)), (4, (4.0, 0.4, 0.3)), (2, (2.0 ** -30, 2.0 ** 30, 0.3)), (3, (2.0 ** 30, 0.0, 2.0 ** -30)),
                          (5, (0.0, 0.0, 0.0)), (8, (1.0, 0.0, 0.3))]:
            _check(gpu_ctx, film, state, d, d_state, w, h, tile, L, sigmas)
    # the inputs and the state are not modified, and nothing is written past the state
    (w, h), tile = (33, 65), (8, 8)
    film, state = _adversarial(w, h, tile, 9)
    d, d_state = IO.upload_film(film), _device_state(state, w, h, tile)
    before = d_state.cpu().numpy().copy()
    _run(gpu_ctx, d, d_state, w, h, tile, 5, (4.0, 0.4, 0.3))
    for k, v in film.items():
        IO.assert_is_host(d[k], v, k)
    assert np.array_equal(d_state.cpu().numpy(), before)
    assert np.all(before[P.state_bytes(w, h, tile):] == 0xA5)


# ---- real progressive renders -------------------------------------------------------------------------------------------------------

W, H, TILE, SAMPLES, BOUNCES = 48, 32, (16, 16), 1, 3
# scene s3 under these parameters retires its tiles after 3, 8, 11 and 12 epochs (the numpy restatement of the loop driven by the CPU
# oracle, progressive_np.run, shows [11 12 12 8 3 12])
ADAPTIVE = dict(target_error=0.2, noise_floor=0.05, min_epochs=3, max_epochs=12, outlier_permille=100)
KINDS = lambda R: [R.ChannelKind.Color, R.ChannelKind.Alpha, R.ChannelKind.Background, R.ChannelKind.WorldNormal]


def _scene(name, w=W, h=H):
    import rayn_amd as R
    from rayn_amd import setup as S
    cam, world = S.SCENES[name]((w, h))
    return R, cam, world, R.PathTracingIntegrator(max_bounces=BOUNCES, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE), R.BlackmanHarrisFilter(1.5)


def _restated_from_film(film, params):
    """the restatement fed with the film's mean film and Film._progressive_arrays()"""
    arrays, pr = film._progressive_arrays()
    host = IO.host_film(film)
    w, h = film.res
    tile = (pr["params"].tile_w, pr["params"].tile_h)
    return VN.denoise(host["color"], host["alpha"], host["normal"], arrays["m2"], arrays["epochs"], w, h, tile, params.iterations,
                      params.sigma_luminance, params.sigma_normal, params.sigma_alpha)


def test_a_real_adaptive_render_fresh_and_resumed(tmp_path, oracle):
    R, cam, world, integ, filt = _scene("s3")
    film = R.Film(KINDS(R), (W, H))
    rep = film.render_progressive(world, cam, integ, filt, TILE, 1, None, SAMPLES, R.Progressive(**ADAPTIVE))
    assert len(set(rep["tile_epochs"].tolist())) >= 2, rep["tile_epochs"]
    for params in (R.VarianceDenoise(), R.VarianceDenoise(3, 2.0, 0.0, 0.3), R.VarianceDenoise(1, 4.0, 0.4, 0.0)):
        want_c, want_v = _restated_from_film(film, params)
        got = film.denoised_color(params).cpu().numpy()
        IO.assert_bits_equal(got, want_c, ("fresh", params, "colour"))
        IO.assert_bits_equal(film.denoised_variance(params), want_v.reshape(H, W), ("fresh", params, "variance"))
        assert not np.array_equal(got, film.channel(R.ChannelKind.Color).reshape(-1, 3))
        assert np.isfinite(want_v).all()  # 48x32 in 16x16 tiles is covered and every tile has run >= 3 epochs
    # a checkpoint after 5 epochs, resumed to the end: the restored state is the state
    a = R.Film(KINDS(R), (W, H))
    a.render_progressive(world, cam, integ, filt, TILE, 1, None, SAMPLES, R.Progressive(**dict(ADAPTIVE, max_epochs=5)))
    path = str(tmp_path / "ck.npz")
    a.save_checkpoint(path)
    b = R.Film(KINDS(R), (W, H))
    rep_b = b.render_progressive(world, cam, integ, filt, TILE, 1, None, SAMPLES, R.Progressive(**ADAPTIVE), resume=path)
    assert np.array_equal(rep_b["tile_epochs"], rep["tile_epochs"])
    params = R.VarianceDenoise()
    want_c, want_v = _restated_from_film(b, params)
    IO.assert_bits_equal(b.denoised_color(params).cpu().numpy(), want_c, "resumed colour")
    IO.assert_bits_equal(b.denoised_variance(params), want_v.reshape(H, W), "resumed variance")
    IO.assert_bits_equal(b.denoised_color(params).cpu().numpy(), film.denoised_color(params).cpu().numpy(), "resumed against fresh")
    # a resume that renders nothing more (the checkpoint already holds max_epochs epochs) still carries the state
    c = R.Film(KINDS(R), (W, H))
    rep_c = c.render_progressive(world, cam, integ, filt, TILE, 1, None, SAMPLES, R.Progressive(**dict(ADAPTIVE, max_epochs=5)), resume=path)
    assert rep_c["epochs"] == 5 and len(rep_c["stats"]) == 0
    IO.assert_bits_equal(c.denoised_color(params).cpu().numpy(), a.denoised_color(params).cpu().numpy(), "restored only")


def test_entry_is_stream_ordered(gpu_ctx, oracle):
    """The entry and the post-process run on the side stream they are given, after the copies queued there, with no sync in between."""
    import torch
    from rayn_amd import VarianceDenoise
    from rayn_amd import film as F
    from rayn_amd import progressive as P
    w, h, tile = 640, 360, (16, 16)
    film, state = random_film(w, h, 5), _random_state(w, h, tile, 5)
    film["background"] = np.zeros((w * h, 3), np.float32)
    want_c, want_v = _restated(film, state, w, h, tile, 3, (4.0, 0.4, 0.3))
    want = image.color_image(want_c.reshape(h, w, 3), background=film["background"].reshape(h, w, 3))
    src = IO.upload_film(film)
    src_state = torch.from_numpy(P.join_state(state, w, h, tile)).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dst = {k: torch.zeros_like(v) for k, v in src.items()}
        for k in dst:
            dst[k].copy_(src[k])  # queued on s before the denoiser: it must see the copied film and state, not zeros
        dst_state = torch.zeros_like(src_state)
        dst_state.copy_(src_state)
        den = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
        var = torch.zeros(w * h, dtype=torch.float32, device="cuda")
        scratch = torch.empty(F.denoise_variance_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
        gpu_ctx.denoise_variance(_params(w, h, tile), dst, dst_state, den, VarianceDenoise(3, 4.0, 0.4, 0.3), var, scratch, s.cuda_stream)
        img = torch.zeros(w * h * 3, dtype=torch.uint8, device="cuda")
        gpu_ctx.save_to_pixels(0, 15, False, w, h, dict(dst, color=den), img, s.cuda_stream)
        host = torch.empty(w * h * 3, dtype=torch.uint8, pin_memory=True)
        host.copy_(img, non_blocking=True)
        host_v = torch.empty(w * h, dtype=torch.float32, pin_memory=True)
        host_v.copy_(var, non_blocking=True)
    s.synchronize()
    assert np.array_equal(host.numpy().reshape(h, w, 3), want)
    IO.assert_bits_equal(host_v.numpy(), want_v, "variance on the side stream")


def test_multi_device_context_runs_on_the_first_device(oracle):
    import rayn_amd
    (w, h), tile = (33, 17), (8, 8)
    film, state = random_film(w, h, 2), _random_state(w, h, tile, 2)
    ctx = rayn_amd.Context([0, 0])
    try:
        _check(ctx, film, state, IO.upload_film(film), _device_state(state, w, h, tile), w, h, tile, 4, (4.0, 0.4, 0.3), "multi-device")
    finally:
        ctx.close()


def test_bad_arguments_return_invalid_arg_with_a_text(gpu_ctx):
    import torch
    from rayn_amd import VarianceDenoise, _lib
    from rayn_amd import film as F
    from rayn_amd import progressive as P
    L = _lib.lib()
    w, h, tile = 20, 12, (8, 8)
    film, st = random_film(w, h, 1), _random_state(w, h, tile, 1)
    d = IO.upload_film(film)
    p0 = _params(w, h, tile)
    need_state = P.state_bytes(w, h, tile)
    state = torch.zeros(need_state + 16, dtype=torch.uint8, device="cuda")
    state[:need_state] = torch.from_numpy(P.join_state(st, w, h, tile)).cuda()
    out = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
    var = torch.zeros(w * h, dtype=torch.float32, device="cuda")
    need = F.denoise_variance_scratch_bytes(w, h)
    scratch = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")
    p = lambda t: None if t is None else (t if isinstance(t, C.c_void_p) else C.c_void_p(t.data_ptr()))
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(fp=p0, L_=5, sl=4.0, sn=0.4, sa=0.3, color=d["color"], alpha=d["alpha"], normal=d["normal"], st=state, st_bytes=need_state, dst=out,
             dvar=var, scr=scratch, nbytes=need, ctx=gpu_ctx.h):
        return L.rayn_hip_denoise_variance_device(ctx, None if fp is None else C.byref(fp), L_, sl, sn, sa, p(color), p(alpha), p(normal), p(st), st_bytes,
                                                  p(dst), p(dvar), p(scr), nbytes, s)

    def geom(**kw):
        q = _params(w, h, tile)
        for k, v in kw.items():
            setattr(q, k, v)
        return q
    nan, inf = float("nan"), float("inf")
    small = "state smaller than rayn_progressive_state_bytes(width, height, tile_w, tile_h)"
    cases = [(dict(fp=None), "null frame parameters"), (dict(fp=geom(width=0)), "zero-sized film"), (dict(fp=geom(height=0)), "zero-sized film"),
             (dict(fp=geom(tile_w=0)), "zero-sized tile"), (dict(fp=geom(tile_h=0)), "zero-sized tile"),
             (dict(fp=geom(width=1 << 16, height=1 << 15)), "film larger than 2^31 pixels unsupported (32-bit pixel indices)"),
             (dict(fp=geom(width=3, height=3, tile_w=8, tile_h=8)), "the tile size leaves the film without tiles"),
             (dict(st=None), "null buffer"), (dict(st_bytes=need_state - 1), small), (dict(fp=geom(tile_w=4)), small),
             (dict(st=C.c_void_p(state.data_ptr() + 4)), "state not 16-byte aligned"),
             (dict(L_=0), "iterations must be in 1..8"), (dict(L_=9), "iterations must be in 1..8")]
    for name, arg in (("sigma_luminance", "sl"), ("sigma_normal", "sn"), ("sigma_alpha", "sa")):
        for v in (nan, inf, -inf, -0.5, 2.0 ** 31, 2.0 ** -31):
            cases.append(({arg: v}, f"{name} must be 0 (off) or in [2^-30, 2^30]"))
    alias = "d_out_variance must not be an input or d_out_color"
    cases += [(dict(color=None), "null buffer"), (dict(dst=None), "null buffer"), (dict(scr=None), "null buffer"),
              (dict(normal=None), "null normal guide with sigma_normal != 0"), (dict(alpha=None), "null alpha guide with sigma_alpha != 0"),
              (dict(nbytes=need - 1), "scratch smaller than rayn_denoise_variance_scratch_bytes(width, height)"),
              (dict(scr=C.c_void_p(scratch.data_ptr() + 4)), "scratch not 16-byte aligned"),
              (dict(dst=d["color"]), "d_out_color must not be d_color"),
              (dict(dvar=d["color"]), alias), (dict(dvar=d["alpha"]), alias), (dict(dvar=d["normal"]), alias), (dict(dvar=state), alias),
              (dict(dvar=out), alias)]
    for kwargs, text in cases:
        assert call(**kwargs) == -1, kwargs  # RAYN_ERR_INVALID_ARG
        assert gpu_ctx.last_error() == text, kwargs
    assert call(ctx=None) == -1
    # good calls after the bad ones: null guides whose sigma is 0, -0 switching a term off, no variance buffer
    assert call(sn=0.0, normal=None, sa=-0.0, alpha=None) == 0
    assert call(sl=2.0 ** 30, sn=2.0 ** -30) == 0
    assert call(dvar=None) == 0 and call(sl=0.0) == 0
    torch.cuda.synchronize()
    # the Python wrapper refuses buffers too small for the image before anything is enqueued
    with pytest.raises(ValueError):
        gpu_ctx.denoise_variance(p0, d, state, torch.zeros(w * h * 3 - 1, dtype=torch.float32, device="cuda"), VarianceDenoise())
    with pytest.raises(ValueError):
        gpu_ctx.denoise_variance(p0, d, state, out, VarianceDenoise(), torch.zeros(w * h - 1, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        gpu_ctx.denoise_variance(p0, d, state[: need_state - 16], out, VarianceDenoise())
    with pytest.raises(ValueError):
        gpu_ctx.denoise_variance(_params(w + 1, h, tile), d, torch.zeros(P.state_bytes(w + 1, h, tile), dtype=torch.uint8, device="cuda"),
                                 torch.zeros(3 * (w + 1) * h, dtype=torch.float32, device="cuda"), VarianceDenoise())


# ---- Film.save_to / pixels / denoised_variance with a VarianceDenoise ---------------------------------------------------------------

def test_save_to_with_a_variance_denoise(tmp_path, oracle):
    R, cam, world, integ, filt = _scene("s3")
    K = R.ChannelKind
    params = R.VarianceDenoise(4, 4.0, 0.4, 0.3)
    film = R.Film(KINDS(R), (W, H))
    film.render_progressive(world, cam, integ, filt, TILE, 2, None, SAMPLES, R.Progressive(min_epochs=2, max_epochs=4, adaptive=False))
    host = IO.host_film(film)
    restated = _restated_from_film(film, params)[0].reshape(H, W, 3)
    for transparent in (False, True):
        out = tmp_path / f"t{int(transparent)}"
        film.save_to([K.Color, K.Alpha, K.WorldNormal], str(out), "x", transparent, denoise=params)
        assert sorted(os.listdir(out)) == ["x_alpha.png", "x_color_denoised.png", "x_normal.png"]
        want = (image.color_image(restated, alpha=host["alpha"], transparent_background=True) if transparent
                else image.color_image(restated, background=host["background"]))
        assert (out / "x_color_denoised.png").read_bytes() == IO.png_bytes(tmp_path, want)
        assert (out / "x_alpha.png").read_bytes() == IO.png_bytes(tmp_path, image.alpha_image(host["alpha"]))
        assert np.array_equal(film.pixels(K.Color, transparent, denoise=params), want)
    # the fixed-sigma filter still works on the same film
    fixed = denoise_np.atrous(host["color"], host["alpha"], host["normal"], W, H, 2, 0.5, 0.4, 0.3)
    IO.assert_bits_equal(film.denoised_color(R.Denoise(2, 0.5, 0.4, 0.3)).cpu().numpy(), fixed, "Denoise on a progressive film")
    # a guide the film lacks is switched off
    no_normal = R.Film([K.Color, K.Alpha, K.Background], (W, H))
    no_normal.render_progressive(world, cam, integ, filt, TILE, 2, None, SAMPLES, R.Progressive(min_epochs=2, max_epochs=2, adaptive=False))
    arrays, _ = no_normal._progressive_arrays()
    want_c, _ = VN.denoise(no_normal.channel(K.Color), no_normal.channel(K.Alpha), None, arrays["m2"], arrays["epochs"], W, H, TILE, 4, 4.0, 0.0, 0.3)
    IO.assert_bits_equal(no_normal.denoised_color(params).cpu().numpy(), want_c, "no WorldNormal")
    # no progressive render, one that another render has replaced, one of a single epoch, a sequence, a film without Color
    plain = R.Film(KINDS(R), (W, H))
    plain.render_frame_into(world, cam, integ, filt, TILE, 2, None, 2)
    for call in (lambda: plain.denoised_color(params), lambda: plain.denoised_variance(params), lambda: plain.pixels(K.Color, denoise=params),
                 lambda: plain.save_to([K.Color], str(tmp_path / "plain"), "x", denoise=params)):
        with pytest.raises(ValueError, match="progressive render"):
            call()
    plain.save_to([K.Alpha], str(tmp_path / "alpha_only"), "x", denoise=params)  # Alpha alone is not denoised
    film.render_frame_into(world, cam, integ, filt, TILE, 2, None, 2)
    with pytest.raises(ValueError, match="progressive render"):
        film.denoised_color(params)
    one = R.Film(KINDS(R), (W, H))
    one.render_progressive(world, cam, integ, filt, TILE, 2, None, SAMPLES, R.Progressive(min_epochs=2, max_epochs=4), on_epoch=lambda r: False)
    with pytest.raises(ValueError, match="two epochs"):
        one.denoised_color(params)
    with pytest.raises(ValueError, match="progressive render"):
        plain.render_sequence(world, cam, integ, filt, TILE, [1], 24, 1.0 / 24.0, 2, [K.Color], str(tmp_path / "seq"), "a", denoise=params)
    assert not os.path.exists(tmp_path / "seq")
    no_color = R.Film([K.Alpha, K.WorldNormal], (W, H))
    no_color.render_progressive(world, cam, integ, filt, TILE, 2, None, SAMPLES, R.Progressive(min_epochs=2, max_epochs=2, adaptive=False))
    with pytest.raises(ValueError, match="Color"):
        no_color.denoised_color(params)


# ---- does it do its job -------------------------------------------------------------------------------------------------------------

def quality_figures(grid=()):
    """The shipped scene at 160x96: MSE of the saturated Color + Background against 1024 spp (render_frame_into at samples=256) of the
    mean film of a progressive render, of Denoise() on it and of VarianceDenoise() (and of every VarianceDenoise of `grid`) on it, for a
    non-adaptive run of 4 epochs at samples=2 (32 spp) and an adaptive run with the default Progressive() capped at 16 epochs."""
    import dataclasses
    import rayn_amd as R
    from rayn_amd import setup as S
    Wq, Hq = 160, 96
    cam, world = S.setup((Wq, Hq))
    integ = R.PathTracingIntegrator(max_bounces=3, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE)
    filt = R.BlackmanHarrisFilter(S.FILTER_RADIUS)
    reference = R.Film(KINDS(R), (Wq, Hq))
    reference.render_frame_into(world, cam, integ, filt, S.TILE_SIZE, 1, None, 256)
    ref = IO.host_film(reference)
    want = np.clip(ref["color"].astype(np.float64) + ref["background"], 0.0, 1.0)
    runs = {"non-adaptive": R.Progressive(min_epochs=2, max_epochs=4, adaptive=False),
            "adaptive": dataclasses.replace(R.Progressive(), max_epochs=16)}
    figures = {}
    for name, prog in runs.items():
        film = R.Film(KINDS(R), (Wq, Hq))
        rep = film.render_progressive(world, cam, integ, filt, S.TILE_SIZE, 1, None, 2, prog)
        noisy = IO.host_film(film)
        mse = lambda c: float(np.mean((np.clip(np.asarray(c).reshape(Hq, Wq, 3).astype(np.float64) + noisy["background"], 0.0, 1.0) - want) ** 2))
        fig = {"epochs": sorted(set(rep["tile_epochs"].tolist())), "mean film": mse(noisy["color"]),
               "Denoise()": mse(film.denoised_color(R.Denoise()).cpu().numpy()),
               "VarianceDenoise()": mse(film.denoised_color(R.VarianceDenoise()).cpu().numpy())}
        for params in grid:
            fig[params] = mse(film.denoised_color(params).cpu().numpy())
        figures[name] = fig
    return figures


# variance-guided / undenoised with the defaults.  Computed with the CPU oracle driving progressive_np.run and the
# numpy restatement of the filter - the path the tests above hold the GPU to bit for bit; the figures were not re-taken on a GPU.
MEASURED_RATIOS = {"non-adaptive": 0.7548, "adaptive": 0.8606}


def test_variance_guided_denoiser_lowers_the_error_of_the_shipped_scene():
    """Both runs of quality_figures: the variance-guided filter lowers the MSE of the mean film, does at least as well as the
    fixed-sigma Denoise(), and reaches the measured ratio (times 1.05: the renders are bit-reproducible, the 5 % is room for the other
    fma_policy only)."""
    figures = quality_figures()
    for name, fig in figures.items():
        print(f"{name}: tile epochs {fig['epochs']}, MSE mean film {fig['mean film']:.4e}, Denoise() {fig['Denoise()'] / fig['mean film']:.4f}x, "
              f"VarianceDenoise() {fig['VarianceDenoise()'] / fig['mean film']:.4f}x")
    for name, fig in figures.items():
        assert fig["VarianceDenoise()"] < fig["mean film"], (name, fig)
        assert fig["VarianceDenoise()"] <= fig["Denoise()"], (name, fig)
        assert fig["VarianceDenoise()"] / fig["mean film"] <= MEASURED_RATIOS[name] * 1.05, (name, fig)
