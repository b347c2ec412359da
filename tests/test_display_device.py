"""rayn_hip_display_pixels_device / rayn_hip_display_color_device (rayn_amd/csrc/display.hip): the HDR display transform of the Color
channel on the GPU, bit for bit against the numpy restatement (tests/display_np.py; NaN payloads aside) - the float plane, the 8-bit
image, the metered {m, e} and the bloom plane - for every shape, tone operator, exposure mode, bloom depth and arm, on random and
adversarial films; identity parameters against save_to; guard words and untouched inputs; stream order; the state over two calls; error
codes and texts; the multi-device context; Film.save_to / Film.render_sequence / Film.save_hdr with display=."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import device_io as IO
import display_np as D
from display_cases import film as host_film
from rayn_amd import image

pytestmark = pytest.mark.gpu

# (width, height): degenerate rows and columns, odd sizes, one block of 256 pixels less one / exactly / plus one, and 258 blocks (the
# strided loop of the second metering stage runs twice for threads 0 and 1)
SHAPES = [(1, 1), (1, 7), (7, 1), (17, 13), (33, 65), (255, 1), (256, 1), (257, 1), (300, 220)]
ARMS = [(True, True, True), (False, True, False), (False, False, False)]  # (transparent_background, Background present, Alpha present)
COMBOS = list(itertools.product(("linear", "reinhard", "aces"), ("auto", 1.5), (0, 1, 3, 8)))
GUARD = 16


def _display(tone, exposure, levels):
    from rayn_amd.film import Bloom, Display
    return Display(exposure=exposure, tone=tone, bloom=Bloom(0.8, 0.6, levels) if levels else None)


def _run(ctx, film, w, h, display, transparent, adapt=1.0, state=None, stream=None, d=None):
    """Both entries through Context.display, every output followed by guard words.  `state`: (m, valid) before the call.  Returns the
    float plane, the image, {m, e}, the bloom plane (None without bloom) and the state afterwards."""
    import torch
    from rayn_amd.film import display_scratch_bytes, save_to_bpp
    d = IO.upload_film(film) if d is None else d
    n = w * h
    mask = 1 | (2 if film.get("alpha") is not None else 0) | (4 if film.get("background") is not None else 0)
    bpp = save_to_bpp(0, mask, transparent)
    need = display_scratch_bytes(w, h, display.levels)
    states, outs = [], {}
    for key, dtype, count, fill in (("d", torch.float32, 3 * n, 7.0), ("image", torch.uint8, n * bpp, 0x5A)):
        full_out, out = IO.guarded(count, dtype, fill, GUARD)
        full_meter, meter = IO.guarded(2, torch.float32, 7.0, GUARD)
        full_bloom, bloom = IO.guarded(3 * n, torch.float32, 7.0, GUARD)
        full_scratch, _ = IO.guarded(need, torch.uint8, 0xAB, 64)
        full_st, st = IO.guarded(2, torch.int32, 0x55, GUARD)
        before = np.array([np.float32(0 if state is None else state[0]).view(np.int32), 0 if state is None else state[1]], np.int32)
        st.copy_(torch.from_numpy(before))
        # the entry is handed the whole buffers, as before: it takes their sizes from its arguments
        ctx.display(display, mask, transparent, w, h, d, full_out, full_st, full_scratch, adapt, full_meter, full_bloom, stream)
        torch.cuda.synchronize()
        for whole, size, word, name in ((full_out, count, fill, key), (full_meter, 2, 7.0, "meter"), (full_bloom, 3 * n if display.levels else 0, 7.0, "bloom"),
                                        (full_scratch, need, 0xAB, "scratch"), (full_st, 2, 0x55, "state")):
            IO.assert_guards(whole, size, word, name)
        out, meter, bloom, st = (t.cpu().numpy() for t in (out, meter, bloom, st))
        if not display.auto:
            assert np.array_equal(st, before)  # a manual exposure leaves the state alone
        outs[key] = out
        states.append((st, meter, bloom))
    for a, b in zip(states[0], states[1]):  # both entries meter, adapt and bloom alike
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    st, meter, bloom = states[0]
    for k, v in film.items():  # the inputs are not modified
        if v is not None:
            IO.assert_is_host(d[k], v, k)
    return {"d": outs["d"].reshape(n, 3), "image": outs["image"].reshape(h, w, bpp), "meter": meter,
            "bloom": bloom.reshape(n, 3) if display.levels else None, "state": (st[:1].view(np.float32)[0], int(st[1]))}


def _check(ctx, film, w, h, display, transparent, adapt=1.0, state=None, what=None, **kw):
    got = _run(ctx, film, w, h, display, transparent, adapt, state, **kw)
    want = D.display(film["color"], w, h, display.to_abi(adapt), film.get("background"), film.get("alpha"), transparent,
                     (0.0, 0) if state is None else state)
    IO.assert_bits_equal(got["d"], want["d"], (what, "float plane"))
    assert np.array_equal(got["image"], want["image"]), (what, "image", int((got["image"] != want["image"]).sum()))
    IO.assert_bits_equal(got["meter"], [want["m"], want["e"]], (what, "m, e"))
    if display.levels:
        IO.assert_bits_equal(got["bloom"], want["bloom"], (what, "bloom"))
    if display.auto:
        assert got["state"][1] == want["state"][1], what
        IO.assert_bits_equal([got["state"][0]], [want["state"][0]], (what, "state"))
    return got, want


def _film(w, h, seed, arm, adversarial):
    transparent, with_bg, with_alpha = ARMS[arm]
    color, background, alpha = host_film(w, h, seed, adversarial, with_bg, with_alpha)
    return {"color": color, "background": background, "alpha": alpha}, transparent


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_shape_against_the_restatement(gpu_ctx, oracle, shape):
    """Every tone x exposure mode x bloom depth at this shape; the arm and the film kind (random / adversarial) rotate through them."""
    w, h = shape
    si = SHAPES.index(shape)
    for i, (tone, exposure, levels) in enumerate(COMBOS):
        arm, adversarial = (i + si) % 3, bool((i // 3 + si) % 2)
        film, transparent = _film(w, h, 10 * si + i, arm, adversarial)
        display = _display(tone, exposure, levels)
        _check(gpu_ctx, film, w, h, display, transparent, what=(shape, tone, exposure, levels, arm, adversarial))


@pytest.mark.parametrize("adversarial", [False, True], ids=["random", "adversarial"])
@pytest.mark.parametrize("arm", [0, 1, 2], ids=["rgba", "color_bg", "color_only"])
def test_every_parameter_combination_in_every_arm(gpu_ctx, oracle, arm, adversarial):
    w, h = 33, 65
    film, transparent = _film(w, h, 50 + arm, arm, adversarial)
    d = IO.upload_film(film)
    for tone, exposure, levels in COMBOS:
        display = _display(tone, exposure, levels)
        _check(gpu_ctx, film, w, h, display, transparent, what=(tone, exposure, levels, arm, adversarial), d=d)


@pytest.mark.parametrize("arm", [0, 1, 2], ids=["rgba", "color_bg", "color_only"])
def test_identity_parameters_are_save_to(gpu_ctx, arm):
    import torch
    from rayn_amd.film import Display, save_to_bpp
    w, h = 33, 65
    film, transparent = _film(w, h, 60 + arm, arm, True)
    got = _run(gpu_ctx, film, w, h, Display(exposure=0.0, tone="linear"), transparent)
    mask = 1 | (2 if film["alpha"] is not None else 0) | (4 if film["background"] is not None else 0)
    plain = torch.zeros(w * h * save_to_bpp(0, mask, transparent), dtype=torch.uint8, device="cuda")
    gpu_ctx.save_to_pixels(0, mask, transparent, w, h, IO.upload_film(film), plain)
    assert np.array_equal(got["image"].reshape(-1), plain.cpu().numpy())
    IO.assert_bits_equal(got["d"], D.input_color(film["color"], film["background"], transparent), "d has the bits of c")


def test_state_carries_over_two_calls(gpu_ctx, oracle):
    w, h = 300, 220
    display = _display("aces", "auto", 3)
    first, transparent = _film(w, h, 70, 1, False)
    second, _ = _film(w, h, 71, 1, False)
    second["color"] *= np.float32(6.0)
    a, _ = _check(gpu_ctx, first, w, h, display, transparent, adapt=0.25, what="first")  # a fresh state: its own metered value
    assert a["state"][1] == 1
    b, want = _check(gpu_ctx, second, w, h, display, transparent, adapt=0.25, state=a["state"], what="second")
    alone = D.display(second["color"], w, h, display.to_abi(1.0), second["background"])
    assert a["state"][0] < b["state"][0] < alone["state"][0] and b["meter"][1] > alone["e"]  # a quarter of the way to the brighter frame
    # nothing to meter: e = 1, the state stays
    black = {"color": np.zeros((w * h, 3), np.float32), "background": None, "alpha": None}
    c, _ = _check(gpu_ctx, black, w, h, display, False, adapt=0.25, state=b["state"], what="black")
    assert c["meter"][1] == 1.0 and c["state"] == b["state"]
    nan = {"color": np.full((w * h, 3), np.nan, np.float32), "background": None, "alpha": None}
    c, _ = _check(gpu_ctx, nan, w, h, display, False, what="nan")
    assert c["meter"][1] == 1.0 and c["state"] == (0.0, 0)


def test_entry_is_stream_ordered(gpu_ctx, oracle):
    """The entry runs on the side stream it is given, after the copies queued there, with no sync in between."""
    import torch
    from rayn_amd.film import display_scratch_bytes
    w, h = 640, 360
    film, transparent = _film(w, h, 80, 1, False)
    display = _display("reinhard", "auto", 5)
    want = D.display(film["color"], w, h, display.to_abi(), film["background"])["image"]
    src = IO.upload_film(film)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dst = {k: torch.zeros_like(v) for k, v in src.items()}
        for k in dst:
            dst[k].copy_(src[k])  # queued on s before the transform: it must see the copied film, not zeros
        img = torch.zeros(w * h * 3, dtype=torch.uint8, device="cuda")
        state = torch.zeros(2, dtype=torch.int32, device="cuda")
        scratch = torch.empty(display_scratch_bytes(w, h, 5), dtype=torch.uint8, device="cuda")
        gpu_ctx.display(display, 5, False, w, h, dst, img, state, scratch, stream=s.cuda_stream)
        host = torch.empty(w * h * 3, dtype=torch.uint8, pin_memory=True)
        host.copy_(img, non_blocking=True)
    s.synchronize()
    assert np.array_equal(host.numpy().reshape(h, w, 3), want)


def test_multi_device_context_runs_on_the_first_device(oracle):
    import rayn_amd
    film, transparent = _film(33, 17, 90, 0, False)
    display = _display("aces", "auto", 3)
    ctx = rayn_amd.Context([0, 0])
    try:
        _check(ctx, film, 33, 17, display, transparent, what="multi-device")
    finally:
        ctx.close()


def test_bad_arguments_return_invalid_arg_with_a_text(gpu_ctx):
    import torch
    from rayn_amd import _abi, _lib
    from rayn_amd.film import Bloom, Display, display_scratch_bytes
    L = _lib.lib()
    w, h = 5, 3
    film, _ = _film(w, h, 1, 0, False)
    d = IO.upload_film(film)
    out8 = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    outf = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
    need = display_scratch_bytes(w, h, 3)
    scratch = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")
    state = torch.zeros(2, dtype=torch.int32, device="cuda")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    base = Display(exposure="auto", tone="reinhard", bloom=Bloom(1.0, 0.5, 3)).to_abi()

    def call(fn=L.rayn_hip_display_pixels_device, dst=out8, mask=7, transparent=0, w=w, h=h, color=d["color"], alpha=d["alpha"],
             background=d["background"], st=p(state), scr=p(scratch), nbytes=need, null_params=False, **fields):
        dp = _abi.DisplayParams.from_buffer_copy(base)
        for k, v in fields.items():
            setattr(dp, k, v)
        return fn(gpu_ctx.h, None if null_params else C.byref(dp), mask, transparent, w, h, p(color), p(alpha), p(background), st, scr, nbytes,
                  p(dst), None, None, s)

    nan, inf = float("nan"), float("inf")
    cases = [(dict(null_params=True), "null display params"),
             (dict(mask=1, transparent=1), "Attempted to write Color channel with insufficient channels"),
             (dict(mask=6), "Attempted to write Color channel with insufficient channels"),
             (dict(w=0), "zero-sized image"), (dict(h=0), "zero-sized image"),
             (dict(w=1 << 16, h=1 << 15), "image larger than 2^31 pixels unsupported (32-bit pixel indices)"),
             (dict(tone=3), "unknown tone operator (0 linear, 1 reinhard, 2 aces)"),
             (dict(levels=9), "bloom levels must be in 0..8 (0 = off)"),
             (dict(auto_exposure=2), "auto_exposure must be 0 (manual) or 1 (auto)"),
             (dict(st=None), "null state with auto exposure"),
             (dict(st=C.c_void_p(state.data_ptr() + 2)), "state not 4-byte aligned"),
             (dict(color=None), "null buffer"), (dict(background=None), "null buffer"), (dict(alpha=None, transparent=1), "null buffer"),
             (dict(dst=None), "null buffer"),
             (dict(scr=None), "null scratch with auto exposure or bloom"),
             (dict(nbytes=need - 1), "scratch smaller than rayn_display_scratch_bytes(width, height, levels)"),
             (dict(scr=C.c_void_p(scratch.data_ptr() + 4)), "scratch not 16-byte aligned"),
             (dict(fn=L.rayn_hip_display_color_device, dst=d["color"]), "d_out_color must not be d_color or d_background"),
             (dict(fn=L.rayn_hip_display_color_device, dst=None), "null buffer")]
    cases += [(dict(key=v), "key must be finite and > 0") for v in (nan, inf, 0.0, -1.0)]
    cases += [(dict(adapt=v), "adapt must be in [0, 1]") for v in (nan, -0.5, 1.5)]
    cases += [(dict(auto_exposure=0, exposure_scale=v), "exposure_scale must be finite and >= 0") for v in (nan, inf, -1.0)]
    cases += [(dict(iw2=v), "iw2 must be finite and >= 0") for v in (nan, inf, -1.0)]
    cases += [(dict(threshold=nan), "bloom threshold must be finite and strength finite and >= 0"),
              (dict(strength=-1.0), "bloom threshold must be finite and strength finite and >= 0"),
              (dict(strength=inf), "bloom threshold must be finite and strength finite and >= 0")]
    for kwargs, text in cases:
        assert call(**kwargs) == -1, kwargs  # RAYN_ERR_INVALID_ARG
        assert gpu_ctx.last_error() == text, kwargs
    assert L.rayn_hip_display_pixels_device(None, C.byref(base), 7, 0, w, h, p(d["color"]), p(d["alpha"]), p(d["background"]), p(state), p(scratch),
                                            need, p(out8), None, None, s) == -1
    # good calls after the bad ones: a manual exposure without bloom needs neither state nor scratch; parameters an operator does not read
    assert call(auto_exposure=0, levels=0, st=None, scr=None, nbytes=0) == 0
    assert call(tone=2, iw2=nan, levels=0, threshold=nan) == 0
    assert call(fn=L.rayn_hip_display_color_device, dst=outf, transparent=1) == 0
    torch.cuda.synchronize()
    # the Python wrapper refuses buffers too small for the image, and outputs of another type, before anything is enqueued
    with pytest.raises(ValueError):
        gpu_ctx.display(Display(), 7, False, w, h, d, torch.zeros(w * h * 3 - 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        gpu_ctx.display(Display(), 7, False, w, h, d, torch.zeros(w * h * 3, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        gpu_ctx.display(Display(), 7, False, w + 1, h, d, torch.zeros(3 * (w + 1) * h, dtype=torch.uint8, device="cuda"))


# ---- Film.pixels / Film.save_to / Film.render_sequence / Film.save_hdr with display= ------------------------------------------------

W, H, SAMPLES = 64, 48, 1
FRAMES, RATE, SHUTTER = [3, 4, 6], 24, 1.0 / 24.0


def _scene():
    import rayn_amd as R
    from rayn_amd import setup as S
    cam, world = S.setup((W, H))
    return R, cam, world, R.PathTracingIntegrator(max_bounces=3, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE), R.BlackmanHarrisFilter(S.FILTER_RADIUS), S.TILE_SIZE


def test_film_pixels_save_to_and_save_hdr(tmp_path, oracle):
    R, cam, world, integ, filt, tile = _scene()
    K = R.ChannelKind
    display = R.Display(exposure="auto", tone="aces", bloom=R.Bloom(1.0, 0.5, 3))
    identity = R.Display(exposure=0.0, tone="linear")
    for kinds, transparent in (([K.Color, K.Alpha, K.Background, K.WorldNormal], False), ([K.Color, K.Alpha, K.Background, K.WorldNormal], True),
                               ([K.Color, K.Alpha], False)):
        film = R.Film(kinds, (W, H))
        film.render_frame_into(world, cam, integ, filt, tile, 2, None, SAMPLES)
        # identity parameters: byte-identical to the image without display=
        assert np.array_equal(film.pixels(K.Color, transparent, display=identity), film.pixels(K.Color, transparent))
        color = film.channel(K.Color).reshape(-1, 3)
        background = film.channel(K.Background).reshape(-1, 3) if K.Background in kinds else None
        alpha = film.channel(K.Alpha).reshape(-1) if transparent else None
        want = D.display(color, W, H, display.to_abi(), background, alpha, transparent)
        assert np.array_equal(film.pixels(K.Color, transparent, display=display), want["image"])
        IO.assert_bits_equal(film.display_color(display, transparent_background=transparent).cpu().numpy(), want["d"], "display_color")
        assert np.array_equal(film.pixels(K.Alpha, transparent, display=display), film.pixels(K.Alpha, transparent))  # other channels ignore it
        out = tmp_path / f"{len(kinds)}{int(transparent)}"
        film.save_to([K.Color, K.Alpha], str(out), "x", transparent, display=display)
        assert sorted(os.listdir(out)) == ["x_alpha.png", "x_color_display.png"]
        assert (out / "x_color_display.png").read_bytes() == IO.png_bytes(tmp_path, want["image"])
        # the exposure did something: the shipped scene's emitters are far above 1 and its mean is far below
        assert not np.array_equal(want["image"], film.pixels(K.Color, transparent))
        film.save_hdr(str(out / "x.pfm"), transparent)
        hdr = D.input_color(color, background, transparent).reshape(H, W, 3)
        assert np.array_equal(image.load_pfm(out / "x.pfm").view(np.uint32), hdr.view(np.uint32))
    den = R.Denoise(2, 0.5, 0.4, 0.3)
    film.save_to([K.Color], str(tmp_path / "den"), "x", denoise=den, display=display)
    assert os.listdir(tmp_path / "den") == ["x_color_denoised_display.png"]
    with pytest.raises(ValueError, match="Display"):
        film.pixels(K.Color, display="aces")


def test_sequence_with_display_equals_per_frame_calls(tmp_path, oracle):
    R, cam, world, integ, filt, tile = _scene()
    K = R.ChannelKind
    kinds = [K.Color, K.Alpha, K.Background, K.WorldNormal]
    display = R.Display(exposure="auto", tone="aces", bloom=R.Bloom(1.0, 0.5, 3), adaptation=0.1)
    film = R.Film(kinds, (W, H))
    seq = tmp_path / "seq"
    film.render_sequence(world, cam, integ, filt, tile, FRAMES, RATE, SHUTTER, SAMPLES, [K.Alpha, K.Color], str(seq), "a", display=display)
    assert sorted(os.listdir(seq)) == sorted(f"a_{f:04d}_{s}.png" for f in FRAMES for s in ("alpha", "color_display"))
    plain = R.Film(kinds, (W, H))
    state = plain.ctx.display_state()
    f32 = np.float32
    prev, adapts = None, []
    for frame in FRAMES:
        start = f32(frame) * (f32(1.0) / f32(RATE))
        plain.render_frame_into(world, cam, integ, filt, tile, frame, (float(start), float(f32(start + f32(SHUTTER)))), SAMPLES)
        adapts.append(1.0 if prev is None else display.adapt(float(start) - float(prev)))
        prev = start
        img = plain.pixels(K.Color, display=display, display_state=state, adapt=adapts[-1])
        assert (seq / f"a_{frame:04d}_color_display.png").read_bytes() == IO.png_bytes(tmp_path, img), frame
        assert (seq / f"a_{frame:04d}_alpha.png").read_bytes() == IO.png_bytes(tmp_path, plain.pixels(K.Alpha)), frame
    assert adapts[0] == 1.0 and 0.0 < adapts[1] < adapts[2] < 1.0  # frames 3 -> 4 -> 6: one and two frame times
    # the suffix goes after whatever the Color file would have been called
    both = tmp_path / "both"
    film.render_sequence(world, cam, integ, filt, tile, FRAMES[:2], RATE, SHUTTER, SAMPLES, [K.Color], str(both), "a", denoise=R.Denoise(1, 0.5, 0.4, 0.3),
                         temporal=R.Temporal(), display=R.Display(exposure=1.0, tone="reinhard"))
    assert sorted(os.listdir(both)) == [f"a_{f:04d}_color_temporal_denoised_display.png" for f in FRAMES[:2]]
    # a sequence that does not write Color ignores display=
    none = tmp_path / "none"
    film.render_sequence(world, cam, integ, filt, tile, FRAMES[:1], RATE, SHUTTER, SAMPLES, [K.Alpha], str(none), "a", display=display)
    assert os.listdir(none) == ["a_0003_alpha.png"]
