"""rayn_hip_save_to_pixels_device (rayn_amd/csrc/save_to.hip): Film::save_to's per-pixel post-process (src/film.rs:205-378) on the
GPU, byte-equal to the oracle's arm-by-arm restatement (oracle_save_to_pixels) and to rayn_amd/image.py, on adversarial and
oracle-rendered films; exhaustively over every f32 bit pattern in [0, 1] through the gamma arm and every bit pattern through the
alpha quantiser; stream order; error codes and texts."""
import ctypes as C

import numpy as np
import pytest

import device_io as IO
from common import case
from rayn_amd import image

pytestmark = pytest.mark.gpu

ALL = 15  # have_mask: bit k = ChannelKind k (0 Color, 1 Alpha, 2 Background, 3 WorldNormal)


def _oracle_pixels(oracle, kind, film, mask, transparent):
    L = oracle.lib()
    h, w = film["alpha"].shape
    L.oracle_save_to_pixels.restype = C.c_int
    arrs = {k: np.ascontiguousarray(film[k], np.float32) for k in ("color", "alpha", "background", "normal")}
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    out = np.zeros(h * w * 4, np.uint8)
    bpp = L.oracle_save_to_pixels(C.c_uint32(kind), mask & 1, (mask >> 1) & 1, (mask >> 2) & 1, (mask >> 3) & 1, int(transparent), C.c_uint32(w), C.c_uint32(h),
                                  fp(arrs["color"]), fp(arrs["alpha"]), fp(arrs["background"]), fp(arrs["normal"]), out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return None if bpp < 0 else out[: h * w * bpp].reshape(h, w, bpp)


def _image_py(kind, film, mask, transparent):
    """image.py's arm for the combination (the host reference), or None where save_to fails."""
    have = lambda k: bool(mask >> k & 1)
    if kind == 0:
        if have(0) and have(1) and transparent:
            return image.color_image(film["color"], alpha=film["alpha"], transparent_background=True)
        if have(0) and have(2) and not transparent:
            return image.color_image(film["color"], background=film["background"])
        if have(0) and not have(2) and not transparent:
            return image.color_image(film["color"])
        return None
    if not have(kind):
        return None
    return {1: lambda: image.alpha_image(film["alpha"]), 2: lambda: image.background_image(film["background"]),
            3: lambda: image.normal_image(film["normal"])}[kind]()


def _adversarial(h, w, seed):
    """test_image.py's adversarial film at any size: random values around [0, 1], the specials (NaN, +-inf, +-0, 1, tiny, huge, tiny
    negative), values whose gamma-corrected image sits next to an 8-bit step and alphas on the 8-bit steps, as far as the film holds them."""
    rng = np.random.default_rng(seed)
    f = {"color": rng.uniform(-0.2, 1.4, (h, w, 3)).astype(np.float32), "alpha": rng.uniform(-0.1, 1.1, (h, w)).astype(np.float32),
         "background": rng.uniform(0.0, 0.5, (h, w, 3)).astype(np.float32), "normal": rng.uniform(-1.2, 1.2, (h, w, 3)).astype(np.float32)}
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, 1e-30, 3.0e38, -1e-10, 1e-45, -np.nan], np.float32)

    def put(key, at, vals):
        flat = f[key].reshape(-1)
        n = max(0, min(vals.size, flat.size - at))
        flat[at: at + n] = vals[:n]

    put("color", 0, special)
    put("alpha", 0, special)
    put("background", 0, special[::-1].copy())
    put("normal", 0, special)
    k = np.arange(1, 255, dtype=np.float64)
    edge = ((k / 255.0) ** 2.2).astype(np.float32)
    edge = np.concatenate([edge, np.nextafter(edge, np.float32(0)), np.nextafter(edge, np.float32(2))])
    put("color", 20, edge)
    put("background", 40, edge)
    put("alpha", 20, (k / 255.0).astype(np.float32))
    put("normal", 20, (k / 127.5 - 1.0).astype(np.float32))
    return f


def _device_pixels(ctx, kind, film_d, mask, transparent, w, h, stream=None):
    import torch
    from rayn_amd import film as F
    bpp = F.save_to_bpp(kind, mask, transparent)
    full, out = IO.guarded(h * w * bpp, torch.uint8, 0xA5, 64)  # 64 guard bytes after the image
    ctx.save_to_pixels(kind, mask, transparent, w, h, film_d, out, stream)
    torch.cuda.synchronize()
    IO.assert_guards(full, h * w * bpp, 0xA5, "the image")
    return out.cpu().numpy().reshape(h, w, bpp)


def _films(oracle):
    wd, p = case("s2", 40, 24, 2, 3)
    tabs = oracle.build_tables(8, 3, p.volume_marches, p.frame, 40, 24)
    rendered, _ = oracle.render(wd, p, tabs)
    return [("rendered 40x24", rendered)] + [(f"adversarial {w}x{h}", _adversarial(h, w, seed)) for seed, (w, h) in enumerate([(1, 1), (3, 257), (257, 3), (1280, 720)])]


def test_every_arm_matches_the_oracle_and_image_py(gpu_ctx, oracle):
    arms = [(0, ALL, True), (0, ALL, False), (0, ALL & ~4, False), (0, 1, False), (0, 3, True), (0, 5, False),
            (1, ALL, False), (1, 2, True), (2, ALL, False), (2, 4, True), (3, ALL, False), (3, 8, False)]
    for name, film in _films(oracle):
        h, w = film["alpha"].shape
        d = IO.upload_film(film)
        for kind, mask, transparent in arms:
            want = _oracle_pixels(oracle, kind, film, mask, transparent)
            assert want is not None
            assert np.array_equal(_image_py(kind, film, mask, transparent), want), (name, kind, mask, transparent)
            got = _device_pixels(gpu_ctx, kind, d, mask, transparent, w, h)
            assert got.shape == want.shape and np.array_equal(got, want), (name, kind, mask, transparent, int((got != want).sum()))
        # channels the arm does not read may be absent (null pointers)
        got = _device_pixels(gpu_ctx, 0, {"color": d["color"]}, 1, False, w, h)
        assert np.array_equal(got, _oracle_pixels(oracle, 0, film, 1, False))
        got = _device_pixels(gpu_ctx, 3, {"normal": d["normal"]}, ALL, False, w, h)
        assert np.array_equal(got, _oracle_pixels(oracle, 3, film, ALL, False))


def test_error_arms_agree_with_the_oracle(gpu_ctx, oracle):
    from rayn_amd import film as F
    film = _adversarial(4, 5, 9)
    d = IO.upload_film(film)
    for kind in range(4):
        for mask in range(16):
            for transparent in (False, True):
                want = _oracle_pixels(oracle, kind, film, mask, transparent)
                assert (F.save_to_bpp(kind, mask, transparent) < 0) == (want is None)
                if want is None:
                    assert _image_py(kind, film, mask, transparent) is None
                else:
                    assert np.array_equal(_device_pixels(gpu_ctx, kind, d, mask, transparent, 5, 4), want), (kind, mask, transparent)


def _thresholds(f, lo, hi):
    """For k = 1..255 the smallest int32 bit pattern b in [lo, hi] with f(b) >= k (f: monotone map of non-negative f32 bit patterns to
    bytes, evaluated with image.py); bisection over bit patterns, all 255 steps at once."""
    k = np.arange(1, 256, dtype=np.int64)
    a, b = np.full(255, lo, np.int64), np.full(255, hi, np.int64)  # invariant: f(b) >= k, and f(a - 1) < k unless a == lo
    assert np.all(f(np.full(255, hi, np.int64)) >= k)
    while np.any(a < b):
        m = (a + b) // 2
        ok = f(m) >= k
        b = np.where(ok, m, b)
        a = np.where(ok, a, m + 1)
    return a


def _bits_to_f32(b):
    return np.asarray(b, np.int64).astype(np.uint32).view(np.float32)


def test_gamma_arm_exhaustive_over_every_f32_in_0_1(gpu_ctx, oracle):
    """Background arm (saturated().gamma_corrected(2.2), quantised) for every f32 bit pattern 0x00000000 .. 0x3F800000 (and the patterns
    just above 1.0 that complete the last chunk, which saturate to 255), against the 255 step thresholds found with image.py."""
    import torch
    one = int(np.float32(1.0).view(np.int32))
    f = lambda b: image.background_image(np.repeat(_bits_to_f32(b)[:, None], 3, axis=1)[None])[0, :, 0].astype(np.int64)
    thr = _thresholds(f, 0, one)
    # the thresholds agree with the oracle on both sides of every step
    film = {"background": np.stack([_bits_to_f32(thr), _bits_to_f32(thr - 1)])[..., None].repeat(3, -1)}
    film.update(color=np.zeros_like(film["background"]), normal=np.zeros_like(film["background"]), alpha=np.zeros(film["background"].shape[:2], np.float32))
    o = _oracle_pixels(oracle, 2, film, ALL, False)[::-1, :, 0].astype(np.int64)  # image rows are top-down: film row 0 is the last
    assert np.array_equal(o[0], np.arange(1, 256)) and np.array_equal(o[1], np.arange(0, 255))
    thr_d = torch.from_numpy(thr.astype(np.int32)).cuda()
    chunk = 3 << 24
    base = torch.arange(chunk, dtype=torch.int32, device="cuda")
    bits = torch.empty_like(base)
    out = torch.empty(chunk, dtype=torch.uint8, device="cuda")
    n_px = chunk // 3
    checked = 0
    for lo in range(0, one + 1, chunk):
        torch.add(base, lo, out=bits)
        gpu_ctx.save_to_pixels(2, ALL, False, n_px, 1, {"background": bits.view(torch.float32)}, out)
        want = torch.searchsorted(thr_d, bits, right=True)  # steps at or below the value (bit order = value order for non-negative f32)
        bad = int((out.to(torch.int64) != want).sum())
        assert bad == 0, f"{bad} mismatches in the chunk from 0x{lo:08x}"
        checked += chunk
    torch.cuda.synchronize()
    assert checked > one


def test_alpha_quantiser_exhaustive_over_every_f32(gpu_ctx):
    """Alpha arm ((v * 255.0).min(255.0).max(0.0) as u8) for all 2^32 bit patterns: NaN (either sign) -> 255 (f32::min yields the other
    operand), negatives and -0 -> 0, non-negative values against the 255 step thresholds found with image.py."""
    import torch
    inf = int(np.float32(np.inf).view(np.int32))
    f = lambda b: image.alpha_image(_bits_to_f32(b)[None])[0, :, 0].astype(np.int64)
    thr = _thresholds(f, 0, inf)
    assert np.all(f(thr) == np.arange(1, 256)) and np.all(f(thr - 1) == np.arange(0, 255))
    with np.errstate(invalid="ignore"):
        assert np.all(f(np.array([0x7FC00000, 0x7F800001, -1, -0x00400000])) == 255)
        assert np.all(f(np.array([-(1 << 31), -(1 << 31) + 1, int(np.float32(-1.0).view(np.int32)), int(np.float32(-np.inf).view(np.int32))])) == 0)
    thr_d = torch.from_numpy(thr.astype(np.int32)).cuda()
    chunk = 1 << 26
    base = torch.arange(chunk, dtype=torch.int32, device="cuda")
    bits = torch.empty_like(base)
    out = torch.empty(chunk, dtype=torch.uint8, device="cuda")
    for lo in range(-(1 << 31), 1 << 31, chunk):
        torch.add(base, lo, out=bits)
        gpu_ctx.save_to_pixels(1, ALL, False, chunk, 1, {"alpha": bits.view(torch.float32)}, out)
        mag = bits & 0x7FFFFFFF
        want = torch.where(mag > inf, 255, torch.where(bits < 0, 0, torch.searchsorted(thr_d, bits, right=True)))
        bad = int((out.to(torch.int64) != want).sum())
        assert bad == 0, f"{bad} mismatches in the chunk from {lo:#x}"
    torch.cuda.synchronize()


def test_entry_is_stream_ordered(gpu_ctx, oracle):
    """The kernel runs on the stream it is given, after the work already queued there; its result is read after a synchronise of
    that stream alone."""
    import torch
    film = _adversarial(720, 1280, 5)
    want = _oracle_pixels(oracle, 0, film, ALL, False)
    src = IO.upload_film(film)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dst = {k: torch.zeros_like(v) for k, v in src.items()}
        for k in dst:
            dst[k].copy_(src[k])  # queued on s before the post-process: the kernel must see the copied film, not zeros
        out = torch.zeros(want.size, dtype=torch.uint8, device="cuda")
        gpu_ctx.save_to_pixels(0, ALL, False, 1280, 720, dst, out, s.cuda_stream)
        host = torch.empty(want.size, dtype=torch.uint8, pin_memory=True)
        host.copy_(out, non_blocking=True)
    s.synchronize()
    assert np.array_equal(host.numpy().reshape(want.shape), want)


def test_multi_device_context_runs_on_the_first_device(oracle):
    import rayn_amd
    film = _adversarial(17, 33, 2)
    ctx = rayn_amd.Context([0, 0])
    try:
        got = _device_pixels(ctx, 0, IO.upload_film(film), ALL, True, 33, 17)
    finally:
        ctx.close()
    assert np.array_equal(got, _oracle_pixels(oracle, 0, film, ALL, True))


def test_bad_arguments_return_invalid_arg_with_the_reference_text(gpu_ctx):
    import torch
    from rayn_amd import _lib
    L = _lib.lib()
    d = IO.upload_film(_adversarial(2, 3, 1))
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(kind, mask, transparent, w=3, h=2, film=d, dst=out):
        return L.rayn_hip_save_to_pixels_device(gpu_ctx.h, kind, mask, transparent, w, h, p(film.get("color")), p(film.get("alpha")),
                                                p(film.get("background")), p(film.get("normal")), p(dst), s)

    texts = {(0, ALL & ~2, 1): "Attempted to write Color channel with insufficient channels",
             (0, ALL & ~1, 0): "Attempted to write Color channel with insufficient channels",
             (1, ALL & ~2, 0): "Attempted to write Alpha channel but it didn't exist",
             (2, ALL & ~4, 0): "Attempted to write Background channel but it didn't exist",
             (3, ALL & ~8, 0): "Attempted to write WorldNormal channel but it didn't exist"}
    for (kind, mask, transparent), text in texts.items():
        assert call(kind, mask, transparent) == -1  # RAYN_ERR_INVALID_ARG
        assert gpu_ctx.last_error() == text
    assert call(4, ALL, 0) == -1 and "ChannelKind" in gpu_ctx.last_error()
    assert call(0, ALL, 0, w=0) == -1 and gpu_ctx.last_error() == "zero-sized image"
    assert call(0, ALL, 0, h=0) == -1 and gpu_ctx.last_error() == "zero-sized image"
    assert call(0, ALL, 0, film=dict(d, background=None)) == -1 and gpu_ctx.last_error() == "null buffer"
    assert call(0, ALL, 1, film=dict(d, alpha=None)) == -1 and gpu_ctx.last_error() == "null buffer"
    assert call(3, ALL, 0, dst=None) == -1 and gpu_ctx.last_error() == "null buffer"
    assert L.rayn_hip_save_to_pixels_device(None, 0, ALL, 0, 3, 2, None, None, None, None, None, None) == -1
    assert call(0, ALL, 0) == 0  # a good call after the bad ones
    torch.cuda.synchronize()
    # the Python wrapper refuses buffers too small for the image before anything is enqueued
    with pytest.raises(ValueError):
        gpu_ctx.save_to_pixels(0, ALL, True, 3, 2, d, torch.zeros(23, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        gpu_ctx.save_to_pixels(3, ALL, False, 4, 2, d, out)
