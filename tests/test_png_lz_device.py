"""rayn_hip_deflate_lz77_device and rayn_hip_png_encode_lz77_device (rayn_amd/csrc/png_lz.hip): byte-equal - the header words included - to
the restatement in tests/png_lz_np.py on the hand-written and the coverage blocks of tests/png_lz_cases.py, on the sizes around one block,
with and without a row stride, and on images of every family; outputs and scratch between guard words, inputs untouched; the argument
checks of both entries; Film.save_to and Film.render_sequence with png="device-lz77" against "host" and "device"."""
import ctypes as C
import functools
import struct
import zlib

import numpy as np
import pytest

import device_io as IO
import png_cases as K
import png_lz_cases as KZ
import png_lz_np as Z
import png_np as P
from rayn_amd import image

pytestmark = pytest.mark.gpu

GUARD = 0xA5


def _assert_bytes(got, want, what):
    if got != P.padded(want):
        hg, hw = struct.unpack("<IIII", got[:16]), struct.unpack("<IIII", want[:16])
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError((what, "header", hg, hw, "first difference at byte", first, got[first:first + 8].hex(), want[first:first + 8].hex()))


def _written(out, bound):
    """The bytes the device wrote - header and stream padded to its word - with nothing behind them touched"""
    got = out.cpu().numpy()
    n = int(got[:4].view("<u4")[0])
    assert 6 <= n <= bound - 16, n
    written = 16 + (n + 3) // 4 * 4
    assert np.all(got[written:] == GUARD), "bytes behind the stream's last word were written"
    return got[:written].tobytes(), image.png_stream_of(got)


@functools.lru_cache(maxsize=None)
def _deflate_cases():
    return {name: (data, stride, Z.encode_filtered(data, stride)[0]) for name, data, stride in KZ.deflate_cases()}


@pytest.mark.parametrize("name", [c[0] for c in KZ.deflate_cases()])
def test_deflate_entry_is_the_restatement_byte_for_byte(gpu_ctx, name):
    import torch
    from rayn_amd import film as F
    data, stride, want = _deflate_cases()[name]
    n = len(data)
    bound, need = F.deflate_stream_bound(n), F.deflate_scratch_bytes(n)
    assert bound == Z.deflate_stream_bound(n) and bound % 16 == 0 and need % 16 == 0
    src_full, src = IO.guarded(n, torch.uint8, 0)
    src = src_full[1:n + 1] if n > 4 else src   # an input that is not aligned
    src.copy_(IO.upload_bytes(data))
    out_full, out = IO.guarded(bound, torch.uint8, GUARD)
    scr_full, scr = IO.guarded(need, torch.uint8, GUARD)
    gpu_ctx.deflate(src, out, stride, scr)
    torch.cuda.synchronize()
    IO.assert_guards(out_full, bound, GUARD, "d_out")
    IO.assert_guards(scr_full, need, GUARD, "d_scratch")
    IO.assert_is_host(src, data, "d_data", np.uint8)
    got, z = _written(out, bound)
    _assert_bytes(got, want, name)
    assert zlib.decompress(bytes(z)) == data.tobytes(), name


@functools.lru_cache(maxsize=None)
def _family(family, shape):
    w, h, bpp = shape
    img = K.family_image(family, w, h, bpp, seed=w + h)
    img.setflags(write=False)
    return img, Z.encode(img)


# 1x1; 32 800 filtered bytes, two blocks of which the second has 32; bpp 1 and 4; nine blocks
PNG_SHAPES = ((1, 1, 1), (109, 100, 3), (255, 128, 1), (300, 220, 4), (256, 256, 4))
assert P.filtered_bytes(109, 100, 3) == P.BLOCK + 32 and P.n_blocks(256, 256, 4) == 9


@pytest.mark.parametrize("shape,family", [(s, f) for s in PNG_SHAPES[:4] for f in K.FAMILIES] + [(PNG_SHAPES[4], "gradient")],
                         ids=lambda v: v if isinstance(v, str) else "%dx%dx%d" % v)
def test_png_entry_is_the_restatement_byte_for_byte(gpu_ctx, shape, family):
    import torch
    from rayn_amd import film as F
    img, want = _family(family, shape)
    h, w, bpp = img.shape
    bound, need = F.png_stream_bound(w, h, bpp), F.png_scratch_bytes_lz77(w, h, bpp)
    assert need >= F.png_scratch_bytes(w, h, bpp) + 65536 * P.n_blocks(w, h, bpp) and need % 16 == 0
    d_img = IO.upload_bytes(img)
    out_full, out = IO.guarded(bound, torch.uint8, GUARD)
    scr_full, scr = IO.guarded(need, torch.uint8, GUARD)
    gpu_ctx.png_encode_lz77(w, h, bpp, d_img, out, scr)
    torch.cuda.synchronize()
    IO.assert_guards(out_full, bound, GUARD, "d_out")
    IO.assert_guards(scr_full, need, GUARD, "d_scratch")
    IO.assert_is_host(d_img, img, "d_img", np.uint8)
    got, z = _written(out, bound)
    _assert_bytes(got, want, (shape, family))
    assert zlib.decompress(bytes(z)) == P.filter_rows(img)[0].tobytes()
    assert np.array_equal(K.decode_png(image.png_from_stream(w, h, bpp, z)), img)


def test_bad_arguments_return_invalid_arg_with_a_text(gpu_ctx):
    import torch
    from rayn_amd import _lib
    from rayn_amd import film as F
    L = _lib.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    w, h, bpp = 17, 13, 3
    n = 1000
    img = torch.zeros(max(w * h * bpp, n) + 64, dtype=torch.uint8, device="cuda")
    for png in (True, False):
        bound = F.png_stream_bound(w, h, bpp) if png else F.deflate_stream_bound(n)
        need = F.png_scratch_bytes_lz77(w, h, bpp) if png else F.deflate_scratch_bytes(n)
        out_full, out = IO.guarded(bound, torch.uint8, GUARD)
        scr_full, scr = IO.guarded(need, torch.uint8, GUARD)
        base = dict(w=w, h=h, bpp=bpp, n=n, stride=7, img=img.data_ptr(), out=out.data_ptr(), out_bytes=bound, scr=scr.data_ptr(), scr_bytes=need)

        def call(**kw):
            a = dict(base, **kw)
            if png:
                return L.rayn_hip_png_encode_lz77_device(gpu_ctx.h, a["w"], a["h"], a["bpp"], C.c_void_p(a["img"]), C.c_void_p(a["out"]), a["out_bytes"],
                                                         C.c_void_p(a["scr"]), a["scr_bytes"], s)
            return L.rayn_hip_deflate_lz77_device(gpu_ctx.h, C.c_void_p(a["img"]), a["n"], a["stride"], C.c_void_p(a["out"]), a["out_bytes"],
                                                  C.c_void_p(a["scr"]), a["scr_bytes"], s)

        shared = (({"img": None}, "null buffer"), ({"out": None}, "null buffer"), ({"scr": None}, "null buffer"),
                  ({"out": out.data_ptr() + 4}, "misaligned"), ({"scr": scr.data_ptr() + 8}, "misaligned"),
                  ({"out": img.data_ptr(), "out_bytes": bound}, "must not overlap d_"), ({"scr": out.data_ptr()}, "d_scratch overlaps"))
        if png:
            own = (({"w": 0}, "zero-sized image"), ({"h": 0}, "zero-sized image"), ({"bpp": 2}, "bpp must be 1, 3 or 4"), ({"bpp": 0}, "bpp must be 1, 3 or 4"),
                   ({"w": 1 << 24, "bpp": 1}, "row longer than 2^24 bytes"), ({"w": 1 << 16, "h": 1 << 15, "bpp": 1}, "larger than 2^31 filtered bytes"),
                   ({"out_bytes": bound - 1}, "rayn_png_stream_bound"), ({"scr_bytes": need - 1}, "rayn_png_scratch_bytes_lz77"))
        else:
            own = (({"n": 0}, "empty buffer"), ({"n": 1 << 31}, "2^31 bytes or more"), ({"n": 1 << 40}, "2^31 bytes or more"),
                   ({"out_bytes": bound - 1}, "rayn_deflate_stream_bound"), ({"scr_bytes": need - 1}, "rayn_deflate_scratch_bytes"))
        for kw, text in own + shared:
            assert call(**kw) == -1, kw  # RAYN_ERR_INVALID_ARG
            assert text in gpu_ctx.last_error(), (kw, gpu_ctx.last_error())
        torch.cuda.synchronize()
        IO.assert_guards(out_full, 0, GUARD, "d_out after rejected calls")  # nothing was written
        IO.assert_guards(scr_full, 0, GUARD, "d_scratch after rejected calls")
        assert call() == 0  # a good call after the bad ones
        torch.cuda.synchronize()
    assert L.rayn_hip_png_encode_lz77_device(None, w, h, bpp, None, None, 0, None, 0, None) == -1
    assert L.rayn_hip_deflate_lz77_device(None, None, 0, 0, None, 0, None, 0, None) == -1
    # the size helpers need no context; the Python wrappers refuse tensors too small before anything is enqueued
    for bad in (0, 1 << 31, 1 << 40):
        assert F.deflate_stream_bound(bad) == 0 == F.deflate_scratch_bytes(bad) == Z.deflate_stream_bound(bad)
    assert F.png_scratch_bytes_lz77(5, 5, 2) == 0 == F.png_scratch_bytes_lz77(0, 5, 3)
    with pytest.raises(ValueError, match="d_out"):
        gpu_ctx.deflate(img[:n], out[:16])
    with pytest.raises(ValueError, match="d_out"):
        gpu_ctx.png_encode_lz77(w, h, bpp, img, out[:16])


# ---- Film.save_to and Film.render_sequence with png="device-lz77" ---------------------------------------------------------------------------

W, H, SAMPLES = 64, 48, 1
FRAMES, RATE, SHUTTER = [3, 4], 24, 1.0 / 24.0


def _scene():
    import rayn_amd as R
    from rayn_amd import setup as S
    cam, world = S.setup((W, H))
    return R, cam, world, R.PathTracingIntegrator(max_bounces=3, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE), R.BlackmanHarrisFilter(S.FILTER_RADIUS), S.TILE_SIZE


def _assert_same_pixels_lz_stream(other_dir, lz_dir):
    """The same file names; every lz77 file decodes to exactly the pixels of the other file of its name and is png_from_stream of the
    restatement on those pixels"""
    other, lz = IO.read_folder(str(other_dir)), IO.read_folder(str(lz_dir))
    assert sorted(other) == sorted(lz) and other
    for name in other:
        pixels = K.decode_png(other[name])
        assert np.array_equal(K.decode_png(lz[name]), pixels), name
        h, w, bpp = pixels.shape
        assert (w, h) == (W, H)
        assert lz[name] == image.png_from_stream(w, h, bpp, Z.encode(pixels)[16:]), name
        assert lz[name] != other[name]  # another encoder's bytes


def test_save_to_with_lz77_writes_the_pixels_of_the_host_encoder(tmp_path):
    R, cam, world, integ, filt, tile = _scene()
    Kd = R.ChannelKind
    film = R.Film([Kd.Color, Kd.Alpha, Kd.Background, Kd.WorldNormal], (W, H))
    film.render_frame_into(world, cam, integ, filt, tile, 2, None, SAMPLES)
    for transparent in (False, True):  # RGB and RGBA Color, grey Alpha
        host, lz = tmp_path / f"host{int(transparent)}", tmp_path / f"lz{int(transparent)}"
        film.save_to([Kd.Color, Kd.Alpha, Kd.WorldNormal], str(host), "x", transparent)
        film.save_to([Kd.Color, Kd.Alpha, Kd.WorldNormal], str(lz), "x", transparent, png="device-lz77")
        _assert_same_pixels_lz_stream(host, lz)


def test_two_frames_of_a_sequence_with_lz77_are_the_files_of_device(tmp_path):
    R, cam, world, integ, filt, tile = _scene()
    Kd = R.ChannelKind
    write = [Kd.Alpha, Kd.WorldNormal, Kd.Color]
    film = R.Film([Kd.Color, Kd.Alpha, Kd.Background, Kd.WorldNormal], (W, H))
    dev, lz = tmp_path / "device", tmp_path / "lz"
    film.render_sequence(world, cam, integ, filt, tile, FRAMES, RATE, SHUTTER, SAMPLES, write, str(dev), "a", png="device")
    stats = film.render_sequence(world, cam, integ, filt, tile, FRAMES, RATE, SHUTTER, SAMPLES, write, str(lz), "a", png="device-lz77")
    assert [st["frame"] for st in stats] == FRAMES
    _assert_same_pixels_lz_stream(dev, lz)
