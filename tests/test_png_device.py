"""rayn_hip_png_encode_device (rayn_amd/csrc/png.hip): the zlib stream of a PNG's IDAT chunk encoded on the GPU, byte-equal - the header
words included - to the restatement in tests/png_np.py on single pixels, on filtered streams around one 32 KiB block, on several blocks
and on every content family; outputs and scratch between guard words, inputs untouched; stream order; error codes and texts; a
multi-device context; Film.save_to and Film.render_sequence with png="device" against png="host"."""
import ctypes as C
import functools
import os
import struct
import zlib

import numpy as np
import pytest

import device_io as IO
import png_cases as K
import png_np as P
from rayn_amd import image

pytestmark = pytest.mark.gpu

GUARD = 0xA5


@functools.lru_cache(maxsize=None)
def _family(family, shape):
    w, h, bpp = shape
    img = K.family_image(family, w, h, bpp, seed=w + h)
    img.setflags(write=False)
    return img, P.encode(img)


def _encode(ctx, img, stream=None, d_img=None):
    """(the bytes the device wrote: header + stream padded to its word, the zlib stream) with guard words behind the output and the
    scratch checked and the input compared with the host's"""
    import torch
    from rayn_amd import film as F
    h, w, bpp = img.shape
    bound, need = F.png_stream_bound(w, h, bpp), F.png_scratch_bytes(w, h, bpp)
    assert bound == P.stream_bound(w, h, bpp) and bound % 16 == 0 and need % 16 == 0
    d_img = IO.upload_bytes(img) if d_img is None else d_img
    out_full, out = IO.guarded(bound, torch.uint8, GUARD)
    scr_full, scr = IO.guarded(need, torch.uint8, GUARD)
    ctx.png_encode(w, h, bpp, d_img, out, scr, stream=stream)
    torch.cuda.synchronize()
    IO.assert_guards(out_full, bound, GUARD, "d_out")
    IO.assert_guards(scr_full, need, GUARD, "d_scratch")
    IO.assert_is_host(d_img, img, "d_img", np.uint8)
    got = out.cpu().numpy()
    n = int(got[:4].view("<u4")[0])
    assert 6 <= n <= bound - 16, n
    written = 16 + (n + 3) // 4 * 4
    assert np.all(got[written:] == GUARD), "bytes behind the stream's last word were written"
    return got[:written].tobytes(), image.png_stream_of(got)


def _assert_stream(ctx, img, want, what):
    got, z = _encode(ctx, img)
    if got != P.padded(want):
        hg, hw = struct.unpack("<IIII", got[:16]), struct.unpack("<IIII", want[:16])
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError((what, "header", hg, hw, "first difference at byte", first, got[first:first + 8].hex(), want[first:first + 8].hex()))
    assert zlib.decompress(bytes(z)) == P.filter_rows(img)[0].tobytes(), what


@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_stream_is_the_restatement_byte_for_byte(gpu_ctx, shape, family):
    img, want = _family(family, shape)
    _assert_stream(gpu_ctx, img, want, (shape, family))


def test_random_blocks_are_stored_and_zero_blocks_are_a_few_bytes(gpu_ctx):
    """What the header's words say: every block of a uniform-random image is stored, none of an all-zero one, whose blocks are a few bytes
    behind their 1222-bit header"""
    for family, stored in (("random", 3), ("zero", 0)):
        img, _ = _family(family, (300, 100, 3))
        got, z = _encode(gpu_ctx, img)
        n, r, blocks, st = struct.unpack("<IIII", got[:16])
        assert (r, blocks, st) == (P.filtered_bytes(300, 100, 3), 3, stored), family
        if not stored:
            assert n <= 2 + 3 * (153 + 40 + 5) + 4


@pytest.mark.parametrize("case", ["run_edges_1", "run_edges_3", "run_edges_4", "fibonacci", "three_symbols", "run_across_blocks"])
def test_token_and_length_limit_edges_laid_into_rows(gpu_ctx, case):
    """png_cases' blocks as images: the runs of every edge length (behind the filter they stay runs), the Fibonacci counts on one row, which
    the filter leaves alone, so that the kernel halves its frequencies once; a block of one literal, one length code and end-of-block; a
    run that lies across a block start"""
    if case.startswith("run_edges"):
        bpp = int(case[-1])
        img = K.rows_of(K.run_edges_bytes(), 97, bpp)
    elif case == "fibonacci":
        data = K.fibonacci_bytes()
        img = K.rows_of(data, len(data), 1)
        r, types = P.filter_rows(img)
        info = P.huffman_block(r, True)[2]
        assert types.tolist() == [0] and info["halvings"] == 1 and max(P.tree_depths(info["freq"])) > 15  # the case does what it is for
    elif case == "three_symbols":
        img = np.zeros((1, 258 * 20, 1), np.uint8)  # R: the filter type 0 and 5160 zeros
        assert sum(1 for f in P.token_frequencies(P.block_tokens(P.filter_rows(img)[0])) if f) == 3
    else:
        img = np.zeros((2, P.BLOCK - 101, 1), np.uint8)  # row 1 of R, zeros from its type byte on, lies across byte 32768
        img[0, :50] = 9
    _assert_stream(gpu_ctx, img, P.encode(img), case)


def test_entry_is_stream_ordered(gpu_ctx):
    """On a stream of the caller's, behind a copy that writes the input: the encoder sees the copied image"""
    import torch
    img, want = _family("gradient", (300, 100, 3))
    src = IO.upload_bytes(img)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_img = torch.zeros_like(src)
        d_img.copy_(src)  # queued on s before the encoder
        got, _ = _encode(gpu_ctx, img, stream=s.cuda_stream, d_img=d_img)
    assert got == P.padded(want)


def test_multi_device_context_runs_on_the_first_device():
    import rayn_amd
    img, want = _family("mask", (300, 100, 3))
    ctx = rayn_amd.Context([0, 0])
    try:
        got, _ = _encode(ctx, img)
    finally:
        ctx.close()
    assert got == P.padded(want)


def test_bad_arguments_return_invalid_arg_with_a_text(gpu_ctx):
    import torch
    from rayn_amd import _lib
    from rayn_amd import film as F
    L = _lib.lib()
    w, h, bpp = 17, 13, 3
    img = torch.zeros(w * h * bpp + 64, dtype=torch.uint8, device="cuda")
    bound, need = F.png_stream_bound(w, h, bpp), F.png_scratch_bytes(w, h, bpp)
    out_full, out = IO.guarded(bound, torch.uint8, GUARD)
    scr_full, scr = IO.guarded(need, torch.uint8, GUARD)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    base = dict(w=w, h=h, bpp=bpp, img=img.data_ptr(), out=out.data_ptr(), out_bytes=bound, scr=scr.data_ptr(), scr_bytes=need)

    def call(**kw):
        a = dict(base, **kw)
        return L.rayn_hip_png_encode_device(gpu_ctx.h, a["w"], a["h"], a["bpp"], C.c_void_p(a["img"]), C.c_void_p(a["out"]), a["out_bytes"],
                                            C.c_void_p(a["scr"]), a["scr_bytes"], s)

    for kw, text in (({"w": 0}, "zero-sized image"), ({"h": 0}, "zero-sized image"), ({"bpp": 2}, "bpp must be 1, 3 or 4"), ({"bpp": 0}, "bpp must be 1, 3 or 4"),
                     ({"w": 1 << 24, "bpp": 1}, "row longer than 2^24 bytes"), ({"w": 1 << 16, "h": 1 << 15, "bpp": 1}, "larger than 2^31 filtered bytes"),
                     ({"img": None}, "null buffer"), ({"out": None}, "null buffer"), ({"scr": None}, "null buffer"),
                     ({"out": out.data_ptr() + 4}, "misaligned"), ({"scr": scr.data_ptr() + 8}, "misaligned"),
                     ({"out_bytes": bound - 1}, "rayn_png_stream_bound"), ({"scr_bytes": need - 1}, "rayn_png_scratch_bytes"),
                     ({"out": img.data_ptr(), "out_bytes": bound}, "must not overlap d_img"), ({"scr": out.data_ptr()}, "d_scratch overlaps")):
        assert call(**kw) == -1, kw  # RAYN_ERR_INVALID_ARG
        assert text in gpu_ctx.last_error(), (kw, gpu_ctx.last_error())
    assert L.rayn_hip_png_encode_device(None, w, h, bpp, None, None, 0, None, 0, None) == -1
    torch.cuda.synchronize()
    IO.assert_guards(out_full, 0, GUARD, "d_out after rejected calls")  # nothing was written
    IO.assert_guards(scr_full, 0, GUARD, "d_scratch after rejected calls")
    assert call() == 0  # a good call after the bad ones
    torch.cuda.synchronize()
    # the Python wrapper refuses tensors too small for the image before anything is enqueued
    with pytest.raises(ValueError, match="d_out"):
        gpu_ctx.png_encode(w, h, bpp, img, out[:bound - 16], scr)
    with pytest.raises(ValueError, match="d_img"):
        gpu_ctx.png_encode(w, h, bpp, img[:10], out, scr)


# ---- Film.save_to and Film.render_sequence with png="device" -----------------------------------------------------------------------------------

W, H, SAMPLES = 64, 48, 1
FRAMES, RATE, SHUTTER = [3, 4, 6], 24, 1.0 / 24.0


def _scene():
    import rayn_amd as R
    from rayn_amd import setup as S
    cam, world = S.setup((W, H))
    return R, cam, world, R.PathTracingIntegrator(max_bounces=3, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE), R.BlackmanHarrisFilter(S.FILTER_RADIUS), S.TILE_SIZE


def _assert_same_pixels_other_stream(host_dir, device_dir):
    """The same file names; every device file decodes to exactly the pixels of the host file of its name and is png_from_stream of the
    restatement on those pixels"""
    host, dev = IO.read_folder(str(host_dir)), IO.read_folder(str(device_dir))
    assert sorted(host) == sorted(dev) and host
    for name in host:
        pixels = K.decode_png(host[name])
        assert np.array_equal(K.decode_png(dev[name]), pixels), name
        h, w, bpp = pixels.shape
        assert (w, h) == (W, H)
        assert dev[name] == image.png_from_stream(w, h, bpp, P.encode(pixels)[16:]), name
        assert dev[name] != host[name]  # another encoder's bytes


def test_save_to_on_the_device_writes_the_same_pixels(tmp_path):
    R, cam, world, integ, filt, tile = _scene()
    Kd = R.ChannelKind
    film = R.Film([Kd.Color, Kd.Alpha, Kd.Background, Kd.WorldNormal], (W, H))
    film.render_frame_into(world, cam, integ, filt, tile, 2, None, SAMPLES)
    for transparent in (False, True):  # RGB and RGBA Color, grey Alpha
        host, dev = tmp_path / f"host{int(transparent)}", tmp_path / f"device{int(transparent)}"
        film.save_to([Kd.Color, Kd.Alpha, Kd.WorldNormal], str(host), "x", transparent)
        film.save_to([Kd.Color, Kd.Alpha, Kd.WorldNormal], str(dev), "x", transparent, png="device")
        _assert_same_pixels_other_stream(host, dev)
    assert (tmp_path / "host0" / "x_color.png").read_bytes() == IO.png_bytes(tmp_path, film.pixels(Kd.Color))  # the default is what it was
    with pytest.raises(ValueError, match="png must be one of"):
        film.save_to([Kd.Color], str(tmp_path / "never"), "x", png="gpu")
    assert not (tmp_path / "never").exists()


def test_sequence_on_the_device_writes_the_same_pixels(tmp_path):
    R, cam, world, integ, filt, tile = _scene()
    Kd = R.ChannelKind
    kinds = [Kd.Color, Kd.Alpha, Kd.Background, Kd.WorldNormal]
    write = [Kd.Alpha, Kd.WorldNormal, Kd.Color]
    film = R.Film(kinds, (W, H))
    host, dev = tmp_path / "host", tmp_path / "device"
    film.render_sequence(world, cam, integ, filt, tile, FRAMES, RATE, SHUTTER, SAMPLES, write, str(host), "a")
    stats = film.render_sequence(world, cam, integ, filt, tile, FRAMES, RATE, SHUTTER, SAMPLES, write, str(dev), "a", png="device")
    assert [st["frame"] for st in stats] == FRAMES
    assert sorted(os.listdir(dev)) == sorted(f"a_{f:04d}_{s}.png" for f in FRAMES for s in ("alpha", "normal", "color"))
    _assert_same_pixels_other_stream(host, dev)
    # with a display transform and a denoiser in front, and frames generated between keys: the encoder takes whatever image the job made
    shown = dict(denoise=R.Denoise(1, 0.5, 0.4, 0.3), display=R.Display(exposure=1.0, tone="reinhard"), interpolate=R.Interpolate(2))
    film.render_sequence(world, cam, integ, filt, tile, FRAMES, RATE, SHUTTER, SAMPLES, [Kd.Color], str(tmp_path / "host2"), "a", **shown)
    film.render_sequence(world, cam, integ, filt, tile, FRAMES, RATE, SHUTTER, SAMPLES, [Kd.Color], str(tmp_path / "device2"), "a", png="device", **shown)
    _assert_same_pixels_other_stream(tmp_path / "host2", tmp_path / "device2")
    with pytest.raises(ValueError, match="png must be one of"):
        film.render_sequence(world, cam, integ, filt, tile, FRAMES, RATE, SHUTTER, SAMPLES, write, str(tmp_path / "never"), "a", png="zlib")
    assert not (tmp_path / "never").exists()
