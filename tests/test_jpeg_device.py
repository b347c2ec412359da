"""The device JPEG encoder (rayn_hip_jpeg_encode_device, an extension) against the restatement of include/rayn_hip.h in
tests/jpeg_np.py, byte for byte, on the named cases of tests/jpeg_cases.py; its argument checks; Film.save_jpeg and
Film.render_sequence(jpeg=, video=) on a rendered scene, the AVI read back by tests/avi_read.py."""
import ctypes as C
import io
import os
import struct

import numpy as np
import pytest
from PIL import Image

import avi_read
import device_io as IO
import jpeg_cases as K
import jpeg_np as J
from rayn_amd import image

pytestmark = pytest.mark.gpu

GUARD = 0xA5


def _encode(ctx, c):
    """The bytes the device wrote for case c - header words, scan, zero padding to its word - with the output and the scratch between
    guards and the input compared with the host's"""
    import torch
    from rayn_amd import film as F
    args = (c.width, c.height, c.bpp, c.subsampling, c.ri)
    bound, need = F.jpeg_scan_bound(*args), F.jpeg_scratch_bytes(*args)
    assert bound and need and bound % 16 == 0 and need % 16 == 0
    d_img = IO.upload_bytes(c.img)
    out_full, out = IO.guarded(bound, torch.uint8, GUARD)
    scr_full, scr = IO.guarded(need, torch.uint8, GUARD)
    ctx.jpeg_encode(c.width, c.height, c.bpp, d_img, out, c.quality, c.subsampling, c.ri, scr)
    torch.cuda.synchronize()
    IO.assert_guards(out_full, bound, GUARD, "d_out")
    IO.assert_guards(scr_full, need, GUARD, "d_scratch")
    IO.assert_is_host(d_img, c.img, "d_img", np.uint8)
    got = out.cpu().numpy()
    n = int(got[:4].view("<u4")[0])
    assert 1 <= n <= bound - 16, n
    written = 16 + (n + 3) // 4 * 4
    assert np.all(got[written:] == GUARD), "bytes behind the scan's last word were written"
    return got[:written].tobytes()


@pytest.mark.parametrize("name", K.NAMES)
def test_scan_is_the_restatement_byte_for_byte(gpu_ctx, name):
    from rayn_amd import Jpeg
    c = K.cases()[name]
    got, want = _encode(gpu_ctx, c), c.ref.encoded
    if got != want:
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError((name, "header", struct.unpack("<4I", got[:16]), c.ref.header, "first difference at byte", first,
                              got[first:first + 8].hex(), want[first:first + 8].hex()))
    data = image.jpeg_from_scan(c.width, c.height, c.bpp, Jpeg(c.quality, "420" if c.subsampling else "444", c.ri), got)
    assert data == c.ref.file
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), np.asarray(Image.open(io.BytesIO(c.ref.file))))


def test_bad_arguments_return_invalid_arg_with_a_text(gpu_ctx):
    import torch
    from rayn_amd import _lib
    from rayn_amd import film as F
    L = _lib.lib()
    w, h, bpp = 17, 13, 3
    img = torch.zeros(w * h * bpp + 64, dtype=torch.uint8, device="cuda")
    bound, need = F.jpeg_scan_bound(w, h, bpp, 0, 2), F.jpeg_scratch_bytes(w, h, bpp, 0, 2)
    for variant in ((w, h, bpp, 1, 2), (w, h, 1, 0, 2)):  # the buffers serve every good variant below
        assert bound >= F.jpeg_scan_bound(*variant) and need >= F.jpeg_scratch_bytes(*variant)
    out_full, out = IO.guarded(bound, torch.uint8, GUARD)
    scr_full, scr = IO.guarded(need, torch.uint8, GUARD)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    base = dict(w=w, h=h, bpp=bpp, q=90, sub=0, ri=2, img=img.data_ptr(), out=out.data_ptr(), out_bytes=bound, scr=scr.data_ptr(), scr_bytes=need)

    def call(**kw):
        a = dict(base, **kw)
        return L.rayn_hip_jpeg_encode_device(gpu_ctx.h, a["w"], a["h"], a["bpp"], a["q"], a["sub"], a["ri"], C.c_void_p(a["img"]), C.c_void_p(a["out"]),
                                             a["out_bytes"], C.c_void_p(a["scr"]), a["scr_bytes"], s)

    for kw, text in (({"w": 0}, "zero-sized image"), ({"h": 0}, "zero-sized image"), ({"w": 65536}, "at most 65535"),
                     ({"bpp": 2}, "bpp must be 1 or 3"), ({"bpp": 4}, "bpp must be 1 or 3"), ({"q": 0}, "quality must be in 1..100"),
                     ({"q": 101}, "quality must be in 1..100"), ({"ri": 0}, "restart_interval must be in 1..65535"),
                     ({"ri": 65536}, "restart_interval must be in 1..65535"), ({"sub": 2}, "subsampling must be 0"),
                     ({"bpp": 1, "sub": 1}, "4:2:0 needs three components"), ({"w": 65535, "h": 65535, "ri": 1}, "scan bound of 2^31"),
                     ({"img": None}, "null buffer"), ({"out": None}, "null buffer"), ({"scr": None}, "null buffer"),
                     ({"out": out.data_ptr() + 4}, "misaligned"), ({"scr": scr.data_ptr() + 8}, "misaligned"),
                     ({"out_bytes": bound - 1}, "rayn_jpeg_scan_bound"), ({"scr_bytes": need - 1}, "rayn_jpeg_scratch_bytes"),
                     ({"out": img.data_ptr(), "out_bytes": bound}, "must not overlap d_img"), ({"scr": out.data_ptr()}, "d_scratch overlaps")):
        assert call(**kw) == -1, kw  # RAYN_ERR_INVALID_ARG
        assert text in gpu_ctx.last_error(), (kw, gpu_ctx.last_error())
    assert L.rayn_hip_jpeg_encode_device(None, w, h, bpp, 90, 0, 2, None, None, 0, None, 0, None) == -1
    torch.cuda.synchronize()
    IO.assert_guards(out_full, 0, GUARD, "d_out after rejected calls")  # nothing was written
    IO.assert_guards(scr_full, 0, GUARD, "d_scratch after rejected calls")
    assert call() == 0 and call(sub=1) == 0 and call(bpp=1) == 0  # good calls after the bad ones
    torch.cuda.synchronize()
    # the Python wrapper refuses tensors too small for the image before anything is enqueued
    with pytest.raises(ValueError, match="d_out"):
        gpu_ctx.jpeg_encode(w, h, bpp, img, out[:bound - 16], 90, 0, 2, scr)
    with pytest.raises(ValueError, match="d_img"):
        gpu_ctx.jpeg_encode(w, h, bpp, img[:10], out, 90, 0, 2, scr)


# ---- Film.save_jpeg and Film.render_sequence(jpeg=, video=) -------------------------------------------------------------------------------

W, H, SAMPLES = 32, 24, 1
FRAMES, RATE, SHUTTER = [3, 4, 6], 24, 1.0 / 24.0


def _scene():
    import rayn_amd as R
    from rayn_amd import setup as S
    cam, world = S.setup((W, H))
    return R, cam, world, R.PathTracingIntegrator(max_bounces=3, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE), R.BlackmanHarrisFilter(S.FILTER_RADIUS), S.TILE_SIZE


def _restated(pixels, options):
    h, w, bpp = pixels.shape
    return J.encode(pixels, options.quality, options.mode(bpp), options.restart).file


def _png_pixels(data):
    a = np.asarray(Image.open(io.BytesIO(data)))
    return a.reshape(a.shape[0], a.shape[1], -1)


def test_save_jpeg_is_the_restatement_of_the_films_pixels(tmp_path):
    R, cam, world, integ, filt, tile = _scene()
    Kd = R.ChannelKind
    film = R.Film([Kd.Color, Kd.Alpha, Kd.Background, Kd.WorldNormal], (W, H))
    film.render_frame_into(world, cam, integ, filt, tile, 2, None, SAMPLES)
    display = R.Display(exposure=1.0, tone="reinhard")
    for options in (R.Jpeg(), R.Jpeg(75, "444", 5)):
        out = tmp_path / f"q{options.quality}"
        film.save_jpeg([Kd.Color, Kd.Alpha, Kd.WorldNormal], str(out), "x", options)
        film.save_jpeg([Kd.Color], str(out), "x", options, display=display)
        got = IO.read_folder(str(out))
        assert sorted(got) == ["x_alpha.jpg", "x_color.jpg", "x_color_display.jpg", "x_normal.jpg"]
        assert got["x_color.jpg"] == _restated(film.pixels(Kd.Color), options)
        assert got["x_color_display.jpg"] == _restated(film.pixels(Kd.Color, display=display), options)
        assert got["x_alpha.jpg"] == _restated(film.pixels(Kd.Alpha), options)  # grey: 4:2:0 falls back to the only form
        assert got["x_normal.jpg"] == _restated(film.pixels(Kd.WorldNormal), options)
        assert got["x_color.jpg"] != got["x_color_display.jpg"]
    with pytest.raises(ValueError, match="no alpha"):
        film.save_jpeg([Kd.Alpha, Kd.Color], str(tmp_path / "never"), "x", transparent_background=True)
    with pytest.raises(ValueError, match="must be a Jpeg"):
        film.save_jpeg([Kd.Color], str(tmp_path / "never"), "x", 90)
    assert not (tmp_path / "never").exists()


def _check_video(folder, avi_path, options, suffix):
    """The AVI's frames are the folder's {frame}_{suffix}.jpg files, in frame order, and every .jpg is the restatement of its PNG's pixels"""
    files = IO.read_folder(str(folder))
    a = avi_read.read(open(avi_path, "rb").read())
    want = [files[f"a_{f:04d}_{suffix}.jpg"] for f in FRAMES]
    assert a["frames"] == want and len(set(want)) == len(FRAMES)  # distinct frames: the order is told
    assert a["avih"][4] == len(FRAMES) and a["avih"][8:10] == (W, H) and (a["strh"]["rate"], a["strh"]["scale"]) == (RATE, 1)
    for name, data in files.items():
        if name.endswith(".jpg"):
            assert data == _restated(_png_pixels(files[name[:-4] + ".png"]), options), name
    return files


def test_sequence_writes_jpegs_and_a_video_and_leaves_the_pngs_alone(tmp_path):
    R, cam, world, integ, filt, tile = _scene()
    Kd = R.ChannelKind
    write = [Kd.Alpha, Kd.WorldNormal, Kd.Color]
    film = R.Film([Kd.Color, Kd.Alpha, Kd.Background, Kd.WorldNormal], (W, H))
    plain, both = tmp_path / "plain", tmp_path / "both"
    options = R.Jpeg(85, "420", 2)
    film.render_sequence(world, cam, integ, filt, tile, FRAMES, RATE, SHUTTER, SAMPLES, write, str(plain), "a")
    stats = film.render_sequence(world, cam, integ, filt, tile, FRAMES, RATE, SHUTTER, SAMPLES, write, str(both), "a", jpeg=options,
                                 video=R.Video(str(tmp_path / "both.avi"), options))
    assert [st["frame"] for st in stats] == FRAMES
    files = _check_video(both, tmp_path / "both.avi", options, "color")
    before = IO.read_folder(str(plain))
    assert {n: d for n, d in files.items() if n.endswith(".png")} == before  # byte for byte
    assert sorted(files) == sorted(list(before) + [n[:-4] + ".jpg" for n in before])
    # the video's own parameters beside jpeg='s (above they were equal, and the Color image encoded once for both), and the video alone
    other = R.Jpeg(60, "444", 7)
    film.render_sequence(world, cam, integ, filt, tile, FRAMES, RATE, SHUTTER, SAMPLES, write, str(tmp_path / "two"), "a", jpeg=options,
                         video=R.Video(str(tmp_path / "two.avi"), other))
    assert IO.read_folder(str(tmp_path / "two")) == files
    assert avi_read.read((tmp_path / "two.avi").read_bytes())["frames"] == [_restated(_png_pixels(before[f"a_{f:04d}_color.png"]), other) for f in FRAMES]
    film.render_sequence(world, cam, integ, filt, tile, FRAMES, RATE, SHUTTER, SAMPLES, write, str(tmp_path / "alone"), "a",
                         video=R.Video(str(tmp_path / "alone" / "v.avi"), other, images=False), png="device", exr="device")
    assert os.listdir(tmp_path / "alone") == ["v.avi"]
    frames = avi_read.read((tmp_path / "alone" / "v.avi").read_bytes())["frames"]
    assert frames == [_restated(_png_pixels(before[f"a_{f:04d}_color.png"]), other) for f in FRAMES]
    # wrong values raise before anything renders
    for kw, text in ((dict(jpeg=90), "must be a Jpeg"), (dict(video="v.avi"), "must be a Video"),
                     (dict(jpeg=options, transparent_background=True), "no alpha"),
                     (dict(video=R.Video(str(tmp_path / "never.avi")), transparent_background=True), "no alpha")):
        with pytest.raises(ValueError, match=text):
            film.render_sequence(world, cam, integ, filt, tile, FRAMES, RATE, SHUTTER, SAMPLES, write, str(tmp_path / "never"), "a", **kw)
    with pytest.raises(ValueError, match="Color"):
        film.render_sequence(world, cam, integ, filt, tile, FRAMES, RATE, SHUTTER, SAMPLES, [Kd.Alpha], str(tmp_path / "never"), "a",
                             video=R.Video(str(tmp_path / "never.avi")))
    assert not (tmp_path / "never").exists() and not (tmp_path / "never.avi").exists()


@pytest.mark.parametrize("shown", ["preview", "interpolate"])
def test_the_video_shows_the_image_the_color_png_shows(tmp_path, shown):
    R, cam, world, integ, filt, tile = _scene()
    Kd = R.ChannelKind
    film = R.Film([Kd.Color, Kd.Alpha, Kd.Background, Kd.WorldNormal], (W, H))
    kw, suffix = {"preview": (dict(preview=R.Preview()), "color_preview"),
                  "interpolate": (dict(interpolate=R.Interpolate(2), display=R.Display(exposure=1.0, tone="reinhard")), "color_interp_display")}[shown]
    options = R.Jpeg(90, "444", 32)
    film.render_sequence(world, cam, integ, filt, tile, FRAMES, RATE, SHUTTER, SAMPLES, [Kd.Color, Kd.Alpha], str(tmp_path / "s"), "a", jpeg=options,
                         video=R.Video(str(tmp_path / "s.avi"), options), **kw)
    files = _check_video(tmp_path / "s", tmp_path / "s.avi", options, suffix)
    assert sorted(files) == sorted(f"a_{f:04d}_{s}.{ext}" for f in FRAMES for s in (suffix, "alpha") for ext in ("png", "jpg"))
