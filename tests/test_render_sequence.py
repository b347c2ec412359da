"""Film.render_sequence (rayn's main loop, src/main.rs:58-96, on the GPU): every PNG of an animated sequence is byte-identical to
image.py applied to the oracle's film of that frame at that frame's time range, and to image.py applied to the host copy of the film
the plain render_frame_into loop renders; file names, the up-front channel check and the film's final state."""
import os

import numpy as np
import pytest

from rayn_amd import image

pytestmark = pytest.mark.gpu

W, H, SAMPLES, BOUNCES = 48, 32, 2, 3
FRAMES = [3, 4, 7]  # not contiguous: the R_d tables and the time range follow the frame number, not the loop index
FRAME_RATE, SHUTTER = 24, 1.0 / 24.0


def _scene():
    import rayn_amd as R
    from rayn_amd import setup as S
    cam, world = S.setup_s3((W, H))  # the camera origin and the fractal both move with time
    return R, cam, world, R.PathTracingIntegrator(max_bounces=BOUNCES, volume_marches=2), R.BlackmanHarrisFilter(1.5)


def _time_range(frame):
    f32 = np.float32
    start = f32(frame) * (f32(1.0) / f32(FRAME_RATE))  # src/main.rs:61-62
    return float(start), float(f32(start + f32(SHUTTER)))


def _images(film, kinds, transparent):
    """image.py's images for a film dict of numpy arrays (h, w[, 3]), in save_to's arms; suffix -> uint8 image."""
    out = {}
    for kind in kinds:
        name = kind.name
        if name == "Color":
            out["color"] = (image.color_image(film["color"], alpha=film["alpha"], transparent_background=True) if transparent
                            else image.color_image(film["color"], background=film["background"]))
        elif name == "Alpha":
            out["alpha"] = image.alpha_image(film["alpha"])
        elif name == "Background":
            out["background"] = image.background_image(film["background"])
        else:
            out["normal"] = image.normal_image(film["normal"])
    return out


def _png_bytes(tmp_path, img):
    p = tmp_path / "ref.png"
    image.save(str(p), img)
    return p.read_bytes()


@pytest.mark.parametrize("transparent", [False, True])
def test_sequence_pngs_equal_the_oracle_and_the_plain_loop(tmp_path, oracle, transparent):
    R, cam, world, integ, filt = _scene()
    K = R.ChannelKind
    kinds = [K.Color, K.Alpha, K.Background, K.WorldNormal]
    film = R.Film(kinds, (W, H))
    out_dir = tmp_path / "seq"
    stats = film.render_sequence(world, cam, integ, filt, (16, 16), FRAMES, FRAME_RATE, SHUTTER, SAMPLES, kinds, str(out_dir), "anim",
                                 transparent_background=transparent)
    assert [s["frame"] for s in stats] == FRAMES and all(s["paths"] > 0 for s in stats)
    suffixes = ["color", "alpha", "background", "normal"]
    assert sorted(os.listdir(out_dir)) == sorted(f"anim_{f:04d}_{s}.png" for f in FRAMES for s in suffixes)
    assert film.progressive_epoch == len(FRAMES)

    plain = R.Film(kinds, (W, H))
    wd = world.to_desc(cam)
    seen = set()
    for frame in FRAMES:
        tr = _time_range(frame)
        p = R.frame_params(W, H, SAMPLES, BOUNCES, 2, frame, tr, (16, 16))
        ref, _ = oracle.render(wd, p, oracle.build_tables(4 * SAMPLES, BOUNCES, 2, frame, W, H), threads=16)
        plain.render_frame_into(world, cam, integ, filt, (16, 16), frame, tr, SAMPLES)
        host = {"color": plain.channel(K.Color), "alpha": plain.channel(K.Alpha), "background": plain.channel(K.Background),
                "normal": plain.channel(K.WorldNormal)}
        want_oracle, want_plain = _images(ref, kinds, transparent), _images(host, kinds, transparent)
        for s in suffixes:
            got = (out_dir / f"anim_{frame:04d}_{s}.png").read_bytes()
            assert got == _png_bytes(tmp_path, want_oracle[s]), (frame, s, "oracle")
            assert got == _png_bytes(tmp_path, want_plain[s]), (frame, s, "plain loop")
        seen.add((out_dir / f"anim_{frame:04d}_color.png").read_bytes())
    assert len(seen) == len(FRAMES), "the frames of an animated scene differ"
    # film.channels holds the last frame, as the plain loop leaves it
    for key in ("color", "alpha", "background", "normal"):
        assert np.array_equal(film.channels[key].cpu().numpy().view(np.uint32), plain.channels[key].cpu().numpy().view(np.uint32)), key


def test_insufficient_channels_raise_before_anything_renders(tmp_path):
    R, cam, world, integ, filt = _scene()
    K = R.ChannelKind
    film = R.Film([K.Color, K.Background], (W, H))
    out_dir = tmp_path / "never"
    with pytest.raises(ValueError, match="Attempted to write Color channel with insufficient channels"):
        film.render_sequence(world, cam, integ, filt, (16, 16), [1, 2], FRAME_RATE, SHUTTER, SAMPLES, [K.Background, K.Color], str(out_dir), "x",
                             transparent_background=True)
    with pytest.raises(ValueError, match="Attempted to write Alpha channel but it didn't exist"):
        film.render_sequence(world, cam, integ, filt, (16, 16), [1, 2], FRAME_RATE, SHUTTER, SAMPLES, [K.Color, K.Alpha], str(out_dir), "x")
    assert not out_dir.exists()
    assert film.channels is None and film.progressive_epoch == 0


def test_a_writer_error_stops_the_sequence_and_leaves_no_thread(tmp_path):
    import threading
    R, cam, world, integ, filt = _scene()
    K = R.ChannelKind
    film = R.Film([K.Color, K.Alpha], (W, H))
    out_dir = tmp_path / "blocked"
    out_dir.mkdir()
    (out_dir / "x_0002_alpha.png").mkdir()  # a directory where frame 2's image goes: its writer fails
    before = set(threading.enumerate())
    with pytest.raises(IsADirectoryError):
        film.render_sequence(world, cam, integ, filt, (16, 16), range(1, 9), FRAME_RATE, SHUTTER, SAMPLES, [K.Color, K.Alpha], str(out_dir), "x")
    assert set(threading.enumerate()) <= before
    assert film.progressive_epoch < 8, "the sequence went on after the writer failed"
    assert (out_dir / "x_0001_color.png").exists()
