"""rayn_hip_exr_encode_device (rayn_amd/csrc/exr.hip): byte-equal - the header words and the chunk table included - to the restatement in
tests/exr_np.py on every byte-compared case of tests/exr_cases.py under both block formats; outputs and scratch between guard bytes,
nothing behind the body's last word touched, the planes unchanged; the conversion sweep decoded by the independent reader of
tests/exr_read.py against numpy; the size helpers and every rejected argument; Film.save_exr in every mode on a small rendered film, its
G-buffer layers, and render_sequence(exr="device") against a run without exr= and the "host" run."""
import ctypes as C
import struct

import numpy as np
import pytest

import device_io as IO
import exr_cases as K
import exr_np as E
import exr_read
from rayn_amd import image

pytestmark = pytest.mark.gpu

GUARD = 0xA5


def _upload(channels):
    """The cases' planes on the device, one tensor per distinct plane: [(name, tensor, stride, offset, type)], {id: (tensor, host array)}"""
    planes = {}
    for _, p, _, _, _ in channels:
        if id(p) not in planes:
            planes[id(p)] = (IO.upload(np.ascontiguousarray(p).view(np.int32), np.int32), p)
    return [(n, planes[id(p)][0], s, o, t) for n, p, s, o, t in channels], planes


def _encode(ctx, w, h, channels, matches):
    """Context.exr_encode between guards -> the bytes written (header, table, body to its last word)"""
    import torch
    from rayn_amd import film as F
    layout = K.layout_of(channels)
    bound, need = F.exr_stream_bound(w, h, layout), F.exr_scratch_bytes(w, h, layout, bool(matches))
    assert bound == E.stream_bound(w, h, layout) and bound % 16 == 0 and need % 16 == 0 and need > 0
    d_channels, planes = _upload(channels)
    out_full, out = IO.guarded(bound, torch.uint8, GUARD)
    scr_full, scr = IO.guarded(need, torch.uint8, GUARD)
    ctx.exr_encode(w, h, d_channels, out, scr, lz77=bool(matches))
    torch.cuda.synchronize()
    IO.assert_guards(out_full, bound, GUARD, "d_out")
    IO.assert_guards(scr_full, need, GUARD, "d_scratch")
    for t, host in planes.values():
        IO.assert_is_host(t, host, "a plane", np.uint32)
    got = out.cpu().numpy()
    body, chunks = (int(v) for v in got[:8].view("<u4"))
    assert chunks == E.n_chunks(h) and 10 * chunks <= body <= bound - E.body_at(h)
    written = E.body_at(h) + (body + 3) // 4 * 4
    assert np.all(got[written:] == GUARD), "bytes behind the body's last word were written"
    return got[:written].tobytes()


@pytest.mark.parametrize("matches", (0, 1))
@pytest.mark.parametrize("name", list(K.BYTE_CASES))
def test_entry_is_the_restatement_byte_for_byte(gpu_ctx, name, matches):
    w, h, channels = K.case(name)
    want, info = K.encoded(name, matches)
    got = _encode(gpu_ctx, w, h, channels, matches)
    if got != E.padded(want):
        hg, hw = struct.unpack("<IIII", got[:16]), struct.unpack("<IIII", want[:16])
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError((name, matches, "header", hg, hw, info, "first difference at byte", first, got[first:first + 8].hex(), want[first:first + 8].hex()))
    data = image.exr_from_chunks(w, h, [(n, t) for n, _, _, _, t in channels], got)
    assert data == E.file_of(w, h, [(n.encode(), t) for n, _, _, _, t in channels], want)
    got_planes = exr_read.read(data)
    for n, p, s, o, t in channels:
        words = E.channel_words(p, s, o, w, h).reshape(h, w)[::-1]
        if t == E.HALF:
            with np.errstate(over="ignore", invalid="ignore"):
                assert np.array_equal(got_planes[n].view(np.uint16), words.view(np.float32).astype(np.float16).view(np.uint16)), n
        else:
            assert np.array_equal(got_planes[n].view(np.uint32), words), n


@pytest.mark.parametrize("matches", (0, 1))
def test_conversion_sweep_decodes_to_numpys_halves(gpu_ctx, matches):
    w, h, channels = K.sweep_case()
    got = _encode(gpu_ctx, w, h, channels, matches)
    planes = exr_read.read(image.exr_from_chunks(w, h, [("Y", E.HALF)], got))
    words = channels[0][1].reshape(h, w)[::-1]
    with np.errstate(over="ignore", invalid="ignore"):
        want = words.view(np.float32).astype(np.float16).view(np.uint16)
    bad = np.argwhere(planes["Y"].view(np.uint16) != want)
    assert bad.size == 0, [(hex(words[y, x]), hex(planes["Y"].view(np.uint16)[y, x]), hex(want[y, x])) for y, x in bad[:8]]


def test_bad_arguments_return_invalid_arg_with_a_text(gpu_ctx):
    import torch
    from rayn_amd import _lib
    from rayn_amd import film as F
    L = _lib.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    w, h = 17, 19
    base_layout = [(3, 0, 1), (3, 2, 2), (1, 0, 0)]
    bound, need = F.exr_stream_bound(w, h, base_layout), F.exr_scratch_bytes(w, h, base_layout, True)
    assert bound == E.stream_bound(w, h, base_layout) and need > F.exr_scratch_bytes(w, h, base_layout, False) > 0
    plane = torch.zeros(w * h * 4 + 64, dtype=torch.int32, device="cuda")
    out_full, out = IO.guarded(bound, torch.uint8, GUARD)
    scr_full, scr = IO.guarded(need, torch.uint8, GUARD)
    base = dict(w=w, h=h, layout=base_layout, planes=[plane.data_ptr()] * 3, matches=1, out=out.data_ptr(), out_bytes=bound, scr=scr.data_ptr(),
                scr_bytes=need)

    def call(**kw):
        a = dict(base, **kw)
        n = a.get("n", len(a["layout"]))
        flat = [v for tr in a["layout"] for v in tr] or [0]
        planes = None if a["planes"] is None else (C.c_void_p * max(len(a["planes"]), 1))(*a["planes"])
        return L.rayn_hip_exr_encode_device(gpu_ctx.h, a["w"], a["h"], n, planes, (C.c_uint32 * len(flat))(*flat), a["matches"], C.c_void_p(a["out"]),
                                            a["out_bytes"], C.c_void_p(a["scr"]), a["scr_bytes"], s)

    cases = (({"w": 0}, "zero-sized image"), ({"h": 0}, "zero-sized image"),
             ({"layout": [], "planes": []}, "n_channels must be 1..16"),
             ({"layout": [(1, 0, 1)] * 17, "planes": [plane.data_ptr()] * 17}, "n_channels must be 1..16"),
             ({"layout": [(3, 0, 3)] + base_layout[1:]}, "channel type"), ({"layout": [(0, 0, 1)] + base_layout[1:]}, "stride"),
             ({"layout": [(3, 3, 1)] + base_layout[1:]}, "offset"),
             ({"w": 1 << 25, "layout": [(1, 0, 2)], "planes": [plane.data_ptr()]}, "16 rows of 2^31 bytes"),
             ({"w": 1 << 14, "h": 1 << 15, "layout": [(1, 0, 2)], "planes": [plane.data_ptr()]}, "output of 2^31 bytes"),
             ({"matches": 2}, "matches must be 0 or 1"),
             ({"planes": None}, "null buffer"), ({"planes": [plane.data_ptr(), None, plane.data_ptr()]}, "null buffer"),
             ({"out": None}, "null buffer"), ({"scr": None}, "null buffer"),
             ({"out": out.data_ptr() + 4}, "misaligned"), ({"scr": scr.data_ptr() + 8}, "misaligned"),
             ({"out_bytes": bound - 1}, "rayn_exr_stream_bound"), ({"scr_bytes": need - 1}, "rayn_exr_scratch_bytes"),
             ({"scr": out.data_ptr()}, "d_scratch overlaps d_out"),
             ({"planes": [plane.data_ptr(), out.data_ptr() + 16, plane.data_ptr()]}, "d_out must not overlap a plane"),
             ({"planes": [scr.data_ptr() + 32, plane.data_ptr(), plane.data_ptr()]}, "d_scratch overlaps a plane"))
    for kw, text in cases:
        assert call(**kw) == -1, kw  # RAYN_ERR_INVALID_ARG
        assert text in gpu_ctx.last_error(), (kw, gpu_ctx.last_error())
    torch.cuda.synchronize()
    IO.assert_guards(out_full, 0, GUARD, "d_out after rejected calls")  # nothing was written
    IO.assert_guards(scr_full, 0, GUARD, "d_scratch after rejected calls")
    assert not bool(plane.any())
    assert call() == 0  # a good call after the bad ones
    torch.cuda.synchronize()
    assert L.rayn_hip_exr_encode_device(None, w, h, 0, None, None, 0, None, 0, None, 0, None) == -1
    # the size helpers need no context and give 0 for what the entry rejects; the wrapper refuses names and tensors before anything is enqueued
    for bw, bh, bl in ((0, 1, base_layout), (1, 1, []), (1, 1, [(1, 0, 1)] * 17), (1, 1, [(1, 0, 3)]), (1, 1, [(0, 0, 1)]), (1, 1, [(2, 2, 1)]),
                       (1 << 25, 1, [(1, 0, 2)]), (1 << 14, 1 << 15, [(1, 0, 2)])):
        assert F.exr_stream_bound(bw, bh, bl) == 0 == F.exr_scratch_bytes(bw, bh, bl) == E.stream_bound(bw, bh, bl), (bw, bh, bl)
    good = [("A", plane, 3, 0, 1), ("B", plane, 3, 2, 2)]
    for names, text in ((("B", "A"), "sorted"), (("A", "A"), "twice"), (("", "A"), "1..31"), (("A", "x" * 32), "1..31")):
        with pytest.raises(ValueError, match=text):
            gpu_ctx.exr_encode(w, h, [(n,) + c[1:] for n, c in zip(names, good)], out, scr)
    with pytest.raises(ValueError, match="d_out"):
        gpu_ctx.exr_encode(w, h, good, out[:16], scr)
    with pytest.raises(ValueError, match="channel 'B'"):
        gpu_ctx.exr_encode(w, h, [good[0], ("B", plane[:100], 3, 2, 2)], out, scr)


# ---- Film.save_exr and Film.render_sequence(exr=) --------------------------------------------------------------------------------------------

W, H, SAMPLES = 64, 48, 1
FRAMES, RATE, SHUTTER = [3, 4], 24, 1.0 / 24.0
LAYERS = {"Color": ("R", "G", "B"), "Alpha": ("A",), "Background": ("background.R", "background.G", "background.B"), "WorldNormal": ("N.X", "N.Y", "N.Z")}


def _scene():
    import rayn_amd as R
    from rayn_amd import setup as S
    cam, world = S.setup((W, H))
    return R, cam, world, R.PathTracingIntegrator(max_bounces=3, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE), R.BlackmanHarrisFilter(S.FILTER_RADIUS), S.TILE_SIZE


def _film_layers(film, kinds):
    """name -> (h, w) float32, rows top-down, from the film's own planes"""
    out = {}
    for k in kinds:
        plane = film.channel(k)
        plane = plane[..., None] if plane.ndim == 2 else plane
        for i, n in enumerate(LAYERS[k.name]):
            out[n] = np.ascontiguousarray(plane[::-1, :, i])
    return out


def _assert_layers(got, want, half, what):
    for n, a in want.items():
        if a.dtype == np.uint32 or not half:
            assert got[n].dtype.itemsize == 4 and np.array_equal(got[n].view(np.uint32), a.view(np.uint32)), (what, n)
        else:
            with np.errstate(over="ignore", invalid="ignore"):
                assert got[n].dtype == np.float16 and np.array_equal(got[n].view(np.uint16), a.astype(np.float16).view(np.uint16)), (what, n)


def test_save_exr_decodes_to_the_films_bits_in_every_mode(tmp_path):
    R, cam, world, integ, filt, tile = _scene()
    Kd = R.ChannelKind
    kinds = [Kd.Color, Kd.Alpha, Kd.Background, Kd.WorldNormal]
    film = R.Film(kinds, (W, H))
    film.render_frame_into(world, cam, integ, filt, tile, 2, None, SAMPLES)
    want = _film_layers(film, kinds)
    g = film.gbuffer()
    want_g = {"P.X": g["position"][::-1, :, 0], "P.Y": g["position"][::-1, :, 1], "P.Z": g["position"][::-1, :, 2], "Z": g["t"][::-1], "id": g["object"][::-1]}
    want_g = {n: np.ascontiguousarray(a) for n, a in want_g.items()}
    decoded = {}
    for half in (True, False):
        for mode in ("host", "device", "device-lz77"):
            path = tmp_path / f"{mode}_{int(half)}.exr"
            film.save_exr(str(path), half=half, gbuffer=True, exr=mode)
            info = {}
            got = exr_read.read(path.read_bytes(), info)
            assert sorted(got) == sorted(list(want) + list(want_g)) and (info["width"], info["height"]) == (W, H)
            assert [n for n, _ in info["channels"]] == sorted(got, key=str.encode)
            _assert_layers(got, want, half, (mode, half))
            _assert_layers(got, want_g, False, (mode, half, "gbuffer"))
            decoded[mode, half] = got
        for n in decoded["host", half]:  # "host" and "device" decode identically
            for mode in ("device", "device-lz77"):
                a, b = decoded["host", half][n], decoded[mode, half][n]
                assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (mode, half, n)
    # a subset, the foreground alone, a bad mode, a kind the film lacks: nothing is written for the last two
    film.save_exr(str(tmp_path / "sub.exr"), channels=[Kd.Alpha, Kd.Color])
    assert sorted(exr_read.read((tmp_path / "sub.exr").read_bytes())) == ["A", "B", "G", "R"]
    film.save_exr(str(tmp_path / "fg.exr"), transparent_background=True)
    assert sorted(exr_read.read((tmp_path / "fg.exr").read_bytes())) == sorted(["A", "B", "G", "R", "N.X", "N.Y", "N.Z"])
    with pytest.raises(ValueError, match="exr must be one of"):
        film.save_exr(str(tmp_path / "bad.exr"), exr="gpu")
    with pytest.raises(ValueError, match="didn't exist"):
        R.Film([Kd.Color], (W, H)).save_exr(str(tmp_path / "bad.exr"), channels=[Kd.Alpha])
    assert not (tmp_path / "bad.exr").exists()
    # an upscaled film and a denoised colour go the same way
    up = film.upscaled(R.Upscale(factor=2))
    up.save_exr(str(tmp_path / "up.exr"), half=False)
    info = {}
    got = exr_read.read((tmp_path / "up.exr").read_bytes(), info)
    assert (info["width"], info["height"]) == (2 * W, 2 * H)
    _assert_layers(got, _film_layers(up, kinds), False, "upscaled")
    den = R.Denoise()
    film.save_exr(str(tmp_path / "den.exr"), channels=[Kd.Color], half=False, denoise=den)
    got = exr_read.read((tmp_path / "den.exr").read_bytes())
    dc = film.denoised_color(den).cpu().numpy().reshape(H, W, 3)[::-1]
    assert all(np.array_equal(got[n].view(np.uint32), np.ascontiguousarray(dc[..., i]).view(np.uint32)) for i, n in enumerate("RGB"))


def test_save_exr_after_preview_and_progressive(tmp_path):
    R, cam, world, integ, filt, tile = _scene()
    Kd = R.ChannelKind
    kinds = [Kd.Color, Kd.Alpha, Kd.Background, Kd.WorldNormal]
    film = R.Film(kinds, (W, H))
    film.render_progressive(world, cam, integ, filt, tile, 2, None, SAMPLES, R.Progressive(min_epochs=2, max_epochs=2))
    film.save_exr(str(tmp_path / "prog.exr"), half=False)
    _assert_layers(exr_read.read((tmp_path / "prog.exr").read_bytes()), _film_layers(film, kinds), False, "progressive")
    pre = film.render_preview(R.Preview(), frame=2, world=world, camera=cam)
    pre.save_exr(str(tmp_path / "pre.exr"), gbuffer=True)
    got = exr_read.read((tmp_path / "pre.exr").read_bytes())
    _assert_layers(got, _film_layers(pre, pre.channel_kinds), True, "preview")
    assert np.array_equal(got["id"], pre.gbuffer()["object"][::-1])


def test_two_frames_of_a_sequence_with_exr(tmp_path):
    R, cam, world, integ, filt, tile = _scene()
    Kd = R.ChannelKind
    write = [Kd.Alpha, Kd.WorldNormal, Kd.Color]
    film = R.Film([Kd.Color, Kd.Alpha, Kd.Background, Kd.WorldNormal], (W, H))
    plain, dev, host = tmp_path / "plain", tmp_path / "device", tmp_path / "host"
    film.render_sequence(world, cam, integ, filt, tile, FRAMES, RATE, SHUTTER, SAMPLES, write, str(plain), "a", png="device")
    stats = film.render_sequence(world, cam, integ, filt, tile, FRAMES, RATE, SHUTTER, SAMPLES, write, str(dev), "a", png="device", exr="device")
    assert [st["frame"] for st in stats] == FRAMES
    film.render_sequence(world, cam, integ, filt, tile, FRAMES, RATE, SHUTTER, SAMPLES, write, str(host), "a", png="device", exr="host")
    a, b, c = IO.read_folder(str(plain)), IO.read_folder(str(dev)), IO.read_folder(str(host))
    exrs = ["a_%04d.exr" % f for f in FRAMES]
    assert sorted(b) == sorted(list(a) + exrs) == sorted(c) and len(a) == 3 * len(FRAMES)
    for name in a:  # the PNGs are byte for byte those of a run without exr=
        assert a[name] == b[name] == c[name], name
    want_names = sorted(n for k in write for n in LAYERS[k.name])
    for name in exrs:
        got, ref = exr_read.read(b[name]), exr_read.read(c[name])
        assert sorted(got) == want_names == sorted(ref)
        for n in got:
            assert got[n].dtype == np.float16 == ref[n].dtype and np.array_equal(got[n].view(np.uint16), ref[n].view(np.uint16)), (name, n)
    # the last frame's film is what the last file holds
    _assert_layers(exr_read.read(b[exrs[-1]]), _film_layers(film, write), True, "last frame")
    with pytest.raises(ValueError, match="exr must be one of"):
        film.render_sequence(world, cam, integ, filt, tile, FRAMES, RATE, SHUTTER, SAMPLES, write, str(tmp_path / "bad"), "a", exr="gpu")
    assert not (tmp_path / "bad").exists()
