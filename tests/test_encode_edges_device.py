"""The device PNG, LZ77 and EXR encoders at their decision edges (tests/encode_edge_cases.py): every case through every entry it applies
to - rayn_hip_png_encode_device, rayn_hip_png_encode_lz77_device, rayn_hip_deflate_lz77_device, rayn_hip_exr_encode_device with matches 0
and 1 - and the bytes written compared bit for bit with the restatements', header words included; outputs and scratch between 0xA5 guard
bytes, nothing behind the last written word touched, the inputs unchanged.  What the device wrote is also decoded by what shares nothing
with the restatements: zlib.decompress, zlib.adler32, PIL, tests/exr_read.py.  rayn_hip_probe_huffman - huffman_code<286> and
huffman_code<30> alone - against the restatement's lengths and the canonical codes of RFC 1951 3.2.2 computed from those lengths."""
import ctypes as C
import io
import struct
import zlib

import numpy as np
import pytest

import device_io as IO
import encode_edge_cases as EC
import exr_np as E
import exr_read
import png_np as P
from rayn_amd import image

pytestmark = pytest.mark.gpu

GUARD = 0xA5
RUNS = [(c.name, entry) for c in EC.cases() for entry in EC.entries(c)]


def _assert_bytes(got, want, what):
    if got != want + b"\x00" * (-len(want) % 4):
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


def _stream(ctx, c, entry):
    """A "png" or "deflate" case through its entry -> (the bytes written, the zlib stream, the bytes the stream holds)"""
    import torch
    from rayn_amd import film as F
    if c.kind == "png":
        h, w, bpp = c.img.shape
        bound, need = F.png_stream_bound(w, h, bpp), (F.png_scratch_bytes if entry == "png" else F.png_scratch_bytes_lz77)(w, h, bpp)
        host, src = c.img, IO.upload_bytes(c.img)
    else:
        n = len(c.data)
        bound, need = F.deflate_stream_bound(n), F.deflate_scratch_bytes(n)
        src_full, _ = IO.guarded(n, torch.uint8, 0)
        host, src = c.data, src_full[1:n + 1]   # an input that is not aligned
        src.copy_(IO.upload_bytes(c.data))
    assert bound % 16 == 0 and need % 16 == 0 and need > 0
    out_full, out = IO.guarded(bound, torch.uint8, GUARD)
    scr_full, scr = IO.guarded(need, torch.uint8, GUARD)
    if entry == "png":
        ctx.png_encode(w, h, bpp, src, out, scr)
    elif entry == "png_lz":
        ctx.png_encode_lz77(w, h, bpp, src, out, scr)
    else:
        ctx.deflate(src, out, c.stride, scr)
    torch.cuda.synchronize()
    IO.assert_guards(out_full, bound, GUARD, "d_out")
    IO.assert_guards(scr_full, need, GUARD, "d_scratch")
    IO.assert_is_host(src, host, "the input", np.uint8)
    got, z = _written(out, bound)
    return got, bytes(z), (EC.filtered(c.name) if c.kind == "png" else c.data).tobytes()


def _exr(ctx, c, matches):
    """An "exr" case through rayn_hip_exr_encode_device -> the bytes written (header, table, body to its last word)"""
    import torch
    from rayn_amd import film as F
    layout = [(s, o, t) for _, _, s, o, t in c.channels]
    bound, need = F.exr_stream_bound(c.w, c.h, layout), F.exr_scratch_bytes(c.w, c.h, layout, bool(matches))
    assert bound == E.stream_bound(c.w, c.h, layout) and bound % 16 == 0 and need % 16 == 0 and need > 0
    planes = [IO.upload(np.ascontiguousarray(p).view(np.int32), np.int32) for _, p, _, _, _ in c.channels]
    out_full, out = IO.guarded(bound, torch.uint8, GUARD)
    scr_full, scr = IO.guarded(need, torch.uint8, GUARD)
    ctx.exr_encode(c.w, c.h, [(n, d, s, o, t) for (n, _, s, o, t), d in zip(c.channels, planes)], out, scr, lz77=bool(matches))
    torch.cuda.synchronize()
    IO.assert_guards(out_full, bound, GUARD, "d_out")
    IO.assert_guards(scr_full, need, GUARD, "d_scratch")
    for d, (_, p, _, _, _) in zip(planes, c.channels):
        IO.assert_is_host(d, p, "a plane", np.uint32)
    got = out.cpu().numpy()
    body, chunks = (int(v) for v in got[:8].view("<u4"))
    assert chunks == E.n_chunks(c.h) and 10 * chunks <= body <= bound - E.body_at(c.h)
    written = E.body_at(c.h) + (body + 3) // 4 * 4
    assert np.all(got[written:] == GUARD), "bytes behind the body's last word were written"
    return got[:written].tobytes()


def _pil_pixels(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        im.load()
        return np.asarray(im)


@pytest.mark.parametrize("name,entry", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_entry_writes_the_restatements_bytes(gpu_ctx, name, entry):
    c = EC.case(name)
    want = EC.expected(name, entry)
    if c.kind == "exr":
        got = _exr(gpu_ctx, c, int(entry[3]))
        _assert_bytes(got, want, (name, entry))
        # the device's own bytes through the independent reader: header words, chunk table, every chunk
        body, chunks, raws, blocks = struct.unpack("<IIII", got[:16])
        sizes = E.chunk_bytes(c.w, c.h, [t for _, _, _, _, t in c.channels])
        starts = struct.unpack("<%dI" % chunks, got[16:16 + 4 * chunks])
        at0 = E.body_at(c.h)
        payload = [struct.unpack("<ii", got[at0 + s:at0 + s + 8]) for s in starts]
        assert [y for y, _ in payload] == list(range(0, c.h, E.ROWS)) and blocks == sum(-(-n // P.BLOCK) for n in sizes)
        assert raws == sum(1 for (_, size), n in zip(payload, sizes) if size == n) and body == sum(8 + size for _, size in payload)
        if "raw" in c.expect:
            assert [size == n for (_, size), n in zip(payload, sizes)] == c.expect["raw"]
        named = [(n, t) for n, _, _, _, t in c.channels]
        planes = exr_read.read(image.exr_from_chunks(c.w, c.h, named, got))
        for n, p, s, o, t in c.channels:
            words = E.channel_words(p, s, o, c.w, c.h).reshape(c.h, c.w)[::-1]
            if t == E.HALF:
                assert np.array_equal(planes[n].view(np.uint16), E.half_bits(words)), n
            else:
                assert np.array_equal(planes[n].view(np.uint32), words), n
        return
    got, z, source = _stream(gpu_ctx, c, entry)
    _assert_bytes(got, want, (name, entry))
    n_stream, n, blocks, stored = struct.unpack("<IIII", got[:16])
    assert (n_stream, n, blocks) == (len(z), len(source), -(-len(source) // P.BLOCK))
    assert zlib.decompress(z) == source and int.from_bytes(z[-4:], "big") == zlib.adler32(source)
    if "stored" in c.expect and entry != "png_lz":
        assert stored == sum(c.expect["stored"])
    if c.kind == "png":
        h, w, bpp = c.img.shape
        assert np.array_equal(_pil_pixels(image.png_from_stream(w, h, bpp, z)).reshape(h, w, bpp), c.img)


@pytest.mark.parametrize("n", (286, 30))
def test_huffman_probe_builds_the_restatements_lengths_and_rfc_codes(gpu_ctx, n):
    """huffman_code<n> alone on every count set of encode_edge_cases.huffman_sets: the lengths of png_np.code_lengths /
    png_lz_np.distance_lengths exactly, and as table entries the canonical codes computed here from the lengths alone, bit-reversed.
    This is where the distance code's builder is driven past depth 15, which no 32 KiB block does."""
    from rayn_amd import _lib
    L = _lib.lib()
    sets = EC.huffman_sets(n)
    counts = np.ascontiguousarray([c for _, c, _, _ in sets], np.uint32)
    clen, tab = np.full(counts.shape, 0xA5A5A5A5, np.uint32), np.full(counts.shape, 0xA5A5A5A5, np.uint32)
    up = C.POINTER(C.c_uint32)
    keep = counts.copy()
    assert L.rayn_hip_probe_huffman(gpu_ctx.h, n, len(sets), counts.ctypes.data_as(up), clen.ctypes.data_as(up), tab.ctypes.data_as(up)) == 0, gpu_ctx.last_error()
    assert np.array_equal(counts, keep)
    for k, (name, c, in_block, _) in enumerate(sets):
        lengths = EC.expected_lengths(c)
        assert clen[k].tolist() == lengths, (name, in_block, "lengths")
        assert tab[k].tolist() == EC.table_entries(lengths), (name, in_block, "codes")
    # what the entry rejects, with a text and nothing written
    clen[:] = tab[:] = 0xA5A5A5A5
    big = np.zeros((1, n), np.uint32)
    big[0, :2] = 1 << 31
    for args, text in (((31, 1, counts), "n_symbols must be 286 or 30"), ((n, 0, counts), "probe size out of range"), ((n, 1, big), "2^32 or more")):
        assert L.rayn_hip_probe_huffman(gpu_ctx.h, args[0], args[1], args[2].ctypes.data_as(up), clen.ctypes.data_as(up), tab.ctypes.data_as(up)) == -1
        assert text in gpu_ctx.last_error(), (text, gpu_ctx.last_error())
    assert L.rayn_hip_probe_huffman(gpu_ctx.h, n, 1, None, clen.ctypes.data_as(up), tab.ctypes.data_as(up)) == -1 and "null buffer" in gpu_ctx.last_error()
    assert L.rayn_hip_probe_huffman(None, n, 1, None, None, None) == -1
    assert np.all(clen == 0xA5A5A5A5) and np.all(tab == 0xA5A5A5A5)
