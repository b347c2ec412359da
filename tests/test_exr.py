"""The EXR writer without a GPU: the restatement's integer half conversion against numpy's, the files of the restatement and of
rayn_amd.image.save_exr_host read back to the exact bits by the independent reader of tests/exr_read.py, the offsets, y and sizes of
the chunks, the raw rule on the case built for it, the buffers exr_from_chunks refuses, and the name checks."""
import struct

import numpy as np
import pytest

import exr_cases as K
import exr_np as E
import exr_read
from rayn_amd import image


def _named(channels):
    return [(n.encode(), t) for n, _, _, _, t in channels]


def _want(w, h, channels):
    """name -> (h, w) array of the bits a reader must find, rows top-down"""
    out = {}
    for n, plane, s, o, t in channels:
        words = E.channel_words(plane, s, o, w, h).reshape(h, w)[::-1]
        if t == E.HALF:
            with np.errstate(over="ignore", invalid="ignore"):
                out[n] = words.view(np.float32).astype(np.float16).view(np.uint16)
        else:
            out[n] = words
    return out


def _assert_decodes(data, w, h, channels, what):
    info = {}
    got = exr_read.read(data, info)
    want = _want(w, h, channels)
    assert sorted(got) == sorted(want) and (info["width"], info["height"]) == (w, h), what
    for n in want:
        g = got[n].view(np.uint16 if got[n].dtype.itemsize == 2 else np.uint32)
        assert g.dtype == want[n].dtype and np.array_equal(g, want[n]), (what, n)
    return info


def test_integer_half_conversion_is_numpys_on_the_sweep():
    words = K.sweep_words()
    with np.errstate(over="ignore", invalid="ignore"):
        want = words.view(np.float32).astype(np.float16).view(np.uint16)
    got = E.half_bits(words)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(hex(words[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]
    # the definition's own words: signalling NaNs stay signalling, a payload in the low 13 bits alone sets the lowest bit
    assert [int(x) for x in E.half_bits(np.array([0x7F800001, 0xFF800001, 0x7FA00000, 0x7FC00000, 0x477FF000, 0x477FEFFF, 0x80000001], np.uint32))] == \
        [0x7C01, 0xFC01, 0x7D00, 0x7E00, 0x7C00, 0x7BFF, 0x8000]


def test_integer_half_conversion_on_random_bits():
    words = np.random.default_rng(5).integers(0, 1 << 32, 1 << 18, dtype=np.uint64).astype(np.uint32)
    with np.errstate(over="ignore", invalid="ignore"):
        want = words.view(np.float32).astype(np.float16).view(np.uint16)
    assert np.array_equal(E.half_bits(words), want)


@pytest.mark.parametrize("matches", (0, 1))
@pytest.mark.parametrize("name", list(K.BYTE_CASES))
def test_reader_takes_the_restatements_files_back_to_the_bits(name, matches):
    w, h, channels = K.case(name)
    enc, chunk_info = K.encoded(name, matches)
    assert len(enc) <= E.stream_bound(w, h, K.layout_of(channels)) and len(chunk_info) == E.n_chunks(h)
    data = E.file_of(w, h, _named(channels), enc)
    info = _assert_decodes(data, w, h, channels, name)
    # offsets, y and sizes: the chunks follow the offset table without a gap, in order, and the file ends with the last
    at = info["header_bytes"] + 8 * len(chunk_info)
    sizes = E.chunk_bytes(w, h, [t for *_, t in channels])
    for k, ((off, y, size, raw), (want_raw, want_size)) in enumerate(zip(info["chunks"], chunk_info)):
        assert (off, y, size, raw) == (at, 16 * k, want_size, want_raw), (name, k)
        assert size <= sizes[k] and (size == sizes[k]) == raw
        at += 8 + size
    assert at == len(data)
    # the product's framing of the same buffer is the same file
    assert image.exr_from_chunks(w, h, [(n, t) for n, _, _, _, t in channels], E.padded(enc)) == data


@pytest.mark.parametrize("matches", (0, 1))
def test_raw_rule_one_raw_and_one_compressed_chunk(matches):
    _, info = K.encoded("64x32-raw-and-ramp", matches)
    assert [r for r, _ in info] == [True, False]
    assert info[0][1] == 64 * 4 * 16 and info[1][1] < 64 * 4 * 16
    enc, _ = K.encoded("64x32-raw-and-ramp", matches)
    assert struct.unpack("<IIII", enc[:16])[1:] == (2, 1, 2)


def test_small_chunks_are_raw():
    """A Huffman header alone is 153 bytes, a stored block costs 11 more than its bytes: 1x1 HALF is 2 raw bytes"""
    enc, info = K.encoded("1x1", 0)
    w, h, channels = K.case("1x1")
    half = E.half_bits(channels[0][1]).astype("<u2").tobytes()
    assert info == [(True, 2)]
    assert enc == struct.pack("<IIII", 10, 1, 1, 1) + struct.pack("<I", 0) + b"\0" * 12 + struct.pack("<ii", 0, 2) + half
    assert all(r for r, _ in K.encoded("37x1", 1)[1])


@pytest.mark.parametrize("name", ("37x17", "61x20-mixed", "64x32-raw-and-ramp"))
def test_save_exr_host_reads_back_to_the_bits(tmp_path, name):
    w, h, channels = K.case(name)
    path = tmp_path / "a.exr"
    image.save_exr_host(str(path), w, h, [(n, t, E.channel_words(p, s, o, w, h)) for n, p, s, o, t in channels])
    data = path.read_bytes()
    info = _assert_decodes(data, w, h, channels, name)
    assert data.startswith(E.header(w, h, _named(channels)))  # the same header as the restatement's
    if name == "64x32-raw-and-ramp":
        assert [c[3] for c in info["chunks"]] == [True, False]


def test_sweep_through_the_host_writer_and_the_reader():
    w, h, channels = K.sweep_case()
    data = image.exr_bytes_host(w, h, [(n, t, p) for n, p, _, _, t in channels], level=1)
    _assert_decodes(data, w, h, channels, "sweep")


def test_exr_from_chunks_rejects_what_is_not_an_encoded_buffer():
    w, h, channels = K.case("37x33")
    named = [(n, t) for n, _, _, _, t in channels]
    enc = E.padded(K.encoded("37x33", 0)[0])
    assert image.exr_from_chunks(w, h, named, enc)
    with pytest.raises(ValueError, match="not an encoded EXR body"):
        image.exr_from_chunks(w, h, named, enc[:-4])           # truncated: the body runs past the end
    with pytest.raises(ValueError, match="not an encoded EXR body"):
        image.exr_from_chunks(w, h, named, enc[:20])           # not even the table
    with pytest.raises(ValueError, match="not an encoded EXR body"):
        image.exr_from_chunks(w, 16, named, enc)               # another height's chunk count
    bad = bytearray(enc)
    bad[20:24] = struct.pack("<I", 5)                           # a start inside the chunk in front of it
    with pytest.raises(ValueError, match="do not ascend"):
        image.exr_from_chunks(w, h, named, bytes(bad))


def test_names_must_be_sorted_unique_and_short():
    assert image.check_exr_names(["A", "B", "G", "N.X", "R", "Z", "background.B", "id"]) == [b"A", b"B", b"G", b"N.X", b"R", b"Z", b"background.B", b"id"]
    for bad, text in ((["B", "A"], "sorted"), (["R", "R"], "twice"), ([""], "1..31"), (["x" * 32], "1..31"), (["a\0b"], "NUL"), (["a", "Z"], "sorted")):
        with pytest.raises(ValueError, match=text):
            image.check_exr_names(bad)
    assert image.check_exr_names(["x" * 31])
    with pytest.raises(ValueError, match="sorted"):
        image.exr_header(4, 4, [("R", 1), ("G", 1)])
    with pytest.raises(ValueError, match="type"):
        image.exr_header(4, 4, [("R", 3)])


def test_bound_is_exact_and_zero_for_what_is_rejected():
    assert E.stream_bound(1, 1, [(1, 0, E.HALF)]) == 32 + 16
    assert E.stream_bound(37, 33, [(3, 0, E.HALF)] * 3) == 32 + (3 * 8 + 37 * 6 * 33 + 15) // 16 * 16
    for w, h, layout in ((0, 1, [(1, 0, 1)]), (1, 0, [(1, 0, 1)]), (1, 1, []), (1, 1, [(1, 0, 1)] * 17), (1, 1, [(1, 0, 3)]), (1, 1, [(0, 0, 1)]),
                         (1, 1, [(2, 2, 1)]), (1 << 25, 1, [(1, 0, 2)]), (1 << 14, 1 << 15, [(1, 0, 2)])):
        assert E.stream_bound(w, h, layout) == 0, (w, h, layout)
