"""tests/encode_edge_cases.py held to account without a GPU: every case's expected bytes (by the restatements) go through decoders that
share nothing with them - zlib.decompress, zlib.adler32, tests/exr_read.py, PIL for whole PNG files - and through the hand-written
outcome of its family; every searched input sits where it claims to; every mutant of the restatements is killed by a named case and goes
unnoticed by the older case tables (png_cases, png_lz_cases, exr_cases) - or is counted where they do notice it; the count sets of rayn_hip_probe_huffman have the lengths,
halvings and canonical codes the device test asks the probe for."""
import functools
import io
import struct
import zlib

import numpy as np
import pytest

import encode_edge_cases as C
import exr_cases as KE
import exr_np as E
import exr_read
import png_cases as K
import png_lz_cases as KZ
import png_lz_np as Z
import png_np as P
from rayn_amd import image

CASES = C.cases()
BY_FAMILY = {f: [c for c in CASES if c.family == f] for f in dict.fromkeys(c.family for c in CASES)}


def test_the_table_is_what_the_summary_counts():
    assert {f: len(v) for f, v in BY_FAMILY.items()} == {"raw_tie": 6, "stored_tie": 12, "depth": 5, "many_blocks": 2, "many_chunks": 2,
                                                         "chunks_of_blocks": 2, "pack_tiles": 3, "exit": 11}
    assert sum(len(C.entries(c)) for c in CASES) == 60   # device runs
    for n in (286, 30):
        assert len(C.huffman_sets(n)) == 211   # 11 named, 200 seeded
    assert set(m for c in CASES for m in c.kills) == set(C.MUTANTS)


# ---- every case, every entry: independent decoders ---------------------------------------------------------------------------------------------

def _stream_words(buf, source, what):
    """The header words and the zlib stream of a PNG or deflate buffer, held against zlib: -> (blocks, stored blocks)"""
    n_stream, n, blocks, stored = struct.unpack("<IIII", buf[:16])
    z = buf[16:]
    assert (n_stream, n, blocks) == (len(z), len(source), -(-len(source) // P.BLOCK)), what
    assert z[:2] == b"\x78\x01" and zlib.decompress(z) == source, what
    assert int.from_bytes(z[-4:], "big") == zlib.adler32(source), what
    return blocks, stored


def _pil_pixels(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        im.load()
        return np.asarray(im)


def _chunks(c, buf):
    """[(y, size, payload)] of an EXR buffer and its header words, the table followed"""
    body, chunks, raws, blocks = struct.unpack("<IIII", buf[:16])
    starts = struct.unpack("<%dI" % chunks, buf[16:16 + 4 * chunks])
    at0 = E.body_at(c.h)
    assert chunks == E.n_chunks(c.h) and len(buf) == at0 + body and not any(buf[16 + 4 * chunks:at0])
    out, want = [], 0
    for s in starts:
        assert s == want
        y, size = struct.unpack("<ii", buf[at0 + s:at0 + s + 8])
        out.append((y, size, buf[at0 + s + 8:at0 + s + 8 + size]))
        want = s + 8 + size
    assert want == body
    return out, raws, blocks


def _types(c):
    return [t for _, _, _, _, t in c.channels]


def _scanline_bytes(c):
    return E.scanlines(c.w, c.h, [(p, s, o, t) for _, p, s, o, t in c.channels])


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_expected_bytes_decode_to_the_input(c):
    for entry in C.entries(c):
        buf = C.expected(c.name, entry)
        if c.kind == "exr":
            chunks, raws, blocks = _chunks(c, buf)
            sizes, rows = E.chunk_bytes(c.w, c.h, _types(c)), _scanline_bytes(c)
            assert [y for y, _, _ in chunks] == list(range(0, c.h, E.ROWS))
            assert raws == sum(1 for (_, size, _), n in zip(chunks, sizes) if size == n)
            assert blocks == sum(-(-n // P.BLOCK) for n in sizes)
            for k, ((y, size, payload), n) in enumerate(zip(chunks, sizes)):
                raw = rows[y:y + E.ROWS].reshape(-1).tobytes()
                assert size <= n and (payload == raw if size == n else zlib.decompress(payload) == E.preprocess(np.frombuffer(raw, np.uint8)).tobytes()), (entry, k)
            named = [(n, t) for n, _, _, _, t in c.channels]
            data = image.exr_from_chunks(c.w, c.h, named, E.padded(buf))
            assert data == E.file_of(c.w, c.h, [(n.encode(), t) for n, t in named], buf)
            planes = exr_read.read(data)
            for n, p, s, o, t in c.channels:
                words = E.channel_words(p, s, o, c.w, c.h).reshape(c.h, c.w)[::-1]
                if t == E.HALF:
                    assert np.array_equal(planes[n].view(np.uint16), E.half_bits(words)), (entry, n)
                else:
                    assert np.array_equal(planes[n].view(np.uint32), words), (entry, n)
        elif c.kind == "deflate":
            _stream_words(buf, c.data.tobytes(), (c, entry))
        else:
            h, w, bpp = c.img.shape
            _stream_words(buf, C.filtered(c.name).tobytes(), (c, entry))
            pixels = _pil_pixels(image.png_from_stream(w, h, bpp, buf[16:]))
            assert np.array_equal(pixels.reshape(h, w, bpp), c.img), (c, entry)


# ---- the hand-written outcome of every family -----------------------------------------------------------------------------------------------------

def _zlib_stream_of_chunk(c, matches, k=0):
    """(the pre-processed bytes of chunk k, its whole zlib stream) - whether or not the raw rule keeps it"""
    rows = _scanline_bytes(c)
    p = E.preprocess(rows[E.ROWS * k:E.ROWS * (k + 1)].reshape(-1))
    enc = Z.encode_filtered(p, rows.shape[1] // 2)[0] if matches else P.encode_filtered(p)[0]
    return p, enc[16:]


@pytest.mark.parametrize("c", BY_FAMILY["raw_tie"], ids=repr)
def test_raw_ties_sit_where_they_claim(c):
    """The searched chunks: the zlib stream is n - 1, n and n + 1 bytes; compressed, raw, raw"""
    (matches,) = c.matches
    p, z = _zlib_stream_of_chunk(c, matches)
    n = E.chunk_bytes(c.w, c.h, _types(c))[0]
    assert n == 1024 and len(z) - n == c.expect["stream_minus_n"] and zlib.decompress(z) == p.tobytes()
    chunks, raws, _ = _chunks(c, C.expected(c.name, "exr%d" % matches))
    assert [size == n for _, size, _ in chunks] == c.expect["raw"] and raws == sum(c.expect["raw"])
    if not c.expect["raw"][0]:
        assert chunks[0][2] == z and len(z) == n - 1
    # at the tie both forms are n bytes long and differ: a reader takes a payload of n bytes as the scanlines themselves
    if c.expect["stream_minus_n"] == 0:
        assert len(z) == len(chunks[0][2]) and z != chunks[0][2]


def _first_block(c):
    """(kernel module, the first block's bytes, its stride, final?) of a stored-tie case"""
    if c.kind == "png":
        r = C.filtered(c.name)
        return P, r[:P.BLOCK], 0, len(r) <= P.BLOCK
    return Z, c.data[:P.BLOCK], c.stride, len(c.data) <= P.BLOCK


@pytest.mark.parametrize("c", BY_FAMILY["stored_tie"], ids=repr)
def test_stored_ties_sit_where_they_claim(c):
    """The searched blocks: the Huffman form is one byte shorter than, as long as, and one byte longer than the stored form of len + 5"""
    mod, blk, stride, final = _first_block(c)
    assert c.expect["kernel"] == {P: "P", Z: "Z"}[mod] and final == (len(c.expect["stored"]) == 1)
    data = (mod.huffman_block(blk, final) if mod is P else mod.huffman_block(blk, final, stride))[0]
    assert len(data) - (len(blk) + 5) == c.expect["huffman_minus_stored"]
    assert (len(blk) < 400) if final else (len(blk) == P.BLOCK)
    entry = "png" if c.kind == "png" else "deflate"
    buf = C.expected(c.name, entry)
    assert struct.unpack("<IIII", buf[:16])[3] == sum(c.expect["stored"])
    first = buf[18:18 + 5 + len(blk)]
    stored_form = struct.pack("<BHH", 1 if final else 0, len(blk) & 0xFFFF, ~len(blk) & 0xFFFF) + blk.tobytes()
    assert (first == stored_form) == c.expect["stored"][0]
    if c.expect["huffman_minus_stored"] == 0:   # the same size, other bytes
        assert first != data + b"\x00" * (len(first) - len(data)) and len(data) == len(stored_form)


@pytest.mark.parametrize("c", [c for c in BY_FAMILY["depth"] if "lengths" in c.expect], ids=repr)
def test_depth_15_and_16_blocks_have_the_lengths_written_out_by_hand(c):
    blk = c.expect["block"]
    if c.kind == "png":
        r, types = P.filter_rows(c.img)
        assert types.tolist() == [0] and np.array_equal(r, blk)            # the filter leaves the row alone
    else:
        raw = _scanline_bytes(c).reshape(-1)
        assert np.array_equal(E.preprocess(raw), blk)
        assert np.array_equal(E.half_bits(c.channels[0][1]), raw.view("<u2"))
    assert not np.any(blk[1:] == blk[:-1])                                     # literals alone
    data, bits, info = P.huffman_block(blk, True)
    assert max(P.tree_depths(info["freq"])) == c.expect["first_depth"] and info["halvings"] == c.expect["halvings"] and not info["has_match"]
    assert {s: n for s, n in enumerate(info["lengths"]) if n} == c.expect["lengths"]
    assert sum(2.0 ** -n for n in c.expect["lengths"].values()) == 1.0        # a complete code
    if c.expect["halvings"] == 0:
        assert max(info["lengths"]) == 15 and info["lengths"].count(15) == 2   # 15-bit codes, and the 4-bit header code 15
    assert zlib.decompressobj(-15).decompress(data) == blk.tobytes()


@pytest.mark.parametrize("c", [c for c in BY_FAMILY["depth"] if "lengths" not in c.expect], ids=repr)
def test_the_lz77_kernel_finds_matches_in_the_fibonacci_blocks(c):
    """What encode_edge_cases says it cannot arrange: through the LZ77 kernel these bytes are no literal-only block"""
    info = Z.huffman_block(c.data, True, c.stride)[2]
    assert any(t[0] == "match" for t in info["tokens"]) and max(info["lengths"]) < 15 and info["halvings"] == 0


def _thread_boundaries(stored):
    """What meets at the starts of the layout threads' ranges (chunk = 2: every even block): the set of (stored?, stored?)"""
    assert -(-len(stored) // P.LAYOUT_THREADS) == 2
    return {(stored[k - 1], stored[k]) for k in range(2, len(stored), 2)}


ALL_FOUR = {(False, False), (False, True), (True, False), (True, True)}


def test_258_blocks_of_four_contents():
    c = C.case("many_blocks/deflate_258")
    blocks = [c.data[o:o + P.BLOCK] for o in range(0, len(c.data), P.BLOCK)]
    assert len(c.data) == 257 * P.BLOCK + 5 and len(blocks) == c.expect["blocks"] == 258 and len({b.tobytes() for b in blocks}) == 4
    enc = C.memo_encoder("Z", 0)
    stored = [enc(b, k == 257)[1] for k, b in enumerate(blocks)]
    assert stored == c.expect["stored"] and _thread_boundaries(stored) == ALL_FOUR
    assert struct.unpack("<IIII", C.expected(c.name, "deflate")[:16])[2:] == (258, sum(stored))


def test_257_blocks_of_filtered_rows():
    c = C.case("many_blocks/png_4096x2049")
    r = C.filtered(c.name)
    blocks = [r[o:o + P.BLOCK] for o in range(0, len(r), P.BLOCK)]
    assert len(blocks) == c.expect["blocks"] == 257 == P.n_blocks(C.BIG_W, C.BIG_H, 1) and len(blocks[-1]) == 6145
    distinct = len({b.tobytes() for b in blocks})
    assert distinct == 26   # the two flat contents, and what the type bytes every 4097 bytes make of the rest
    assert all(np.all(blocks[k] == 2) for k in c.expect["flat_blocks"]) and sum(1 for b in blocks if not b.any()) > 150
    for kernel, entry, stride in (("P", "png", 0), ("Z", "png_lz", C.BIG_W + 1)):
        enc = C.memo_encoder(kernel, stride)
        stored = [enc(b, k == 256)[1] for k, b in enumerate(blocks)]
        assert all(stored[k] for k in c.expect["stored_blocks"]) and _thread_boundaries(stored) == ALL_FOUR, kernel
        assert struct.unpack("<IIII", C.expected(c.name, entry)[:16])[2:] == (257, sum(stored))
    # the periodic blocks are what the LZ77 kernel finds matches in and the run-only kernel does not
    k = C.BIG_PERIODIC[1]
    assert len(C.memo_encoder("Z", C.BIG_W + 1)(blocks[k], False)[0]) < len(C.memo_encoder("P", 0)(blocks[k], False)[0]) // 4


@pytest.mark.parametrize("c", BY_FAMILY["many_chunks"] + BY_FAMILY["chunks_of_blocks"] + BY_FAMILY["pack_tiles"], ids=repr)
def test_exr_shapes_reach_their_edges(c):
    sizes = E.chunk_bytes(c.w, c.h, _types(c))
    assert len(sizes) == c.expect["chunks"]
    if "chunk_bytes" in c.expect:
        assert sizes[0] == c.expect["chunk_bytes"]
    for m in c.matches:
        chunks, raws, blocks = _chunks(c, C.expected(c.name, "exr%d" % m))
        if "raw" in c.expect:
            assert [size == n for (_, size, _), n in zip(chunks, sizes)] == c.expect["raw"], m
        if "blocks" in c.expect:
            assert blocks == c.expect["blocks"]
    if c.family == "many_chunks":
        assert -(-len(sizes) // 256) == 2 and 0 < sum(c.expect["raw"])
    if c.name.endswith("64x4112_float"):
        assert sum(c.expect["raw"]) == 109 and _thread_boundaries(c.expect["raw"]) == ALL_FOUR
    if c.family == "chunks_of_blocks":
        assert sizes == [32832, 32832, 16416] and [-(-n // P.BLOCK) for n in sizes] == [2, 2, 1] and sizes[-1] == c.expect["last_chunk_bytes"]
    if c.family == "pack_tiles":
        assert [n // 2 for n in sizes] == c.expect["units"] and -(-sizes[0] // 2 // 4096) == 2   # two tiles a chunk
        last = c.expect["units"][-1]
        assert last <= 4096 or (last - 4096) % 2 == 1                                            # tile 1 of the last chunk: absent, or odd
    if c.name.endswith("101x33_mixed"):
        assert 4096 % 505 == 56 and 56 < 101 < 505   # tile 1 starts in row 8's HALF channel, whose FLOAT channel starts inside the tile


@pytest.mark.parametrize("c", BY_FAMILY["exit"], ids=repr)
def test_exit_blocks_have_the_tokens_written_out_by_hand(c):
    want, p = [], 0
    for t in c.expect["tokens"]:
        want.append(("lit", p, t[1]) if t[0] == "lit" else ("match", p, t[1], t[2]))
        p += 1 if t[0] == "lit" else t[1]
    assert p == len(c.data) and Z.block_tokens(c.data, c.stride) == want
    assert Z.encode_block(c.data, True, c.stride)[1] is False
    if "exit" in c.expect:
        _, start, length, _ = next(t for t in want if t[0] == "match")
        assert start + length - (start // Z.SPAN + 1) * Z.SPAN == c.expect["exit"]
        assert (start % Z.SPAN >= Z.SPAN - 2 and length >= 257) == (c.expect["exit"] >= 256)
        if c.stride:   # the row above reaches as far as the run where the second match starts; distance 1 wins
            _, at, m, d = want[-2]
            assert Z.match_length(c.data.tobytes(), at, c.stride, m) == m and d == 1
    else:
        assert want[-1] == ("match", P.BLOCK - 258, 258, 1)


# ---- the mutants --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mutant", C.MUTANTS)
def test_every_mutant_is_killed_by_the_cases_that_name_it(mutant):
    killers = [c for c in CASES if mutant in c.kills]
    assert killers, mutant
    for c in killers:
        assert any(C.expected(c.name, e, mutant) != C.expected(c.name, e) for e in C.entries(c)), (mutant, c)


def _rounds(freq):
    """The depth of the tree of every round of the length limit, the accepted one last"""
    out, f = [], list(freq)
    while True:
        out.append(max(P.tree_depths(f)) if any(f) else 0)
        if out[-1] <= 15:
            return out
        f = [(v + 1) >> 1 if v else 0 for v in f]


def block_facts(kernel, blk, stride=0, final=True):
    """What decides whether a block-level mutant changes this block's bytes, from ONE run of the statement: the size difference of the two
    forms, the rounds of both length limits, the largest exit; and the block's size in its stream"""
    blk = np.asarray(blk, np.uint8)
    data, bits, info = P.huffman_block(blk, final) if kernel == "P" else Z.huffman_block(blk, final, stride)
    d = len(data) - (len(blk) + 5)
    rounds = [_rounds(info["freq"])] + ([_rounds(info["dfreq"])] if kernel == "Z" else [])
    exits = [t[1] + t[2] - min((t[1] // Z.SPAN + 1) * Z.SPAN, len(blk)) for t in info["tokens"] if t[0] == "match"] if kernel == "Z" else []
    size = len(blk) + 5 if d >= 0 else len(data) if final else (bits + 3 + 7) // 8 + 4
    return dict(kernel=kernel, d=d, rounds=rounds, exit=max(exits, default=0), size=size)


def notices(mutant, f):
    """Whether the mutant changes the bytes of a block with the facts f (the argument is each mutant's one changed line)"""
    if mutant in ("P:stored_gt", "Z:stored_gt"):
        return f["kernel"] == mutant[0] and f["d"] == 0
    if mutant == "P:limit_16":   # the statement halves a tree of depth 16, the mutant keeps it
        return any(16 in r[:-1] for r in f["rounds"])
    if mutant == "P:limit_14":   # the statement keeps a tree of depth 15, the mutant halves it
        return any(r[-1] == 15 for r in f["rounds"])
    assert mutant == "Z:exit_bit8"
    return f["exit"] >= 256


def _blocks_of(data):
    data = np.asarray(data, np.uint8)
    return [(data[o:o + P.BLOCK], o + P.BLOCK >= len(data)) for o in range(0, len(data), P.BLOCK)]


SMALL = 16384   # bytes of input up to which a case is cheap enough to run under every block mutant


@pytest.mark.parametrize("c", [c for c in CASES if c.kind != "exr" and (c.img.size if c.kind == "png" else c.data.size) <= SMALL], ids=repr)
def test_the_facts_predict_what_every_block_mutant_does(c):
    """block_facts / notices, which stand in for the mutants on the older tables, against the mutants themselves on the new cases"""
    for entry in C.entries(c):
        kernel = "P" if entry == "png" else "Z"
        data, stride = (C.filtered(c.name), (1 + c.img.shape[1] * c.img.shape[2]) if kernel == "Z" else 0) if c.kind == "png" else (c.data, c.stride)
        facts = [block_facts(kernel, b, stride, final) for b, final in _blocks_of(data)]
        assert 2 + sum(f["size"] for f in facts) + 4 == len(C.expected(c.name, entry)) - 16
        for mutant in C.BLOCK_MUTANTS:
            assert any(notices(mutant, f) for f in facts) == (C.expected(c.name, entry, mutant) != C.expected(c.name, entry)), (entry, mutant)


@functools.lru_cache(maxsize=None)
def _old_tables():
    """The facts of every block of the older tables: [(table, case, facts)], and per EXR case and `matches` the chunks' (n, stream bytes)"""
    blocks, chunks = [], []
    for shape in K.SHAPES:
        for family in K.FAMILIES:
            w, h, bpp = shape
            r = P.filter_rows(K.family_image(family, w, h, bpp, seed=w + h))[0]
            blocks += [("png_cases", (shape, family), block_facts("P", b, 0, final)) for b, final in _blocks_of(r)]
    for name, blk in (("run_edges", K.run_edges_bytes()), ("fibonacci", K.fibonacci_bytes()), ("three_symbols", K.three_symbol_block())):
        blocks.append(("png_cases", name, block_facts("P", blk)))
    blocks += [("png_cases", ("run", n), block_facts("P", K.run_block(n))) for n in K.RUN_LENGTHS]
    for name, data, stride in KZ.deflate_cases():
        blocks += [("png_lz_cases", name, block_facts("Z", b, stride, final)) for b, final in _blocks_of(data)]
    for name in KE.BYTE_CASES:
        w, h, channels = KE.case(name)
        rows = E.scanlines(w, h, [(p, s, o, t) for _, p, s, o, t in channels])
        for matches, kernel in ((0, "P"), (1, "Z")):
            sizes = []
            for y in range(0, h, E.ROWS):
                p = E.preprocess(rows[y:y + E.ROWS].reshape(-1))
                facts = [block_facts(kernel, b, rows.shape[1] // 2 if matches else 0, final) for b, final in _blocks_of(p)]
                blocks += [("exr_cases", (name, matches), f) for f in facts]
                sizes.append((len(p), 2 + sum(f["size"] for f in facts) + 4))
            chunks.append((name, matches, sizes))
    return blocks, chunks


def test_what_the_older_tables_notice_of_the_mutants():
    """The counts, over the 188 blocks and 30 chunks of png_cases, png_lz_cases and exr_cases.  Seven of the ten mutants go unnoticed: no
    block at the stored tie (the nearest is 4 bytes off), no tree that is 16 deep in a round (the Fibonacci block's is 17, then 9), no
    exit above 249, no stream of more than 9 blocks or 3 chunks, no last chunk with fewer blocks than a full one.  Three are noticed, by
    cases that do not say so and would not fail by name:
      P:limit_14              by 12 blocks, all of png_cases' gradient images: their first tree is 15 deep, so they do emit 15-bit codes
      E:raw_gt                by 1 chunk: 37x1 with matches = 0, whose zlib stream happens to be exactly its 222 bytes
      E:raw_size_plus_header  by 3 chunks: that one, and the one-row last chunks of 37x17 and 37x33 (224 and 226 bytes for 222)"""
    blocks, chunks = _old_tables()
    assert len(blocks) == 188 and sum(len(s) for _, _, s in chunks) == 30
    noticed = {m: [(t, n) for t, n, f in blocks if notices(m, f)] for m in C.BLOCK_MUTANTS}
    assert {m: len(v) for m, v in noticed.items()} == {"P:stored_gt": 0, "P:limit_16": 0, "P:limit_14": 12, "Z:stored_gt": 0, "Z:exit_bit8": 0}
    assert {(t, n[1]) for t, n in noticed["P:limit_14"]} == {("png_cases", "gradient")}
    assert min(abs(f["d"]) for _, _, f in blocks) == 4 and max(f["exit"] for _, _, f in blocks) == 249
    assert max(max(f["rounds"][1]) for _, _, f in blocks if f["kernel"] == "Z") == 11   # the deepest distance code
    assert sorted({tuple(r) for _, _, f in blocks for r in f["rounds"] if max(r) > 14}) == [(15,), (17, 9)]
    # the stream mutants act where a layout thread has two blocks or chunks
    per_stream = {}
    for table, name, _ in blocks:
        per_stream[table, name] = per_stream.get((table, name), 0) + 1
    assert max(per_stream.values()) == 9 and max(len(s) for _, _, s in chunks) == 3
    nine = K.family_image("gradient", 300, 220, 4, seed=520)
    r = P.filter_rows(nine)[0]
    parts = [C.memo_encoder("P")(b, final)[0] for b, final in _blocks_of(r)]
    for m in C.STREAM_MUTANTS:   # and are the statement itself there
        assert len(parts) == 9 and P.join_blocks(parts, m) == b"".join(parts) and P.adler32(r, m) == P.adler32(r) == zlib.adler32(r.tobytes())
    # the raw rule: E:raw_gt differs at stream == n, E:raw_size_plus_header where n <= stream < n + 6
    near = [(name, m, n, s) for name, m, sizes in chunks for n, s in sizes if n <= s < n + 6]
    assert near == [("37x1", 0, 222, 222), ("37x17", 0, 222, 224), ("37x33", 0, 222, 226)]
    # E:last_chunk_full_blocks: every older image's last chunk has the blocks of a full one
    for name in KE.BYTE_CASES:
        w, h, channels = KE.case(name)
        types = [t for _, _, _, _, t in channels]
        assert -(-E.chunk_bytes(w, h, types)[-1] // P.BLOCK) == -(-E.ROWS * E.row_bytes(w, types) // P.BLOCK), name
    # the mutants themselves on the small older images, against what the facts say
    for m, want in (("E:raw_gt", [("37x1", 0)]), ("E:raw_size_plus_header", [("37x1", 0), ("37x17", 0), ("37x33", 0)]), ("E:last_chunk_full_blocks", [])):
        got = []
        for name in ("1x1", "37x1", "37x15", "37x16", "37x17", "37x33"):
            w, h, channels = KE.case(name)
            got += [(name, k) for k in (0, 1) if E.encode(w, h, [(p, s, o, t) for _, p, s, o, t in channels], k, m)[0] != KE.encoded(name, k)[0]]
        assert got == want, m


# ---- the count sets of rayn_hip_probe_huffman ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (286, 30))
def test_huffman_sets_reach_what_they_name(n):
    sets = C.huffman_sets(n)
    by_name = {name: (counts, in_block, halvings) for name, counts, in_block, halvings in sets}
    assert len(by_name) == len(sets) and all(len(c) == n and sum(c) < 1 << 32 for c, _, _ in by_name.values())
    for name, (counts, in_block, halvings) in by_name.items():
        lengths = C.expected_lengths(counts)
        assert max(lengths) <= 15 and (halvings is None or P.code_lengths(counts)[1] == halvings), name
        used = [v for v in lengths if v]
        assert len(used) == max(sum(1 for v in counts if v), 1)
        if len(used) > 1:
            assert sum(2.0 ** -v for v in used) == 1.0, name
        assert C.rfc_codes(lengths) == P.canonical_codes(lengths)   # the test's own codes against the restatement's
    assert C.expected_lengths(by_name["all_zero"][0]) == [1] + [0] * (n - 1) == C.expected_lengths(C._placed(n, [4], 0))
    assert sorted(set(C.expected_lengths(by_name["all_equal"][0]))) == ([8, 9] if n == 286 else [4, 5])
    for k, first_depth in ((16, 15), (17, 16)):
        for where in ("low", "high"):
            counts = by_name["fib%d_%s" % (k, where)][0]
            assert max(P.tree_depths(counts)) == first_depth and (max(C.expected_lengths(counts)) == 15) == (k == 16)
    assert sum(by_name["fib30_times_1024"][0]) == 2230587392 and 2048 * sum(C.FIB[:30]) >= 1 << 32   # the largest power of two times F1..F30 below 2^32
    assert [name for name, (_, in_block, _) in by_name.items() if not in_block and not name.startswith("random")] == \
        ["fib24_times_4", "fib30_times_1024"]
    # the leaf-before-internal tie of tests/test_png_lz.py: 1 + 1 makes an internal 2 that meets the leaf 2; the leaf goes first
    lengths = C.expected_lengths(by_name["leaf_before_internal"][0])
    assert [lengths[s] for s in (3, 5, 9, 20)] == [3, 3, 2, 1]
    deep = [name for name, (counts, _, _) in by_name.items() if name.startswith("random") and P.code_lengths(counts)[1] > 0]
    fifteen = [name for name, (counts, _, _) in by_name.items() if name.startswith("random") and max(C.expected_lengths(counts)) == 15]
    assert len(deep) >= 10 and len(fifteen) >= 10, (len(deep), len(fifteen))
    # the two 15-bit codes of F1..F16 are the last of the canonical order, 111 1111 1111 1110 and 111 1111 1111 1111; reversed:
    tab = C.table_entries(C.expected_lengths(by_name["fib16_high"][0]))
    assert tab[n - 16:n - 14] == [0x3FFF | 15 << 16, 0x7FFF | 15 << 16]
