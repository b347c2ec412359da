"""The device PNG encoder's stream as tests/png_np.py restates it (include/rayn_hip.h, "PNG encoding on the device"), without a GPU: any
inflate accepts it and gives back the filtered rows, which un-filter to the image; the token rule, the length limit and the stored
fallback at their edges; rayn_png_stream_bound; the size against the host encoder on oracle renders; the png= argument's validation."""
import ctypes as C
import functools
import struct
import zlib

import numpy as np
import pytest

import png_cases as K
import png_np as P
import scenes
from rayn_amd import image


@functools.lru_cache(maxsize=None)
def _family(family, shape):
    w, h, bpp = shape
    img = K.family_image(family, w, h, bpp, seed=w + h)
    img.setflags(write=False)
    r, types = P.filter_rows(img)
    stream, info = P.encode_filtered(r)
    return img, r, types, stream, info


@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_stream_inflates_to_the_filtered_rows_and_they_unfilter_to_the_image(shape, family):
    w, h, bpp = shape
    img, r, types, stream, info = _family(family, shape)
    n, nr, blocks, stored = struct.unpack("<IIII", stream[:16])
    assert (n, nr, blocks, stored) == (len(stream) - 16, h * (1 + w * bpp), P.n_blocks(w, h, bpp), sum(s for s, _ in info))
    assert stream[16:18] == b"\x78\x01"
    assert zlib.decompress(stream[16:]) == r.tobytes()
    assert np.array_equal(r.reshape(h, -1)[:, 0], types) and set(types.tolist()) <= {0, 1, 2, 3, 4}
    if w * h * bpp <= 40000:  # the byte-by-byte decoder on every small shape; the larger ones go through it once, below
        assert np.array_equal(K.unfilter(r, w, h, bpp), img)
    # every block is at most len + 5 bytes plus its alignment (000 in a byte of its own, 00 00 FF FF), and the whole within the bound
    lens = [min(P.BLOCK, nr - o) for o in range(0, nr, P.BLOCK)]
    for (st, size), ln in zip(info, lens):
        assert size <= ln + 5 + (0 if st else 5) and (not st or size == ln + 5)
    assert len(stream) <= P.stream_bound(w, h, bpp)
    if family == "random" and nr >= 1024:
        assert all(st for st, _ in info)  # nothing to gain: stored
    if family == "zero":  # a few bytes behind the 1222-bit header (a tiny block cannot pay for those 153 bytes)
        assert all(not st and size <= 153 + 40 + 5 for (st, size), ln in zip(info, lens) if ln >= 1024)


def test_png_from_stream_frames_a_file_that_parses():
    for family, shape in (("gradient", (300, 100, 3)), ("mask", (17, 13, 3)), ("gradient", (7, 1, 4)), ("mask", (150, 217, 1))):
        w, h, bpp = shape
        img, r, types, stream, info = _family(family, shape)
        data = image.png_from_stream(w, h, bpp, image.png_stream_of(stream))
        chunks = K.parse_png(data)
        assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
        assert struct.unpack(">IIBBBBB", chunks[0][1]) == (w, h, 8, {1: 0, 3: 2, 4: 6}[bpp], 0, 0, 0)
        assert chunks[1][1] == stream[16:] and chunks[2][1] == b""
        assert np.array_equal(K.decode_png(data), img)
    with pytest.raises(ValueError, match="length word"):
        image.png_stream_of(struct.pack("<IIII", 1000, 0, 0, 0) + b"\x78\x01")


def test_the_host_encoder_still_writes_what_it_wrote(tmp_path):
    """image.save goes through png_from_stream now: filter 0 on every row, zlib level 6, the same bytes as before"""
    img = K.family_image("gradient", 17, 13, 3)
    image.save(str(tmp_path / "a.png"), img)
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(13))
    chunk = lambda tag, d: struct.pack(">I", len(d)) + tag + d + struct.pack(">I", zlib.crc32(tag + d) & 0xFFFFFFFF)
    want = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 17, 13, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b"")
    assert (tmp_path / "a.png").read_bytes() == want


@pytest.mark.parametrize("n", K.RUN_LENGTHS)
def test_token_rule_at_its_edges(n):
    tokens = P.block_tokens(K.run_block(n))
    assert [("lit",) if t[0] == "lit" else ("match", t[2]) for t in tokens] == K.expected_run_tokens(n)
    covered = sum(1 if t[0] == "lit" else t[2] for t in tokens)
    assert covered == n and all(t[2] == 7 for t in tokens if t[0] == "lit")
    data, stored = P.encode_block(K.run_block(n), True)
    assert zlib.decompress(b"\x78\x01" + data + struct.pack(">I", zlib.adler32(bytes([7]) * n))) == bytes([7]) * n


def test_every_edge_run_in_one_block_and_a_run_cut_at_a_block_start():
    data = K.run_edges_bytes()
    tokens = P.block_tokens(data)
    want = [("lit",)] + [t for n in K.RUN_LENGTHS[:-1] for t in K.expected_run_tokens(n)] + [("lit",)]
    assert [("lit",) if t[0] == "lit" else ("match", t[2]) for t in tokens] == want
    # a run of 600 bytes of which 100 lie in the first block: it is two runs, of 100 and of 500
    r = np.concatenate([np.arange(P.BLOCK - 100, dtype=np.uint32).astype(np.uint8) | 1, np.zeros(600, np.uint8), np.array([5], np.uint8)])
    first, second = P.block_tokens(r[:P.BLOCK]), P.block_tokens(r[P.BLOCK:])
    assert [(t[0], t[2]) for t in first[-2:]] == [("lit", 0), ("match", 99)]
    assert [(t[0], t[2]) for t in second] == [("lit", 0), ("match", 258), ("match", 241), ("lit", 5)]
    stream, info = P.encode_filtered(r)
    assert zlib.decompress(stream[16:]) == r.tobytes() and len(info) == 2


def test_a_block_of_one_literal_one_length_code_and_end_of_block():
    blk = K.three_symbol_block()
    data, bits, info = P.huffman_block(blk, True)
    used = {s: n for s, n in enumerate(info["freq"]) if n}
    assert used == {0: 1, 285: 20, 256: 1} and info["has_match"]
    assert [info["lengths"][s] for s in (0, 256, 285)] == [2, 2, 1]
    assert bits == P.HEADER_BITS + 2 + 20 * (1 + 1) + 2 and len(data) == (bits + 7) // 8
    assert zlib.decompress(b"\x78\x01" + data + struct.pack(">I", zlib.adler32(blk.tobytes()))) == blk.tobytes()


def test_length_limit_on_fibonacci_counts():
    """18 symbols with the counts F1..F18 (end-of-block is F1): plain Huffman gives depth 17; one halving brings it under 15.  The lengths
    are pinned.  (The 18 counts sum to 6764, the 17 literals to the 6763 bytes of the block.)"""
    blk = K.fibonacci_bytes()
    assert len(blk) == 6763 and not np.any(blk[1:] == blk[:-1])
    tokens = P.block_tokens(blk)
    assert all(t[0] == "lit" for t in tokens)
    freq = P.token_frequencies(tokens)
    assert sorted(f for f in freq if f) == [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584]
    assert max(P.tree_depths(freq)) == 17
    lengths, halvings = P.code_lengths(freq)
    assert halvings == 1
    assert max(P.tree_depths([(f + 1) >> 1 if f else 0 for f in freq])) <= 15  # one halving suffices, as the restatement says
    assert max(lengths) <= 15 and sum(2.0 ** -n for n in lengths if n) == 1.0  # Kraft-complete
    assert [lengths[v] for v in K.FIBONACCI_VALUES] == [2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 9] and lengths[P.END_OF_BLOCK] == 9
    data, stored = P.encode_block(blk, True)
    assert not stored and zlib.decompress(b"\x78\x01" + data + struct.pack(">I", zlib.adler32(blk.tobytes()))) == blk.tobytes()
    # and a count set that needs two halvings is limited too
    deep = [0] * P.N_SYMBOLS
    a, b = 1, 1
    for s in range(24):
        deep[s] = a
        a, b = b, a + b
    lengths, halvings = P.code_lengths(deep)
    assert halvings >= 1 and max(lengths) <= 15 and sum(2.0 ** -n for n in lengths if n) == 1.0


def test_tree_order_is_weight_then_index():
    """Equal weights: the lower index merges first, a leaf before an internal node"""
    f = [0] * P.N_SYMBOLS
    f[10], f[20], f[30], f[256] = 1, 1, 2, 2   # 10 + 20 -> node 286 (weight 2); then the leaves 30 and 256 go before it
    assert [P.tree_depths(f)[s] for s in (10, 20, 30, 256)] == [2, 2, 2, 2]
    f[10], f[20], f[30], f[256] = 1, 1, 1, 1
    assert [P.tree_depths(f)[s] for s in (10, 20, 30, 256)] == [2, 2, 2, 2]
    f[10], f[20], f[30], f[256] = 1, 1, 2, 3   # 286 = 10 + 20 (2); 30 (leaf, 2) and 286 (2) -> 287 (4); 256 (3) and 287
    assert [P.tree_depths(f)[s] for s in (10, 20, 30, 256)] == [3, 3, 2, 1]
    assert P.canonical_codes([2, 1, 3, 3]) == [2, 0, 6, 7]  # RFC 1951 3.2.2's rule


def test_stored_fallback_and_the_block_bound():
    rng = np.random.default_rng(5)
    blk = rng.integers(0, 256, P.BLOCK, dtype=np.uint8)
    for final in (False, True):
        data, stored = P.encode_block(blk, final)
        assert stored and data[:5] == struct.pack("<BHH", int(final), P.BLOCK & 0xFFFF, (P.BLOCK & 0xFFFF) ^ 0xFFFF) and data[5:] == blk.tobytes()
    zero = np.zeros(P.BLOCK, np.uint8)
    data, stored = P.encode_block(zero, False)
    assert not stored and len(data) <= 153 + 40 + 5 and data[-4:] == b"\x00\x00\xff\xff"
    # a tiny block cannot pay for the 153-byte header: stored
    data, stored = P.encode_block(np.zeros(2, np.uint8), True)
    assert stored and data == b"\x01\x02\x00\xfd\xff\x00\x00"
    # just compressible: the Huffman form is taken exactly when it is shorter than len + 5
    for n in (140, 150, 160, 170, 200):
        blk = (np.arange(n) % 2).astype(np.uint8)
        h, bits, _ = P.huffman_block(blk, True)
        data, stored = P.encode_block(blk, True)
        assert stored == (len(h) >= n + 5) and len(data) == min(len(h), n + 5) if len(h) != n + 5 else stored


def test_stream_bound_through_the_library_needs_no_gpu():
    from rayn_amd import _lib
    L = _lib.lib()
    for w, h, bpp in K.SHAPES + ((1280, 720, 3), (1920, 1080, 4), (640, 360, 1)):
        n, blocks = P.filtered_bytes(w, h, bpp), P.n_blocks(w, h, bpp)
        assert L.rayn_png_stream_bound(w, h, bpp) == P.stream_bound(w, h, bpp) == (16 + 2 + n + 10 * blocks + 4 + 15) // 16 * 16
        assert L.rayn_png_scratch_bytes(w, h, bpp) >= n + blocks * (P.BLOCK + 10)
    for w, h, bpp in ((0, 5, 3), (5, 0, 3), (5, 5, 2), (5, 5, 0), (1 << 24, 1, 1), (1 << 16, 1 << 15, 1)):
        assert L.rayn_png_stream_bound(w, h, bpp) == 0 == P.stream_bound(w, h, bpp) and L.rayn_png_scratch_bytes(w, h, bpp) == 0
    assert L.rayn_png_stream_bound((1 << 24) - 1, 1, 1) == P.stream_bound((1 << 24) - 1, 1, 1) > 0


# ---- size against the host encoder ------------------------------------------------------------------------------------------------------------

# stream bytes of the restatement / bytes of zlib.compress(unfiltered rows, 6) on CPU-oracle renders at 160x96, 4 samples per pixel, 2
# bounces, as measured (DESIGN.md section 8 has the table); the encoder is deterministic, the 2 % only absorb changes of the scene fixtures
MEASURED_RATIO = {("s2", "color"): 1.0144, ("s2", "normal"): 0.9425, ("s2", "alpha"): 1.1823,
                  ("s0", "color"): 1.2832, ("s0", "normal"): 0.6457, ("s0", "alpha"): 1.5726}


@pytest.fixture(scope="module")
def rendered_images(oracle):
    import rayn_amd
    out = {}
    for name in ("s2", "s0"):  # the shipped scene, the sphere scene
        wd, _, _ = scenes.scene(name, (160, 96))
        p = rayn_amd.frame_params(160, 96, 1, 2)
        tabs = rayn_amd.build_tables(4, 2, p.volume_marches, p.frame, 160, 96)
        ref, _ = oracle.render(wd, p, tabs)
        out[name, "color"] = image.color_image(ref["color"], background=ref["background"])
        out[name, "normal"] = image.normal_image(ref["normal"])
        out[name, "alpha"] = image.alpha_image(ref["alpha"])
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


@pytest.mark.parametrize("key", sorted(MEASURED_RATIO), ids="-".join)
def test_size_against_the_host_encoder_on_oracle_renders(rendered_images, key):
    img = rendered_images[key]
    h, w, bpp = img.shape
    stream = P.encode(img)
    host = zlib.compress(b"".join(b"\x00" + img[y].tobytes() for y in range(h)), 6)
    ratio = (len(stream) - 16) / len(host)
    print(key, "device stream", len(stream) - 16, "host", len(host), "ratio %.4f" % ratio, "raw", h * (1 + w * bpp))
    assert ratio <= MEASURED_RATIO[key] + 0.02
    assert np.array_equal(K.decode_png(image.png_from_stream(w, h, bpp, stream[16:])), img)


# ---- the png= argument -------------------------------------------------------------------------------------------------------------------------

def test_png_argument_is_validated_before_anything_else():
    import rayn_amd as R
    from rayn_amd import film as F
    K_ = R.ChannelKind
    kinds = (K_.Color, K_.Alpha, K_.Background, K_.WorldNormal)
    assert F.plan_sequence(kinds, [K_.Color]).png == "host"
    assert F.plan_sequence(kinds, [K_.Color], png="device").png == "device"
    host, dev = F.plan_sequence(kinds, [K_.Color, K_.Alpha, K_.WorldNormal]), F.plan_sequence(kinds, [K_.Color, K_.Alpha, K_.WorldNormal], png="device")
    assert host.jobs == dev.jobs  # the file names do not change
    for bad in ("gpu", "", None, 1, "Device"):
        with pytest.raises(ValueError, match="png must be one of"):
            F.plan_sequence(kinds, [K_.Color], png=bad)
        with pytest.raises(ValueError, match="png must be one of"):  # before the channels are looked at: a film that cannot write Color
            F.plan_sequence((K_.Alpha,), [K_.Color], png=bad)
        bare = F.Film.__new__(F.Film)  # no context, no channels: the rule needs nothing of the film
        with pytest.raises(ValueError, match="png must be one of"):
            bare.save_to([K_.Color], "/nonexistent/never_made", "x", png=bad)
        with pytest.raises(ValueError, match="png must be one of"):
            bare.render_sequence(None, None, None, None, None, [1], 24, 1.0 / 24.0, 1, [K_.Color], "/nonexistent/never_made", "x", png=bad)
