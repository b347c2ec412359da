"""The LZ77 device encoder's stream as tests/png_lz_np.py restates it (include/rayn_hip.h, "PNG encoding on the device, with LZ77
matches"), without a GPU: any inflate gives back the filtered rows and the file decodes to the image; the tokens of small blocks written
out by hand; the symbols the cases reach together; the distance code's special cases and its halving; the sizes against the host encoder
and the run-only device encoder on oracle renders; the png= argument's new value."""
import struct
import zlib

import numpy as np
import pytest

import png_cases as K
import png_lz_cases as KZ
import png_lz_np as Z
import png_np as P
import scenes
from rayn_amd import image


@pytest.mark.parametrize("name", [c[0] for c in KZ.deflate_cases()])
def test_every_case_inflates_to_its_bytes(name):
    data, stride = next((c[1], c[2]) for c in KZ.deflate_cases() if c[0] == name)
    stream, info = Z.encode_filtered(data, stride)
    n, nr, blocks, stored = struct.unpack("<IIII", stream[:16])
    assert (n, nr, blocks, stored) == (len(stream) - 16, len(data), -(-len(data) // P.BLOCK), sum(s for s, _ in info))
    assert stream[16:18] == b"\x78\x01" and zlib.decompress(stream[16:]) == data.tobytes()
    assert len(stream) <= Z.deflate_stream_bound(len(data))
    if "_rows" in name and len(data) > 1000:  # the row candidate is used: the stream differs from the one without it, and is smaller
        assert len(stream) < len(Z.encode_filtered(data, 0)[0]) if stride else len(stream) > len(Z.encode_filtered(data, 97)[0])


@pytest.mark.parametrize("shape,family", [((1, 1, 1), "mask"), ((109, 100, 3), "gradient"), ((109, 100, 3), "mask"), ((255, 128, 1), "gradient"),
                                          ((17, 13, 3), "random"), ((7, 1, 4), "zero"), ((150, 217, 1), "mask")],
                         ids=lambda v: v if isinstance(v, str) else "%dx%dx%d" % v)
def test_image_streams_frame_a_file_that_decodes_to_the_pixels(shape, family):
    w, h, bpp = shape
    img = K.family_image(family, w, h, bpp, seed=w + h)
    stream = Z.encode(img)
    r, _ = P.filter_rows(img)
    assert zlib.decompress(stream[16:]) == r.tobytes() and len(stream) <= P.stream_bound(w, h, bpp)
    data = image.png_from_stream(w, h, bpp, image.png_stream_of(stream))
    assert [t for t, _ in K.parse_png(data)] == [b"IHDR", b"IDAT", b"IEND"]
    assert np.array_equal(K.decode_png(data), img)


@pytest.mark.parametrize("case", [c for c in KZ.HAND_CASES if c[3] is not None], ids=lambda c: c[0])
def test_hand_written_tokens(case):
    name, data, stride, _ = case
    assert Z.block_tokens(data, stride) == KZ.expected(case)
    # behind a run that makes the block a Huffman block - what the device test compares bytes of - the tokens are the same
    _, long, _ = KZ.prefixed(case)
    tokens = Z.block_tokens(long, stride)
    assert [t for t in tokens if t[1] >= KZ.PREFIX] == [(t[0], t[1] + KZ.PREFIX) + t[2:] for t in KZ.expected(case)]
    assert not Z.encode_block(long, True, stride)[1]


def test_length_three_is_taken_up_to_4096_and_the_last_two_positions_are_literals():
    for dist, want in ((4096, ("match", 4096, 3, 4096)), (4097, ("lit", 4097, ord("a")))):
        tokens = Z.block_tokens(KZ.far_three(dist))
        assert [t for t in tokens if t[1] == dist] == [want]
        assert all(t[0] == "lit" for t in tokens if t[1] < dist)
        long = Z.block_tokens(KZ.prefixed(("far", KZ.far_three(dist), 0))[1])
        assert [t for t in long if t[1] == KZ.PREFIX + dist] == [want[:1] + (want[1] + KZ.PREFIX,) + want[2:]]
    assert Z.prev_positions(np.frombuffer(b"abcdab", np.uint8)).tolist() == [-1] * 6           # no prev where fewer than three bytes are left
    assert Z.prev_positions(np.frombuffer(b"abcabcab", np.uint8)).tolist() == [-1, -1, -1, 0, 1, 2, -1, -1]
    assert Z.best_match(b"abcabcab", 6, -1, 0) == (0, 0) and Z.best_match(b"abcabcab", 6, -1, 3) == (2, 3)


def test_a_match_does_not_start_in_the_previous_block():
    r = KZ.across_blocks()
    second = Z.block_tokens(r[P.BLOCK:])
    assert second == [("lit", k, c) for k, c in enumerate(b"uvwxyz")] + [("match", 6, 6, 6)]
    stream, info = Z.encode_filtered(r)
    assert len(info) == 2 and zlib.decompress(stream[16:]) == r.tobytes()


def test_the_cases_reach_every_symbol():
    near, want_near = KZ.near_block()
    far, want_far = KZ.far_block()
    got_near = [(t[2], t[3]) for t in Z.block_tokens(near) if t[0] == "match"]
    got_far = [(t[2], t[3]) for t in Z.block_tokens(far) if t[0] == "match"]
    assert got_near == want_near and got_far == want_far  # the blocks give the matches they were built for, and no other
    pairs = got_near + got_far
    dist, lens = {d for _, d in pairs}, {n for n, _ in pairs}
    assert {Z.distance_symbol(d)[0] for d in dist} == set(range(30))
    assert {P.length_symbol(n)[0] for n in lens} == set(range(257, 286))
    # both ends of the extra-bit ranges of symbols 4 and 17; of symbol 29 the low end and the largest distance a taken match can have:
    # a match at i needs D <= i and i + 3 <= 32768, and at i = 32765 only three bytes are left, which D > 4096 does not take.  So
    # 32767 and 32768, the top of symbol 29's range, do not occur in this format; 32764 does.
    assert {5, 6, 385, 512, 24577, KZ.MAX_DISTANCE} <= dist and KZ.MAX_DISTANCE == 32764
    assert Z.distance_symbol(32764) == (29, 13, 8187) and Z.distance_symbol(24577) == (29, 13, 0)
    assert [Z.distance_symbol(d)[0] for d in (1, 2, 3, 4, 5, 6, 7, 8, 9, 384, 385, 512, 513, 24576)] == [0, 1, 2, 3, 4, 4, 5, 5, 6, 16, 17, 17, 18, 28]
    cases = {c[0]: c for c in KZ.coverage_cases()}
    info = {k: Z.huffman_block(c[1], True, c[2])[2] for k, c in cases.items()}
    assert not any(info["no_match"]["dfreq"]) and info["no_match"]["dlengths"] == [1] + [0] * 29 and not Z.encode_block(cases["no_match"][1], True)[1]
    assert sum(1 for f in info["one_distance"]["dfreq"] if f) == 1 and info["one_distance"]["dlengths"] == [0, 0, 1] + [0] * 27
    assert not Z.encode_block(cases["one_distance"][1], True)[1] and Z.encode_block(cases["stored"][1], True)[1]


def test_distance_code_special_cases_and_its_halving():
    """No block here drives the 30 distance symbols past depth 15: that takes Fibonacci-like counts of 17 symbols, some 4000 matches at
    chosen distances in one block, and no such block was constructed.  The halving is pinned here on the tree function with synthetic
    counts; on the device the distance code's own instantiation of the builder, huffman_code<30> of png_device.h, runs alone through
    rayn_hip_probe_huffman on the count sets of tests/encode_edge_cases.py - depth 15, depth 16, three and eleven halvings, the tie
    below, 200 seeded sets - in tests/test_encode_edges_device.py."""
    assert Z.distance_lengths([0] * 30) == ([1] + [0] * 29, 0)
    one = [0] * 30
    one[7] = 12
    assert Z.distance_lengths(one) == ([0] * 7 + [1] + [0] * 22, 0)
    two = list(one)
    two[29] = 1
    assert Z.distance_lengths(two)[0] == [0] * 7 + [1] + [0] * 21 + [1]
    fib, a, b = [0] * 30, 1, 1
    for s in range(24):
        fib[29 - s] = a
        a, b = b, a + b
    assert max(P.tree_depths(fib)) == 23
    lengths, halvings = Z.distance_lengths(fib)
    assert halvings >= 1 and max(lengths) <= 15 and sum(2.0 ** -n for n in lengths if n) == 1.0
    assert all(n > 0 for n in lengths[6:]) and not any(lengths[:6])
    # internal nodes are 30, 31, ...: equal weights merge by index, a leaf before an internal node
    f = [0] * 30
    f[3], f[5], f[9], f[20] = 1, 1, 2, 3   # 30 = 3 + 5 (2); 9 (leaf, 2) and 30 (2) -> 31 (4); 20 (3) and 31
    assert [P.tree_depths(f)[s] for s in (3, 5, 9, 20)] == [3, 3, 2, 1]


# ---- size against the host encoder and the run-only device encoder ---------------------------------------------------------------------------

# stream bytes / bytes of zlib.compress(unfiltered rows, 6) on the CPU-oracle renders of test_png.py's table (160x96, 4 samples per pixel,
# 2 bounces): (device-lz77, device), as measured (DESIGN.md section 8 has the table); the encoders are deterministic, the 2 % only absorb
# changes of the scene fixtures
MEASURED_RATIO = {("s2", "color"): (0.9844, 1.0144), ("s2", "normal"): (0.9347, 0.9425), ("s2", "alpha"): (1.4511, 1.1823),
                  ("s0", "color"): (1.4178, 1.2832), ("s0", "normal"): (0.7276, 0.6457), ("s0", "alpha"): (1.8750, 1.5726)}
# On four of the six the LZ77 stream is LARGER than the run-only one: at this size a match's distance costs 7 to 8 bits where the
# run-only format spends one, and the greedy parse takes every match of three bytes.  Only the shipped scene's Color and WorldNormal gain.
SMALLER_THAN_RUN_ONLY = {("s2", "color"), ("s2", "normal")}


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
def test_size_against_the_host_and_the_run_only_encoder_on_oracle_renders(rendered_images, key):
    img = rendered_images[key]
    h, w, bpp = img.shape
    stream, runs = Z.encode(img), P.encode(img)
    host = zlib.compress(b"".join(b"\x00" + img[y].tobytes() for y in range(h)), 6)
    ratio, ratio_runs = (len(stream) - 16) / len(host), (len(runs) - 16) / len(host)
    print(key, "device-lz77 stream", len(stream) - 16, "device", len(runs) - 16, "host", len(host), "ratios %.4f %.4f" % (ratio, ratio_runs))
    assert ratio <= MEASURED_RATIO[key][0] + 0.02 and ratio_runs <= MEASURED_RATIO[key][1] + 0.02
    assert (len(stream) < len(runs)) == (key in SMALLER_THAN_RUN_ONLY)
    assert np.array_equal(K.decode_png(image.png_from_stream(w, h, bpp, stream[16:])), img)


# ---- the png= argument -------------------------------------------------------------------------------------------------------------------------

def test_png_argument_takes_device_lz77():
    import rayn_amd as R
    from rayn_amd import film as F
    K_ = R.ChannelKind
    kinds = (K_.Color, K_.Alpha, K_.Background, K_.WorldNormal)
    assert F.PNG_ENCODERS == ("host", "device", "device-lz77")
    write = [K_.Color, K_.Alpha, K_.WorldNormal]
    assert F.plan_sequence(kinds, write, png="device-lz77").png == "device-lz77"
    assert F.plan_sequence(kinds, write, png="device-lz77").jobs == F.plan_sequence(kinds, write).jobs  # the file names do not change
    for bad in ("device_lz77", "lz77", "device-lz", "DEVICE-LZ77"):
        with pytest.raises(ValueError, match="png must be one of"):
            F.plan_sequence(kinds, [K_.Color], png=bad)


def test_size_helpers_through_the_library_need_no_gpu():
    from rayn_amd import _lib
    L = _lib.lib()
    for n in (1, 2, 32767, 32768, 32769, 65537, (1 << 31) - 1):
        blocks = -(-n // P.BLOCK)
        assert L.rayn_deflate_stream_bound(n) == Z.deflate_stream_bound(n) == (16 + 2 + n + 10 * blocks + 4 + 15) // 16 * 16
        assert L.rayn_deflate_scratch_bytes(n) >= n + blocks * (P.BLOCK + 10 + 65536)
    for n in (0, 1 << 31, 1 << 40):
        assert L.rayn_deflate_stream_bound(n) == 0 == Z.deflate_stream_bound(n) and L.rayn_deflate_scratch_bytes(n) == 0
    for w, h, bpp in K.SHAPES + ((1280, 720, 3),):
        assert L.rayn_png_scratch_bytes_lz77(w, h, bpp) == L.rayn_png_scratch_bytes(w, h, bpp) + 65536 * P.n_blocks(w, h, bpp)
        assert L.rayn_deflate_stream_bound(P.filtered_bytes(w, h, bpp)) == L.rayn_png_stream_bound(w, h, bpp)
    for w, h, bpp in ((0, 5, 3), (5, 5, 2), (1 << 24, 1, 1), (1 << 16, 1 << 15, 1)):
        assert L.rayn_png_scratch_bytes_lz77(w, h, bpp) == 0
