"""The device PNG, LZ77 and EXR encoders at their decision edges: named cases, each the inputs, the outcome written out by hand (`expect`)
and `kills`, the mutants of the restatements (png_np's "P:", png_lz_np's "Z:", exr_np's "E:") whose bytes differ from the statement's on
that case.  A case is one of three kinds, and goes through every entry of its kind:
  "png"      img (h, w, bpp) uint8              rayn_hip_png_encode_device (png_np.encode), rayn_hip_png_encode_lz77_device (png_lz_np.encode)
  "deflate"  data uint8, stride                 rayn_hip_deflate_lz77_device (png_lz_np.encode_filtered)
  "exr"      w, h, channels, matches            rayn_hip_exr_encode_device with every value of `matches` (exr_np.encode)
HUFFMAN_SETS are the count sets of rayn_hip_probe_huffman, the Huffman construction alone.

Searched inputs - the ties of the raw rule and of the stored rule - are committed as the generator's parameters; the searches were a seeded
walk over those parameters on the CPU and are not part of the repository.  tests/test_encode_edge_cases.py asserts that every found input
sits where it claims to.

The restatements cost 0.1 to 0.3 s per 32 KiB block, so everything here is cached: expected() once per (case, entry), and the streams of
257 blocks are assembled by the restatement's own framing (png_np.encode_filtered's block_encoder) from per-block encodings memoised by
(kernel, stride, bytes, final) - the block encoders are pure functions of those.

tests/test_encode_edge_cases.py holds all of this to account without a GPU; tests/test_encode_edges_device.py pushes every case through
every entry it applies to.  TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this."""
import functools

import numpy as np

import exr_np as E
import png_cases as K
import png_lz_cases as KZ
import png_lz_np as Z
import png_np as P

BLOCK = P.BLOCK
BLOCK_MUTANTS = ("P:stored_gt", "P:limit_16", "P:limit_14", "Z:stored_gt", "Z:exit_bit8")   # change a block's own bytes
STREAM_MUTANTS = ("P:adler_behind_off", "P:layout_carry")                                      # change how blocks become a stream
EXR_MUTANTS = ("E:raw_gt", "E:raw_size_plus_header", "E:last_chunk_full_blocks")
MUTANTS = BLOCK_MUTANTS + STREAM_MUTANTS + EXR_MUTANTS


class Case:
    def __init__(self, name, family, kind, kills, **fields):
        self.name, self.family, self.kind, self.kills = name, family, kind, tuple(kills)
        self.big = False      # a stream of 257 blocks: only the stream mutants are run on it
        self.__dict__.update(fields)

    def __repr__(self):
        return self.name


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


FIB = [1, 1]
while len(FIB) < 30:
    FIB.append(FIB[-1] + FIB[-2])   # FIB[k - 1] = Fk


# ---- family 1: the raw rule at the tie (EXR) -------------------------------------------------------------------------------------------------
# One chunk of 16x16 UINT words, n_k = 1024: the word TIE_FLAT everywhere but in the first `random` words of the film's layout, which are
# rng(seed)'s, and then single bytes of that buffer replaced.  The zlib stream of the chunk is n_k - 1, n_k and n_k + 1 bytes long.
TIE_W, TIE_H, TIE_FLAT = 16, 16, 0x3F800000
RAW_TIES = {  # matches -> {stream - n_k: (seed, random words, ((byte index, value), ...))}
    0: {-1: (1, 202, ((983, 60),)), 0: (1, 201, ((988, 157),)), 1: (1, 203, ())},
    1: {-1: (1, 214, ((775, 144),)), 0: (1, 213, ((1007, 83),)), 1: (1, 213, ((981, 129),))},
}


def tie_words(seed, random, nudges=()):
    a = np.full(TIE_W * TIE_H, TIE_FLAT, np.uint32)
    a[:random] = np.random.default_rng(seed).integers(0, 1 << 32, random, dtype=np.uint64).astype(np.uint32)
    b = a.view(np.uint8).copy()
    for i, v in nudges:
        b[i] = v
    return _frozen(b.view(np.uint32))


def raw_tie_cases():
    out = []
    for matches, ties in RAW_TIES.items():
        for d, (seed, random, nudges) in sorted(ties.items()):
            kills = {-1: (), 0: ("E:raw_gt", "E:raw_size_plus_header"), 1: ("E:raw_size_plus_header",)}[d]
            out.append(Case("raw_tie/matches%d/stream_is_n%+d" % (matches, d), "raw_tie", "exr", kills, w=TIE_W, h=TIE_H,
                            channels=[("Y", tie_words(seed, random, nudges), 1, 0, E.UINT)], matches=(matches,),
                            expect=dict(stream_minus_n=d, raw=[d >= 0])))
    return out


# ---- family 2: the stored rule at the tie (both block kernels) -------------------------------------------------------------------------------
# huffman_bytes - (len + 5) in {-1, 0, +1}.  A block that is not the last of its stream has 32768 bytes, whatever the stream: the "short"
# ties are final blocks of a few hundred bytes, the "full" ones first blocks of 32768 bytes in front of a second block of a few bytes, which
# is stored as every tiny block is.
# Run-only kernel (through the PNG entry, one image row): the block is the filtered row, its type byte included.
# LZ77 kernel (through the deflate entry): the block is the data.
STORED_TIES = {  # kernel -> form -> {huffman_bytes - (len + 5): generator parameters}
    "P": {"short": {-1: (1, 331), 0: (1, 329), 1: (1, 327)}, "full": {-1: (5, 24461), 0: (5, 24477), 1: (5, 24491)}},
    "Z": {"short": {-1: (1, 334), 0: (1, 332), 1: (1, 330)}, "full": {-1: (5, 25890), 0: (5, 25903), 1: (5, 25910)}},
}
TAIL = np.array([1, 2, 3, 4, 5], np.uint8)   # the short second block


def short_bytes(seed, n, alphabet=16):
    """n bytes of rng(seed) below `alphabet`: about four bits a byte"""
    return np.random.default_rng(seed).integers(0, alphabet, n, dtype=np.uint8)


def full_bytes(seed, k, alphabet=64):
    """32768 bytes of rng(seed) below `alphabet`, the first k of them replaced by bytes below 256: k moves the Huffman form's size"""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, alphabet, BLOCK, dtype=np.uint8)
    b[:k] = rng.integers(0, 256, k, dtype=np.uint8)
    return b


def one_row(data):
    return _frozen(np.asarray(data, np.uint8).reshape(1, -1, 1))


def stored_tie_cases():
    out = []
    for kernel, kind, mutant in (("P", "png", "P:stored_gt"), ("Z", "deflate", "Z:stored_gt")):
        for form in ("short", "full"):
            for d, (seed, par) in sorted(STORED_TIES[kernel][form].items()):
                data = short_bytes(seed, par) if form == "short" else np.concatenate([full_bytes(seed, par), TAIL])
                fields = dict(img=one_row(data)) if kind == "png" else dict(data=_frozen(data), stride=0)
                out.append(Case("stored_tie/%s/%s/huffman_is_stored%+d" % (kernel, form, d), "stored_tie", kind, (mutant,) if d == 0 else (),
                                expect=dict(kernel=kernel, huffman_minus_stored=d, stored=[d >= 0] + ([True] if form == "full" else [])), **fields))
    return out


# ---- family 3: code lengths of 15, and a first tree of depth 16, through real blocks -----------------------------------------------------------
def fib_block(literals):
    """png_cases.fibonacci_bytes' construction for `literals` values with the counts F2..F(literals + 1): no two neighbours are equal, so
    the run-only kernel sees literals alone; with end-of-block, which counts F1 = 1, the counts are F1..F(literals + 1).  The first byte
    is the most frequent value, 0."""
    counts = sorted(FIB[1:literals + 1], reverse=True)
    left = dict(zip(K.FIBONACCI_VALUES, counts))
    out, prev = [], None
    for _ in range(sum(counts)):
        v = max((k for k in left if k != prev and left[k]), key=lambda k: (left[k], -K.FIBONACCI_VALUES.index(k)))
        out.append(v)
        left[v] -= 1
        prev = v
    return np.array(out, np.uint8)


# the code lengths by hand.  F1..F16: every merge takes the two smallest, the tree is a chain: the two counts of 1 (end-of-block and the
# value 249) get 15 bits, then one value per length down to the most frequent, 0, with 1 bit.  Values by falling count: 0, 1, 255, 2, 254, ...
DEPTH15_LENGTHS = {0: 1, 1: 2, 255: 3, 2: 4, 254: 5, 3: 6, 253: 7, 4: 8, 252: 9, 5: 10, 251: 11, 6: 12, 250: 13, 7: 14, 249: 15, 256: 15}
# F1..F17 is a chain of depth 16; halved once the counts are 1 1 1 2 3 4 7 11 17 28 45 72 117 189 305 494 799, whose tree has depth 9
DEPTH16_LENGTHS = {0: 2, 1: 2, 255: 3, 2: 3, 254: 4, 3: 4, 253: 5, 4: 5, 252: 6, 5: 6, 251: 7, 6: 7, 250: 8, 7: 8, 249: 9, 8: 9, 256: 8}


def unpreprocess(p):
    """The bytes whose exr_np.preprocess is p (of even length)"""
    p = np.asarray(p, np.uint8).astype(np.int64)
    t = np.cumsum(np.concatenate([p[:1], p[1:] - 128])) & 255
    raw = np.empty(len(p), np.uint8)
    raw[0::2], raw[1::2] = t[:len(p) // 2], t[len(p) // 2:]
    return raw


def f32_of_half(h):
    """float32 words that exr_np.half_bits takes to the binary16 bits h: the exact value, and for a NaN its ten payload bits"""
    h = np.asarray(h, np.uint16)
    with np.errstate(invalid="ignore"):
        exact = h.view(np.float16).astype(np.float32).view(np.uint32)
    x = h.astype(np.uint32)
    nan = ((x & 0x7C00) == 0x7C00) & ((x & 0x3FF) != 0)
    return np.where(nan, ((x & 0x8000) << 16) | 0x7F800000 | ((x & 0x3FF) << 13), exact).astype(np.uint32)


def depth_cases():
    out = []
    for literals, lengths, halvings, mutant in ((15, DEPTH15_LENGTHS, 0, "P:limit_14"), (16, DEPTH16_LENGTHS, 1, "P:limit_16")):
        blk = fib_block(literals)
        depth = literals   # of the first tree: a chain over literals + 1 symbols
        expect = dict(lengths=lengths, halvings=halvings, first_depth=depth, block=_frozen(blk))
        # the filter type byte of the one row, 0, is the block's first byte
        out.append(Case("depth/%d/png" % depth, "depth", "png", (mutant,), img=one_row(blk[1:]), expect=expect))
        # the LZ77 kernel finds matches in these bytes (0 1 0 1 ... repeats): no literal-only block with these counts exists for it, since
        # a block without a repeated trigram needs about as many distinct trigrams as bytes, and 16 values of which one holds 38 % of the
        # bytes have far fewer.  The bytes still go through it, compared as bytes; huffman_code at depth 15 and 16 is the probe's part.
        out.append(Case("depth/%d/deflate" % depth, "depth", "deflate", (), data=_frozen(blk), stride=0, expect=dict(literal_only=False)))
    # one chunk of 1291x1 HALF whose pre-processed bytes are the depth-15 block (2582 bytes; the depth-16 block has an odd length, which
    # no chunk has).  With matches = 0 the block kernel sees that block; with matches = 1 the bytes are compared as bytes.
    blk = fib_block(15)
    words = f32_of_half(unpreprocess(blk).view("<u2"))
    out.append(Case("depth/15/exr", "depth", "exr", ("P:limit_14",), w=len(blk) // 2, h=1, channels=[("Y", _frozen(words), 1, 0, E.HALF)], matches=(0, 1),
                    expect=dict(lengths=DEPTH15_LENGTHS, halvings=0, first_depth=15, block=_frozen(blk), raw=[False])))
    return out


# ---- family 4: the builder alone (rayn_hip_probe_huffman) ----------------------------------------------------------------------------------------
def expected_lengths(counts):
    """What huffman_code<N> leaves in clen: png_np.code_lengths / png_lz_np.distance_lengths - the same construction - and, with no
    symbol in use, length 1 for symbol 0"""
    if not any(counts):
        return [1] + [0] * (len(counts) - 1)
    return P.code_lengths(list(counts))[0]


def _placed(n, values, at):
    c = [0] * n
    c[at:at + len(values)] = values
    return c


@functools.lru_cache(maxsize=None)
def huffman_sets(n):
    """[(name, counts, a 32 KiB block can produce it?, halvings or None)] for huffman_code<n>, n = 286 or 30.  A block has at most 32768
    tokens and one end-of-block, and at most 32768 / 3 matches: a set with a larger sum is the builder's own edge, not an encoder's."""
    assert n in (P.N_SYMBOLS, Z.N_DISTANCES)
    most = BLOCK + 1 if n == P.N_SYMBOLS else BLOCK // 3
    sets = [("all_zero", [0] * n, None), ("one_symbol", _placed(n, [7], 5), 0), ("two_symbols", _placed(n, [9], 3)[:n - 1] + [2], 0)]
    for k, halvings in ((16, 0), (17, 1)):   # depth 15: no halving; depth 16: one
        sets += [("fib%d_low" % k, _placed(n, FIB[:k], 0), halvings), ("fib%d_high" % k, _placed(n, FIB[:k], n - k), halvings)]
    sets += [("all_equal", [3] * n, 0),                                       # lengths {8, 9} / {4, 5}: ties go by symbol index
             ("fib24_times_4", _placed(n, [4 * f for f in FIB[:24]], 0), 3),
             ("fib30_times_1024", _placed(n, [1024 * f for f in FIB[:30]], 0), 11),   # sum 2 230 587 392: the largest such set below 2^32
             ("leaf_before_internal", [1 if s in (3, 5) else 2 if s == 9 else 3 if s == 20 else 0 for s in range(n)], 0)]
    rng = np.random.default_rng(1000 + n)
    for k in range(200):   # steep and flat spectra over some of the symbols: shallow trees, deep ones, halvings
        steep = rng.uniform(0.0, 14.0)
        c = np.floor(np.exp(rng.uniform(0.0, steep, n))).astype(np.int64)
        c[rng.random(n) < rng.uniform(0.0, 0.9)] = 0
        sets.append(("random%03d" % k, c.tolist(), None))
    return [(name, c, sum(c) <= most, halvings) for name, c, halvings in sets]


def rfc_codes(lengths):
    """RFC 1951 3.2.2 from the lengths alone: bl_count, next_code, codes in symbol order"""
    bl_count = [0] * 16
    for n in lengths:
        if n:
            bl_count[n] += 1
    code, next_code = 0, [0] * 16
    for bits in range(1, 16):
        code = (code + bl_count[bits - 1]) << 1
        next_code[bits] = code
    out = []
    for n in lengths:
        out.append(next_code[n] if n else 0)
        if n:
            next_code[n] += 1
    return out


def table_entries(lengths):
    """huffman_code's tab: the code, bit-reversed in its length, | length << 16"""
    return [(int(format(c, "0%db" % n)[::-1], 2) | n << 16) if n else 0 for c, n in zip(rfc_codes(lengths), lengths)]


# ---- family 5: more than 256 blocks --------------------------------------------------------------------------------------------------------------
# k_png_layout gives thread t the blocks [t * chunk, (t + 1) * chunk), chunk = ceil(blocks / 256): with 257 or 258 blocks chunk is 2 and a
# thread's range starts at every even block.
_MEMO = {}


def memo_encoder(kernel, stride=0):
    """png_np.encode_block / png_lz_np.encode_block behind a cache by (kernel, stride, bytes, final)"""
    def encode(blk, final):
        key = (kernel, stride, blk.tobytes(), final)
        if key not in _MEMO:
            _MEMO[key] = P.encode_block(blk, final) if kernel == "P" else Z.encode_block(blk, final, stride)
        return _MEMO[key]
    return encode


BIG_PATTERN = "FSSMSFFS"   # flat, stored, ramp with matches: at the even blocks S|S, M|S, F|F and S|F meet


@functools.lru_cache(maxsize=None)
def big_stream():
    """257 * 32768 + 5 bytes of four block contents: a flat one, a ramp of period 251 (matches at distance 251), random bytes, and the
    last, short one.  258 blocks."""
    kinds = {"F": np.full(BLOCK, 7, np.uint8), "M": (np.arange(BLOCK) % 251).astype(np.uint8),
             "S": np.random.default_rng(5).integers(0, 256, BLOCK, dtype=np.uint8)}
    return _frozen(np.concatenate([kinds[BIG_PATTERN[i % 8]] for i in range(257)] + [TAIL]))


BIG_W, BIG_H = 4096, 2049
BIG_STORED, BIG_TWOS, BIG_PERIODIC = (3, 4, 8, 11, 253, 254), range(20, 41), range(50, 54)
PERIOD17 = (2, 1, 255, 1, 2, 254, 3, 1, 1, 255, 0, 0, 0, 0, 5, 251, 2)   # 4097 = 17 * 241: a row's type byte, 2, is the period's first


@functools.lru_cache(maxsize=None)
def big_image():
    """4096x2049x1: 257 blocks of filtered rows.  A row takes its kind from the blocks its 4097 filtered bytes touch: random where one of
    BIG_STORED is among them (those blocks are random throughout, and stored); the row above plus PERIOD17 where one of BIG_PERIODIC is
    (the Up filter wins, the filtered stream repeats every 17 bytes: matches for the LZ77 kernel); the row above plus 2 where one of
    BIG_TWOS is (Up again: the filtered bytes and the type byte are all 2, a flat block); else zeros (filter None, a flat block of 0).
    The first row of a periodic or a twos region is random, so that Up beats None below it.  The adaptive filter puts a type byte every
    4097 bytes, so only constant blocks repeat exactly: the flat blocks are two contents, the others are a few dozen of their own."""
    rng = np.random.default_rng(4096)
    stride = BIG_W + 1
    img = np.zeros((BIG_H, BIG_W), np.uint8)
    add17 = np.array([PERIOD17[(1 + j) % 17] for j in range(BIG_W)], np.uint8)
    before = "Z"
    for r in range(BIG_H):
        touched = range(r * stride // BLOCK, ((r + 1) * stride - 1) // BLOCK + 1)
        kind = ("S" if any(b in BIG_STORED for b in touched) else "M" if any(b in BIG_PERIODIC for b in touched)
                else "T" if any(b in BIG_TWOS for b in touched) else "Z")
        if kind == "S" or (kind in "MT" and before != kind):
            img[r] = rng.integers(0, 256, BIG_W, dtype=np.uint8)
        elif kind == "M":
            img[r] = img[r - 1] + add17
        elif kind == "T":
            img[r] = img[r - 1] + np.uint8(2)
        before = kind
    return _frozen(img.reshape(BIG_H, BIG_W, 1))


def big_cases():
    kills = STREAM_MUTANTS
    a = Case("many_blocks/deflate_258", "many_blocks", "deflate", kills, data=big_stream(), stride=0,
             expect=dict(blocks=258, stored=[BIG_PATTERN[i % 8] == "S" for i in range(257)] + [True]))
    b = Case("many_blocks/png_4096x2049", "many_blocks", "png", kills, img=big_image(),
             expect=dict(blocks=257, stored_blocks=BIG_STORED, flat_blocks=tuple(BIG_TWOS)[2:-2]))
    a.big = b.big = True
    return [a, b]


# ---- families 6, 7, 8: EXR chunk layout, chunks of blocks, pack tiles ----------------------------------------------------------------------------
def _ramp(w, h, seed, noise=0.02):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    return (x / max(w - 1, 1) + 0.25 * y / max(h - 1, 1) + noise * rng.random((h, w))).astype(np.float32)


def _words(a):
    return _frozen(np.ascontiguousarray(a).reshape(-1).view(np.uint32).copy())


def _banded(w, h, seed, random_bands, flat=None):
    """(h, w) uint32 words in the film's layout (rows bottom-up) by file chunk: the chunks of `random_bands` are random bits, the others
    flat (one value per chunk) or, with flat = None, a noisy ramp in steps of 1 / 256 (the low mantissa bytes are zero: it compresses)"""
    rng = np.random.default_rng(seed)
    a = (np.round(_ramp(w, h, seed) * 256.0) / 256.0).astype(np.float32) if flat is None else np.zeros((h, w), np.float32)
    a = a.view(np.uint32)[::-1].copy()   # file order, top-down
    for c in range(E.n_chunks(h)):
        rows = slice(E.ROWS * c, min(E.ROWS * (c + 1), h))
        if c in random_bands:
            a[rows] = rng.integers(0, 1 << 32, a[rows].shape, dtype=np.uint64).astype(np.uint32)
        elif flat is not None:
            a[rows] = np.float32(flat + 0.5 * c).view(np.uint32)
    return _words(a[::-1])


def exr_layout_cases():
    out = []
    # 6: more than 256 chunks - k_exr_layout's per = ceil(chunks / 256) = 2
    rng = np.random.default_rng(257)
    raw = [bool(v) for v in rng.random(257) < 0.4]
    out.append(Case("many_chunks/64x4112_float", "many_chunks", "exr", (), w=64, h=4112, matches=(0, 1),
                    channels=[("Z", _banded(64, 4112, 6, {c for c in range(257) if raw[c]}, flat=1.0), 1, 0, E.FLOAT)],
                    expect=dict(chunks=257, raw=raw, chunk_bytes=4096)))
    out.append(Case("many_chunks/1x4097_half", "many_chunks", "exr", (), w=1, h=4097, matches=(0, 1),
                    channels=[("Y", _words(_ramp(1, 4097, 7)), 1, 0, E.HALF)], expect=dict(chunks=257, raw=[True] * 257, chunk_bytes=32)))
    # 7: chunks of two blocks, the last chunk shorter by a block: 513x40 FLOAT, chunks of 32768 + 64 bytes, the last of 8 rows, 16 416 bytes
    for name, band, raws in (("middle_raw", 1, [False, True, False]), ("first_raw", 0, [True, False, False])):
        out.append(Case("chunks_of_blocks/513x40_%s" % name, "chunks_of_blocks", "exr", ("E:last_chunk_full_blocks",), w=513, h=40, matches=(0, 1),
                        channels=[("Z", _banded(513, 40, 513 + band, {band}), 1, 0, E.FLOAT)],
                        expect=dict(chunks=3, raw=raws, blocks=5, chunk_bytes=32832, last_chunk_bytes=16416)))
    # 8: k_exr_pack's tiles of 4096 units.  300x17 HALF: 4800 units a chunk, two tiles; the last chunk has 300, its tile 1 has none.
    # 301x31: the last chunk has 4515, its tile 1 the odd 419.  101x33 HALF + FLOAT + UINT: 505 units a row, 8080 a chunk; unit 4096 is
    # unit 56 of row 8, in the HALF channel, and the row's FLOAT channel starts at unit 101: a channel boundary inside tile 1.
    out.append(Case("pack_tiles/300x17_half", "pack_tiles", "exr", (), w=300, h=17, matches=(0, 1), channels=[("Y", _words(_ramp(300, 17, 8)), 1, 0, E.HALF)],
                    expect=dict(chunks=2, units=[4800, 300])))
    out.append(Case("pack_tiles/301x31_half", "pack_tiles", "exr", (), w=301, h=31, matches=(0, 1), channels=[("Y", _words(_ramp(301, 31, 9)), 1, 0, E.HALF)],
                    expect=dict(chunks=2, units=[4816, 4515])))
    w, h = 101, 33
    rng = np.random.default_rng(101)
    ids = _frozen((np.mgrid[0:h, 0:w][1] // 7 + 1000 * (rng.random((h, w)) < 0.1)).astype(np.uint32).reshape(-1))
    out.append(Case("pack_tiles/101x33_mixed", "pack_tiles", "exr", (), w=w, h=h, matches=(0, 1),
                    channels=[("G", _words(_ramp(w, h, 10)), 1, 0, E.HALF), ("Z", _words(1.0 + 4.0 * _ramp(w, h, 11)), 1, 0, E.FLOAT), ("id", ids, 1, 0, E.UINT)],
                    expect=dict(chunks=3, units=[8080, 8080, 505])))
    return out


# ---- family 9: the ninth bit of an exit (LZ77) -----------------------------------------------------------------------------------------------------
# unique_bytes(k), 300 times the byte 126, the byte 127 (neither occurs in unique_bytes): the literal 126 at k, a match of 258 at distance 1
# from k + 1, one of 41, the literal 127.  The first match's exit - where it ends, from the end of the 128-byte span it starts in - is
# k + 259 - 128 for k < 127: 255, 256, 257.  For k = 127 and 128 the match starts in the next span.
EXITS = {124: 255, 125: 256, 126: 257, 127: 130, 128: 131}


def exit_block(k):
    return np.concatenate([KZ.unique_bytes(k), np.full(300, 126, np.uint8), np.array([127], np.uint8)])


def ends_at_block_end():
    """32 409 times 200, 100 unique bytes, 259 times 126: the last token is a match of 258 that ends at byte 32768"""
    return np.concatenate([np.full(32409, 200, np.uint8), KZ.unique_bytes(100), np.full(259, 126, np.uint8)])


def exit_cases():
    out = []
    for k, x in EXITS.items():
        tokens = [("lit", int(b)) for b in KZ.unique_bytes(k)] + [("lit", 126), ("match", 258, 1), ("match", 41, 1), ("lit", 127)]
        for stride in (0, 127):   # with rows of 127 the row above ties the run from k + 127 on; the run's distance 1 wins
            out.append(Case("exit/k%d_stride%d" % (k, stride), "exit", "deflate", ("Z:exit_bit8",) if x >= 256 else (), data=_frozen(exit_block(k)),
                            stride=stride, expect=dict(tokens=tokens, exit=x, stored=[False])))
    tokens = ([("lit", 200)] + [("match", 258, 1)] * 125 + [("match", 158, 1)] + [("lit", int(b)) for b in KZ.unique_bytes(100)]
              + [("lit", 126), ("match", 258, 1)])
    out.append(Case("exit/match_ends_at_32768", "exit", "deflate", (), data=_frozen(ends_at_block_end()), stride=0, expect=dict(tokens=tokens, stored=[False])))
    return out


# ---- the table, and what every entry should write ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    out = raw_tie_cases() + stored_tie_cases() + depth_cases() + big_cases() + exr_layout_cases() + exit_cases()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


def entries(c):
    """The entries a case goes through: "png", "png_lz", "deflate", "exr0", "exr1" """
    return {"png": ("png", "png_lz"), "deflate": ("deflate",), "exr": tuple("exr%d" % m for m in getattr(c, "matches", ()))}[c.kind]


@functools.lru_cache(maxsize=None)
def filtered(name):
    """The filtered stream of a "png" case"""
    return _frozen(P.filter_rows(case(name).img)[0])


@functools.lru_cache(maxsize=None)
def expected(name, entry, mutant=None):
    """The bytes the entry writes for the case (unpadded), by the restatements.  On a case of 257 blocks only None and the stream mutants
    are computed: its blocks come from the cache."""
    c = case(name)
    assert entry in entries(c) and (not c.big or mutant is None or mutant in STREAM_MUTANTS), (name, entry, mutant)
    if entry == "png":
        return P.encode_filtered(filtered(name), mutant, memo_encoder("P") if c.big else None)[0]
    if entry == "png_lz":
        stride = 1 + c.img.shape[1] * c.img.shape[2]
        return Z.encode_filtered(filtered(name), stride, mutant, memo_encoder("Z", stride) if c.big else None)[0]
    if entry == "deflate":
        return Z.encode_filtered(c.data, c.stride, mutant, memo_encoder("Z", c.stride) if c.big else None)[0]
    return E.encode(c.w, c.h, [(p, s, o, t) for _, p, s, o, t in c.channels], int(entry[3]), mutant)[0]
