"""The device JPEG encoder at its decision edges: named cases, each with a `claim` on the restatement (tests/jpeg_np.py), asserted when the
case is built, and `kills`, the mutants of jpeg_np.MUTANTS whose scan differs from the definition's on that case.  Two kinds:
  "image"  img (h, w, bpp) uint8, quality, subsampling, ri    through rayn_hip_jpeg_encode_device (the scan), rayn_hip_probe_jpeg_transform (the
                                                              coefficients) and rayn_hip_probe_jpeg_entropy on the restatement's coefficients
  "coef"   coef (blocks, 64) in zigzag and scan order, the    through rayn_hip_probe_jpeg_entropy with every byte of FILL_BYTES: coefficient
           geometry w, h, bpp, subsampling, ri                patterns no image produces on demand
A coefficient case's file is jpeg_np.frame at quality 100 (every Q = 1: the coefficients are the dequantised values, and all of them are
within a decoder's reach).  tests/jpeg_read.py reads every case's file back into the coefficients that went in.

Where an edge is found rather than built - quantiser ties, colours on a rounding edge - the search is a seeded or exhaustive walk that
runs when the case is built; it takes well under a second, and the claim says what it has to find.

ff_runs and a whole word of FF.  The Annex K codes do not allow one.  The longest code is 0xFFFE (16 bits, symbol 0xFA in both AC tables):
15 one bits and a zero.  Every code ends in a zero or is followed by its own value bits, and value bits are at most 11 (a DC difference of
2047) or 10 (an AC of 1023) ones.  So a run of ones is at most the 11 ones of a DC difference of 2047 and the 15 that open the code 0xFFFE
behind it - 26 bits, 25 between two AC coefficients - and the padding adds at most 7 to at most 10 value bits.  32 aligned ones never occur.
26 ones hold three aligned FF bytes: ff_runs has FF FF FF, the longest run there is, and says so in its claim.
TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this."""
import functools

import numpy as np

import jpeg_np as J

FILL_BYTES = (0x00, 0xFF, 0xA5)
NEW_MUTANTS = ("zrl_at_most_two", "tie_positive_toward_zero", "ties_toward_zero_above_q1", "chroma_offset_32768", "luma_truncates", "box_truncates",
               "pad_unstuffed", "stuff_one_per_word", "y_pred_from_y00", "first_mcu_resets_every_y", "cbcr_share_predictor")
OLD_MUTANTS = tuple(m for m in J.MUTANTS if m not in NEW_MUTANTS)   # jpeg_cases.MUTANTS
COMPONENTS = {(1, 0): [0], (3, 0): [0, 1, 2], (3, 1): [0, 0, 0, 0, 1, 2]}   # (bpp, subsampling) -> the components of an MCU's blocks


class Case:
    def __init__(self, name, kind, kills, claim, **fields):
        self.name, self.kind, self.kills, self.claim = name, kind, tuple(kills), claim
        self.__dict__.update(fields)
        if kind == "image":
            self.img = _frozen(self.img)
            self.height, self.width, self.bpp = self.img.shape
            self.ref = J.encode(self.img, self.quality, self.subsampling, self.ri)
        else:
            self.coef, self.quality = _frozen(np.asarray(self.coef, np.int16).reshape(-1, 64)), 100
            self.ref = self.encode_coef()
            self.ref.file = J.frame(self.width, self.height, self.bpp, 100, self.subsampling, self.ri, self.ref.scan)
        ok = claim(self.ref)
        assert ok is True or ok is np.True_, f"case {name} does not reach what it is for"

    def encode_coef(self, mutant=None):
        side = 16 if self.subsampling else 8
        per = COMPONENTS[(self.bpp, self.subsampling)]
        mcus = -(-self.width // side) * -(-self.height // side)
        assert len(self.coef) == mcus * len(per), (self.name, len(self.coef), mcus)
        return J.entropy(self.coef, np.tile(per, mcus), self.bpp, self.subsampling, self.ri, mutant)

    def mutant(self, m):
        return J.encode(self.img, self.quality, self.subsampling, self.ri, mutant=m) if self.kind == "image" else self.encode_coef(m)

    def __repr__(self):
        return self.name


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _noise(w, h, bpp, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, bpp), dtype=np.uint8)


def _block(dc=0, **ac):
    """One block: _block(5, k17=-3) has the DC 5 and -3 at zigzag position 17"""
    c = np.zeros(64, np.int64)
    c[0] = dc
    for k, v in ac.items():
        c[int(k[1:])] = v
    return c


def _grey(name, kills, claim, blocks, ri):
    """A grey strip, a block per MCU"""
    return Case(name, "coef", kills, claim, coef=np.array(blocks), width=8 * len(blocks), height=8, bpp=1, subsampling=0, ri=ri)


def _triple(name, kills, claim, blocks, ri):
    """The same strip in 4:4:4 with every block three times: Y, Cb and Cr, the last two through the chrominance tables"""
    return Case(name, "coef", kills, claim, coef=np.repeat(np.array(blocks), 3, axis=0), width=8 * len(blocks), height=8, bpp=3, subsampling=0, ri=ri)


# ---- transform: images ---------------------------------------------------------------------------------------------------------------------------
def transform_cases():
    out = []
    half = np.zeros((8, 8, 1), np.uint8)
    half[:, 4:] = 255
    out.append(Case("ac_size_10/grey_0_255", "image", ("row_truncates",), lambda e: int(e.coef[0][1]) == -924 and e.stats[0][1] == 10, img=half, quality=100, subsampling=0, ri=1))
    out.append(Case("ac_size_10/grey_255_0", "image", (), lambda e: int(e.coef[0][1]) == 924 and e.stats[0][1] == 10, img=half[:, ::-1], quality=100, subsampling=0, ri=1))
    red_cyan = np.zeros((8, 8, 3), np.uint8)
    red_cyan[:, :4, 0] = 255
    red_cyan[:, 4:, 1:] = 255
    out.append(Case("ac_size_10/red_cyan_444", "image", (), lambda e: e.stats[2][1] == 10 and abs(int(e.coef[2][1])) >= 512,
                    img=red_cyan, quality=100, subsampling=0, ri=1))
    for quality, kills in ((100, ("tie_positive_toward_zero", "ties_toward_zero")), (95, ("ties_toward_zero_above_q1", "tie_positive_toward_zero", "ties_toward_zero"))):
        img, claim = _tie_blocks(quality)
        out.append(Case("tie_signs/q%d" % quality, "image", kills, claim, img=img, quality=quality, subsampling=0, ri=2))
    img, claim = _colour_halves()
    out.append(Case("colour_halves", "image", ("chroma_offset_32768", "luma_truncates"), claim, img=img, quality=100, subsampling=0, ri=1))
    for (w, h), seed in (((16, 16), 31), ((1, 1), 32), ((17, 17), 33)):
        # (1, 1): every box is one replicated pixel, the sum 4 c and the remainder 0 - nothing to round, the box of the padding alone
        img = _noise(w, h, 3, seed)
        out.append(Case("box_remainders/%dx%d" % (w, h), "image", ("box_truncates",) if w > 1 else (), _box_claim(img), img=img, quality=100, subsampling=1, ri=1))
    return out


def _ties(F, Q):
    """Where |F| sits exactly between two multiples of Q 2^15"""
    return np.abs(F) % (Q * 32768) == Q * 16384


def _tie_blocks(quality):
    """From 20000 grey noise blocks of seed 77 the first with a positive tie at Q = 1 (quality 100), or the first with a positive and the
    first with a negative tie at Q > 1 (quality 95), beside a block that has none"""
    strip = _noise(8 * 20000, 8, 1, 77)
    F = J.transform(strip[..., 0].astype(np.int64))[0][0]
    Q = J.quant_table(quality, 0).reshape(8, 8)
    tie = _ties(F, Q) & ((Q == 1) if quality == 100 else (Q > 1))
    pos, neg = np.flatnonzero((tie & (F > 0)).any(axis=(1, 2))), np.flatnonzero((tie & (F < 0)).any(axis=(1, 2)))
    picks = [pos[0]] if quality == 100 else [pos[0], neg[0]]
    img = np.concatenate([strip[:, 8 * b:8 * b + 8] for b in picks + [0]], axis=1)

    def claim(e):
        F, Q = e.F[0][0], e.Q[0].reshape(8, 8)
        t = _ties(F, Q) & ((Q == 1) if quality == 100 else (Q > 1))
        want = [(0, 1)] if quality == 100 else [(0, 1), (1, -1)]
        return all(bool((t[b] & (np.sign(F[b]) == s)).any()) for b, s in want)
    return img, claim


def _colour_halves():
    """8x8 4:4:4.  Cb's sum before its shift is x + 8388608 + 32767 with x = -11059 R - 21709 G + 32768 B: + 32768 gives another Cb exactly
    where x is 32768 mod 65536, which is 32768 colours; likewise Cr with 32768 R - 27439 G - 5329 B.  Y's sum 19595 R + 38470 G + 7471 B is
    exactly 32768 mod 65536, the smallest that rounds up, at 274 colours.  The image takes 24, 24 and 16 of them, spread over each set."""
    v = np.arange(256, dtype=np.int64)
    R, G, B = np.meshgrid(v, v, v, indexing="ij")
    sets = [np.flatnonzero(((x % 65536) == 32768).reshape(-1)) for x in
            (-11059 * R - 21709 * G + 32768 * B, 32768 * R - 27439 * G - 5329 * B, 19595 * R + 38470 * G + 7471 * B)]
    counts = [len(s) for s in sets]
    picks = np.concatenate([s[np.linspace(0, len(s) - 1, n).astype(np.int64)] for s, n in zip(sets, (24, 24, 16))])
    img = np.stack([picks >> 16, (picks >> 8) & 255, picks & 255], -1).astype(np.uint8).reshape(8, 8, 3)

    def claim(e):
        moved = [int((a != b).sum()) for a, b in zip(J.planes(img, 0, "chroma_offset_32768"), e.planes)]
        low = int((J.planes(img, 0, "luma_truncates")[0] != e.planes[0]).sum())
        return counts == [32768, 32768, 274] and moved[0] == 0 and moved[1] >= 24 and moved[2] >= 24 and low >= 16
    return img, claim


def _box_claim(img):
    h, w, _ = img.shape

    def claim(e):
        full = J.planes(np.pad(img, ((0, -h % 16), (0, -w % 16), (0, 0)), mode="edge"), 0)
        rem = set()
        for p in full[1:]:
            rem |= set(((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]) % 4).reshape(-1).tolist())
        return e.mcus == (-(-w // 16)) ** 2 and (rem == {0} if w == 1 else rem == {0, 1, 2, 3})
    return claim


# ---- entropy: coefficients ---------------------------------------------------------------------------------------------------------------------------
LADDER = (15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63)


def _ladder_claim(e, step=1):
    stats = e.stats[::step]
    return [s[2] for s in stats] == [(k - 1) // 16 for k in LADDER] == [0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3] and [s[3] for s in stats] == [k < 63 for k in LADDER]


def _basis_image(k, sign):
    """128 + 127 basis function of zigzag position k, rounded: at quality 50 the one coefficient k"""
    v, u = divmod(int(J.ZIGZAG[k]), 8)
    x = np.arange(8)
    b = np.outer(np.cos((2 * x + 1) * v * np.pi / 16), np.cos((2 * x + 1) * u * np.pi / 16))
    return np.rint(128 + sign * 127 * b).astype(np.uint8)[..., None]


def zrl_cases():
    out = []
    for ri in (1, 65535):
        out.append(_grey("zrl_ladder/grey_ri%d" % ri, ("zrl_at_most_two", "eob_always"), _ladder_claim, [_block(**{"k%d" % k: 1 - 2 * (k & 1)}) for k in LADDER], ri))
    out.append(_triple("zrl_ladder/444", ("zrl_at_most_two",), lambda e: _ladder_claim(e, 3) and _ladder_claim(type("", (), {"stats": e.stats[2:]}), 3),
                       [_block(**{"k%d" % k: -5}) for k in LADDER], 4))
    img = np.concatenate([_basis_image(k, s) for k in (49, 62, 63) for s in (1, -1)], axis=1)
    out.append(Case("zrl_ladder/basis_images", "image", ("zrl_at_most_two",),
                    lambda e: all(np.flatnonzero(e.coef[b][1:]).tolist() == [k - 1] and e.stats[b][2] == 3 and e.stats[b][3] == (k < 63)
                                  for b, k in enumerate((49, 49, 62, 62, 63, 63))), img=img, quality=50, subsampling=0, ri=4))
    return out


def _dc_walk(diffs):
    """DC values whose successive differences hold every one of `diffs`, inside [-1024, 1023]: a block that moves the predictor to where
    the difference fits, then the block with the difference"""
    out = []
    for d in diffs:
        p = (-1024 if d >= 1024 else 1023 if d <= -1024 else 300 if d == 0 else 0)
        out += [p, p + d]
    return out


def category_cases():
    edges = sorted({s * v for k in range(11) for v in ((1 << k) - 1, 1 << k) for s in (1, -1)} | {2047, -2047})
    dcs = _dc_walk(edges)
    acs = sorted({s * v for k in range(1, 11) for v in ((1 << k) - 1, 1 << (k - 1)) for s in (1, -1)})
    assert max(acs) == 1023 and 512 in acs and 0 not in acs and min(dcs) == -1024 and max(dcs) == 1023
    blocks = [_block(d) for d in dcs] + [_block(0, **{k: v}) for v in acs for k in ("k1", "k16")]

    def claim(e, step=1):
        c = e.coef[::step].astype(np.int64)
        d = np.diff(np.concatenate([[0], c[:, 0]]))
        runs = {(int(v), k) for row in c for k in (1, 16) for v in [row[k]] if v}
        return (set(edges) <= set(d.tolist()) and {s[0] for s in e.stats[::step]} == set(range(12)) and bool(((d == 0) & (c[:, 0] == 300)).any())
                and runs == {(v, k) for v in acs for k in (1, 16)} and {s[1] for s in e.stats} == set(range(11)))
    return [_grey("category_edges/grey", (), claim, blocks, 65535), _triple("category_edges/444", (), lambda e: claim(e, 3), blocks, 65535)]


def _size10_16bit_symbols(ident):
    return [sym for sym, (_, n) in J.codes(1, ident).items() if n == 16 and sym & 15 == 10]


def bit_phase_cases():
    """[a block of 32 bits - DC difference 0 (2 bits), the 26-bit code of run 1, size 10 at position 2, EOB (4) - and one of 9 bits - DC
    difference +-2 (5), EOB] 32 times: the 26-bit put starts at bit 2 + 41 i, which is every phase of a word once"""
    assert 0x1A in _size10_16bit_symbols(0) and J.codes(0, 0)[0][1] == 2 and J.codes(0, 0)[2][1] == 3 and J.codes(1, 0)[0][1] == 4
    blocks, dc = [], 0
    for i in range(32):
        blocks.append(_block(dc, k2=(-1) ** i * (512 + 13 * i)))
        dc = 2 - dc
        blocks.append(_block(dc))

    def claim(e):
        long = [at for _, at, n in e.puts if n == 26]
        inside = [b for b in range(1, len(e.block_bits) - 1) for _, a, z in [e.block_bits[b]] if a >> 5 == (z - 1) >> 5 and a & 31 and z & 31]
        return (max(n for _, _, n in e.puts) == 26 and {at & 31 for at in long} == set(range(32)) and any((at + 26) & 31 == 0 for at in long)
                and any(at & 31 == 31 for at in long) and bool(inside) and any(a & 31 == 0 for _, a, _ in e.block_bits[1:]))
    return [_grey("bit_phases", (), claim, blocks, 65535)]


def _bits_of(block):
    return J.entropy(np.array([block]), [0], 1, 0, 1).segment_bits[0]


@functools.lru_cache(None)
def _blocks_by_residue():
    """{bits mod 32: a block of that many bits as a segment of its own}, the first found in a fixed walk over a DC value, a value at
    position 1 and whether position 63 is set (no EOB)"""
    found = {}
    for dc in (0, 1, 2, 5, 9, 17, 33, 65, 129, 257, 513, 1023):
        for a in (0, 1, 2, 4, 8, 16, 32, 64, 128, 256, 512):
            for last in (0, 1, 7):
                b = _block(dc, k1=a, k63=last)
                found.setdefault(_bits_of(b) % 32, b)
    return found


def pad_cases():
    residues = (0, 8, 16, 24, 25, 26, 27, 28, 29, 30, 31)
    by = _blocks_by_residue()
    blocks = [by[r] for r in residues]
    # DC 0 (2 bits), three ZRLs and the code of run 14, size 10 (33), ten 1 bits: 61 bits; the five value bits in the last byte and three
    # padding bits make an FF
    made = _block(0, k63=1023)

    def claim(e):
        return [n % 32 for n in e.segment_bits[:len(residues)]] == list(residues) and e.segment_bits[-1] == 61 and e.raw_segments[-1][-1] == 0xFF \
            and e.scan.endswith(b"\xff\x00") and e.pad_bits == 3
    return [_grey("pad_edges", ("pad_zero", "pad_unstuffed"), claim, blocks + [made], 1)]


def _ff_pairs(raw):
    """the indices i with raw[i] == raw[i + 1] == FF"""
    a = np.frombuffer(raw, np.uint8)
    return np.flatnonzero((a[:-1] == 255) & (a[1:] == 255))


def ff_cases():
    """A block whose positions 1, 17, 33 and 49 hold 1023: behind the first, three times ten 1 bits and the code 0xFFFE of run 15, size 10 -
    25 ones.  With a 9-bit block behind it, 119 bits: a hundred pairs put those runs at every bit phase of a word and of a thread's two
    words.  The short case starts with the DC difference 2047 (11 ones) in front of 0xFFFE: 26 ones, the longest run there is."""
    assert J.codes(1, 0)[0xFA] == (0xFFFE, 16) and J.codes(1, 1)[0xFA] == (0xFFFE, 16)
    blocks, dc = [], 0
    for i in range(100):
        blocks.append(_block(dc, k1=1023, k17=1023, k33=1023, k49=1023))
        dc = 2 - dc
        blocks.append(_block(dc))

    def long_claim(e):
        raw = e.raw_segments[0]
        i = _ff_pairs(raw)
        words = -(-len(raw) // 4)
        return (e.segments == 1 and 256 < words <= 512 and -(-words // 2) < 256 and {int(v) for v in i % 8} == set(range(8))
                and b"\xff\x00\xff\x00" in e.scan)

    def short_claim(e):   # three FF in a row, the longest run, over the end of a word
        raw = e.raw_segments[0]
        return b"\xff\xff\xff" in raw and b"\xff\xff\xff\xff" not in raw and 3 in _ff_pairs(raw) % 4 and b"\xff\x00\xff\x00\xff\x00" in e.scan
    # the DC -1024 and then 1023: the difference 2047.  The first block's position 1 and 63 move the 26 ones to where they fill three bytes
    short = next(blocks for a in (0, 1, 2, 4, 8, 16, 32, 64, 128, 256, 512) for last in (0, 1, 7)
                 for blocks in [[_block(-1024, k1=a, k63=last), _block(1023, k16=-1023), _block(1023)]]
                 if short_claim(J.entropy(np.array(blocks), [0] * 3, 1, 0, 65535)))
    return [_grey("ff_runs/two_words_per_thread", ("stuff_one_per_word",), long_claim, blocks, 65535),
            _grey("ff_runs/three_in_a_row", ("stuff_one_per_word",), short_claim, short, 65535),
            _triple("ff_runs/three_in_a_row_444", ("stuff_one_per_word",), lambda e: any(len(_ff_pairs(r)) for r in e.raw_segments), short, 1)]


def predictor_cases():
    """Four 4:2:0 MCUs at Ri 2: every block has a DC of its own, so every other choice of predictor block gives other bits"""
    dc = np.random.default_rng(420).permutation(np.arange(-1000, 1000, 7))[:24]
    blocks = [_block(int(d)) for d in dc]
    kills = ("y_pred_from_y00", "first_mcu_resets_every_y", "cbcr_share_predictor", "predictor_kept")
    return [Case("predictor_420", "coef", kills, lambda e: e.segments == 2 and e.mcus == 4 and len(set(e.coef[:, 0].tolist())) == 24,
                 coef=np.array(blocks), width=64, height=16, bpp=3, subsampling=1, ri=2)]


# ---- layout and compaction ---------------------------------------------------------------------------------------------------------------------------
def _sparse_blocks(n, seed):
    """n blocks of a few random coefficients each: segments of unequal sizes"""
    rng = np.random.default_rng(seed)
    c = np.zeros((n, 64), np.int64)
    c[:, 0] = rng.integers(-200, 200, n)
    for b in range(n):
        k = rng.integers(0, 6)
        c[b, rng.integers(1, 64, k)] = rng.integers(-40, 41, k)
    return c


def _marker_offsets(e):
    at, out = 0, []
    for s in e.segment_bytes[:-1]:
        at += len(s) + 2
        out.append(at - 2)
    return out


def layout_cases():
    out = []
    for w in (64, 2056):
        n = w // 8
        want = b"".join(b"\x2b" + bytes([0xFF, 0xD0 + k % 8]) for k in range(n))[:-2]
        out.append(Case("one_byte_segments/%d" % n, "image", (), lambda e, n=n, want=want: e.segments == n and e.scan == want and want[:6] == bytes.fromhex("2bffd02bffd1"),
                        img=np.full((8, w, 1), 128, np.uint8), quality=75, subsampling=0, ri=1))
    for n in (8, 9, 16, 17, 256, 512, 513):
        kills = ("marker_unwrapped",) if n > 9 else ()
        out.append(_grey("segment_counts/%d" % n, kills, lambda e, n=n: e.segments == n and len({len(s) for s in e.segment_bytes}) >= 3, _sparse_blocks(n, 1000 + n), 1))
    # scan lengths 3 n - 2 of n one-byte segments, and of unequal segments found below: every residue modulo 4, and output words that
    # begin on a marker's first byte (its offset is 0 modulo 4) and on its second (its offset is 3 modulo 4)
    for n in (1, 2, 3, 4):
        out.append(_grey("scan_residues/one_byte_x%d" % n, (), lambda e, n=n: len(e.scan) == 3 * n - 2 and len(e.scan) % 4 == (3 * n - 2) % 4, [_block(0)] * n, 1))
    seen = set()
    for seed in range(200):
        c = _sparse_blocks(5, 5000 + seed)
        e = J.entropy(c, [0] * 5, 1, 0, 1)
        r, first, second = len(e.scan) % 4, any(o % 4 == 0 for o in _marker_offsets(e)), any(o % 4 == 3 for o in _marker_offsets(e))
        if r not in seen and first and second:
            seen.add(r)
            out.append(_grey("scan_residues/five_segments_%dmod4" % r, (), lambda e, r=r: len(e.scan) % 4 == r and {o % 4 for o in _marker_offsets(e)} >= {0, 3}, c, 1))
        if len(seen) == 4:
            break
    assert len(seen) == 4
    return out


# ---- state: what the device test encodes twice into the same buffers -------------------------------------------------------------------------------------
def stale_pair():
    """(a large noisy image, a small flat one), both 4:4:4 at the same quality: encoded one after the other into one output and one scratch
    that are never refilled, in both orders"""
    big = Case("stale_buffers/noise_96x64", "image", (), lambda e: len(e.scan) > 96 * 64 * 3, img=_noise(96, 64, 3, 808), quality=100, subsampling=0, ri=5)
    small = Case("stale_buffers/flat_24x16", "image", (), lambda e: len(e.scan) < 100, img=np.full((16, 24, 3), 90, np.uint8), quality=100, subsampling=0, ri=5)
    return big, small


@functools.lru_cache(None)
def cases():
    out = transform_cases() + zrl_cases() + category_cases() + bit_phase_cases() + pad_cases() + ff_cases() + predictor_cases() + layout_cases() + list(stale_pair())
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


NAMES = [c.name for c in cases()]
IMAGE_NAMES = [c.name for c in cases() if c.kind == "image"]
COEF_NAMES = [c.name for c in cases() if c.kind == "coef"]


@functools.lru_cache(None)
def kill_matrix():
    """{mutant: [names of the cases whose scan it changes]} over every mutant of jpeg_np.MUTANTS"""
    return {m: [c.name for c in cases() if c.mutant(m).scan != c.ref.scan] for m in J.MUTANTS}
