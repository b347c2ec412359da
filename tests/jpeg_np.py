"""The baseline JPEG encoder of include/rayn_hip.h ("Baseline JPEG scans on the device"), restated with numpy and plain Python from the
definition alone: it shares no code with the library.  Its tables do not come from the library either: they are read out of a file
libjpeg wrote (Pillow, quality 50: scale 100, so the DQT segments hold the Annex K base tables, and the DHT segments the Annex K codes).

encode(img, quality, subsampling, ri) returns an Encoded: the quantised coefficients in scan order, the scan with its markers, what the
device entry writes (header words + scan, zero-padded to a word) and the file.  It is its two halves one after the other, as the
library's launch is: coefficients(img, quality, subsampling) and entropy(coef, comp, bpp, subsampling, ri), which takes any coefficients
in scan order (rayn_hip_probe_jpeg_transform and rayn_hip_probe_jpeg_entropy run the same halves on the device).  `mutant` plants one
wrong reading of the definition (tests/jpeg_cases.py and tests/jpeg_edge_cases.py show that the cases tell each from the real thing)."""
import functools
import io
import struct

import numpy as np

MUTANTS = ("row_truncates", "ties_toward_zero", "predictor_kept", "marker_unwrapped", "eob_always", "pad_zero",
           # the readings tests/jpeg_edge_cases.py tells from the definition
           "zrl_at_most_two",            # a run of 48 or more gets two ZRL codes, and the run code what is left modulo 16
           "tie_positive_toward_zero",   # the quantiser rounds a positive tie down
           "ties_toward_zero_above_q1",  # the quantiser rounds ties down wherever Q > 1
           "chroma_offset_32768",        # Cb and Cr round with + 32768 as Y does
           "luma_truncates",             # Y without its + 32768
           "box_truncates",              # the 4:2:0 box without its + 2
           "pad_unstuffed",              # an FF that the padding completes gets no 00
           "stuff_one_per_word",         # at most one 00 per four bytes of a segment
           "y_pred_from_y00",            # 4:2:0: Y00 is predicted from the previous MCU's Y00, not its Y11
           "first_mcu_resets_every_y",   # 4:2:0: all four Y blocks of a segment's first MCU have the predictor 0
           "cbcr_share_predictor")       # Cb and Cr share one predictor

K = [4096, 4017, 3784, 3406, 2896, 2276, 1567, 799]


def _transform_matrix():
    T = np.zeros((8, 8), np.int64)
    for u in range(8):
        for x in range(8):
            if u == 0:
                T[u, x] = 2896
                continue
            c = np.cos((2 * x + 1) * u * np.pi / 16)
            k = int(round(np.arccos(abs(c)) * 16 / np.pi))
            assert abs(abs(c) - np.cos(k * np.pi / 16)) < 1e-12
            T[u, x] = K[k] if c > 0 else -K[k]
    assert list(T[1]) == [4017, 3406, 2276, 799, -799, -2276, -3406, -4017] and list(T[2]) == [3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784]
    return T


T = _transform_matrix()


def _zigzag():
    order, v, u, up = [], 0, 0, True
    for _ in range(64):  # the walk of T.81 figure 5: along the anti-diagonals, turning at the edges
        order.append(v * 8 + u)
        if up:
            if u == 7:
                v, up = v + 1, False
            elif v == 0:
                u, up = u + 1, False
            else:
                v, u = v - 1, u + 1
        else:
            if v == 7:
                u, up = u + 1, True
            elif u == 0:
                v, up = v + 1, True
            else:
                v, u = v + 1, u - 1
    return np.array(order)


ZIGZAG = _zigzag()  # ZIGZAG[k]: the row-major index of zigzag position k


def segments_of(data):
    """[(marker, payload)] of a JPEG file up to and including SOS"""
    out, i = [], 2
    assert data[:2] == b"\xff\xd8"
    while True:
        assert data[i] == 0xFF, i
        m, n = data[i + 1], struct.unpack(">H", data[i + 2:i + 4])[0]
        out.append((m, bytes(data[i + 4:i + 2 + n])))
        i += 2 + n
        if m == 0xDA:
            return out, i


@functools.lru_cache(None)
def tables():
    """(base quantisation tables [2] of 64 in row-major order, {(class, id): (bits[16], vals)}) read from a file Pillow saved at quality 50"""
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray((np.arange(32 * 32 * 3) % 251).astype(np.uint8).reshape(32, 32, 3)).save(b, "JPEG", quality=50)
    quant, huff = {}, {}
    for m, seg in segments_of(b.getvalue())[0]:
        p = 0
        while m == 0xDB and p < len(seg):
            assert seg[p] >> 4 == 0
            nat = np.zeros(64, np.int64)
            nat[ZIGZAG] = list(seg[p + 1:p + 65])
            quant[seg[p] & 15] = nat
            p += 65
        while m == 0xC4 and p < len(seg):
            bits = list(seg[p + 1:p + 17])
            huff[(seg[p] >> 4, seg[p] & 15)] = (bits, list(seg[p + 17:p + 17 + sum(bits)]))
            p += 17 + sum(bits)
    assert sorted(quant) == [0, 1] and sorted(huff) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    return [quant[0], quant[1]], huff


def quant_table(quality, which):
    """row-major"""
    assert 1 <= quality <= 100
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((tables()[0][which] * scale + 50) // 100, 1, 255)


@functools.lru_cache(None)
def codes(cls, ident):
    """{symbol: (code, length)}: the canonical code of T.81 Annex C"""
    bits, vals = tables()[1][(cls, ident)]
    out, code, at = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[at]] = (code, length)
            code, at = code + 1, at + 1
        code <<= 1
    return out


def planes(img, subsampling, mutant=None):
    """The component planes, padded to whole MCUs: [Y] or [Y, Cb, Cr] as int64, chroma at half size in 4:2:0"""
    img = np.asarray(img, np.uint8)
    h, w, bpp = img.shape
    assert bpp in (1, 3) and subsampling in (0, 1) and not (subsampling and bpp == 1)
    side = 16 if subsampling else 8
    img = np.pad(img, ((0, -h % side), (0, -w % side), (0, 0)), mode="edge").astype(np.int64)
    if bpp == 1:
        return [img[..., 0]]
    R, G, B = img[..., 0], img[..., 1], img[..., 2]
    half = 32768 if mutant == "chroma_offset_32768" else 32767
    out = [(19595 * R + 38470 * G + 7471 * B + (0 if mutant == "luma_truncates" else 32768)) >> 16,
           (-11059 * R - 21709 * G + 32768 * B + 8388608 + half) >> 16, (32768 * R - 27439 * G - 5329 * B + 8388608 + half) >> 16]
    assert mutant == "chroma_offset_32768" or all(0 <= p.min() and p.max() <= 255 for p in out)
    if subsampling:
        bias = 0 if mutant == "box_truncates" else 2
        out[1:] = [(p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2 for p in out[1:]]
    return out


def transform(plane, mutant=None):
    """(F, S): F[by, bx, v, u] the coefficients times 2^15 of the plane's 8x8 blocks, S[by, bx, y, u] the row sums in front of their shift"""
    H, W = plane.shape
    s = plane.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3) - 128
    S = np.einsum("ux,abyx->abyu", T, s)
    if mutant == "row_truncates":
        a = np.sign(S + 1024) * (np.abs(S + 1024) >> 11)
    else:
        a = (S + 1024) >> 11
    assert np.abs(a).max() <= 1448
    F = np.einsum("vy,abyu->abvu", T, a)
    assert np.abs(F).max() < 2 ** 25
    return F, S


def quantise(F, Q, mutant=None):
    """the quantised coefficients of F[..., v, u] in zigzag order: [..., 64]"""
    Q = Q.reshape(8, 8)
    down = {"ties_toward_zero": 1, "tie_positive_toward_zero": F > 0, "ties_toward_zero_above_q1": Q > 1}.get(mutant, 0)
    m = (np.abs(F) + Q * 16384 - down) // (Q * 32768)
    return (np.sign(F) * m).reshape(F.shape[:-2] + (64,))[..., ZIGZAG]


def block_order(comps, subsampling):
    """The blocks in the order of the scan: (n, 64) coefficients and (n,) component indices, from per-component [by, bx, 64] arrays"""
    if subsampling == 0:
        by, bx = comps[0].shape[:2]
        coef = np.stack(comps, axis=2).reshape(by * bx * len(comps), 64)
        return coef, np.tile(np.arange(len(comps)), by * bx)
    Y, Cb, Cr = comps
    my, mx = Cb.shape[:2]
    Yb = Y.reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, 4, 64)  # Y00 Y01 Y10 Y11: Y01 is the right neighbour
    coef = np.concatenate([Yb, Cb[:, :, None], Cr[:, :, None]], axis=2).reshape(my * mx * 6, 64)
    return coef, np.tile(np.array([0, 0, 0, 0, 1, 2]), my * mx)


class Bits:
    """bits, most significant first, into bytes"""

    def __init__(self):
        self.out, self.acc, self.n, self.total, self.log = bytearray(), 0, 0, 0, []

    def put(self, v, n):
        assert 0 <= v < (1 << n)
        self.total += n
        self.acc, self.n = (self.acc << n) | v, self.n + n
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 255)
        self.acc &= (1 << self.n) - 1

    def pad(self, ones=True):
        if self.n:
            k = 8 - self.n
            self.put((1 << k) - 1 if ones else 0, k)


def _value_bits(v):
    s = int(abs(v)).bit_length()
    return s, (v if v >= 0 else v + (1 << s) - 1)


def encode_block(bw, c, pred, dc, ac, mutant=None):
    """one block's codes; returns (DC category, largest AC size, ZRLs written, whether an EOB was written)"""
    s, v = _value_bits(int(c[0]) - pred)
    assert s <= 11, "DC category beyond the table"
    bw.log.append((bw.total, dc[s][1] + s))  # the kernels put a code and its value bits at once: (where, how many bits)
    bw.put(*dc[s])
    if s:
        bw.put(v, s)
    run, zrl, big = 0, 0, 0
    for k in range(1, 64):
        x = int(c[k])
        if x == 0:
            run += 1
            continue
        while run >= 16 and not (mutant == "zrl_at_most_two" and zrl == 2):
            bw.log.append((bw.total, ac[0xF0][1]))
            bw.put(*ac[0xF0])
            run, zrl = run - 16, zrl + 1
        run &= 15
        s2, v2 = _value_bits(x)
        assert s2 <= 10, "AC size beyond the table"
        big = max(big, s2)
        bw.log.append((bw.total, ac[(run << 4) | s2][1] + s2))
        bw.put(*ac[(run << 4) | s2])
        bw.put(v2, s2)
        run = 0
    eob = run > 0 or mutant == "eob_always"
    if eob:
        bw.log.append((bw.total, ac[0x00][1]))
        bw.put(*ac[0x00])
    return s, big, zrl, eob


class Encoded:
    pass


def _stuff(raw, padded, mutant):
    """The segment's bytes with 00 behind every FF; padded: the padding wrote bits into the last byte"""
    out = bytearray()
    for k, b in enumerate(raw):
        out.append(b)
        if b == 0xFF:
            if mutant == "pad_unstuffed" and padded and k == len(raw) - 1:
                continue
            if mutant == "stuff_one_per_word" and 0xFF in raw[k & ~3:k]:
                continue
            out.append(0)
    return bytes(out)


def entropy(coef, comp, bpp, subsampling, ri, mutant=None, e=None):
    """The entropy-coded half: coef (blocks, 64) in zigzag and scan order and comp (blocks,), the component of every block, to the scan.
    Fills an Encoded: scan, header, encoded, segment_bytes (stuffed) and raw_segments (not), stats per block, and what the bit-level cases
    are about - block_bits [(segment, first bit, bit behind the last)] and puts [(segment, bit, count)] in the segment's unstuffed bits"""
    coef = np.asarray(coef)
    assert coef.ndim == 2 and coef.shape[1] == 64 and len(comp) == len(coef) and 1 <= ri <= 65535
    e = Encoded() if e is None else e
    bpm = {1: 1, 3: 6 if subsampling else 3}[bpp]
    assert len(coef) % bpm == 0
    total = len(coef) // bpm
    e.bpp, e.subsampling, e.ri = bpp, subsampling, ri
    e.coef, e.block_comp = coef.astype(np.int16), np.asarray(comp)
    assert (e.coef == coef).all()
    e.mcus, e.blocks, e.segments = total, len(coef), -(-total // ri)
    scan, e.segment_bytes, e.raw_segments, e.stats, e.block_bits, e.puts, e.segment_bits = bytearray(), [], [], [], [], [], []
    for k in range(e.segments):
        bw = Bits()
        if not (mutant == "predictor_kept" and k):
            pred = [0, 0, 0]
        first = k * ri * bpm
        for b in range(first, min((k + 1) * ri, total) * bpm):
            c, j, at = int(comp[b]), b % bpm, bw.total
            p = pred[c]
            if subsampling and c == 0:
                if mutant == "y_pred_from_y00" and j == 0 and b - first >= bpm:
                    p = int(coef[b - bpm][0])
                if mutant == "first_mcu_resets_every_y" and b - first < bpm:
                    p = 0
            if mutant == "cbcr_share_predictor" and c:
                p = pred[1]
            e.stats.append(encode_block(bw, coef[b], p, codes(0, 1 if c else 0), codes(1, 1 if c else 0), mutant))
            pred[1 if (mutant == "cbcr_share_predictor" and c) else c] = int(coef[b][0])
            e.block_bits.append((k, at, bw.total))
        e.puts += [(k, at, n) for at, n in bw.log]
        e.segment_bits.append(bw.total)
        e.pad_bits = (8 - bw.n) % 8  # of the last segment, in the end
        bw.pad(ones=mutant != "pad_zero")
        raw = bytes(bw.out)
        seg = _stuff(raw, e.pad_bits > 0, mutant)
        e.raw_segments.append(raw)
        e.segment_bytes.append(seg)
        scan += seg
        if k + 1 < e.segments:
            scan += bytes([0xFF, (0xD0 + k) & 255 if mutant == "marker_unwrapped" else 0xD0 + k % 8])
    e.scan = bytes(scan)
    e.header = (len(e.scan), e.segments, ri, e.blocks)
    e.encoded = struct.pack("<4I", *e.header) + e.scan + b"\0" * (-len(e.scan) % 4)
    return e


def coefficients(img, quality, subsampling, mutant=None, e=None):
    """The transform half: the image to the quantised coefficients in scan order (e.coef, e.block_comp), with what led there"""
    img = np.asarray(img, np.uint8)
    h, w, bpp = img.shape
    e = Encoded() if e is None else e
    e.width, e.height, e.bpp, e.quality, e.subsampling = w, h, bpp, quality, subsampling
    e.planes = planes(img, subsampling, mutant)
    e.Q = [quant_table(quality, 0 if i == 0 else 1) for i in range(len(e.planes))]
    e.F, e.S = zip(*[transform(p, mutant) for p in e.planes])
    e.comp_coef = [quantise(F, Q, mutant) for F, Q in zip(e.F, e.Q)]
    coef, comp = block_order(e.comp_coef, subsampling)
    e.coef, e.block_comp = coef.astype(np.int16), comp
    assert (e.coef == coef).all()
    return e


def encode(img, quality, subsampling, ri, mutant=None):
    e = coefficients(img, quality, subsampling, mutant)
    entropy(e.coef, e.block_comp, e.bpp, subsampling, ri, mutant, e)
    e.file = frame(e.width, e.height, e.bpp, quality, subsampling, ri, e.scan)
    return e


def _segment(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


def frame(w, h, bpp, quality, subsampling, ri, scan):
    """SOI, APP0 JFIF 1.1, DQT (one segment per table), SOF0, DHT (one segment per table: DC 0, AC 0, DC 1, AC 1), DRI, SOS, the scan, EOI"""
    n = 1 if bpp == 1 else 3
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t in range(2 if n == 3 else 1):
        out += _segment(0xDB, bytes([t]) + bytes(int(v) for v in quant_table(quality, t)[ZIGZAG]))
    sof = struct.pack(">BHHB", 8, h, w, n)
    for i in range(n):
        sof += bytes([i + 1, 0x22 if (subsampling and i == 0) else 0x11, 1 if i else 0])
    out += _segment(0xC0, sof)
    for ident in range(2 if n == 3 else 1):
        for cls in (0, 1):
            bits, vals = tables()[1][(cls, ident)]
            out += _segment(0xC4, bytes([(cls << 4) | ident]) + bytes(bits) + bytes(vals))
    out += _segment(0xDD, struct.pack(">H", ri))
    sos = bytes([n])
    for i in range(n):
        sos += bytes([i + 1, 0x11 if i else 0x00])
    out += _segment(0xDA, sos + bytes([0, 63, 0]))
    return out + bytes(scan) + b"\xff\xd9"


def reconstruct(e):
    """What a float64 decoder makes of the coefficients: per component the plane at its own resolution (padded size): dequantise, the
    orthonormal inverse DCT, + 128, round, clamp"""
    from scipy.fft import idctn
    out = []
    for c, Q in zip(e.comp_coef, e.Q):
        nat = np.zeros(c.shape, np.float64)
        nat[..., ZIGZAG] = c
        blocks = (nat * Q).reshape(c.shape[:2] + (8, 8))
        px = idctn(blocks, axes=(2, 3), norm="ortho") + 128.0
        by, bx = c.shape[:2]
        out.append(np.clip(np.rint(px), 0, 255).transpose(0, 2, 1, 3).reshape(by * 8, bx * 8))
    return out
