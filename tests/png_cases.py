"""Inputs of the PNG encoder's tests (tests/test_png.py on the restatement, tests/test_png_device.py on the kernels): blocks that sit on
the edges of the token rule and of the length limit, and small images of the content families a renderer writes.  TEST INFRASTRUCTURE."""
import struct
import zlib

import numpy as np

import png_np as P

RUN_LENGTHS = (1, 2, 3, 4, 258, 259, 260, 261, 262, 517, 32768)


def expected_run_tokens(n):
    """The token kinds and lengths the rule gives a run of n equal bytes, written out by hand: ("lit",) or ("match", length)"""
    return {1: [("lit",)], 2: [("lit",)] * 2, 3: [("lit",)] * 3, 4: [("lit",), ("match", 3)], 258: [("lit",), ("match", 257)],
            259: [("lit",), ("match", 258)], 260: [("lit",), ("match", 258), ("lit",)], 261: [("lit",), ("match", 258), ("lit",), ("lit",)],
            262: [("lit",), ("match", 258), ("match", 3)], 517: [("lit",), ("match", 258), ("match", 258)],
            32768: [("lit",)] + [("match", 258)] * 127 + [("lit",)]}[n]  # 32767 = 127 * 258 + 1


def run_block(n, value=7):
    return np.full(n, value, np.uint8)


def run_edges_bytes():
    """Every run length of RUN_LENGTHS but the block-sized one, one after the other with changing values, framed by single bytes"""
    parts = [np.array([200], np.uint8)]
    for k, n in enumerate(RUN_LENGTHS[:-1]):
        parts.append(np.full(n, 10 + k, np.uint8))
    parts.append(np.array([201], np.uint8))
    return np.concatenate(parts)


def three_symbol_block():
    """One literal, one length code and end-of-block: a run of 1 + 258 * 20 bytes"""
    return np.full(1 + 258 * 20, 0, np.uint8)


# 18 symbols with the counts F1..F18: end-of-block, which counts 1, is F1; these are the 17 literals' F2..F18 (6763 bytes)
FIBONACCI = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584)
# the values by falling count: small |int8| for the frequent ones, signs alternating, so that on a single row no filter beats None
FIBONACCI_VALUES = (0, 1, 255, 2, 254, 3, 253, 4, 252, 5, 251, 6, 250, 7, 249, 8, 248)


def fibonacci_bytes():
    """6763 bytes whose 17 values have the counts F2..F18 and of which no two neighbours are equal (so every byte is a literal): with
    end-of-block 18 symbols 1, 1, 2, 3, 5, ..., 2584, the frequencies that drive a Huffman tree deepest - depth 17"""
    left = dict(zip(FIBONACCI_VALUES, sorted(FIBONACCI, reverse=True)))
    out, prev = [], None
    for _ in range(sum(FIBONACCI)):
        v = max((k for k in left if k != prev and left[k]), key=lambda k: (left[k], -FIBONACCI_VALUES.index(k)))
        out.append(v)
        left[v] -= 1
        prev = v
    return np.array(out, np.uint8)


def rows_of(data, w, bpp, fill=0):
    """The bytes laid into rows of a (h, w, bpp) image, the last row filled up"""
    row = w * bpp
    h = -(-len(data) // row)
    img = np.full(h * row, fill, np.uint8)
    img[:len(data)] = data
    return img.reshape(h, w, bpp)


# ---- content families ---------------------------------------------------------------------------------------------------------------------

FAMILIES = ("random", "zero", "mask", "gradient")


def family_image(family, w, h, bpp, seed=0):
    rng = np.random.default_rng(1000 + seed)
    if family == "random":   # nothing to gain: every block takes the stored path
        return rng.integers(0, 256, (h, w, bpp), dtype=np.uint8)
    if family == "zero":
        return np.zeros((h, w, bpp), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    if family == "mask":     # flat regions with a few edges, as an Alpha channel has
        m = ((xx - 0.4 * w) ** 2 + (yy - 0.5 * h) ** 2 < (0.3 * max(w, h)) ** 2) | (xx + 2 * yy < 0.2 * (w + h))
        return np.repeat((m * 255).astype(np.uint8)[..., None], bpp, axis=2)
    if family == "gradient":  # a smooth ramp under renderer-like noise
        base = (xx * (200.0 / max(w - 1, 1)) + yy * (50.0 / max(h - 1, 1)))[..., None] + 10.0 * np.arange(bpp)
        return np.clip(base + rng.normal(0.0, 4.0, (h, w, bpp)), 0, 255).astype(np.uint8)
    raise ValueError(family)


# (w, h, bpp): single pixels and rows, R one byte short of a block, exactly a block, a block and a byte, three blocks of RGB, RGBA
SHAPES = ((1, 1, 1), (1, 7, 3), (7, 1, 4), (17, 13, 3), (150, 217, 1), (255, 128, 1), (3640, 9, 1), (300, 100, 3), (300, 220, 4))
assert [P.filtered_bytes(*s) for s in SHAPES[4:7]] == [P.BLOCK - 1, P.BLOCK, P.BLOCK + 1] and P.n_blocks(*SHAPES[7]) == 3


# ---- a PNG decoder of the tests' own: chunks, CRCs, inflate, the five filters -----------------------------------------------------------------

def unfilter(r, w, h, bpp):
    """The five-filter decoder of the PNG specification, byte by byte"""
    stride = w * bpp
    out = np.zeros((h, stride), np.int64)
    rows = np.asarray(r, np.uint8).reshape(h, 1 + stride).astype(np.int64)
    for y in range(h):
        t, line = int(rows[y, 0]), rows[y, 1:]
        up = out[y - 1] if y else np.zeros(stride, np.int64)
        if t == 0:
            out[y] = line
        elif t == 2:
            out[y] = (line + up) & 255
        else:
            cur = out[y]
            for x in range(stride):
                a = int(cur[x - bpp]) if x >= bpp else 0
                b = int(up[x])
                c = int(up[x - bpp]) if x >= bpp else 0
                if t == 1:
                    pred = a
                elif t == 3:
                    pred = (a + b) // 2
                elif t == 4:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
                else:
                    raise AssertionError(("filter type", t))
                cur[x] = (int(line[x]) + pred) & 255
    return out.astype(np.uint8).reshape(h, w, bpp)


def parse_png(data):
    """[(tag, payload)] of a PNG file, every chunk's CRC checked"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, tag = struct.unpack(">I4s", data[at:at + 8])
        payload = data[at + 8:at + 8 + n]
        (crc,) = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(tag + payload) & 0xFFFFFFFF, tag
        chunks.append((tag, payload))
        at += 12 + n
    assert at == len(data)
    return chunks


def decode_png(data):
    """The (h, w, bpp) image of an 8-bit, non-interlaced PNG file"""
    chunks = parse_png(data)
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0)
    bpp = {0: 1, 2: 3, 6: 4}[ctype]
    return unfilter(np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8), w, h, bpp)
