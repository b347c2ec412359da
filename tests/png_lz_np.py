"""The LZ77 device encoder's stream (include/rayn_hip.h, "PNG encoding on the device, with LZ77 matches") restated in numpy and plain
Python on top of png_np: the same filtered stream R, blocks, stored fallback, alignment, Adler-32 and header words; per block the three
match candidates (distance 1, the last equal trigram, the row above), the greedy parse, and a second Huffman code over the 30 distance
symbols.  Integer arithmetic throughout; tests/test_png_lz_device.py asks the kernels for exactly these bytes.

`mutant` (None: the statement; see png_np, whose mutants pass through to the parts shared with it - the length limit, the layout, the
Adler-32): Z:stored_gt, png_np's P:stored_gt in this block kernel; Z:exit_bit8, the block kernel's exit - the first token start behind the
128-byte span a token starts in, relative to the span's end, 0..257 - kept in 8 bits: a token that ends 256 or 257 bytes behind its
span's end sends the parse 256 bytes back, into the bytes the match covers.  TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this."""
import struct

import numpy as np

import png_np as P

HEADER_BITS = 1338      # of a dynamic-Huffman block: 17 + 19 * 3 + 286 * 4 + 30 * 4
N_DISTANCES = 30
MAX_MATCH = 258
FAR = 4096              # a match of length 3 is taken up to this distance
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


def deflate_stream_bound(n):
    """rayn_deflate_stream_bound: rayn_png_stream_bound's formula on n bytes; 0 for a size the entry rejects"""
    if not 1 <= n < 1 << 31:
        return 0
    return (P.HEADER_BYTES + 2 + n + 10 * (-(-n // P.BLOCK)) + 4 + 15) // 16 * 16


# ---- matches ----------------------------------------------------------------------------------------------------------------------------

def distance_symbol(d):
    """(symbol, extra bits, extra value) of a match distance 1..32768, RFC 1951 3.2.5"""
    for k in range(N_DISTANCES - 1, -1, -1):
        if d >= DIST_BASE[k]:
            return k, DIST_EXTRA[k], d - DIST_BASE[k]
    raise ValueError(d)


def prev_positions(blk):
    """prev(i) for every i of the block: the largest j < i with blk[j:j+3] == blk[i:i+3], -1 where there is none or i + 3 > len.  Exact
    byte equality: the positions are sorted by their three bytes, stably, and an equal neighbour in that order is the predecessor."""
    blk = np.asarray(blk, np.uint8)
    n = len(blk)
    prev = np.full(n, -1, np.int64)
    if n < 3:
        return prev
    b = blk.astype(np.int64)
    key = b[:n - 2] | (b[1:n - 1] << 8) | (b[2:] << 16)
    order = np.argsort(key, kind="stable")
    same = key[order[1:]] == key[order[:-1]]
    prev[order[1:][same]] = order[:-1][same]
    return prev


def match_length(data, i, d, cap):
    """m(i, d) on the bytes object `data`: the largest L <= cap with data[i-d+k] == data[i+k] for all k < L; overlap allowed"""
    a, b = data[i - d:i - d + cap], data[i:i + cap]
    if a == b:
        return cap
    x = int.from_bytes(a, "little") ^ int.from_bytes(b, "little")
    return ((x & -x).bit_length() - 1) // 8


def best_match(data, i, prev_i, stride):
    """(M(i), D(i)): the longest match over the candidates d = 1, d = i - prev(i) and d = stride that do not reach before the block start,
    and the smallest distance that reaches it; (0, 0) without a candidate"""
    cap = min(MAX_MATCH, len(data) - i)
    cands = {1}
    if prev_i >= 0:
        cands.add(i - prev_i)
    if stride:
        cands.add(stride)
    best, dist = 0, 0
    for d in sorted(cands):
        if i - d >= 0:
            m = match_length(data, i, d, cap)
            if m > best:
                best, dist = m, d
    return best, dist


SPAN = 128              # bytes of the block a thread of the block kernel tokenises


def block_tokens(blk, stride=0, mutant=None):
    """The tokens of one block, in order, by the greedy parse from 0: ("match", pos, M, D) if M(pos) >= 3 and not (M == 3 and D > 4096),
    else ("lit", pos, byte)"""
    blk = np.asarray(blk, np.uint8)
    data, prev = blk.tobytes(), prev_positions(blk).tolist()
    out, p, n = [], 0, len(data)
    while p < n:
        m, d = best_match(data, p, prev[p], stride)
        if m >= 3 and not (m == 3 and d > FAR):
            out.append(("match", p, m, d))
            span_end = min((p // SPAN + 1) * SPAN, n)
            p += m
            if mutant == "Z:exit_bit8" and p - span_end >= 256:
                p -= 256
        else:
            out.append(("lit", p, data[p]))
            p += 1
    return out


def token_frequencies(tokens):
    """(the 286 literal/length counts, end-of-block counting 1; the 30 distance counts)"""
    f, g = [0] * P.N_SYMBOLS, [0] * N_DISTANCES
    for t in tokens:
        if t[0] == "lit":
            f[t[2]] += 1
        else:
            f[P.length_symbol(t[2])[0]] += 1
            g[distance_symbol(t[3])[0]] += 1
    f[P.END_OF_BLOCK] += 1
    return f, g


def distance_lengths(freq, limit=15):
    """(lengths, halvings) of the distance code: png_np's construction over 30 symbols (internal nodes 30, 31, ...), halved on its own;
    with one symbol in use that one gets length 1, with none symbol 0 does - the incomplete code RFC 1951 allows"""
    if not any(freq):
        return [1] + [0] * (N_DISTANCES - 1), 0
    return P.code_lengths(freq, limit)


# ---- blocks and the stream ------------------------------------------------------------------------------------------------------------------

def huffman_block(blk, final, stride=0, mutant=None):
    """The dynamic-Huffman encoding of a block, zero-padded to a byte and WITHOUT the alignment block: (bytes, bits, info)"""
    tokens = block_tokens(blk, stride, mutant)
    freq, dfreq = token_frequencies(tokens)
    lengths, halvings = P.code_lengths(freq, P.length_limit(mutant))
    dlengths, dhalvings = distance_lengths(dfreq, P.length_limit(mutant))
    codes, dcodes = P.canonical_codes(lengths), P.canonical_codes(dlengths)
    b = P._Bits()
    b.put(1 if final else 0, 1)
    b.put(2, 2)
    b.put(29, 5)   # HLIT: 286 codes
    b.put(29, 5)   # HDIST: 30 codes
    b.put(15, 4)   # HCLEN: 19 code-length code lengths
    for s in P.CLEN_ORDER:
        b.put(4 if s < 16 else 0, 3)
    for n in lengths + dlengths:   # the code-length code is the 4-bit binary code: symbol n has code n
        b.put_code(n, 4)
    assert b.n == HEADER_BITS
    for t in tokens:
        if t[0] == "lit":
            b.put_code(codes[t[2]], lengths[t[2]])
        else:
            sym, xbits, xval = P.length_symbol(t[2])
            b.put_code(codes[sym], lengths[sym])
            b.put(xval, xbits)
            sym, xbits, xval = distance_symbol(t[3])
            b.put_code(dcodes[sym], dlengths[sym])
            b.put(xval, xbits)
    b.put_code(codes[P.END_OF_BLOCK], lengths[P.END_OF_BLOCK])
    return b.bytes(), b.n, {"tokens": tokens, "freq": freq, "dfreq": dfreq, "lengths": lengths, "dlengths": dlengths, "halvings": halvings,
                            "dhalvings": dhalvings}


def encode_block(blk, final, stride=0, mutant=None):
    """(bytes of the block with its alignment, stored?)"""
    blk = np.asarray(blk, np.uint8)
    n = len(blk)
    data, bits, _ = huffman_block(blk, final, stride, mutant)
    if len(data) > n + 5 if mutant == "Z:stored_gt" else len(data) >= n + 5:
        return struct.pack("<BHH", 1 if final else 0, n & 0xFFFF, (n & 0xFFFF) ^ 0xFFFF) + blk.tobytes(), True
    if final:
        return data, False
    data = data + b"\x00" * ((bits + 3 + 7) // 8 - len(data))  # 000: an empty stored block, not final; zero padding to the byte
    return data + b"\x00\x00\xff\xff", False


def encode_filtered(r, stride=0, mutant=None, block_encoder=None):
    """What rayn_hip_deflate_lz77_device writes for the bytes r with the row stride `stride` (0: no row candidate): the header words and
    the zlib stream; info: per-block (stored?, bytes).  block_encoder(blk, final): as png_np.encode_filtered's."""
    r = np.asarray(r, np.uint8)
    n = len(r)
    blocks = [r[o:o + P.BLOCK] for o in range(0, n, P.BLOCK)]
    parts, info = [], []
    for k, blk in enumerate(blocks):
        data, stored = block_encoder(blk, k == len(blocks) - 1) if block_encoder else encode_block(blk, k == len(blocks) - 1, stride, mutant)
        parts.append(data)
        info.append((stored, len(data)))
    z = b"\x78\x01" + P.join_blocks(parts, mutant) + struct.pack(">I", P.adler32(r, mutant))
    head = struct.pack("<IIII", len(z), n, len(blocks), sum(1 for s, _ in info if s))
    return head + z, info


def encode(img, mutant=None):
    """What rayn_hip_png_encode_lz77_device writes for an 8-bit image (h, w, bpp): the 16-byte header, then the zlib stream"""
    img = np.asarray(img, np.uint8)
    r, _ = P.filter_rows(img)
    return encode_filtered(r, 1 + img.shape[1] * img.shape[2], mutant)[0]
