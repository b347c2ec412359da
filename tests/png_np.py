"""The device PNG encoder's stream (include/rayn_hip.h, "PNG encoding on the device") restated in numpy and plain Python: the adaptive row
filter, the distance-1 run tokens, one dynamic-Huffman block per BLOCK bytes with the stored fallback, the empty stored blocks that align
every block to a byte, the Adler-32 and the 16-byte header.  Integer arithmetic throughout; tests/test_png_device.py asks the kernels for
exactly these bytes.

`mutant` (None: the statement) names one deliberate departure, for tests/test_encode_edge_cases.py to show that a named case notices it and
that the older case tables do not:
  P:stored_gt         the stored form only when the Huffman form is LONGER (> for >=): differs where both take len + 5 bytes
  P:limit_16          frequencies halved only while a depth exceeds 16; P:limit_14: while it exceeds 14
  P:adler_behind_off  the layout kernel's Adler-32 B sum without the (bytes behind the block) * A term for every block that is not the first
                      of its thread's range [t * chunk, (t + 1) * chunk), chunk = ceil(blocks / 256): the statement itself up to 256 blocks
  P:layout_carry      the layout kernel's offsets do not advance inside a thread's range: with more than 256 blocks the blocks of a range
                      land on one another and zeros fill what is left of the stream's length
A mutant of another module's prefix is ignored here.  TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this."""
import heapq
import struct

import numpy as np

BLOCK = 32768           # bytes of the filtered stream per deflate block: part of the format
HEADER_BYTES = 16       # the words (stream length, filtered bytes, blocks, stored blocks) in front of the zlib stream
HEADER_BITS = 1222      # of a dynamic-Huffman block: 17 + 19 * 3 + 286 * 4 + 4
N_SYMBOLS = 286
END_OF_BLOCK = 256
ADLER = 65521
CLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)  # RFC 1951, 3.2.7
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)


# ---- sizes ------------------------------------------------------------------------------------------------------------------------------

def filtered_bytes(w, h, bpp):
    return h * (1 + w * bpp)


def n_blocks(w, h, bpp):
    return -(-filtered_bytes(w, h, bpp) // BLOCK)


def stream_bound(w, h, bpp):
    """rayn_png_stream_bound: the header, 78 01, every block as a stored block (len + 5) plus its alignment (a 3-bit header that may open a
    new byte, and 00 00 FF FF), the Adler-32; rounded up to 16.  0 for a geometry the encoder rejects."""
    n = filtered_bytes(w, h, bpp)
    if w <= 0 or h <= 0 or bpp not in (1, 3, 4) or 1 + w * bpp > 1 << 24 or n >= 1 << 31:
        return 0
    return (HEADER_BYTES + 2 + n + 10 * n_blocks(w, h, bpp) + 4 + 15) // 16 * 16


# ---- the row filter ---------------------------------------------------------------------------------------------------------------------

def filter_candidates(img):
    """(5, h, w * bpp) uint8: the rows under PNG filters 0..4; the row above the first is zeros"""
    h, w, bpp = img.shape
    x = img.reshape(h, w * bpp).astype(np.int32)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, bpp:] = x[:-1, :-bpp]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]).astype(np.uint8)


def filter_rows(img):
    """The filtered stream R (uint8, h * (1 + w * bpp)) and the filter type of every row: the smallest sum of |int8(byte)|, the lowest
    type on a tie"""
    img = np.ascontiguousarray(img, np.uint8)
    h, w, bpp = img.shape
    cand = filter_candidates(img)
    cost = np.abs(cand.view(np.int8).astype(np.int64)).sum(axis=2)  # (5, h)
    pick = np.argmin(cost, axis=0)                                 # the first minimum: the lowest type
    out = np.empty((h, 1 + w * bpp), np.uint8)
    out[:, 0] = pick
    out[:, 1:] = cand[pick, np.arange(h)]
    return out.reshape(-1), pick


# ---- tokens -----------------------------------------------------------------------------------------------------------------------------

def length_symbol(n):
    """(symbol, extra bits, extra value) of a match length 3..258"""
    for k in range(28, -1, -1):
        if n >= LENGTH_BASE[k]:
            return 257 + k, LENGTH_EXTRA[k], n - LENGTH_BASE[k]
    raise ValueError(n)


def block_tokens(blk):
    """The tokens of one block, in order: (position, byte) for a literal -> ("lit", pos, byte); ("match", pos, length).  A maximal run of
    L equal bytes is one literal, then r = L - 1 bytes at distance 1: matches of 258 while r >= 258, then one match of r if r >= 3, else
    r literals."""
    blk = np.asarray(blk, np.uint8)
    n = len(blk)
    starts = np.flatnonzero(np.concatenate([[True], blk[1:] != blk[:-1]]))
    ends = np.concatenate([starts[1:], [n]])
    out = []
    for s, e in zip(starts.tolist(), ends.tolist()):
        v = int(blk[s])
        out.append(("lit", s, v))
        r, pos = e - s - 1, s + 1
        while r >= 258:
            out.append(("match", pos, 258))
            r, pos = r - 258, pos + 258
        if r >= 3:
            out.append(("match", pos, r))
        else:
            out.extend(("lit", pos + k, v) for k in range(r))
    return out


def token_frequencies(tokens):
    f = [0] * N_SYMBOLS
    for t in tokens:
        f[t[2] if t[0] == "lit" else length_symbol(t[2])[0]] += 1
    f[END_OF_BLOCK] += 1
    return f


# ---- the Huffman code -------------------------------------------------------------------------------------------------------------------

def tree_depths(freq):
    """Depth of every symbol with a non-zero frequency in the tree built by merging the two smallest nodes by (weight, index); a leaf's
    index is its symbol, internal nodes are 286, 287, ... in creation order.  One symbol alone gets depth 1."""
    heap = [(f, s) for s, f in enumerate(freq) if f]
    heapq.heapify(heap)
    parent, nxt = {}, len(freq)
    if len(heap) == 1:
        return [1 if f else 0 for f in freq]
    while len(heap) > 1:
        (wa, a), (wb, b) = heapq.heappop(heap), heapq.heappop(heap)
        parent[a] = parent[b] = nxt
        heapq.heappush(heap, (wa + wb, nxt))
        nxt += 1
    depth = [0] * len(freq)
    for s, f in enumerate(freq):
        if f:
            d, k = 0, s
            while k in parent:
                d, k = d + 1, parent[k]
            depth[s] = d
    return depth


def code_lengths(freq, limit=15):
    """(lengths, halvings): while a length exceeds the limit, every non-zero frequency f becomes (f + 1) >> 1 and the tree is rebuilt"""
    freq, halvings = list(freq), 0
    while True:
        d = tree_depths(freq)
        if max(d) <= limit:
            return d, halvings
        freq = [(f + 1) >> 1 if f else 0 for f in freq]
        halvings += 1


def canonical_codes(lengths):
    """RFC 1951, 3.2.2"""
    count = [0] * 17
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = [0] * len(lengths)
    for s, n in enumerate(lengths):
        if n:
            out[s] = nxt[n]
            nxt[n] += 1
    return out


def _reverse(code, n):
    return int(format(code, "0%db" % n)[::-1], 2) if n else 0


class _Bits:
    """least-significant bit first, as deflate packs"""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, nbits):
        self.v |= value << self.n
        self.n += nbits

    def put_code(self, code, nbits):  # a Huffman code goes most-significant bit first
        self.put(_reverse(code, nbits), nbits)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


LAYOUT_THREADS = 256    # of the layout kernel: thread t lays out the blocks [t * chunk, (t + 1) * chunk), chunk = ceil(blocks / 256)


def length_limit(mutant=None):
    return {"P:limit_16": 16, "P:limit_14": 14}.get(mutant, 15)


def huffman_block(blk, final, mutant=None):
    """The dynamic-Huffman encoding of a block, zero-padded to a byte and WITHOUT the alignment block: (bytes, bits, info)"""
    tokens = block_tokens(blk)
    freq = token_frequencies(tokens)
    lengths, halvings = code_lengths(freq, length_limit(mutant))
    codes = canonical_codes(lengths)
    has_match = any(t[0] == "match" for t in tokens)
    b = _Bits()
    b.put(1 if final else 0, 1)
    b.put(2, 2)
    b.put(29, 5)   # HLIT: 286 codes
    b.put(0, 5)    # HDIST: 1 code
    b.put(15, 4)   # HCLEN: 19 code-length code lengths
    for s in CLEN_ORDER:
        b.put(4 if s < 16 else 0, 3)
    for n in lengths:          # the code-length code is the 4-bit binary code: symbol n has code n
        b.put_code(n, 4)
    b.put_code(1 if has_match else 0, 4)
    assert b.n == HEADER_BITS
    for t in tokens:
        if t[0] == "lit":
            b.put_code(codes[t[2]], lengths[t[2]])
        else:
            sym, xbits, xval = length_symbol(t[2])
            b.put_code(codes[sym], lengths[sym])
            b.put(xval, xbits)
            b.put(0, 1)        # the one distance code, length 1
    b.put_code(codes[END_OF_BLOCK], lengths[END_OF_BLOCK])
    return b.bytes(), b.n, {"tokens": tokens, "freq": freq, "lengths": lengths, "halvings": halvings, "has_match": has_match}


def encode_block(blk, final, mutant=None):
    """(bytes of the block with its alignment, stored?)"""
    blk = np.asarray(blk, np.uint8)
    n = len(blk)
    data, bits, _ = huffman_block(blk, final, mutant)
    if len(data) > n + 5 if mutant == "P:stored_gt" else len(data) >= n + 5:
        return struct.pack("<BHH", 1 if final else 0, n, n ^ 0xFFFF) + blk.tobytes(), True
    if final:
        return data, False
    data = data + b"\x00" * ((bits + 3 + 7) // 8 - len(data))  # 000: an empty stored block, not final; zero padding to the byte
    return data + b"\x00\x00\xff\xff", False


def adler32(r, mutant=None):
    """From the per-block sums the kernels keep: A = sum of the bytes, B = sum of (bytes that follow, the byte included) * byte"""
    r = np.asarray(r, np.uint8).astype(np.uint64)
    n = len(r)
    a = int(r.sum()) % ADLER
    b = int((r * (n - np.arange(n, dtype=np.uint64))).sum() % ADLER) if n < 1 << 24 else None
    if b is None:
        raise ValueError("stream too long for this restatement")
    if mutant == "P:adler_behind_off":
        nblocks = -(-n // BLOCK)
        chunk = -(-nblocks // LAYOUT_THREADS)
        for k in range(nblocks):
            if k % chunk:
                b -= (n - min((k + 1) * BLOCK, n)) * int(r[k * BLOCK:(k + 1) * BLOCK].sum())
        b %= ADLER
    return (((n + b) % ADLER) << 16) | ((1 + a) % ADLER)


def join_blocks(parts, mutant=None):
    """The encoded blocks one behind the other, as the layout kernel's offsets and the compaction place them"""
    if mutant != "P:layout_carry":
        return b"".join(parts)
    chunk = -(-len(parts) // LAYOUT_THREADS)
    out = bytearray(sum(len(d) for d in parts))
    at = first = 0
    for k, d in enumerate(parts):   # every block of a range at the range's first offset: a later one lies on top of an earlier one
        if k % chunk == 0:
            first = at
        out[first:first + len(d)] = d
        at += len(d)
    return bytes(out)


def encode_filtered(r, mutant=None, block_encoder=None):
    """The header and the zlib stream of a filtered stream R; info: per-block (stored?, bytes).  block_encoder(blk, final): a stand-in for
    encode_block that returns what it would - a cache, for streams of many equal blocks."""
    r = np.asarray(r, np.uint8)
    n = len(r)
    blocks = [r[o:o + BLOCK] for o in range(0, n, BLOCK)]
    parts, info = [], []
    for k, blk in enumerate(blocks):
        data, stored = block_encoder(blk, k == len(blocks) - 1) if block_encoder else encode_block(blk, k == len(blocks) - 1, mutant)
        parts.append(data)
        info.append((stored, len(data)))
    z = b"\x78\x01" + join_blocks(parts, mutant) + struct.pack(">I", adler32(r, mutant))
    head = struct.pack("<IIII", len(z), n, len(blocks), sum(1 for s, _ in info if s))
    return head + z, info


def encode(img, mutant=None):
    """What rayn_hip_png_encode_device writes for an 8-bit image (h, w, bpp): the 16-byte header, then the zlib stream.  The word holding
    the stream's last byte is zero-padded (see padded)."""
    r, _ = filter_rows(img)
    return encode_filtered(r, mutant)[0]


def padded(stream):
    """The bytes the device writes: the stream, zero-padded to a multiple of 4"""
    return stream + b"\x00" * (-len(stream) % 4)
