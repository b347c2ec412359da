"""The device EXR chunk encoder (include/rayn_hip.h, "OpenEXR scanline chunks with ZIP compression on the device") restated in numpy and
plain Python: the f32 -> half conversion in integers, the scanline bytes, the ZIP pre-process, every chunk's zlib stream through
png_np.encode_filtered / png_lz_np.encode_filtered, the raw rule, the buffer the device writes and the file made of it.
tests/test_exr_device.py asks the kernels for exactly these bytes.

`mutant` (None: the statement; the mutants of png_np and png_lz_np pass through to the chunks' streams):
  E:raw_gt                  a chunk is raw only when its zlib stream is LONGER than its bytes (> for >=): differs at stream == n_k
  E:raw_size_plus_header    the raw rule compares the blocks' bytes, without the stream's 6 framing bytes (78 01 and the Adler-32)
  E:last_chunk_full_blocks  the last chunk counted with the blocks of a full chunk: the header's block count of an image whose last chunk
                            is shorter by a block or more
TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this."""
import struct

import numpy as np

import png_lz_np as Z
import png_np as P

UINT, HALF, FLOAT = 0, 1, 2
ROWS = 16               # scanlines per chunk
HEADER_BYTES = 16       # the words (body bytes, chunks, raw chunks, deflate blocks) in front of the chunk table
MAX_CHANNELS = 16


def size_of(t):
    return 2 if t == HALF else 4


# ---- f32 -> half ---------------------------------------------------------------------------------------------------------------------------

def half_bits(words):
    """uint16 bits of the binary16 nearest (ties to even) to the float32 whose bits are `words` (uint32), in integer arithmetic"""
    x = np.ascontiguousarray(words).view(np.uint32).astype(np.int64)
    sign, a = (x >> 16) & 0x8000, x & 0x7FFFFFFF
    m = (a & 0x7FFFFF) >> 13
    nan = 0x7C00 | m | (m == 0)
    r = a - 0x38000000
    normal = (r + 0xFFF + ((r >> 13) & 1)) >> 13
    shift = np.clip(126 - (a >> 23), 1, 24)
    mant = (a & 0x7FFFFF) | 0x800000
    q, rem, tie = mant >> shift, mant & ((1 << shift) - 1), 1 << (shift - 1)
    denormal = q + ((rem > tie) | ((rem == tie) & ((q & 1) == 1)))
    out = np.where(a > 0x7F800000, nan,
                   np.where(a >= 0x477FF000, 0x7C00,
                            np.where(a >= 0x38800000, normal,
                                     np.where(a <= 0x33000000, 0, denormal))))
    return (sign | out).astype(np.uint16)


# ---- sizes -----------------------------------------------------------------------------------------------------------------------------------

def row_bytes(w, types):
    return w * sum(size_of(t) for t in types)


def n_chunks(h):
    return -(-h // ROWS)


def chunk_bytes(w, h, types):
    s = row_bytes(w, types)
    return [s * (min(y + ROWS, h) - y) for y in range(0, h, ROWS)]


def body_at(h):
    return (HEADER_BYTES + 4 * n_chunks(h) + 15) // 16 * 16


def stream_bound(w, h, layout):
    """rayn_exr_stream_bound: align16(16 + 4 * chunks) + align16(sum of 8 + n_k); 0 for what the entry rejects.  layout: (stride, offset,
    type) per channel."""
    if w <= 0 or h <= 0 or not 1 <= len(layout) <= MAX_CHANNELS:
        return 0
    if any(t not in (UINT, HALF, FLOAT) or s == 0 or o >= s for s, o, t in layout):
        return 0
    types = [t for _, _, t in layout]
    if ROWS * row_bytes(w, types) >= 1 << 31:
        return 0
    bound = body_at(h) + (sum(8 + n for n in chunk_bytes(w, h, types)) + 15) // 16 * 16
    return bound if bound < 1 << 31 else 0


# ---- rows, chunks ----------------------------------------------------------------------------------------------------------------------------

def channel_words(plane, stride, offset, w, h):
    """The h * w words of a channel in the film's order: plane[p * stride + offset]"""
    return np.ascontiguousarray(plane).reshape(-1).view(np.uint32)[offset::stride][:w * h]


def scanlines(w, h, channels):
    """(h, S) uint8, the file's rows top-down.  channels: (plane, stride, offset, type), planes as 32-bit words in the film's layout"""
    parts = []
    for plane, stride, offset, t in channels:
        a = channel_words(plane, stride, offset, w, h).reshape(h, w)[::-1]
        a = half_bits(a).astype("<u2") if t == HALF else a.astype("<u4")
        parts.append(np.ascontiguousarray(a).view(np.uint8).reshape(h, -1))
    return np.concatenate(parts, axis=1)


def preprocess(raw):
    raw = np.asarray(raw, np.uint8)
    t = np.concatenate([raw[0::2], raw[1::2]]).astype(np.int64)
    p = t.copy()
    p[1:] = (t[1:] - t[:-1] + 128) & 255
    return p.astype(np.uint8)


def encode_chunk(raw, half_row, matches, mutant=None):
    """(payload, raw?, blocks): the zlib stream of the pre-processed bytes, or the bytes themselves when it is not shorter"""
    raw = np.asarray(raw, np.uint8)
    p = preprocess(raw)
    enc, info = Z.encode_filtered(p, half_row, mutant) if matches else P.encode_filtered(p, mutant)
    z = enc[P.HEADER_BYTES:]
    size = len(z) - 6 if mutant == "E:raw_size_plus_header" else len(z)
    if size > len(raw) if mutant == "E:raw_gt" else size >= len(raw):
        return raw.tobytes(), True, len(info)
    return z, False, len(info)


def encode(w, h, channels, matches, mutant=None):
    """What rayn_hip_exr_encode_device writes: the four words, the chunk table, zeros to 16, the body.  info: per chunk (raw?, payload)"""
    rows = scanlines(w, h, channels)
    s = rows.shape[1]
    starts, body, info, blocks = [], b"", [], 0
    for y in range(0, h, ROWS):
        payload, is_raw, nb = encode_chunk(rows[y:y + ROWS].reshape(-1), s // 2, matches, mutant)
        if mutant == "E:last_chunk_full_blocks":
            nb = -(-ROWS * s // P.BLOCK)
        starts.append(len(body))
        body += struct.pack("<ii", y, len(payload)) + payload
        info.append((is_raw, len(payload)))
        blocks += nb
    head = struct.pack("<IIII", len(body), len(starts), sum(1 for r, _ in info if r), blocks) + struct.pack("<%dI" % len(starts), *starts)
    return head + b"\x00" * (body_at(h) - len(head)) + body, info


def padded(buf):
    """The bytes the device writes: the body's last word zero-padded"""
    return buf + b"\x00" * (-len(buf) % 4)


# ---- the file ----------------------------------------------------------------------------------------------------------------------------------

def _attr(name, kind, value):
    return name + b"\0" + kind + b"\0" + struct.pack("<i", len(value)) + value


def header(w, h, named):
    """named: (name bytes, type) in the file's order"""
    chlist = b"".join(n + b"\0" + struct.pack("<i", t) + b"\0\0\0\0" + struct.pack("<ii", 1, 1) for n, t in named) + b"\0"
    box = struct.pack("<iiii", 0, 0, w - 1, h - 1)
    return (bytes([0x76, 0x2F, 0x31, 0x01, 2, 0, 0, 0]) + _attr(b"channels", b"chlist", chlist) + _attr(b"compression", b"compression", b"\x03")
            + _attr(b"dataWindow", b"box2i", box) + _attr(b"displayWindow", b"box2i", box) + _attr(b"lineOrder", b"lineOrder", b"\x00")
            + _attr(b"pixelAspectRatio", b"float", struct.pack("<f", 1.0)) + _attr(b"screenWindowCenter", b"v2f", struct.pack("<ff", 0, 0))
            + _attr(b"screenWindowWidth", b"float", struct.pack("<f", 1.0)) + b"\0")


def file_of(w, h, named, encoded):
    """The file of an encoded buffer: the header, the u64 offsets (chunk start + everything in front of the body), the body"""
    body, chunks = struct.unpack("<II", encoded[:8])
    starts = struct.unpack("<%dI" % chunks, encoded[16:16 + 4 * chunks])
    head = header(w, h, named)
    at = len(head) + 8 * chunks
    return head + struct.pack("<%dQ" % chunks, *(at + s for s in starts)) + encoded[body_at(h):body_at(h) + body]
