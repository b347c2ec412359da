"""Film::save_to's per-pixel post-process (src/film.rs:205-378): saturate, gamma 2.2, Color+Background composite,
Color+Alpha RGBA, normal -> RGB, y-flip, 8-bit quantise.  Host-side, after the hot path.  PNG is written with
zlib only (the reference uses the `image` crate); png_from_stream frames a zlib stream made elsewhere, the device encoder's
(Context.png_encode) included.  The OpenEXR writer at the end of the file is an extension: exr_from_chunks frames the chunks of
Context.exr_encode, save_exr_host makes the same file layout with zlib on the host.

Arithmetic follows the reference: f32 throughout, `Srgb::saturated` = x.max(0).min(1) and `gamma_corrected(2.2)` =
x.powf(1/2.2) (src/spectrum.rs:30-40), quantisation `(v * 255.0).min(255.0).max(0.0) as u8` with Rust's f32::min/max
(a NaN operand yields the other operand) and the truncating, saturating cast.  powf is evaluated in float64 and rounded to
float32 - the same "double-evaluated, correctly rounded" result the pinned dm_powf gives (tests compare with the oracle)."""
import struct
import zlib

import numpy as np

F32 = np.float32


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def png_from_stream(w, h, bpp, zstream):
    """The bytes of the PNG file of a w x h image of bpp (1 grey, 3 RGB, 4 RGBA) bytes per pixel around the zlib stream of its filtered
    rows: the signature, IHDR, one IDAT and IEND.  The CRC-32 of the chunk is computed here, on the host."""
    ctype = {1: 0, 3: 2, 4: 6}[bpp]
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)) + _chunk(b"IDAT", bytes(zstream))
            + _chunk(b"IEND", b""))


def png_stream_of(encoded):
    """The zlib stream inside what Context.png_encode writes (a uint8 array or bytes-like): the first little-endian word is its length,
    the stream starts at byte 16"""
    m = memoryview(encoded).cast("B")
    n = int.from_bytes(m[:4], "little")
    if n < 6 or 16 + n > len(m):
        raise ValueError(f"not an encoded stream: length word {n} in a buffer of {len(m)} bytes")
    return m[16:16 + n]


def _png(path, img8):
    h, w, c = img8.shape
    raw = b"".join(b"\x00" + img8[y].tobytes() for y in range(h))
    with open(path, "wb") as f:
        f.write(png_from_stream(w, h, c, zlib.compress(raw, 6)))


def _rust_min(a, b):
    """f32::min: a NaN operand yields the other one."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.minimum(a, b))).astype(F32)


def _rust_max(a, b):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.maximum(a, b))).astype(F32)


def _quant(x):
    """(v * 255.0).min(255.0).max(0.0) as u8"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(x, F32) * F32(255.0)
    return _rust_max(_rust_min(v, F32(255.0)), F32(0.0)).astype(np.uint8)  # truncation toward zero of a value in [0, 255]


def saturated(x):
    """Srgb::saturated, src/spectrum.rs:35-40"""
    return _rust_min(_rust_max(np.asarray(x, F32), F32(0.0)), F32(1.0))


def gamma_corrected(x, gamma=2.2):
    """Srgb::gamma_corrected, src/spectrum.rs:30-33: x.powf(1.0 / gamma) in f32 (libm conventions: negative base -> NaN,
    pow(0, y > 0) = 0, pow(1, y) = 1)."""
    x = np.asarray(x, F32)
    e = F32(1.0) / F32(gamma)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.power(x.astype(np.float64), np.float64(e)).astype(F32)


def color_image(color, background=None, alpha=None, transparent_background=False):
    """The Color arm of save_to (src/film.rs:222-289).  Returns the 8-bit image (rows top-down), RGB or RGBA:
      Color + Alpha, transparent_background      -> RGBA: color.saturated().gamma_corrected(2.2) | alpha          (:231-254)
      Color + Background, not transparent        -> RGB:  (color + background).saturated().gamma_corrected(2.2)   (:255-277)
      Color only, not transparent                -> RGB:  color.gamma_corrected(2.2) - NOT saturated              (:278-ff)
    anything else is the reference's Err("... insufficient channels")."""
    c = np.asarray(color, F32)
    if transparent_background:
        if alpha is None:
            raise ValueError("Attempted to write Color channel with insufficient channels")
        rgb = _quant(gamma_corrected(saturated(c)))
        return np.concatenate([rgb, _quant(np.asarray(alpha, F32))[..., None]], axis=-1)[::-1]
    if background is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            s = (c + np.asarray(background, F32)).astype(F32)
        return _quant(gamma_corrected(saturated(s)))[::-1]
    return _quant(gamma_corrected(c))[::-1]


def background_image(background):
    """saturated().gamma_corrected(2.2) (src/film.rs:290-313)"""
    return _quant(gamma_corrected(saturated(background)))[::-1]


def normal_image(normal):
    """vec * 0.5 + 0.5 (src/film.rs:314-338)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return _quant(np.asarray(normal, F32) * F32(0.5) + F32(0.5))[::-1]


def alpha_image(alpha):
    """grey image of the Alpha channel (src/film.rs:339-362)"""
    return _quant(alpha)[::-1][..., None]


def save(path, img8):
    _png(path, np.ascontiguousarray(img8))


def save_pfm(path, rgb):
    """Write a float image (h, w, 3), rows BOTTOM-UP like the film, as a colour PFM: the header "PF", "w h", "-1.0" (a negative scale =
    little-endian), then the rows bottom-up as little-endian float32 - the film's own order, so the floats are written as they are."""
    a = np.ascontiguousarray(rgb, dtype="<f4")
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"save_pfm takes an (h, w, 3) image, got shape {a.shape}")
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (a.shape[1], a.shape[0]) + a.tobytes())


def load_pfm(path):
    """Read a colour PFM written by save_pfm (either byte order): float32 (h, w, 3), rows bottom-up."""
    with open(path, "rb") as f:
        magic, dims, scale = f.readline().strip(), f.readline().split(), float(f.readline())
        if magic != b"PF" or len(dims) != 2:
            raise ValueError(f"{path} is not a colour PFM")
        w, h = int(dims[0]), int(dims[1])
        return np.frombuffer(f.read(12 * w * h), dtype="<f4" if scale < 0 else ">f4").astype(F32).reshape(h, w, 3)


# ---- OpenEXR (an extension: include/rayn_hip.h, "OpenEXR scanline chunks with ZIP compression on the device") ----------------------------
# Single-part scanline files, ZIP compression (16 rows per chunk), written from the published file layout.  Conformance with real OpenEXR
# readers is unpinned: no OpenEXR library was at hand.

EXR_UINT, EXR_HALF, EXR_FLOAT = 0, 1, 2
EXR_ROWS = 16


def check_exr_names(names):
    """The channel names of an EXR file, in its order: bytes-like or str, 1..31 bytes, no NUL, strictly ascending byte-wise.  Returns them
    as bytes; ValueError otherwise."""
    out = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
    for n in out:
        if not 1 <= len(n) <= 31 or b"\0" in n:
            raise ValueError(f"an EXR channel name has 1..31 bytes and no NUL, got {n!r}")
    for a, b in zip(out, out[1:]):
        if a == b:
            raise ValueError(f"EXR channel {a!r} appears twice")
        if a > b:
            raise ValueError(f"EXR channels must be sorted by name: {a!r} stands in front of {b!r}")
    return out


def _exr_attr(name, kind, value):
    return name + b"\0" + kind + b"\0" + struct.pack("<i", len(value)) + value


def exr_header(w, h, channels):
    """Everything of the file in front of the offset table: the magic, the version and the attributes.  channels: (name, type) in the
    file's order, type one of EXR_UINT, EXR_HALF, EXR_FLOAT."""
    names = check_exr_names([c[0] for c in channels])
    if w <= 0 or h <= 0 or not names:
        raise ValueError("an EXR file has at least one pixel and one channel")
    for _, t in channels:
        if t not in (EXR_UINT, EXR_HALF, EXR_FLOAT):
            raise ValueError(f"an EXR channel type is 0 (UINT), 1 (HALF) or 2 (FLOAT), got {t!r}")
    chlist = b"".join(n + b"\0" + struct.pack("<iB3xii", t, 0, 1, 1) for n, (_, t) in zip(names, channels)) + b"\0"
    box = struct.pack("<iiii", 0, 0, w - 1, h - 1)
    return (b"\x76\x2f\x31\x01" + b"\x02\x00\x00\x00"
            + _exr_attr(b"channels", b"chlist", chlist)
            + _exr_attr(b"compression", b"compression", b"\x03")
            + _exr_attr(b"dataWindow", b"box2i", box)
            + _exr_attr(b"displayWindow", b"box2i", box)
            + _exr_attr(b"lineOrder", b"lineOrder", b"\x00")
            + _exr_attr(b"pixelAspectRatio", b"float", struct.pack("<f", 1.0))
            + _exr_attr(b"screenWindowCenter", b"v2f", struct.pack("<ff", 0.0, 0.0))
            + _exr_attr(b"screenWindowWidth", b"float", struct.pack("<f", 1.0))
            + b"\0")


def _exr_file(w, h, channels, starts, body):
    head = exr_header(w, h, channels)
    at = len(head) + 8 * len(starts)
    return head + struct.pack("<%dQ" % len(starts), *(at + s for s in starts)) + bytes(body)


def exr_from_chunks(w, h, channels, encoded):
    """The bytes of the EXR file of what Context.exr_encode wrote (a uint8 array or bytes-like): the header, the offset table - the
    device's chunk starts plus the length of everything in front of the body - and the body as it is.  ValueError for a buffer that is
    not one: a chunk count other than the height's, a body past the buffer's end, starts that do not ascend inside it."""
    m = memoryview(encoded).cast("B")
    chunks = -(-h // EXR_ROWS)
    body_at = (16 + 4 * chunks + 15) // 16 * 16
    if len(m) < body_at:
        raise ValueError(f"not an encoded EXR body: {len(m)} bytes are less than the header and the table of {chunks} chunks")
    body, count = struct.unpack("<II", m[:8])
    if count != chunks or body < 10 * chunks or body_at + body > len(m):
        raise ValueError(f"not an encoded EXR body: {count} chunks of {body} bytes in a buffer of {len(m)} bytes, {chunks} chunks expected")
    starts = struct.unpack("<%dI" % chunks, m[16:16 + 4 * chunks])
    if starts[0] != 0 or any(b - a < 10 for a, b in zip(starts, starts[1:] + (body,))):
        raise ValueError("not an encoded EXR body: the chunk starts do not ascend inside it")
    return _exr_file(w, h, channels, starts, m[body_at:body_at + body])


def exr_row_bytes(w, h, channels):
    """(h, S) uint8: the scanlines of the file, top-down.  channels: (name, type, words) with words the channel's h * w 32-bit words in
    the film's order (rows bottom-up), uint32 or float32; HALF converts them as float32 with numpy's astype(float16)."""
    parts = []
    for _, t, words in channels:
        a = np.ascontiguousarray(words).reshape(h, w)[::-1]
        if a.dtype.itemsize != 4:
            raise ValueError("an EXR channel is given as 32-bit words")
        if t == EXR_HALF:
            with np.errstate(over="ignore", invalid="ignore"):
                a = a.view(np.float32).astype(np.float16)
        parts.append(np.ascontiguousarray(a).view(np.uint8).reshape(h, -1))
    return np.concatenate(parts, axis=1)


def exr_preprocess(raw):
    """The ZIP pre-process of a chunk's bytes: the even bytes, then the odd ones; then every byte but the first minus its predecessor + 128"""
    raw = np.asarray(raw, np.uint8)
    t = np.concatenate([raw[0::2], raw[1::2]]).astype(np.int32)
    t[1:] = t[1:] - t[:-1] + 128
    return t.astype(np.uint8)


def exr_bytes_host(w, h, channels, level=6):
    """The file exr="host" writes: the layout of exr_from_chunks with zlib.compress(P, level) per chunk and the same raw rule"""
    rows = exr_row_bytes(w, h, channels)
    starts, body = [], b""
    for y in range(0, h, EXR_ROWS):
        raw = rows[y:y + EXR_ROWS].tobytes()
        z = zlib.compress(exr_preprocess(np.frombuffer(raw, np.uint8)).tobytes(), level)
        payload = raw if len(z) >= len(raw) else z
        starts.append(len(body))
        body += struct.pack("<ii", y, len(payload)) + payload
    return _exr_file(w, h, [(n, t) for n, t, _ in channels], starts, body)


def save_exr_host(path, w, h, channels, level=6):
    """Write exr_bytes_host(w, h, channels) to path"""
    data = exr_bytes_host(w, h, channels, level)
    with open(path, "wb") as f:
        f.write(data)


# ---- JPEG and Motion-JPEG (an extension: include/rayn_hip.h, "Baseline JPEG scans on the device") ----------------------------------------
# jpeg_from_scan frames the scan of Context.jpeg_encode with the library's own tables; AviWriter puts such files into an AVI container,
# written from its published layout.  No player was at hand: tests/avi_read.py, a reader written from the same layout, is all that pins it.

def _jpeg_segment(marker, payload):
    return bytes((0xFF, marker)) + struct.pack(">H", len(payload) + 2) + payload


def jpeg_from_scan(w, h, bpp, jpeg, encoded):
    """The bytes of the baseline JPEG file of a w x h image of bpp (1 grey, 3 colour) bytes per pixel around what Context.jpeg_encode wrote
    with the parameters `jpeg` (a Jpeg; 4:2:0 holds for bpp 3 only): SOI, APP0 JFIF 1.1, DQT per table, SOF0, DHT per table, DRI, SOS,
    the scan, EOI.  The tables are the library's (jpeg_quant_table, jpeg_huffman_table).  ValueError for a bpp without a JPEG form, a size
    the format has no field for, and a buffer that is not what that call writes: header words that disagree with the geometry or a scan
    past the buffer's end."""
    from .context import jpeg_huffman_table, jpeg_quant_table
    from .options import Jpeg
    if not isinstance(jpeg, Jpeg):
        raise ValueError(f"jpeg must be a Jpeg, got {jpeg!r}")
    if bpp not in (1, 3):
        raise ValueError(f"a JPEG holds 1 or 3 bytes per pixel, got {bpp!r} (JPEG has no alpha)")
    if not (1 <= w <= 65535 and 1 <= h <= 65535):
        raise ValueError(f"a JPEG has 1..65535 columns and rows, got {w}x{h}")
    sub, n = jpeg.mode(bpp), 1 if bpp == 1 else 3
    side = 16 if sub else 8
    mcus = -(-w // side) * -(-h // side)
    m = memoryview(encoded).cast("B")
    if len(m) < 16:
        raise ValueError(f"not an encoded scan: {len(m)} bytes are less than the header")
    scan, segments, ri, blocks = struct.unpack("<4I", m[:16])
    if ri != jpeg.restart or segments != -(-mcus // ri) or blocks != mcus * (1 if n == 1 else 6 if sub else 3):
        raise ValueError(f"not the scan of a {w}x{h} image of {bpp} bytes per pixel with {jpeg}: {segments} segments at interval {ri}, {blocks} blocks")
    if scan < segments or 16 + scan > len(m):
        raise ValueError(f"not an encoded scan: length word {scan} in a buffer of {len(m)} bytes")
    out = [b"\xff\xd8", _jpeg_segment(0xE0, b"JFIF\0" + bytes((1, 1, 0, 0, 1, 0, 1, 0, 0)))]
    out += [_jpeg_segment(0xDB, bytes((t,)) + jpeg_quant_table(jpeg.quality, t)) for t in range(2 if n == 3 else 1)]
    comps = b"".join(bytes((i + 1, 0x22 if (sub and i == 0) else 0x11, 1 if i else 0)) for i in range(n))
    out.append(_jpeg_segment(0xC0, struct.pack(">BHHB", 8, h, w, n) + comps))
    for which in range(4 if n == 3 else 2):  # DC 0, AC 0, DC 1, AC 1
        bits, vals = jpeg_huffman_table(which)
        out.append(_jpeg_segment(0xC4, bytes((((which & 1) << 4) | (which >> 1),)) + bits + vals))
    out.append(_jpeg_segment(0xDD, struct.pack(">H", ri)))
    out.append(_jpeg_segment(0xDA, bytes((n,)) + b"".join(bytes((i + 1, 0x11 if i else 0x00)) for i in range(n)) + bytes((0, 63, 0))))
    return b"".join(out) + bytes(m[16:16 + scan]) + b"\xff\xd9"


class AviWriter:
    """A Motion-JPEG AVI file of w x h frames at `frame_rate` frames a second (a number or a Fraction; stored as rate / scale): add(jpeg
    file bytes) per frame, in order, then close().  RIFF 'AVI ': LIST 'hdrl' (avih with the HASINDEX flag; LIST 'strl' of strh - vids /
    MJPG - and strf, a 40-byte BITMAPINFOHEADER of 24 bits, MJPG), LIST 'movi' of 00dc chunks padded to even length, idx1 with 16 bytes
    per frame (keyframe flag, offsets counted from the movi fourcc).  close() patches the sizes and frame counts and appends the index;
    it is safe to call twice, and runs at the end of a `with` block whatever happened inside, so that what was written plays.  OpenDML is
    not written: if a frame would take the file past LIMIT (2^31) bytes, add() closes the file and raises ValueError."""
    LIMIT = 1 << 31
    _MOVI_AT = 220  # of the movi fourcc: 12 RIFF + 12 LIST hdrl + 64 avih + 12 LIST strl + 64 strh + 48 strf + 8 LIST movi

    def __init__(self, path, w, h, frame_rate):
        import fractions
        w, h = int(w), int(h)
        if not (1 <= w <= 65535 and 1 <= h <= 65535):
            raise ValueError(f"an MJPG frame has 1..65535 columns and rows, got {w}x{h}")
        rate = fractions.Fraction(frame_rate).limit_denominator(100000)
        if not (0 < rate and rate.numerator < 1 << 31):
            raise ValueError(f"frame_rate must be positive, got {frame_rate!r}")
        self.path, self.w, self.h, self.rate = path, w, h, rate
        self.frames, self._index, self._largest, self._closed = 0, [], 0, False
        self._f = open(path, "wb")
        self._f.write(self._header())
        self._pos = self._MOVI_AT + 4

    def _header(self, movi_bytes=4, riff_bytes=0):
        n, big = self.frames, self._largest
        usec = round(1000000 / self.rate)
        per_sec = min(int(big * self.rate) + 1, 0xFFFFFFFF) if n else 0
        avih = struct.pack("<14I", usec, per_sec, 0, 0x10, n, 0, 1, big, self.w, self.h, 0, 0, 0, 0)
        strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIII4h", 0, 0, 0, 0, self.rate.denominator, self.rate.numerator, 0, n, big, 0xFFFFFFFF, 0,
                                               0, 0, self.w, self.h)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.w, self.h, 1, 24, b"MJPG", self.w * self.h * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        head = b"RIFF" + struct.pack("<I", riff_bytes) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl + b"LIST" + struct.pack("<I", movi_bytes) + b"movi"
        assert len(head) == self._MOVI_AT + 4
        return head

    def add(self, data):
        if self._closed:
            raise ValueError("the AVI file is closed")
        data = bytes(data)
        padded = len(data) + (len(data) & 1)
        if self._pos + 8 + padded + 8 + 16 * (self.frames + 1) > self.LIMIT:
            self.close()
            raise ValueError(f"frame {self.frames} would take {self.path} past {self.LIMIT} bytes: the file is closed at {self.frames} frames (no OpenDML)")
        self._f.write(b"00dc" + struct.pack("<I", len(data)) + data + b"\0" * (padded - len(data)))
        self._index.append((self._pos - self._MOVI_AT, len(data)))
        self._pos += 8 + padded
        self.frames += 1
        self._largest = max(self._largest, len(data))

    def close(self):
        if self._closed:
            return
        self._closed = True
        try:
            idx = b"".join(b"00dc" + struct.pack("<III", 0x10, at, n) for at, n in self._index)
            self._f.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
            total = self._pos + 8 + len(idx)
            self._f.seek(0)
            self._f.write(self._header(self._pos - self._MOVI_AT, total - 8))
        finally:
            self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
