"""A reader of single-part scanline OpenEXR files with NO or ZIP compression, written from the published file layout alone: it imports
neither tests/exr_np.py nor rayn_amd.  The attributes are parsed generically (name, type, size, value), the offset table is followed, a
chunk whose size equals its raw size is taken as it is, any other goes through zlib.decompress, the inverse predictor and the
interleave.  read(data) -> {name: (h, w) array, rows top-down}: float16 for HALF, float32 for FLOAT, uint32 for UINT; info (optional)
receives what the tests look at.  TEST INFRASTRUCTURE."""
import struct
import zlib

import numpy as np

DTYPES = {0: "<u4", 1: "<f2", 2: "<f4"}
ROWS_PER_CHUNK = {0: 1, 2: 1, 3: 16}  # NONE, ZIPS, ZIP


def _cstring(data, at):
    end = data.index(b"\0", at)
    return data[at:end], end + 1


def parse_header(data):
    """(attributes: name -> (type, value bytes), the offset behind the header)"""
    if data[:4] != b"\x76\x2f\x31\x01":
        raise ValueError("not an OpenEXR file: magic")
    version, = struct.unpack("<I", data[4:8])
    if version & 0xFF != 2 or version >> 8:
        raise ValueError(f"only version 2, single-part scanline files without long names: {version:#x}")
    at, attrs = 8, {}
    while data[at] != 0:
        name, at = _cstring(data, at)
        kind, at = _cstring(data, at)
        size, = struct.unpack("<i", data[at:at + 4])
        attrs[name.decode()] = (kind.decode(), data[at + 4:at + 4 + size])
        at += 4 + size
    return attrs, at + 1


def parse_channels(value):
    out, at = [], 0
    while value[at] != 0:
        name, at = _cstring(value, at)
        if len(name) > 31:
            raise ValueError("long channel name without the long-name flag")
        ptype, plinear, xs, ys = struct.unpack("<iB3xii", value[at:at + 16])
        if (xs, ys) != (1, 1) or ptype not in DTYPES:
            raise ValueError((name, ptype, xs, ys))
        out.append((name.decode(), ptype))
        at += 16
    if at + 1 != len(value):
        raise ValueError("bytes behind the channel list")
    return out


def unzip(payload, n):
    """A ZIP chunk's n raw bytes from its payload"""
    if len(payload) == n:
        return np.frombuffer(payload, np.uint8)
    p = np.frombuffer(zlib.decompress(payload), np.uint8)
    if len(p) != n:
        raise ValueError(f"chunk inflates to {len(p)} bytes, {n} expected")
    t = ((np.cumsum(p.astype(np.int64)) - 128 * np.arange(n)) & 255).astype(np.uint8)  # t[i] = p[i] + t[i-1] - 128
    half = (n + 1) // 2
    raw = np.empty(n, np.uint8)
    raw[0::2], raw[1::2] = t[:half], t[half:]
    return raw


def read(data, info=None):
    data = bytes(data)
    attrs, at = parse_header(data)
    for need, kind in (("channels", "chlist"), ("compression", "compression"), ("dataWindow", "box2i"), ("displayWindow", "box2i"),
                       ("lineOrder", "lineOrder"), ("pixelAspectRatio", "float"), ("screenWindowCenter", "v2f"), ("screenWindowWidth", "float")):
        if need not in attrs or attrs[need][0] != kind:
            raise ValueError(f"required attribute {need} of type {kind} is missing")
    channels = parse_channels(attrs["channels"][1])
    if [n for n, _ in channels] != sorted((n for n, _ in channels), key=lambda s: s.encode()) or len({n for n, _ in channels}) != len(channels):
        raise ValueError("channels are not sorted by name")
    compression = attrs["compression"][1][0]
    if compression not in ROWS_PER_CHUNK or attrs["lineOrder"][1][0] != 0:
        raise ValueError("only NONE, ZIPS and ZIP compression with increasing y")
    x0, y0, x1, y1 = struct.unpack("<iiii", attrs["dataWindow"][1])
    w, h, per = x1 - x0 + 1, y1 - y0 + 1, ROWS_PER_CHUNK[compression]
    chunks = -(-h // per)
    offsets = struct.unpack("<%dQ" % chunks, data[at:at + 8 * chunks])
    row = sum(np.dtype(DTYPES[t]).itemsize for _, t in channels) * w
    planes = {n: np.empty((h, w), DTYPES[t]) for n, t in channels}
    seen = []
    for k, off in enumerate(offsets):
        y, size = struct.unpack("<ii", data[off:off + 8])
        rows = min(per, h - k * per)
        if y != y0 + k * per or size <= 0 or size > row * rows or off + 8 + size > len(data):
            raise ValueError(("chunk", k, y, size, row * rows))
        payload = data[off + 8:off + 8 + size]
        raw = np.frombuffer(payload, np.uint8) if compression == 0 else unzip(payload, row * rows)
        raw = raw.reshape(rows, row)
        col = 0
        for n, t in channels:
            nb = np.dtype(DTYPES[t]).itemsize * w
            planes[n][k * per:k * per + rows] = np.ascontiguousarray(raw[:, col:col + nb]).view(DTYPES[t])
            col += nb
        seen.append((off, y, size, size == row * rows))
    if info is not None:
        info.update(width=w, height=h, channels=channels, chunks=seen, header_bytes=at, attributes=attrs)
    return planes
