"""Film::save_to's per-pixel post-process (src/film.rs:205-378): saturate, gamma 2.2, Color+Background composite,
Color+Alpha RGBA, normal -> RGB, y-flip, 8-bit quantise.  Host-side, after the hot path.  PNG is written with
zlib only (the reference uses the `image` crate); png_from_stream frames a zlib stream made elsewhere, the device encoder's
(Context.png_encode) included.

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
