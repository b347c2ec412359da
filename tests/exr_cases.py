"""The shapes the EXR encoder is tested on, each the smallest that reaches its edge, and their encodings by tests/exr_np.py (cached: the
restatements cost about a quarter of a second per 32 KiB block).  A case is (w, h, channels), channels (name, plane, stride, offset,
type) in the file's order, every plane a uint32 array of w * h * stride words in the film's layout (rows bottom-up).  TEST
INFRASTRUCTURE: nothing under rayn_amd/ imports this."""
import functools

import numpy as np

import exr_np as E

f32 = np.float32


def _bits(a):
    a = np.ascontiguousarray(a, f32).reshape(-1).view(np.uint32).copy()
    a.setflags(write=False)
    return a


def _noisy_ramp(w, h, seed, noise=0.02):
    """A ramp along x and y with a little noise: Huffman blocks with some matches"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    return (x / max(w - 1, 1) + 0.25 * y / max(h - 1, 1) + noise * rng.random((h, w))).astype(f32)


def _rgb(w, h, seed):
    """A stride-3 plane: a smooth gradient, a flat band (runs) and a noisy corner"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    c = np.stack([x / max(w - 1, 1), (y + 1.0) / (h + 1.0), 0.5 + 0.0 * x], axis=-1).astype(f32)
    c[:, w // 2:w // 2 + 6] = f32(0.75)
    c[:max(h // 3, 1), :5] += rng.random((max(h // 3, 1), 5, 3)).astype(f32)
    return c


def _one_half(w, h, seed):
    return w, h, [("Y", _bits(_noisy_ramp(w, h, seed)), 1, 0, E.HALF)]


def _w37(h):
    plane = _bits(_rgb(37, h, 37 + h))
    return 37, h, [(n, plane, 3, k, E.HALF) for k, n in ((2, "B"), (1, "G"), (0, "R"))]


def _mixed():
    """61x20: HALF from a stride-3 plane, FLOAT from offset 3 of a stride-4 plane, UINT from a stride-1 plane"""
    w, h = 61, 20
    rng = np.random.default_rng(61)
    records = rng.standard_normal((h, w, 4)).astype(f32)
    records[..., 3] = np.where(rng.random((h, w)) < 0.3, np.inf, 1.0 + 4.0 * _noisy_ramp(w, h, 5)).astype(f32)
    ids = np.where(np.isinf(records[..., 3]), 0xFFFFFFFF, (np.mgrid[0:h, 0:w][1] // 9)).astype(np.uint32).reshape(-1)
    ids.setflags(write=False)
    return w, h, [("G", _bits(_rgb(w, h, 3)), 3, 1, E.HALF), ("Z", _bits(records), 4, 3, E.FLOAT), ("id", ids, 1, 0, E.UINT)]


def _raw_and_ramp():
    """64x32 FLOAT: the film's top 16 rows - the file's first chunk - are random bits, the 16 below a ramp that changes from row to row"""
    w, h = 64, 32
    rng = np.random.default_rng(64)
    a = np.empty((h, w), np.uint32)
    a[16:] = rng.integers(0, 1 << 32, (16, w), dtype=np.uint64).astype(np.uint32)
    a[:16] = (np.arange(16, dtype=f32)[:, None] + np.zeros((1, w), f32)).view(np.uint32)
    a = a.reshape(-1)
    a.setflags(write=False)
    return w, h, [("Z", a, 1, 0, E.FLOAT)]


BYTE_CASES = {
    "1x1": lambda: _one_half(1, 1, 1),
    "1024x16": lambda: _one_half(1024, 16, 2),    # one chunk of exactly one block
    "1025x16": lambda: _one_half(1025, 16, 3),    # 32 800 bytes: a second block of 32
    "37x1": lambda: _w37(1),
    "37x15": lambda: _w37(15),
    "37x16": lambda: _w37(16),
    "37x17": lambda: _w37(17),                    # two chunks, the last of one row
    "37x33": lambda: _w37(33),                    # three
    "61x20-mixed": _mixed,
    "64x32-raw-and-ramp": _raw_and_ramp,
}
assert E.chunk_bytes(1024, 16, [E.HALF]) == [32768] and E.chunk_bytes(1025, 16, [E.HALF]) == [32800]
assert [E.n_chunks(h) for h in (1, 15, 16, 17, 33)] == [1, 1, 1, 2, 3]


@functools.lru_cache(maxsize=None)
def case(name):
    return BYTE_CASES[name]()


def layout_of(channels):
    return [(s, o, t) for _, _, s, o, t in channels]


@functools.lru_cache(maxsize=None)
def encoded(name, matches):
    """(the buffer the device writes, per-chunk (raw?, payload bytes))"""
    w, h, channels = case(name)
    return E.encode(w, h, [(p, s, o, t) for _, p, s, o, t in channels], matches)


# ---- the conversion sweep: compared as decoded bits -----------------------------------------------------------------------------------------

SWEEP_W = 509


@functools.lru_cache(maxsize=None)
def sweep_words():
    """uint32 bits of float32 inputs: for every non-NaN, finite half of both signs the f32 equal to it, the midpoint to the next magnitude
    and that midpoint -/+ 1 ulp; the zeros, infinities, f32 denormals, the values around 65520, FLT_MAX; NaNs of every kind"""
    hb = np.arange(0x7C00, dtype=np.uint16)
    v = hb.view(np.float16).astype(f32)
    nxt = np.concatenate([v[1:], [f32(65536.0)]]).astype(f32)
    mid = ((v.astype(np.float64) + nxt.astype(np.float64)) / 2).astype(f32)  # exact: 12 significant bits
    mag = np.concatenate([v, mid, np.nextafter(mid, f32(0)), np.nextafter(mid, f32(np.inf))]).astype(f32).view(np.uint32)
    extra = np.array([0x00000000, 0x7F800000, 0x00000001, 0x00400000, 0x007FFFFF, 0x00800000, 0x477FE000, 0x477FEFFF, 0x477FF000, 0x477FF001,
                      0x7F7FFFFF, 0x33000000, 0x33000001, 0x32FFFFFF,
                      0x7FC00000, 0x7FC00001, 0x7F800001, 0x7F801FFF, 0x7F802000, 0x7FA00000, 0x7FFFFFFF, 0x7FBFE000], np.uint32)
    mag = np.concatenate([mag, extra])
    words = np.concatenate([mag, mag | np.uint32(0x80000000)])
    h = -(-len(words) // SWEEP_W)
    out = np.zeros(SWEEP_W * h, np.uint32)
    out[:len(words)] = words
    out.setflags(write=False)
    return out


def sweep_case():
    words = sweep_words()
    return SWEEP_W, len(words) // SWEEP_W, [("Y", words, 1, 0, E.HALF)]
