"""Named cases of the baseline JPEG encoder, each with what it must reach on the restatement (tests/jpeg_np.py): cases() builds them
once - images, parameters, the restatement's Encoded - and asserts every case's claim.  tests/test_jpeg.py runs them on the CPU against
libjpeg, tests/test_jpeg_device.py on the GPU against the restatement.  mutant_kills() shows that each planted mutant of MUTANTS (the first six of jpeg_np.MUTANTS) is
told from the real thing by at least one case.  TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this."""
import functools

import numpy as np

import jpeg_np as J

SIZES = [(1, 1), (8, 8), (9, 8), (8, 9), (17, 33), (31, 16)]  # (width, height): padding on either axis, an odd number of MCUs in 4:2:0
MODES = [("grey", 1, 0), ("444", 3, 0), ("420", 3, 1)]        # (name, bytes per pixel, subsampling)


def _smooth(w, h, bpp):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(x * (5 + 3 * c) + y * (7 - 2 * c) + 40 * c) % 256 for c in range(bpp)], -1).astype(np.uint8)


def _noise(w, h, bpp, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, bpp), dtype=np.uint8)


def _segments_with_stuffing_inside(e):
    return [s for s in e.segment_bytes if b"\xff\x00" in s[:-2]]


def _search_blocks():
    """Grey 8x8 blocks of seeded noise whose transform sits on the edges of the two roundings, at quality 100 (Q = 1): a coefficient exactly
    on a quantiser tie, and negative row sums S with S + 1024 one below, on and one above a multiple of 2048"""
    strip = _noise(8 * 4096, 8, 1, 1234)
    F, S = J.transform(strip[..., 0].astype(np.int64))
    F, S = F[0], S[0]  # [block, v, u], [block, y, u]
    tie = np.flatnonzero((np.abs(F) % 32768 == 16384).any(axis=(1, 2)))
    neg = S + 1024 < 0
    picks = [tie[0]] + [np.flatnonzero((neg & ((S + 1024) % 2048 == r)).any(axis=(1, 2)))[0] for r in (2047, 0, 1)]
    return np.concatenate([strip[:, 8 * b:8 * b + 8] for b in picks], axis=1)


def _search_padded_ff():
    """The first seeded 8x8 grey noise block at quality 50 whose only segment ends in padding bits and in the byte FF"""
    for seed in range(2000):
        img = _noise(8, 8, 1, seed)
        e = J.encode(img, 50, 0, 1)
        if e.pad_bits and e.segment_bytes[-1].endswith(b"\xff\x00"):
            return img
    raise AssertionError("no padded FF found")


@functools.lru_cache(None)
def _definitions():
    """[(name, image, quality, subsampling, restart interval, claim)]: claim(e) is what the case must reach"""
    out = []
    for w, h in SIZES:
        for mode, bpp, sub in MODES:
            side = 16 if sub else 8
            mcus = -(-w // side) * -(-h // side)
            out.append((f"size_{w}x{h}_{mode}", _smooth(w, h, bpp), 75, sub, 2, lambda e, mcus=mcus: e.mcus == mcus))
    out.append(("ri_1", _noise(24, 16, 3, 1), 75, 0, 1, lambda e: e.segments == e.mcus == 6))
    out.append(("ri_total_minus_1", _noise(24, 16, 3, 2), 75, 0, 5, lambda e: e.segments == 2 and e.mcus == 6))
    out.append(("ri_above_total", _noise(24, 16, 3, 3), 75, 0, 65535, lambda e: e.segments == 1 and b"\xff\xd0" not in e.scan))
    out.append(("rst_wraps", _noise(88, 16, 1, 4), 60, 0, 1, lambda e: e.segments == 22 and b"\xff\xd7" in e.scan and e.scan.count(b"\xff\xd0") >= 2))
    out.append(("layout_257_segments", _smooth(2056, 8, 1), 50, 0, 1, lambda e: e.segments == 257))
    for q in (1, 49, 50, 100):
        claim = {1: lambda e: e.Q[0].max() == 255 and e.Q[1].min() == 255, 49: lambda e: e.Q[0][0] == (16 * 102 + 50) // 100,
                 50: lambda e: e.Q[0][0] == 16, 100: lambda e: all((Q == 1).all() for Q in e.Q)}[q]
        out.append((f"quality_{q}", _noise(17, 9, 3, 10 + q), q, 1, 3, claim))
    y, x = np.mgrid[0:8, 0:8]
    checker = (((x + y) & 1) * 255).astype(np.uint8)[..., None]
    out.append(("checkerboard", checker, 10, 0, 1, lambda e: e.coef[0][63] != 0 and e.stats[0][2] >= 1 and not e.stats[0][3]))
    stripes = np.zeros((8, 64, 1), np.uint8)
    stripes[:, 8:16] = stripes[:, 24:32] = stripes[:, 40:48] = 255
    out.append(("dc_category_11", stripes, 100, 0, 65535,
                lambda e: [s[0] for s in e.stats[:7]] == [11] * 7 and {int(e.coef[k][0]) - int(e.coef[k - 1][0]) for k in (1, 2)} == {2040, -2040}))
    out.append(("padded_ff", _search_padded_ff(), 50, 0, 1, lambda e: e.pad_bits > 0 and e.scan.endswith(b"\xff\x00")))
    out.append(("ff_inside", _noise(40, 24, 3, 7), 100, 0, 4, lambda e: len(_segments_with_stuffing_inside(e)) >= 1))
    out.append(("rounding_edges", _search_blocks(), 100, 0, 3, _rounding_claim))
    out.append(("flat", np.full((9, 20, 3), 200, np.uint8), 90, 1, 1, lambda e: all(s[3] for s in e.stats) and not (e.coef[:, 1:] != 0).any()))
    out.append(("all_zero", np.zeros((16, 16, 3), np.uint8), 90, 0, 3, lambda e: (e.planes[0] == 0).all() and int(e.coef[0][0]) < 0 and not (e.coef[:, 1:] != 0).any()))
    out.append(("noise_q100", _noise(48, 40, 3, 99), 100, 0, 7, lambda e: len(e.scan) > 48 * 40 * 3))
    # segments beyond the 256 blocks a workgroup takes at a time: exactly one tile, one block more, three tiles, and in 4:2:0 a segment
    # of 258 blocks in front of a short one
    out.append(("segment_256_blocks", _noise(2048, 8, 1, 20), 50, 0, 256, lambda e: e.segments == 1 and e.blocks == 256))
    out.append(("segment_257_blocks", _noise(2056, 8, 1, 21), 50, 0, 65535, lambda e: e.segments == 1 and e.blocks == 257))
    out.append(("segment_600_blocks", _noise(4800, 8, 1, 22), 75, 0, 65535, lambda e: e.blocks / e.segments == 600 > 2 * 256))
    out.append(("segment_258_blocks_420", _noise(800, 16, 3, 23), 75, 1, 43,
                lambda e: e.segments == 2 and e.ri * 6 == 258 > 256 and e.blocks == 300 and e.mcus == 50))
    return out


def _rounding_claim(e):
    F, S = e.F[0][0], e.S[0][0]
    on = lambda b, r: bool(((S[b] + 1024 < 0) & ((S[b] + 1024) % 2048 == r)).any())
    return bool((np.abs(F[0]) % 32768 == 16384).any()) and on(1, 2047) and on(2, 0) and on(3, 1)


class Case:
    def __init__(self, name, img, quality, subsampling, ri, claim):
        self.name, self.img, self.quality, self.subsampling, self.ri = name, img, quality, subsampling, ri
        self.height, self.width, self.bpp = img.shape
        self.ref = J.encode(img, quality, subsampling, ri)
        assert claim(self.ref), f"case {name} does not reach what it is for"

    def mutant(self, m):
        return J.encode(self.img, self.quality, self.subsampling, self.ri, mutant=m)


@functools.lru_cache(None)
def cases():
    """{name: Case}, built once: the restatement's output is the reference every test shares"""
    out = {}
    for d in _definitions():
        assert d[0] not in out, d[0]
        out[d[0]] = Case(*d)
    return out


NAMES = [d[0] for d in _definitions()]
# the mutants these cases are held against; tests/jpeg_edge_cases.py has the cases for the rest of jpeg_np.MUTANTS
MUTANTS = ("row_truncates", "ties_toward_zero", "predictor_kept", "marker_unwrapped", "eob_always", "pad_zero")


@functools.lru_cache(None)
def mutant_kills():
    """{mutant: [names of the cases whose scan it changes]}"""
    return {m: [n for n, c in cases().items() if c.mutant(m).scan != c.ref.scan] for m in MUTANTS}
