"""Seeded inputs of the film-resolve probe (rayn_hip_probe_resolve), shared by tests/test_resolve.py (the numpy statement against a plain loop, and the
check that every case tells the wrong resolves it names from the right one) and tests/test_resolve_device.py (the kernels).  A case is a dict:
    name, width, spp, tiles [n_tiles, 8] (x0, y0, ew, eh, pool_base, n_paths, film_base, film_packed), max_tile_pixels, n_paths, term_info [n_paths] u8,
    term_key [n_paths] u32, col0 [n_paths, 3] f32, aov [n_paths, 3] f32, obj [n_paths] u32, base_hist [n_depths, hist_stride] u32 or None, hist_stride,
    n_depths, out_pixels, kills (the mutants of resolve_np.MUTANTS whose film must differ from the right one), weak (True: the 80 % rule of
    tests/test_resolve.py cannot hold - the order differs from sample order by ONE transposition, or three pixels in five hold values whose sum has no order).

Unless a builder says otherwise: four tiles of 3x2, 1x5, 5x4 and 4x5 pixels (51 pixels) scattered over a 23x12 film that they do not cover, stored in the
pool in another order than the tile list with unused paths in front and between (those hold contributing 1e30 samples: reading one shows); sample values
sign x 2^U(-12, 12) in every colour and normal channel; objects drawn from OBJECTS (eight of them, 0 and 0xFE included) with 20 % OBJ_NONE; for 512 < spp <= 4096 a base_hist row per depth
(121 of them, stride n_tiles + 3) of random non-zero entries up to 2^32 - 2^25, different per tile and depth, under every slot.

What the shapes are for (rayn_amd/csrc/kernels.hip): launch_resolve changes kernel after 64, 128, 256, 512, 1024, 2048 and 4096 spp; k_resolve_reg<KPL>
holds sample r * 64 + lane in register r, k_resolve_blk<NT, 8> and k_resolve_huge (NT = 1024) sample r * NT + tid: a pair of neighbouring samples can sit
in neighbouring lanes, in lane 63 and lane 0 of the next register / wave (63|64), or in the last thread and thread 0 of the next register (NT - 1 | NT).  The kernels share
bitonic_sort, sum_color_background, aov_keys / aov_sums and block_is_sorted, so the paths that random keys do not take - the sorted shortcut, the general-order
sums, one object per pixel, empty pixels - also run at the instantiations FAMILY_SPP leaves out (BOUNDARY_SPP).

The statement of the largest case (51 pixels x 4400 spp) takes about 0.1 s on one CPU core."""
import functools

import numpy as np

from resolve_np import OBJ_NONE, TERM_NONE

WIDTH, HEIGHT = 23, 12
STD_TILES = ((1, 1, 3, 2), (7, 0, 1, 5), (10, 6, 5, 4), (17, 2, 4, 5))  # x0, y0, ew, eh
POOL_ORDER = (2, 0, 3, 1)
SPP_GRID = (4, 12, 64, 68, 128, 132, 256, 260, 512, 516, 600, 1024, 1028, 1600, 2048, 2052, 2800, 4096, 4100, 4400, 16384)
FAMILY_SPP = (256, 1024, 4096, 4400)  # reg<4>, blk<128>, blk<512>, huge
BOUNDARY_SPP = (64, 128, 512, 2048)  # reg<1>, reg<2>, reg<8>, blk<256> at their upper launch boundary: the smallest shapes that use every register
N_DEPTHS = 121
OBJECTS = (0, 1, 3, 7, 0x20, 0x7F, 0x80, 0xFE)  # the default mix
BOUNCES = 16


def is_blk(spp):
    return 512 < spp <= 4096


def block_threads(spp):
    """NT of the kernel that serves spp (the r * NT register boundary); 64 for the one-wave kernels"""
    return 64 if spp <= 512 else 128 if spp <= 1024 else 256 if spp <= 2048 else 512 if spp <= 4096 else 1024


def values(rng, shape):
    """sign x 2^U(-12, 12)"""
    return (rng.choice((-1.0, 1.0), shape) * np.exp2(rng.uniform(-12.0, 12.0, shape))).astype(np.float32)


def distinct_slots(rng, npix, spp, span):
    """[npix, spp] distinct offsets per pixel in [0, span), in random order"""
    step = span // spp
    perm = np.argsort(rng.random((npix, spp)), axis=1).astype(np.uint64)
    return perm * np.uint64(step) + rng.integers(0, step, (npix, spp)).astype(np.uint64)


class Layout:
    """tiles + pool placement; per-pixel arrays are [npix, spp] in tile_pixels order and are scattered into the pool by finish()"""

    def __init__(self, spp, rects=STD_TILES, order=None, width=WIDTH, height=HEIGHT, packed=False, max_tile_pixels=None, seed=0):
        self.spp, self.width, self.rects = spp, width, rects
        order = (POOL_ORDER if len(rects) == 4 else tuple(reversed(range(len(rects))))) if order is None else order
        base, at = {}, 4
        for t in order:
            base[t] = at
            at += rects[t][2] * rects[t][3] * spp + 8
        self.n_paths = at
        film_base, tiles = 0, []
        for t, (x0, y0, ew, eh) in enumerate(rects):
            tiles.append((x0, y0, ew, eh, base[t], ew * eh * spp, film_base, int(packed)))
            film_base += ew * eh
        self.tiles = np.array(tiles, np.uint32)
        self.npix = film_base
        self.out_pixels = self.npix if packed else width * height
        self.max_tile_pixels = max(r[2] * r[3] for r in rects) if max_tile_pixels is None else max_tile_pixels
        self.tile_of = np.repeat(np.arange(len(rects)), [r[2] * r[3] for r in rects])
        self.first = np.concatenate([base[t] + np.arange(r[2] * r[3]) * spp for t, r in enumerate(rects)])
        self.idx = self.first[:, None] + np.arange(spp)[None, :]
        self.rng = np.random.default_rng(seed)
        if is_blk(spp):
            self.hist_stride = len(rects) + 3
            self.base_hist = self.rng.integers(1, (1 << 32) - (1 << 25), (N_DEPTHS, self.hist_stride), dtype=np.uint64).astype(np.uint32)
        else:
            self.hist_stride, self.base_hist = 0, None

    def slots(self, depth, offs):
        """termination slot = the tile's base_hist entry of that depth + offset (no base outside the blk range)"""
        if self.base_hist is None:
            return offs.astype(np.uint32)
        return (self.base_hist[depth.astype(np.int64), self.tile_of[:, None]].astype(np.uint64) + offs.astype(np.uint64)).astype(np.uint32)

    def default_objects(self):
        obj = self.rng.choice(np.array(OBJECTS, np.uint32), (self.npix, self.spp))
        obj[self.rng.random((self.npix, self.spp)) < 0.2] = OBJ_NONE
        return obj

    def finish(self, name, depth, bg, none, offs, kills, obj=None, col=None, aov=None, weak=False):
        """depth / bg / none / offs [npix, spp]: depth, Background flag, TERM_NONE mask, slot offset of every sample"""
        spp, n = self.spp, self.n_paths
        info = (depth.astype(np.uint8) | (bg.astype(np.uint8) << 7))
        info[none] = TERM_NONE
        slot = self.slots(np.where(none, 0, depth), offs)
        term_info, term_key = np.full(n, 0x01, np.uint8), np.zeros(n, np.uint32)  # unused paths: contributing, depth 1, slot 0
        c0, av, ob = np.full((n, 3), 1e30, np.float32), np.full((n, 3), 1e30, np.float32), np.zeros(n, np.uint32)
        term_info[self.idx], term_key[self.idx] = info, slot
        c0[self.idx] = values(self.rng, (self.npix, spp, 3)) if col is None else col
        av[self.idx] = values(self.rng, (self.npix, spp, 3)) if aov is None else aov
        ob[self.idx] = self.default_objects() if obj is None else obj
        return {"name": name, "width": self.width, "spp": spp, "tiles": self.tiles, "max_tile_pixels": self.max_tile_pixels, "n_paths": n,
                "term_info": term_info, "term_key": term_key, "col0": c0, "aov": av, "obj": ob, "base_hist": self.base_hist,
                "hist_stride": self.hist_stride, "n_depths": N_DEPTHS, "out_pixels": self.out_pixels, "kills": tuple(kills), "weak": weak}


SPAN = 1 << 22       # offsets of an ordinary case: what a 1024-pixel tile at 4096 spp spans
FALSE = lambda L: np.zeros((L.npix, L.spp), bool)
ALL_ORDER = ("sample_order", "slot_major", "normal_sample_order")


def _kills(spp, *names):
    """signed_key32 only means something where the 32-bit key runs"""
    return tuple(k for k in names if k != "signed_key32" or is_blk(spp))


# ---- key patterns ------------------------------------------------------------------------------------------------------------------------------------
def k_random(name, spp, seed, bounces=BOUNCES, none_frac=0.0, **kw):
    """random depths 0..bounces (depth 0 = Background, as the renderer emits it) with random distinct slots"""
    L = Layout(spp, seed=seed, **kw)
    depth = L.rng.integers(0, bounces + 1, (L.npix, spp))
    none = L.rng.random((L.npix, spp)) < none_frac
    return L.finish(name, depth, depth == 0, none, distinct_slots(L.rng, L.npix, spp, SPAN), ALL_ORDER + ("ignore_bg", "swap_lx_ly"))


def k_reversed(name, spp, seed):
    """one depth, slots descending in sample order: the order is the full reversal"""
    L = Layout(spp, seed=seed)
    offs = np.broadcast_to((spp - 1 - np.arange(spp)) * 3 + 1, (L.npix, spp))
    return L.finish(name, np.ones((L.npix, spp), np.int64), FALSE(L), FALSE(L), offs, ("sample_order", "normal_sample_order", "swap_lx_ly"))


def k_sorted_sky(name, spp, seed):
    """sky only: depth 0, all Background, slots ascending in sample order - the sortedness shortcut and the all-prefix split"""
    L = Layout(spp, seed=seed)
    offs = np.cumsum(L.rng.integers(1, 5, (L.npix, spp)), axis=1)
    return L.finish(name, np.zeros((L.npix, spp), np.int64), ~FALSE(L), FALSE(L), offs, ("ignore_bg", "normal_sample_order", "swap_lx_ly"))


def k_pair(name, spp, seed, at):
    """sorted, except that samples at and at + 1 are exchanged; even pixels Background at depth 0, odd ones Color at depth 2.  A chain of a thousand terms
    forgets in which order two early ones came (the later, larger partial sums round the difference away), so two pixels in three drop every sample
    after the first at + 2 + pixel % 4 (TERM_NONE at the end leaves the rest sorted), and the exchanged pair holds values of opposite sign from the top
    of the range, sign x 2^U(11, 12): the partial sum before them is lost differently in the two orders, in about every second channel."""
    L = Layout(spp, seed=seed)
    offs = np.cumsum(L.rng.integers(1, 5, (L.npix, spp)), axis=1)
    offs[:, [at, at + 1]] = offs[:, [at + 1, at]]
    p = np.arange(L.npix)
    sky = np.broadcast_to((p % 2 == 0)[:, None], (L.npix, spp))
    none = (p % 3 != 0)[:, None] & (np.arange(spp)[None, :] >= (at + 2 + p % 4)[:, None])
    col = values(L.rng, (L.npix, spp, 3))
    top = np.exp2(L.rng.uniform(11.0, 12.0, (L.npix, 2, 3))).astype(np.float32)
    col[:, at], col[:, at + 1] = top[:, 0], -top[:, 1]
    return L.finish(name, np.where(sky, 0, 2), sky, none, offs, ("sample_order", "ignore_bg"), col=col, weak=True)


def k_deep(name, spp, seed):
    """depths from {0, 63, 64, 119, 120}: bit 31 of the 32-bit key is set from depth 64 on"""
    L = Layout(spp, seed=seed)
    depth = L.rng.choice(np.array((0, 63, 64, 119, 120)), (L.npix, spp))
    return L.finish(name, depth, depth == 0, FALSE(L), distinct_slots(L.rng, L.npix, spp, SPAN), _kills(spp, "signed_key32", *ALL_ORDER, "ignore_bg"))


def k_slot_bit31(name, spp, seed):
    """slots over all 32 bits (reg, huge: the slot << 13 / slot << 15 fields)"""
    assert not is_blk(spp)
    L = Layout(spp, seed=seed)
    depth = L.rng.integers(0, BOUNCES + 1, (L.npix, spp))
    offs = distinct_slots(L.rng, L.npix, spp, 1 << 32)  # about half of them with bit 31
    offs[np.arange(L.npix), offs.argmin(axis=1)], offs[np.arange(L.npix), offs.argmax(axis=1)] = 0, 0xFFFFFFFF
    return L.finish(name, depth, depth == 0, FALSE(L), offs, ALL_ORDER)


def k_offset_top(name, spp, seed):
    """blk: offsets over all 25 bits, with 0 and 2^25 - 1 in every pixel, above base_hist entries that differ per tile and depth"""
    assert is_blk(spp)
    L = Layout(spp, seed=seed)
    depth = L.rng.integers(0, BOUNCES + 1, (L.npix, spp))
    offs = distinct_slots(L.rng, L.npix, spp, 1 << 25)
    # the sample holding the smallest / largest offset of its pixel moves to the very ends of the field
    lo, hi = offs.argmin(axis=1), offs.argmax(axis=1)
    offs[np.arange(L.npix), lo], offs[np.arange(L.npix), hi] = 0, (1 << 25) - 1
    return L.finish(name, depth, depth == 0, FALSE(L), offs, _kills(spp, *ALL_ORDER))


def k_empty(name, spp, seed):
    """per tile: pixel 0 has no contributing sample, pixel 1 no depth-0 object, pixel 2 neither"""
    L = Layout(spp, seed=seed)
    depth = L.rng.integers(0, BOUNCES + 1, (L.npix, spp))
    none, obj = FALSE(L), L.default_objects()
    lp = np.concatenate([np.arange(r[2] * r[3]) for r in L.rects])
    none[(lp == 0) | (lp == 2)] = True
    obj[(lp == 1) | (lp == 2)] = OBJ_NONE
    return L.finish(name, depth, depth == 0, none, distinct_slots(L.rng, L.npix, spp, SPAN), ALL_ORDER, obj=obj)


def k_mixed0(name, spp, seed):
    """max_bounces = 0: Color and Background both at depth 0, interleaved in slot order - the flag-per-term path"""
    L = Layout(spp, seed=seed)
    bg = L.rng.random((L.npix, spp)) < 0.5
    return L.finish(name, np.zeros((L.npix, spp), np.int64), bg, FALSE(L), distinct_slots(L.rng, L.npix, spp, SPAN), ("sample_order", "ignore_bg", "normal_sample_order"))


# ---- object patterns ---------------------------------------------------------------------------------------------------------------------------------
def k_objects(name, spp, seed, pattern):
    L = Layout(spp, seed=seed)
    i = np.arange(spp)
    if pattern == "one":  # every sample hits object 0: the sortedness shortcut of the Alpha / WorldNormal keys
        row, kills = np.zeros(spp, np.uint32), ()
    elif pattern == "interleaved":
        row, kills = np.array((0, 3, 0xFE), np.uint32)[i % 3], ("normal_sample_order",)
    else:  # descending by sample, through all of 0xFE..0
        row, kills = (0xFE - (i * 0xFF) // spp).astype(np.uint32), ("normal_sample_order",)
    depth = L.rng.integers(0, BOUNCES + 1, (L.npix, spp))
    return L.finish(name, depth, depth == 0, FALSE(L), distinct_slots(L.rng, L.npix, spp, SPAN), kills + ("sample_order",), obj=np.broadcast_to(row, (L.npix, spp)))


# ---- value edges -------------------------------------------------------------------------------------------------------------------------------------
def k_values(name, spp, seed):
    """pixel % 5: 0 only -0.0; 1 only subnormals whose sum stays subnormal; 2 +Inf, later in the order -Inf; 3 one NaN; 4 ordinary values"""
    L = Layout(spp, seed=seed)
    depth = L.rng.integers(0, BOUNCES + 1, (L.npix, spp))
    offs = distinct_slots(L.rng, L.npix, spp, SPAN)
    col, aov = values(L.rng, (L.npix, spp, 3)), values(L.rng, (L.npix, spp, 3))
    kind = np.arange(L.npix) % 5
    sub = lambda: (L.rng.choice((-1, 1), (L.npix, spp, 3)) * L.rng.integers(1, 1025, (L.npix, spp, 3))).astype(np.float64) * 2.0 ** -149  # |sum| <= 4400 * 1024 * 2^-149 < 2^-126
    for a in (col, aov):
        a[kind == 0] = -0.0
        a[kind == 1] = sub().astype(np.float32)[kind == 1]
        for p in np.flatnonzero((kind == 2) | (kind == 3)):
            s = np.sort(L.rng.choice(spp, 2, replace=False))
            if kind[p] == 2:
                a[p, s[0]], a[p, s[1]] = np.inf, -np.inf
            else:
                a[p, s[0], L.rng.integers(0, 3)] = np.nan
    obj = L.default_objects()
    for p in np.flatnonzero(kind == 2):  # both infinities land in the same sums, +Inf first: Color (depth 1, smaller slot) and the normal of object 3 (smaller sample)
        s = np.flatnonzero(np.isinf(col[p, :, 0]))
        depth[p, s] = 1
        offs[p, s] = np.sort(offs[p, s])
        obj[p, np.flatnonzero(np.isinf(aov[p, :, 0]))] = 3
    return L.finish(name, depth, depth == 0, FALSE(L), offs, ("flush_subnormals", "sample_order"), obj=obj, col=col, aov=aov, weak=True)


# ---- geometry ----------------------------------------------------------------------------------------------------------------------------------------
def k_tile1024(name, seed):
    """a 32x32 tile (lpix / eh with eh = 32, 1024 blocks in x) beside a 3x2 and a 1x5 one, at spp 4"""
    rects = ((5, 3, 32, 32), (0, 0, 3, 2), (40, 1, 1, 5))
    return k_random(name, 4, seed, bounces=2, rects=rects, width=44, height=36)


def k_wide_grid(name, spp, seed):
    """a 5x3 tile (ew != eh) among the others, launched with 1024 blocks in x: all but 15 / 6 / 5 / 24 of a row exit at once"""
    rects = ((2, 7, 5, 3), (1, 1, 3, 2), (9, 0, 1, 5), (14, 3, 4, 6))
    return k_random(name, spp, seed, rects=rects, max_tile_pixels=1024)


def k_packed(name, spp, seed):
    """film_packed tiles: planes of the tiles' own pixel count, film_base = the pixels of the tiles before"""
    c = k_random(name, spp, seed, packed=True)
    c["kills"] = tuple(k for k in c["kills"] if k != "swap_lx_ly")  # a packed tile has no lx / ly
    return c


def k_spp(spp):
    if spp == 16384:  # 8 pixels: 8 x 16384 paths is the largest input
        return k_random("spp16384", spp, 16384, none_frac=0.1, rects=((1, 1, 2, 2), (7, 0, 1, 3), (10, 6, 1, 1)))
    return k_random("spp%d" % spp, spp, spp, none_frac=0.1)


@functools.lru_cache(maxsize=None)
def builders():
    """name -> zero-argument builder, in a fixed order"""
    B = {}
    for spp in SPP_GRID:
        B["spp%d" % spp] = functools.partial(k_spp, spp)
    for f, spp in enumerate(FAMILY_SPP):
        s = 1000 * (f + 1)
        nt = block_threads(spp)
        B["random_%d" % spp] = functools.partial(k_random, "random_%d" % spp, spp, s + 1)
        B["reversed_%d" % spp] = functools.partial(k_reversed, "reversed_%d" % spp, spp, s + 2)
        B["sorted_sky_%d" % spp] = functools.partial(k_sorted_sky, "sorted_sky_%d" % spp, spp, s + 3)
        B["pair_lane_%d" % spp] = functools.partial(k_pair, "pair_lane_%d" % spp, spp, s + 4, 37)
        B["pair_wave_%d" % spp] = functools.partial(k_pair, "pair_wave_%d" % spp, spp, s + 5, 63)
        if nt > 64:
            B["pair_reg_%d" % spp] = functools.partial(k_pair, "pair_reg_%d" % spp, spp, s + 6, nt - 1)
        B["deep_%d" % spp] = functools.partial(k_deep, "deep_%d" % spp, spp, s + 7)
        if is_blk(spp):
            B["offset_top_%d" % spp] = functools.partial(k_offset_top, "offset_top_%d" % spp, spp, s + 8)
        else:
            B["slot_bit31_%d" % spp] = functools.partial(k_slot_bit31, "slot_bit31_%d" % spp, spp, s + 8)
        B["none30_%d" % spp] = functools.partial(k_random, "none30_%d" % spp, spp, s + 9, none_frac=0.3)
        B["empty_%d" % spp] = functools.partial(k_empty, "empty_%d" % spp, spp, s + 10)
        B["mixed0_%d" % spp] = functools.partial(k_mixed0, "mixed0_%d" % spp, spp, s + 11)
        for j, pat in enumerate(("one", "interleaved", "descending")):
            B["obj_%s_%d" % (pat, spp)] = functools.partial(k_objects, "obj_%s_%d" % (pat, spp), spp, s + 12 + j, pat)
        B["values_%d" % spp] = functools.partial(k_values, "values_%d" % spp, spp, s + 15)
        B["wide_grid_%d" % spp] = functools.partial(k_wide_grid, "wide_grid_%d" % spp, spp, s + 16)
        B["packed_%d" % spp] = functools.partial(k_packed, "packed_%d" % spp, spp, s + 17)
    for spp in BOUNDARY_SPP:  # the non-random paths at the instantiations FAMILY_SPP leaves out
        B["mixed0_%d" % spp] = functools.partial(k_mixed0, "mixed0_%d" % spp, spp, 9000 + spp)
        B["sorted_sky_%d" % spp] = functools.partial(k_sorted_sky, "sorted_sky_%d" % spp, spp, 9100 + spp)
        B["obj_one_%d" % spp] = functools.partial(k_objects, "obj_one_%d" % spp, spp, 9200 + spp, "one")
        B["empty_%d" % spp] = functools.partial(k_empty, "empty_%d" % spp, spp, 9300 + spp)
    B["tile1024_spp4"] =functools.partial(k_tile1024, "tile1024_spp4", 77)
    B["uncovered_256"] = functools.partial(k_random, "uncovered_256", 256, 78)
    return B


NAMES = tuple(builders())


@functools.lru_cache(maxsize=None)
def get(name):
    """the case, built once per process"""
    return builders()[name]()
