"""Seeded, named inputs of the ray-generation probe (rayn_hip_probe_raygen), shared by tests/test_raygen.py (the oracle's export against the numpy statement,
what every case measures, which wrong statements it kills) and tests/test_raygen_device.py (the kernels against the oracle's export).
A case: wd (world + camera), p (frame params), tabs (samples_1d, samples_2d, scramble, inverse CDF), tiles [n, 8] uint32 (x0, y0, ew, eh, pool_base,
n_paths, film_base, film_packed), n_pool, kills (raygen_np.MUTANTS it has to tell from the statement), only (None, or the outputs compared).
Geometry cases use the library's own R_d tables, PCG scramble and Blackman-Harris inverse CDF, so they isolate index mistakes; value cases build their
tables here.  TEST INFRASTRUCTURE."""
import functools

import numpy as np

import raygen_np as RN
from common import case as scene_case
from oracle import oracle_py as O
from rayn_amd import params as P

f32 = np.float32
PINHOLE, THIN_LENS, ORTHO = 0, 1, 2
VALUE_TILES = ((1, 2, 7, 5), (9, 3, 4, 9), (14, 1, 6, 11))  # three unequal tiles, 137 pixels, inside a 24 x 20 film
VALUE_FILM = (24, 20)


# ---- building blocks ---------------------------------------------------------------------------------------------------------------------------------
def layout(rects, spp, order=None, packed=False):
    """tile words for rectangles (x0, y0, ew, eh): pool segments back to back in `order` (a permutation of the list positions; default: list order)"""
    n = len(rects)
    order = list(range(n)) if order is None else list(order)
    tiles = np.zeros((n, 8), np.uint32)
    base = film = 0
    for k in order:
        x0, y0, ew, eh = rects[k]
        tiles[k] = (x0, y0, ew, eh, base, ew * eh * spp, film if packed else 0, 1 if packed else 0)
        base += -(-(ew * eh * spp) // 64) * 64
        film += ew * eh
    return tiles, base


def reference_grid(W, H, tw, th):
    """the reference's tile grid, src/film.rs:399-427 (it under-covers a film whose size is no multiple of the tile)"""
    out = []
    for tx in range((W + W % tw) // tw):
        for ty in range((H + H % th) // th):
            x0, y0 = tx * tw, ty * th
            x1, y1 = min(x0 + tw, W), min(y0 + th, H)
            if x1 > x0 and y1 > y0:
                out.append((x0, y0, x1 - x0, y1 - y0))
    return out


def world(W, H, kind=PINHOLE, animated=0, aperture=0.0, vel_scale=1.0):
    """the s0 scene's world with a camera of the given kind; velocities large enough that a few hundredths of a time unit move every parameter visibly"""
    wd, _ = scene_case("s0", W, H, 1, 1)
    c = wd.camera
    c.kind, c.res_w, c.res_h = kind, float(W), float(H)
    c.vfov_or_size = 2.5 if kind == ORTHO else 55.0
    (c.origin.x, c.origin.y, c.origin.z), (c.at.x, c.at.y, c.at.z), (c.up.x, c.up.y, c.up.z) = (0.4, 0.7, 2.6), (0.1, -0.2, 0.0), (0.05, 1.0, -0.1)
    (c.focus.x, c.focus.y, c.focus.z), c.aperture, c.animated = (0.1, -0.1, 0.3), aperture, animated
    v = vel_scale
    (c.origin_vel.x, c.origin_vel.y, c.origin_vel.z), (c.at_vel.x, c.at_vel.y, c.at_vel.z) = (3.0 * v, -2.0 * v, 1.5 * v), (-2.5 * v, 1.0 * v, 2.0 * v)
    (c.up_vel.x, c.up_vel.y, c.up_vel.z), (c.focus_vel.x, c.focus_vel.y, c.focus_vel.z) = (4.0 * v, 0.5 * v, -3.0 * v), (1.0 * v, 2.0 * v, -6.0 * v)
    return wd


def params(W, H, spp, bounces=1, vm=2, time=(0.5, 1.5)):
    assert spp % 4 == 0
    return P.frame_params(W, H, spp // 4, bounces, volume_marches=vm, time_range=time, tile_size=(16, 16))


def library_tables(p, filt=(0, 1.5, 0.0, 0.0)):
    return O.build_tables(4 * p.samples, p.max_bounces, p.volume_marches, p.frame, p.width, p.height, filter_kind=filt[0], filter_radius=filt[1], filter_params=filt[2:])


def random_tables(p, rng):
    """uniform [0, 1) tables and scramble, the library's Blackman-Harris inverse CDF"""
    spp = 4 * p.samples
    n1, n2 = 1 + (p.max_bounces + 1) * (3 + p.volume_marches), 2 + (p.max_bounces + 1) * (12 + 8 * p.volume_marches)
    fis = np.zeros(512, f32)
    O.lib().oracle_build_fis_table_ex(0, 1.5, 0.0, 0.0, O._fp(fis))
    return [rng.random(spp * n1, dtype=f32), rng.random(spp * 2 * n2, dtype=f32), rng.random(p.width * p.height, dtype=f32), fis]


def make(wd, p, tabs, tiles, n_pool, kills, only=None, **extra):
    c = dict(wd=wd, p=p, tabs=tuple(np.ascontiguousarray(t, f32) for t in tabs), tiles=tiles, n_pool=n_pool, kills=tuple(kills), only=only)
    c.update(extra)
    return c


def geometry(W, H, rects, spp, kills, order=None, packed=False, kind=PINHOLE):
    wd, p = world(W, H, kind), params(W, H, spp)
    tiles, n_pool = layout(rects, spp, order, packed)
    return make(wd, p, library_tables(p), tiles, n_pool, kills)


def value_case(spp, kills, seed, kind=PINHOLE, animated=0, aperture=0.0, time=(0.5, 1.5), tweak=None, fis=None, **extra):
    W, H = VALUE_FILM
    wd, p = world(W, H, kind, animated, aperture), params(W, H, spp, time=time)
    rng = np.random.default_rng(seed)
    tabs = random_tables(p, rng)
    if fis is not None:
        tabs[3] = np.asarray(fis, f32)
    tiles, n_pool = layout(VALUE_TILES, spp, order=(2, 0, 1))
    c = make(wd, p, tabs, tiles, n_pool, kills, **extra)
    if tweak:
        tabs = [t.copy() for t in c["tabs"]]
        tweak(c, tabs, rng)
        c["tabs"] = tuple(tabs)
    return c


def tile_pixels(c):
    """film pixel index of every pixel of every tile, tile by tile in the loop's order"""
    W = int(c["p"].width)
    return [np.array([(x0 + lx) + (y0 + ly) * W for lx in range(ew) for ly in range(eh)]) for x0, y0, ew, eh in c["tiles"][:, :4].astype(np.int64).tolist()]


def raygen_slots(c):
    """indices of the five table words ray generation reads for sample s: 1-D set 0; 2-D set 0 and set 1, both dimensions -> function(s) -> (i1, [i2 x 4])"""
    spp = RN.spp_of(c)
    return lambda s: (s, [d + 2 * s + 2 * spp * set_ for set_ in (0, 1) for d in (0, 1)])


# ---- value cases -------------------------------------------------------------------------------------------------------------------------------------
# (name, table value, scramble value): the binary32 sum is exactly 1, the float below 1, above 1, +0, -0, negative, a subnormal, at least 2^23 (the exact sum
# 2^23 + 0.5 rounds to an integer either way), +inf, NaN; and the scramble values 1.0 and the float below 1
FRACT_CLASSES = (("one", 0.75, 0.25), ("below_one", 0.5, 0.5 - 2.0 ** -25), ("above_one", 0.75, 0.75), ("zero", 0.0, 0.0), ("neg_zero", -0.0, -0.0),
                 ("negative", 0.25, -0.75), ("subnormal", 1e-40, 0.0), ("big_even", 2.0 ** 23, 0.5), ("big_odd", 2.0 ** 23 + 1.0, 0.5), ("inf", np.inf, 0.25),
                 ("nan", np.nan, 0.25), ("scr_one", 0.3, 1.0), ("scr_below_one", 0.3, 1.0 - 2.0 ** -24))


def _fract_edges(c, tabs, rng):
    """class k is planted at sample k of all five ray-gen table words, and every third pixel of every tile gets the scramble of a class in turn"""
    at = raygen_slots(c)
    for k, (_n, tv, _sv) in enumerate(FRACT_CLASSES):
        i1, i2 = at(k)
        tabs[0][i1] = f32(tv)
        tabs[1][i2] = f32(tv)
    scrs = []
    for _n, _tv, sv in FRACT_CLASSES:
        if not any(np.array_equal(f32(sv).view(np.uint32), f32(x).view(np.uint32)) for x in scrs):
            scrs.append(sv)
    k = 0
    for px in tile_pixels(c):
        for i in range(0, len(px), 3):
            tabs[2][px[i]] = f32(scrs[k % len(scrs)])
            k += 1


def exact_index_us():
    """u = 0.5 +- h with 2 h a multiple of 2^-23 and the binary32 product (2 h) * 511 an exact integer j in 1..510: the lerp weight t is 0 at index j.
    k / 1022 itself is representable only for k = 0, so the nearest representable h whose rounded product lands on the integer is searched for."""
    us = []
    for j in range(1, 511):
        base = round(j / 511 * 2 ** 23)
        for m in (base - 1, base, base + 1):
            up = f32(m / 2 ** 23)
            if f32(up * f32(511.0)) == f32(j) and f32(f32(0.5) + up / f32(2)) < 1 and f32(f32(2.0) * f32(f32(f32(0.5) + up / f32(2)) - f32(0.5))) == up:
                us += [f32(0.5) + up / f32(2), f32(0.5) - up / f32(2)]
                break
    return np.array(us, f32)


# u exactly 0.5 and its neighbours on both sides, 0 and the float below 1 (index 510 through the clamp), and index 0 on both sides
FIS_FIXED = (0.5, 0.5 - 2.0 ** -25, 0.5 + 2.0 ** -24, 0.0, 1.0 - 2.0 ** -24, 0.5 + 2.0 ** -12, 0.5 - 2.0 ** -12)


def _fis_edges(c, tabs, rng):
    """every second pixel has scramble 0, so its u is the table word itself; the words of 2-D set 0 cycle through the edge values at three samples in four"""
    us = np.concatenate([np.array(FIS_FIXED, f32), exact_index_us()])
    k = 0
    for s in range(RN.spp_of(c)):
        if s % 4 == 3:
            continue
        for d in (0, 1):
            tabs[1][d + 2 * s] = us[k % len(us)]
            k += 1
    for px in tile_pixels(c):
        tabs[2][px[::2]] = f32(0.0)


def custom_fis():
    """512 distinct entries in no order: idx against idx + 1 and a wrong weight both show"""
    return np.random.default_rng(77).permutation(512).astype(f32) / f32(341.0)


def _thin_lens(c, tabs, rng):
    """every fourth pixel has scramble 0 and, at samples 3 and 6, the lens sample (0.5, 0.5): a = b = 0 in concentric_circle_map"""
    spp = RN.spp_of(c)
    for s in (3, 6):
        for d in (0, 1):
            tabs[1][d + 2 * s + 2 * spp * 1] = f32(0.5)
    for px in tile_pixels(c):
        tabs[2][px[::4]] = f32(0.0)


def records_case(vm, bounces):
    """tables whose every entry is its own index; spp 8, one tile of 2 x 3 pixels"""
    W, H, spp = 6, 5, 8
    wd, p = world(W, H), params(W, H, spp, bounces=bounces, vm=vm)
    n1, n2 = 1 + (bounces + 1) * (3 + vm), 2 + (bounces + 1) * (12 + 8 * vm)
    assert spp * 2 * n2 < 2 ** 24
    fis = np.zeros(512, f32)
    O.lib().oracle_build_fis_table_ex(0, 1.5, 0.0, 0.0, O._fp(fis))
    tabs = [np.arange(spp * n1, dtype=f32), np.arange(spp * 2 * n2, dtype=f32), np.random.default_rng(5).random(W * H, dtype=f32), fis]
    tiles, n_pool = layout([(1, 1, 2, 3)], spp)
    return make(wd, p, tabs, tiles, n_pool, ("records_depth_off",) if bounces else ("no_half",), only=("records",) if bounces else None)


ANIM = [("pinhole", PINHOLE, b) for b in (1, 2, 4, 7)] + [("ortho", ORTHO, b) for b in (1, 2, 4, 7)] + [("thin_lens", THIN_LENS, b) for b in (1, 2, 4, 8, 15)]
FILTERS = {"fis_tables_blackman_harris": (0, 1.5, 0.0, 0.0), "fis_tables_box": (1, 0.5, 0.0, 0.0), "fis_tables_mitchell": (2, 2.0, 1.0 / 3.0, 1.0 / 3.0),
           "fis_tables_lanczos": (3, 3.0, 3.0, 0.0)}
RECORDS = [(vm, b) for vm in (2, 3, 4) for b in (0, 1, 8, 120)]  # volume_marches: every value the ABI accepts (2..4; the probe refuses 0, 1 and 5)


def _permuted():
    rects = [(0, 0, 5, 3), (6, 1, 1, 9), (8, 0, 7, 7), (16, 2, 3, 2), (20, 0, 2, 11), (0, 12, 9, 4), (10, 9, 4, 6), (23, 0, 6, 13)]
    order = [int(k) for k in np.random.default_rng(11).permutation(len(rects))]
    return geometry(30, 17, rects, 4, ("pix_transposed", "ew_for_eh"), order=order)


def _fis_table_case(name):
    fis = np.zeros(512, f32)
    O.lib().oracle_build_fis_table_ex(FILTERS[name][0], *[float(v) for v in FILTERS[name][1:]], O._fp(fis))
    return value_case(16, ("no_half",), 31, fis=fis)


BUILDERS = {
    # geometry
    "one_pixel": lambda: geometry(5, 4, [(2, 1, 1, 1)], 4, ("no_half",)),
    "edge_50x37": lambda: geometry(50, 37, reference_grid(50, 37, 16, 16), 4, ("pix_transposed",)),
    "edge_21x13_spp4": lambda: geometry(21, 13, reference_grid(21, 13, 8, 8), 4, ("ew_for_eh", "pix_transposed")),
    "edge_21x13_spp12": lambda: geometry(21, 13, reference_grid(21, 13, 8, 8), 12, ("ew_for_eh", "pix_transposed")),
    "wide_32x4": lambda: geometry(40, 37, [(3, 5, 32, 4)], 4, ("ew_for_eh",)),
    "tall_4x32": lambda: geometry(40, 37, [(7, 2, 4, 32)], 4, ("ew_for_eh",)),
    "permuted": _permuted,
    "many_tiles": lambda: geometry(80, 64, [(2 * i, 2 * j, 2, 2) for i in range(40) for j in range(32)], 4, ("pix_transposed",)),
    "groups_256": lambda: geometry(40, 36, [(5, 3, 32, 32), (0, 0, 2, 1)], 16, ("no_half",)),
    "groups_320": lambda: geometry(40, 36, [(5, 3, 32, 32), (0, 0, 2, 1)], 20, ("no_half",)),
    "groups_1024": lambda: geometry(40, 36, [(5, 3, 32, 32), (0, 0, 2, 1)], 64, ("no_half",)),
    "spp_16384": lambda: geometry(4, 3, [(1, 2, 1, 1), (3, 0, 1, 1)], 16384, ("no_half",)),
    "far_corner": lambda: geometry(8192, 3, [(8187, 0, 5, 3), (4000, 1, 3, 2), (0, 0, 2, 3)], 4, ("pix_transposed",)),
    "far_bottom": lambda: geometry(3, 8192, [(0, 8185, 3, 7), (1, 4000, 2, 3), (0, 0, 3, 2)], 4, ("pix_transposed",)),
    "packed": lambda: geometry(30, 17, [(0, 0, 5, 3), (6, 1, 1, 9), (8, 0, 7, 7)], 8, ("no_half",), order=(1, 2, 0), packed=True),
    # values
    "fract_edges": lambda: value_case(32, ("no_half",), 21, kind=THIN_LENS, animated=15, aperture=0.1, tweak=_fract_edges),
    "fis_edges": lambda: value_case(32, ("clamp_one", "mult_le0"), 22, tweak=_fis_edges, fis=custom_fis()),  # entry 0 of the library's tables is 0: no sign to tell
    "fis_tables_custom": lambda: value_case(16, ("lerp_swapped", "no_half"), 32, fis=custom_fis()),
    "time_static": lambda: value_case(16, ("time_word_lane0",), 41),
    "time_zero_range": lambda: value_case(16, ("no_half",), 42, animated=7, time=(0.75, 0.75)),
    "time_negative_range": lambda: value_case(16, ("own_lane_time", "time_word_lane0"), 43, animated=7, time=(1.5, 0.25)),
    "time_offset": lambda: value_case(16, ("own_lane_time", "time_word_lane0"), 44, animated=7, time=(3.25, 3.5)),
    "thin_lens_sets": lambda: value_case(16, ("lens_set0",), 51, kind=THIN_LENS, aperture=0.2, tweak=_thin_lens),
}
BUILDERS.update({n: (lambda n=n: _fis_table_case(n)) for n in FILTERS})
BUILDERS.update({"anim_%s_%d" % (n, b): (lambda k=k, b=b: value_case(16, ("own_lane_time",), 60 + b, kind=k, animated=b, aperture=0.1 if k == THIN_LENS else 0.0))
                 for n, k, b in ANIM})
BUILDERS.update({"records_vm%d_b%d" % (vm, b): (lambda vm=vm, b=b: records_case(vm, b)) for vm, b in RECORDS})
NAMES = tuple(BUILDERS)
GEOMETRY = NAMES[:15]
VALUES = tuple(n for n in NAMES[15:] if not n.startswith("records_"))
SHARE_MUTANTS = ("own_lane_time", "lens_set0")  # a case that names one of these changes at least 10 % of its paths


@functools.lru_cache(maxsize=None)
def get(name):
    c = BUILDERS[name]()
    c["name"] = name
    return c


@functools.lru_cache(maxsize=None)
def oracle_rays(name, fma):
    """the oracle's export for every tile of a case, computed once and shared"""
    c = get(name)
    out = []
    for x0, y0, ew, eh in c["tiles"][:, :4].astype(np.int64).tolist():
        out.append(O.raygen_tile(c["wd"], c["p"], c["tabs"], x0, y0, x0 + ew, y0 + eh, fma=bool(fma)))
    return tuple(out)


# ---- what a case measures (the tests print and assert these) ---------------------------------------------------------------------------------------------
def measure(c):
    """condition counts over the paths of a case, from its tables alone: per path the five ray-gen sums (1-D set 0; 2-D sets 0 and 1) and the filter's u"""
    spp = RN.spp_of(c)
    s1d, s2d, scr, _ = c["tabs"]
    sums, us = [], []
    for t in range(len(c["tiles"])):
        xs, ys, s = RN.slot_paths(c, t)
        sc = scr[xs + ys * int(c["p"].width)]
        with np.errstate(all="ignore"):
            five = [s1d[s] + sc] + [s2d[d + 2 * s + 2 * spp * set_] + sc for set_ in (0, 1) for d in (0, 1)]
            sums.append(np.stack(five, 1).astype(f32))
            us.append(np.stack([RN.RS.fract(five[1].astype(f32)), RN.RS.fract(five[2].astype(f32))], 1))
    sums, u = np.concatenate(sums), np.concatenate(us)
    with np.errstate(all="ignore"):
        h = np.abs((f32(2.0) * (u - f32(0.5)).astype(f32)).astype(f32))
        h = np.where(h > 0, h, f32(0))
        h = np.where(h < f32(0.99999), h, f32(0.99999)).astype(f32)
        full = (h * f32(511.0)).astype(f32)
    idx = np.floor(full)
    g0, gc = RN.groups_of(c)
    return {"paths": int(sums.shape[0]), "u_half": int((u == 0.5).any(1).sum()), "index_510": int((idx == 510).any(1).sum()), "index_0": int((idx == 0).any(1).sum()),
            "t_zero": int(((full == idx) & (idx > 0)).any(1).sum()), "nan_sums": int(np.isnan(sums).sum()), "inf_sums": int(np.isinf(sums).sum()),
            "sum_one": int((sums == 1).sum()), "sum_negative": int((sums < 0).sum()), "sum_neg_zero": int(((sums == 0) & np.signbit(sums)).sum()),
            "sum_subnormal": int(((np.abs(sums) < 2.0 ** -126) & (sums != 0)).sum()), "sum_big": int((np.abs(sums) >= 2.0 ** 23).sum() - np.isinf(sums).sum()),
            "sum_below_one": int((sums == f32(1.0 - 2.0 ** -24)).sum()), "sum_above_one": int(((sums > 1) & (sums < 2)).sum()),
            "padding_share": round(RN.padding_share(c), 4), "groups_per_tile": (int(gc.min()), int(gc.max())), "tiles": len(c["tiles"])}
