"""The progressive, a-trous and display kernels at their decision edges: named cases, each the inputs, the pixels or tiles under test, the
outcome written out by hand and `kills`, the mutants of the restatements ("P:e_ge": progressive_np's; D denoise_np, V denoise_variance_np,
TV temporal_variance_np, X display_np) whose result differs from the statement's on something under test - "at the bound, one ulp
inside, one ulp outside" wherever a comparison has two sides.  Everything that is not under test is a control with the ordinary outcome.

The progressive set-up is exact: epoch 1 is an all-zero film and epoch 2 a gray of luminance Y (a power of two, which the luminance
expression reproduces exactly), so with noise_floor = 0 the pixel has m2 = Y^2 / 2, se = Y / 2, mean = Y / 2 and e = 1.0f exactly.  A
control pixel holds the gray 0.25 in both epochs: m2 = 0 and e = 0.

tests/test_post_edge_cases.py holds all of this to account without a GPU; tests/test_post_edges_device.py pushes every case through every
kernel entry it applies to.  TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this."""
import numpy as np

import denoise_np as DN
import denoise_variance_np as VN
import display_np as X
import progressive_np as PN
import temporal_feedback_np as TF
import temporal_np as T
import temporal_variance_np as TV
from common import above, below

f32 = np.float32
INF, NAN = f32(np.inf), f32(np.nan)
FMAX = np.finfo(f32).max
DENORM = f32(1e-45)  # the smallest denormal
MISS = T.MISS
MODULES = {"P": PN, "D": DN, "V": VN, "TV": TV, "X": X}


class Case:
    def __init__(self, name, family, kills, **fields):
        self.name, self.family, self.kills = name, family, tuple(kills)
        self.__dict__.update(fields)

    def __repr__(self):
        return self.name


def bits(v):
    return int(np.asarray(v, f32).reshape(1).view(np.uint32)[0])


# ---- progressive ---------------------------------------------------------------------------------------------------------------------------
ONE, ZERO, NAN0, EINF, ENAN = "one", "zero", "nan0", "inf", "nan"  # the pixel classes of the exact set-up, by their e after two epochs
GRAY = {ONE: (0.0, 1.0), ZERO: (0.25, 0.25), NAN0: (0.0, 0.0), EINF: (0.0, 2.0 ** 127), ENAN: (0.0, np.inf)}  # (epoch 1, epoch 2)


def gray_film(w, h, gray, seed=0):
    """a film whose Color is the gray `gray` (n,) and whose Background is zero: the luminance of a power of two is that power of two"""
    rng = np.random.default_rng(seed)
    n = w * h
    g = np.asarray(gray, f32).reshape(n)
    return {"color": np.repeat(g[:, None], 3, axis=1).copy(), "alpha": rng.choice(np.array([0.0, 0.25, 1.0], f32), n),
            "background": np.zeros((n, 3), f32), "normal": rng.normal(size=(n, 3)).astype(f32)}


def two_epochs(w, h, classes, seed=0):
    """the two films of the exact set-up: classes (n,) of ONE / ZERO / ..."""
    g = np.array([GRAY[c] for c in classes], f32)
    return [gray_film(w, h, g[:, 0], seed), gray_film(w, h, g[:, 1], seed + 1)]


def _tile_pixels(w, h, tile, k):
    return PN.State(w, h, tile).pixels_of(k)


def _prog(name, kills, w, h, tile, films, params, expect, pixels, init=None, tiles=None, **more):
    """films: one per accumulate call; tiles: the list of every call (None = all); init: None (the reset entry) or a function that
    returns the PN.State before the first call; expect: {tile: (epochs, retired, outliers, max_e)}; pixels: the crafted film pixels"""
    kw = dict(target_error=0.5, noise_floor=0.0, min_epochs=2, outlier_permille=50, adaptive=True)
    kw.update(params)
    return Case("progressive/" + name, "progressive", kills, w=w, h=h, tile=tile, films=films, params=kw, expect=expect,
                pixels=np.asarray(pixels, np.int64), init=init, tiles=tiles, **more)


def run_progressive(c, mutant=None, on_step=None):
    """the case through progressive_np: the PN.State after the last call (on_step(state, film, i) after every call)"""
    st = PN.State(c.w, c.h, c.tile) if c.init is None else c.init()
    for i, film in enumerate(c.films):
        PN.accumulate(st, film, c.tiles, mutant=mutant, **c.params)
        if on_step is not None:
            on_step(st, film, i)
    return st


def crafted_state(w, h, tile, **fields):
    """a PN.State with some of its arrays replaced: what join_state uploads"""
    st = PN.State(w, h, tile)
    for k, v in fields.items():
        a = st.sum[k[4:]] if k.startswith("sum_") else getattr(st, k)
        a[...] = v
    return st


def progressive_cases():
    out = []
    w, h, tile, n = 16, 8, (16, 8), 128
    # the outlier bound: five pixels of e = 1.0f, one NaN, the rest 0
    cls = np.array([ZERO] * n, object)
    ones = [0, 63, 64, 127, 37]
    cls[ones], cls[5] = ONE, ENAN
    for tag, target, outliers, kills in (("at", 1.0, 0, ("P:e_ge",)), ("below", below(1.0), 5, ()), ("above", above(1.0), 0, ())):
        out.append(_prog(f"outlier/target_{tag}", kills, w, h, tile, two_epochs(w, h, cls), dict(target_error=float(target), min_epochs=3),
                         {0: (2, 0, outliers, f32(1.0))}, ones + [5], e_is_one=ones))
    cls2 = cls.copy()
    cls2[100] = EINF
    out.append(_prog("outlier/inf_and_nan", (), w, h, tile, two_epochs(w, h, cls2), dict(target_error=1.0, min_epochs=3),
                     {0: (2, 0, 1, INF)}, ones + [5, 100]))
    cls3 = np.array([ZERO] * n, object)
    cls3[[3, 70]] = (ENAN, NAN0)
    out.append(_prog("outlier/zero_and_nan_only", (), w, h, tile, two_epochs(w, h, cls3), dict(target_error=0.0, min_epochs=3),
                     {0: (2, 0, 0, f32(0.0))}, [3, 70]))
    wild = gray_film(w, h, np.resize(np.array([1.0, np.inf, np.nan, -3e38, 0.0, 2.0 ** 127], f32), n), 3)
    out.append(_prog("outlier/one_epoch", (), w, h, tile, [wild], dict(target_error=0.0), {0: (1, 0, 0, f32(0.0))}, np.arange(n)[::2]))

    # the retirement bound on a full 16x16 tile: 256 pixels at 50 permille, 12 outliers against 13, in all four waves, lanes 0 and 63
    spread = [0, 63, 64, 127, 128, 191, 192, 255, 5, 70, 135, 200, 100]
    for k, retired, kills in ((12, 1, ()), (13, 0, ("P:percent",))):
        cls = np.array([ZERO] * 256, object)
        cls[spread[:k]] = ONE
        out.append(_prog(f"retire/full_tile_{k}", kills, 16, 16, (16, 16), two_epochs(16, 16, cls), {}, {0: (2, retired, k, f32(1.0))}, spread[:k]))
    cls = np.array([ZERO] * 256, object)
    cls[np.arange(32) * 8] = ONE  # 32 * 1000 == 125 * 256
    out.append(_prog("retire/equal", ("P:retire_lt",), 16, 16, (16, 16), two_epochs(16, 16, cls), dict(outlier_permille=125),
                     {0: (2, 1, 32, f32(1.0))}, np.arange(32) * 8))
    # the ragged tile: 24x16 in 16x16 tiles, the second tile is 8x16 = 128 pixels: 6 outliers retire it, 7 do not
    for k, retired, kills in ((6, 1, ()), (7, 0, ("P:nominal_tile_pixels",))):
        cls = np.array([ZERO] * (24 * 16), object)
        px = _tile_pixels(24, 16, (16, 16), 1)[[0, 7, 63, 64, 127, 30, 99][:k]]
        cls[px] = ONE
        out.append(_prog(f"retire/ragged_tile_{k}", kills, 24, 16, (16, 16), two_epochs(24, 16, cls), {},
                         {0: (2, 1, 0, f32(0.0)), 1: (2, retired, k, f32(1.0))}, px, tile_pixels={1: 128}))
    # more than one trip of the 256-pixel loop: a 20x15 tile, the outliers and the largest e in the second trip, one at the last pixel
    for k, retired, kills in ((15, 1, ("P:retire_lt",)), (16, 0, ())):
        cls = np.array([ZERO] * 300, object)
        px = list(range(256, 256 + k - 1)) + [299]
        cls[px] = ONE
        cls[299] = EINF
        out.append(_prog(f"retire/second_trip_{k}", kills, 20, 15, (20, 15), two_epochs(20, 15, cls), {}, {0: (2, retired, k, INF)}, px))

    # epochs
    calm = np.array([ZERO] * n, object)
    for steps, retired, kills in ((2, 0, ()), (3, 1, ("P:epochs_gt",))):
        films = two_epochs(w, h, calm) + [gray_film(w, h, np.full(n, 0.25, f32), 9)] * (steps - 2)
        out.append(_prog(f"epochs/min_epochs_3_after_{steps}", kills, w, h, tile, films, dict(min_epochs=3), {0: (steps, retired, 0, f32(0.0))}, [0]))
    # a retired tile that is listed again: 0.25, 0.25, then 1: mean 0.5, m2 0.375, se = sqrt(0.375 / 6) = 0.25, e = 0.5 > 0.25 everywhere
    films = two_epochs(w, h, calm) + [gray_film(w, h, np.ones(n, f32), 9)]
    out.append(_prog("epochs/retired_stays_retired", (), w, h, tile, films, dict(target_error=0.25), {0: (3, 1, n, f32(0.5))}, np.arange(n),
                     all_pixels=True))
    every = np.array([ONE] * n, object)
    out.append(_prog("epochs/not_adaptive", (), w, h, tile, two_epochs(w, h, calm), dict(adaptive=False), {0: (2, 0, 0, f32(0.0))}, [0]))
    out.append(_prog("epochs/permille_0", ("P:retire_lt",), w, h, tile, two_epochs(w, h, calm), dict(outlier_permille=0), {0: (2, 1, 0, f32(0.0))}, [0]))
    out.append(_prog("epochs/permille_1000", ("P:retire_lt",), w, h, tile, two_epochs(w, h, every), dict(outlier_permille=1000),
                     {0: (2, 1, n, f32(1.0))}, np.arange(n), all_pixels=True))

    # crafted epoch counts: rec.x = n - 1; the tested pixels hold m2 = 4 (float)(n (n - 1)) and mean_y = 0, so with noise_floor = 1 and a
    # black epoch e = sqrt(4) / 1 = 2 exactly; their Color sum is n / 2, so the mean film is 0.5.  The controls get a gray of 1.
    # What they separate: 65537 and 2^24 + 1 a product in 32 bits from the 64-bit one (65536 is the control just below the wrap), and
    # 2^24 + 1 pins (float)n = 2^24 through the mean film.  They do NOT separate a product of two floats from the converted 64-bit
    # product: 65537 * 65536 is exact in f32, and (float)(2^24 + 1) * (float)2^24 = 2^48 is what 2^48 + 2^24 rounds to (ties to even).
    tested = np.arange(8) * 16
    for count, kills in ((65536, ()), (65537, ("P:fnn_u32",)), (2 ** 24 + 1, ("P:fnn_u32",))):
        fnn = float(np.array(count * (count - 1), np.uint64).astype(f32))
        m2, gray, sums = np.zeros(n, f32), np.ones(n, f32), np.full((n, 3), -0.0, f32)
        m2[tested], gray[tested], sums[tested] = f32(4.0) * f32(fnn), 0.0, f32(f32(count) / f32(2.0))
        init = (lambda count=count, m2=m2, sums=sums: crafted_state(w, h, tile, epochs=count - 1, m2=m2, sum_color=sums))
        out.append(_prog(f"epochs/crafted_{count}", kills, w, h, tile, [gray_film(w, h, gray, 4)], dict(target_error=2.0, noise_floor=1.0),
                         {0: (count, 1, 0, f32(2.0))}, tested, init=init, fnn=fnn, count=count, mean_color={int(p): 0.5 for p in tested}))

    # compaction: 1x1 tiles, more than one chunk of 1024; one epoch behind, nothing retires (adaptive = 0), every tile is listed.  Three
    # tiles of the last chunk hold m2 = 2 k^2: with a black epoch, n = 2 and noise_floor = 1 their e is k = 3, 5 and 2.
    for cw, ch in ((40, 30), (50, 41)):
        t = cw * ch
        patterns = {"all_active": np.zeros(t, bool), "all_retired": np.ones(t, bool), "only_1023": np.arange(t) != 1023, "only_1024": np.arange(t) != 1024,
                    "only_last": np.arange(t) != t - 1, "alternating": np.arange(t) % 2 == 1, "first_chunk_retired": np.arange(t) < 1024}
        for tag, retired in patterns.items():
            m2 = np.zeros(t, f32)
            loud = [t - 2, t - 5, t - 9]
            m2_px = {k: f32(2.0 * e * e) for k, e in zip(loud, (3.0, 5.0, 2.0))}
            st0 = PN.State(cw, ch, (1, 1))
            for k, v in m2_px.items():
                m2[st0.pixels_of(k)] = v
            init = (lambda cw=cw, ch=ch, m2=m2, retired=retired: crafted_state(cw, ch, (1, 1), epochs=1, m2=m2, retired=retired.astype(np.uint32)))
            expect = {k: (2, int(retired[k]), 1, f32(e)) for k, e in zip(loud, (3.0, 5.0, 2.0))}
            expect[0] = (2, int(retired[0]), 0, f32(0.0))
            # the carry matters where an active tile stands in a chunk before the last chunk that has one
            carried = tag in ("all_active", "only_1023", "alternating") or (t > 2048 and tag in ("only_1024", "first_chunk_retired"))
            out.append(_prog(f"compact/{cw}x{ch}/{tag}", ("P:compact_no_carry",) if carried else (), cw, ch, (1, 1),
                             [gray_film(cw, ch, np.zeros(t, f32), 5)], dict(noise_floor=1.0, adaptive=False), expect, [st0.pixels_of(k)[0] for k in loud],
                             init=init, active=np.flatnonzero(~retired).tolist(), totals=(int((~retired).sum()), f32(5.0), 3)))
    # wide products: one tile of 2048 x 2098 = 4 296 704 pixels, every one an outlier after two epochs, 999 permille: 4 296 704 000 >
    # 4 292 407 296 does not retire; in 32 bits the left side wraps to 1 736 704 and does.  The planes are filled on the device.
    out.append(Case("progressive/wide_products", "progressive_wide", ("P:u32_products",), w=2048, h=2098, tile=(2048, 2098), grays=GRAY[ONE],
                    params=dict(target_error=0.5, noise_floor=0.0, min_epochs=2, outlier_permille=999, adaptive=True),
                    expect={0: (2, 0, 2048 * 2098, f32(1.0))}))
    return out


# ---- the a-trous family --------------------------------------------------------------------------------------------------------------------
SIGMAS = (4.0, 0.4, 0.3)


def _guides(w, h, seed):
    rng = np.random.default_rng(seed)
    n = w * h
    normal = rng.normal(size=(n, 3)).astype(f32)
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    return normal.astype(f32), rng.choice(np.array([0.25, 1.0, 1.0], f32), n)


def _state_arrays(w, h, tile, m2, epochs):
    """the arrays rayn_amd.progressive.join_state takes, for the variance denoiser: only m2 and the epoch counts are read"""
    n, t = w * h, len(PN.tile_rects(w, h, *tile))
    z3 = np.zeros((n, 3), f32)
    return {"sum_color": z3, "sum_alpha": np.zeros(n, f32), "sum_background": z3, "sum_normal": z3, "mean_y": np.zeros(n, f32), "m2": np.asarray(m2, f32),
            "epochs": np.asarray(epochs, np.uint32), "retired": np.zeros(t, np.uint32), "outliers": np.zeros(t, np.uint32), "max_e": np.zeros(t, f32)}


def run_vdenoise(c, mutant=None):
    """(colour, variance, v0) of the progressive variance denoiser"""
    v0 = VN.initial_variance(c.color, c.state["m2"], c.state["epochs"], c.w, c.h, c.tile, mutant)
    col, var = VN.atrous(c.color, c.alpha, c.normal, v0, c.w, c.h, c.iterations, *c.sigmas, mutant=mutant)
    return col, var, v0


def vdenoise_cases():
    out = []
    # 16x8 in 4x4 tiles (x-major: tile = 2 * (x // 4) + y // 4) with the epoch counts below; a tile of n = 2 divides m2 by 2
    w, h, tile = 16, 8, (4, 4)
    epochs = np.array([1, 2, 2, 2, 2, 2, 65537, 0], np.uint32)
    rng = np.random.default_rng(11)
    n = w * h
    color = rng.gamma(0.6, 0.5, (n, 3)).astype(f32)
    normal, alpha = _guides(w, h, 12)
    m2 = rng.gamma(1.0, 0.05, n).astype(f32)
    v0 = np.full(n, -1.0, f32)  # -1: a control, not written down
    p = lambda x, y: x + y * w
    tested = {p(0, 1): (0.7, NAN), p(2, 2): (0.0, NAN),          # tile 0, n = 1: never guided
              p(1, 5): (0.0, 0.0), p(2, 6): (-0.0, -0.0),         # tile 1, n = 2: v = +0 and -0.0 are guided
              p(5, 1): (-2.0 * DENORM, NAN), p(6, 2): (INF, NAN), p(5, 3): (NAN, NAN), p(7, 0): (1.0, 0.5),   # tile 2: below(0), inf, NaN; 1 / 2
              p(13, 2): (0.25 * (2.0 ** 32 + 65536.0), 0.25),      # tile 6, n = 65537: m2 / (float)(65537 * 65536)
              p(14, 6): (0.5, NAN)}                                # tile 7, n = 0
    for q, (m, v) in tested.items():
        m2[q], v0[q] = m, v
    out.append(Case("vdenoise/pack", "vdenoise", ("V:v_gt0", "V:fnn_u32"), w=w, h=h, tile=tile, color=color, normal=normal, alpha=alpha,
                    state=_state_arrays(w, h, tile, m2, epochs), iterations=2, sigmas=SIGMAS, test=np.array(sorted(tested)), v0=v0,
                    below_zero=p(5, 1)))
    # a pixel just outside an under-covering grid: 17 wide in 16x8 tiles has ONE column of tiles, so x = 16 is in no tile
    w, h, tile = 17, 8, (16, 8)
    n = w * h
    color = rng.gamma(0.6, 0.5, (n, 3)).astype(f32)
    normal, alpha = _guides(w, h, 13)
    m2 = np.full(n, 0.5, f32)
    v0 = np.full(n, 0.25, f32)
    v0[16::17] = NAN
    out.append(Case("vdenoise/under_covered", "vdenoise", (), w=w, h=h, tile=tile, color=color, normal=normal, alpha=alpha,
                    state=_state_arrays(w, h, tile, m2, [2]), iterations=2, sigmas=SIGMAS, test=np.sort(np.r_[np.arange(16, n, 17), np.arange(15, n, 17)]), v0=v0))
    # the stencil cut on both sides: an image 2 step + 1 wide, whose last pass has its taps at -2 step .. 2 step: for the centre the
    # inner ring lands exactly on the first and last row and column and the outer ring one step beyond them
    for step, L in ((1, 1), (2, 2), (4, 3)):
        s = 2 * step + 1
        n = s * s
        color = rng.gamma(0.6, 0.5, (n, 3)).astype(f32)
        normal, alpha = _guides(s, s, 14 + step)
        m2 = rng.gamma(1.0, 0.05, n).astype(f32)
        more = {}
        if step == 1:  # by hand: a delta at the centre under the bare kernel weights: W = (1/4 + 3/8 + 1/4)^2 = 49/64, S = 9/64, c' = 9/49;
            color[:] = 0.0  # V = (9/64)^2, v' = (81/4096) / (49/64)^2 = 81/2401
            color[4] = 1.0
            m2[:] = 0.0
            m2[4] = 2.0
            more = dict(centre=4, centre_colour=f32(9.0) / f32(49.0), centre_variance=f32(81.0) / f32(2401.0))
        out.append(Case(f"vatrous/border/step{step}", "vdenoise", ("V:border_le",), w=s, h=s, tile=(s, s), color=color, normal=normal, alpha=alpha,
                        state=_state_arrays(s, s, (s, s), m2, [2]), iterations=L, sigmas=(0.0, 0.0, 0.0) if step == 1 else SIGMAS, test=np.arange(n), **more))
    # a tap that is not guided inside the 3x3 pre-filter, guided taps around it: every pixel a gray of 0.5 with v = 1 (m2 = 2, n = 2),
    # u = (8, 4) holds m2 = NaN; only the luminance term is on, sigma 1.  The pre-filter of u's neighbours leaves u out of both sums:
    # g = 0.875 / 0.875 = 1, inv = 1 / (1 + 1e-8f) = 1, every e = 0 * 1 = 0 and the weights are the bare kernel's.  By hand, with
    # sum h^2 = 70/256: (7, 4) misses the tap of weight 3/32: W = 29/32, V = 4900/65536 - 9/1024, v' = 1081/13456; (6, 4) (u is outside
    # its 3x3, a control of the pre-filter) misses 3/128: W = 125/128, V = 4900/65536 - 9/16384, v' = 1216/15625.  Counting u in the
    # pre-filter makes g, inv and every weight of (7, 4) NaN: all taps skipped, v' = 1.
    w, h, tile = 16, 8, (16, 8)
    n = w * h
    m2 = np.full(n, 2.0, f32)
    m2[p(8, 4)] = NAN
    normal, alpha = _guides(w, h, 19)
    ring = [p(x, y) for y in (3, 4, 5) for x in (7, 8, 9) if (x, y) != (8, 4)]
    out.append(Case("vatrous/prefilter_unguided_tap", "vdenoise", ("V:prefilter_counts_unguided",), w=w, h=h, tile=tile, color=np.full((n, 3), 0.5, f32),
                    normal=normal, alpha=alpha, state=_state_arrays(w, h, tile, m2, [2]), iterations=1, sigmas=(1.0, 0.0, 0.0),
                    test=np.array(sorted(ring + [p(6, 4), p(8, 4)])), variance={p(7, 4): f32(1081.0) / f32(13456.0), p(6, 4): f32(1216.0) / f32(15625.0)},
                    colour={p(7, 4): 0.5, p(6, 4): 0.5, p(8, 4): 0.5}, not_guided=[p(8, 4)]))
    # weights: a NaN weight skips the tap - inf - inf in the alpha term: 0 * inf in the luminance term is out of reach (inv <= 1e8, and
    # the luminance of three finite components is finite: the three f32 coefficients sum to no more than 1); e = +inf gives the weight
    # +0, which is added: a centre of -0.0 comes out as +0
    w, h, tile = 16, 8, (16, 8)
    n = w * h
    color = (0.25 + 0.5 * rng.random((n, 3))).astype(f32)
    normal, alpha = _guides(w, h, 20)
    m2 = np.full(n, 0.5, f32)
    alpha[[p(4, 3), p(5, 3)]] = INF          # two neighbours: their mutual weight is NaN, every other tap of theirs has e = +inf
    color[p(11, 4)] = -0.0                   # its alpha is infinitely far from every tap's
    alpha[p(11, 4)] = 3.0e38
    out.append(Case("vatrous/weights", "vdenoise", ("V:nan_weight_counts", "V:zero_weight_skipped"), w=w, h=h, tile=tile, color=color, normal=normal, alpha=alpha,
                    state=_state_arrays(w, h, tile, m2, [2]), iterations=1, sigmas=SIGMAS, test=np.array([p(4, 3), p(5, 3), p(11, 4)]),
                    keeps=[p(4, 3), p(5, 3)], positive_zero=p(11, 4)))
    return out


def run_denoise(c, mutant=None):
    return DN.atrous(c.color, c.alpha, c.normal, c.w, c.h, c.iterations, *c.sigmas, mutant=mutant)


def denoise_cases():
    out = []
    rng = np.random.default_rng(31)
    for step, L in ((1, 1), (2, 2), (4, 3)):
        s = 2 * step + 1
        n = s * s
        color = rng.gamma(0.6, 0.5, (n, 3)).astype(f32)
        normal, alpha = _guides(s, s, 32 + step)
        more = {}
        if step == 1:
            color[:] = 0.0
            color[4] = 1.0
            more = dict(centre=4, centre_colour=f32(9.0) / f32(49.0))
        out.append(Case(f"atrous/border/step{step}", "denoise", ("D:border_le",), w=s, h=s, color=color, normal=normal, alpha=alpha, iterations=L,
                        sigmas=(0.0, 0.0, 0.0) if step == 1 else (0.5, 0.4, 0.3), test=np.arange(n), **more))
    w, h = 16, 8
    n = w * h
    p = lambda x, y: x + y * w
    color = (0.25 + 0.5 * rng.random((n, 3))).astype(f32)
    normal, alpha = _guides(w, h, 40)
    alpha[[p(4, 3), p(5, 3)]] = INF          # inf - inf in the alpha term: the two are NaN-weight taps of each other
    color[p(11, 4)] = -0.0
    alpha[p(11, 4)] = 3.0e38                 # e = +inf to every tap: weights of +0, which are added
    out.append(Case("atrous/weights", "denoise", ("D:nan_weight_counts", "D:zero_weight_skipped"), w=w, h=h, color=color, normal=normal, alpha=alpha, iterations=1,
                    sigmas=(0.5, 0.4, 0.3), test=np.array([p(4, 3), p(5, 3), p(11, 4)]), keeps=[p(4, 3), p(5, 3)], positive_zero=p(11, 4)))
    return out


def run_tvdenoise(c, mutant=None, beta=None):
    """(colour, variance, v0, k, plane A of the history after the call) of the temporal variance denoiser; beta: the feedback strength
    (None = the case's; 0 leaves the history alone)"""
    beta = c.beta if beta is None else beta
    v0, k = TV.initial_variance(c.w, c.h, c.color, c.obj, c.n1, c.mom, mutant)
    col, var = VN.atrous(c.color, c.alpha, c.normal, v0, c.w, c.h, c.iterations, *c.sigmas)
    A = c.hist[0]
    if beta:
        c1, v1 = VN.atrous(c.color, c.alpha, c.normal, v0, c.w, c.h, 1, *c.sigmas)
        A = TF.write_back(A, c.color, c1, v1, beta)
    return col, var, v0, k, A


def _tv(name, kills, w, h, seed, beta=0.0, iterations=2, sigmas=SIGMAS):
    """the base of a case: one object (1), histories of length 8, moments (0.5, 0.5): the temporal estimate is 0.25 / 8"""
    rng = np.random.default_rng(seed)
    n = w * h
    normal, alpha = _guides(w, h, seed + 1)
    c = Case("tvdenoise/" + name, "tvdenoise", kills, w=w, h=h, color=(0.25 + 0.5 * rng.random((n, 3))).astype(f32), normal=normal, alpha=alpha,
             obj=np.ones(n, np.uint32), n1=np.full(n, 8.0, f32), mom=np.full((n, 2), 0.5, f32), iterations=iterations, sigmas=sigmas, beta=beta,
             v0=np.full(n, -1.0, f32), hist_rgb=rng.random((n, 3)).astype(f32))
    return c


def _tv_done(c):
    n = c.w * c.h
    A = np.concatenate([c.hist_rgb, c.n1[:, None]], axis=1).astype(f32)
    rng = np.random.default_rng(99)
    c.hist = (A, rng.random((n, 4)).astype(f32), rng.random((n, 4)).astype(f32), c.obj.copy())
    c.test = np.asarray(c.test, np.int64)
    return c


def tvdenoise_cases():
    out = []
    # the history length: the tested pixels are object 1 and a gray of 0.5 (so the spatial estimate of any window of them is exactly 0),
    # the controls object 2 with random colours; moments (0.5, 0.5): the temporal estimate is 0.25 / n'
    c = _tv("nprime", ("TV:nprime_gt4", "TV:nprime_gt1"), 16, 8, 50)
    p = lambda x, y: x + y * 16
    c.obj[:] = 2
    c.n1[:] = np.resize(np.array([1.0, 3.0, 8.0], f32), 128)
    lengths = ((1.0, 0.0), (below(1.0), NAN), (4.0, 0.0625), (below(4.0), 0.0), (NAN, NAN), (INF, 0.0), (above(4.0), f32(0.25) / above(4.0)), (0.0, NAN))
    c.test = [p(1 + 2 * i, 1 + (i % 3) * 2) for i in range(len(lengths))]
    for q, (n1, v) in zip(c.test, lengths):
        c.obj[q], c.color[q], c.n1[q], c.v0[q] = 1, 0.5, n1, v
    out.append(_tv_done(c))
    # d = m2 - m1 m1: exactly 0 and one ulp either side (n' = 4); -0.0 on a pixel whose every tap is a miss, so that nothing is added to it
    c = _tv("d_zero", ("TV:d_ge0",), 16, 8, 52, iterations=1)
    c.n1[:] = 4.0
    moments = (((0.5, 0.25), 0.0), ((0.5, above(0.25)), f32(above(0.25) - f32(0.25)) / f32(4.0)), ((0.5, below(0.25)), 0.0))
    c.test = [p(1, 1), p(3, 1), p(13, 6)]
    for q, (m, v) in zip(c.test, moments):
        c.mom[q], c.v0[q] = m, v
    for y in range(2, 7):
        for x in range(6, 11):
            c.obj[p(x, y)] = MISS
    lone = p(8, 4)
    c.obj[lone], c.mom[lone], c.v0[lone] = 1, (0.0, -0.0), 0.0
    c.test.append(lone)
    c.lone, c.lone_variance = lone, f32(0.0)  # V = (9/64)^2 * (+0), W = 9/64: +0, where d = -0.0 let through gives -0.0
    out.append(_tv_done(c))
    # the 7x7 window of a short-history pixel at each corner of the first 16x16 block: it crosses the block's and the image's borders
    c = _tv("corners", (), 37, 23, 54)
    p37 = lambda x, y: x + y * 37
    c.test = [p37(0, 0), p37(15, 0), p37(0, 15), p37(15, 15), p37(16, 16), p37(36, 22)]
    c.n1[c.test] = 1.0
    c.k = dict(zip(c.test, (16.0, 28.0, 28.0, 49.0, 49.0, 16.0)))
    out.append(_tv_done(c))
    # only the centre counts: the one pixel of object 3
    c = _tv("centre_only", (), 16, 8, 56)
    c.test = [p(7, 3)]
    c.obj[c.test], c.n1[c.test], c.v0[c.test] = 3, 1.0, 0.0
    c.k = {p(7, 3): 1.0}
    out.append(_tv_done(c))
    # a block without a short-history pixel beside one with one: the first skips the halo, the second stages it
    c = _tv("uniform_skip", (), 32, 16, 58)
    c.test = [20 + 5 * 32]
    c.n1[c.test] = 2.0
    c.k = {20 + 5 * 32: 49.0}
    out.append(_tv_done(c))
    # the feedback arm at full strength: an ordinary pixel takes c'; a pixel that is not guided (a miss), and one whose fb overflows
    # (3e38 among -3e38 with the luminance term off: c' - c = -inf), keep their history; n' in .w is never written
    c = _tv("feedback", (), 16, 8, 60, beta=1.0, iterations=1, sigmas=(0.0, 0.4, 0.3))
    c.n1[:] = np.resize(np.array([4.0, 5.0, 7.5], f32), 128)
    c.normal[:], c.alpha[:] = (0.0, 0.0, 1.0), 1.0  # one surface: the weights are the bare kernel's
    c.color[:] = -3.0e38
    c.color[:, 1] = 0.5
    c.color[p(5, 3)] = (3.0e38, 0.5, 0.5)
    c.obj[p(12, 2)] = MISS
    c.test = [p(5, 3), p(12, 2), p(9, 5)]
    c.keeps, c.takes = [p(5, 3), p(12, 2)], [p(9, 5)]
    out.append(_tv_done(c))
    return out


# ---- display -------------------------------------------------------------------------------------------------------------------------------
def gray_with_luminance(target):
    """a gray (g, g, g) whose luminance is exactly `target`, searched among the floats next to it"""
    t = f32(target)
    cands = [t]
    lo = hi = t
    for _ in range(16):
        lo, hi = np.nextafter(lo, -INF), np.nextafter(hi, INF)
        cands += [lo, hi]
    for g in cands:
        if X.luminance(np.array([g, g, g], f32), f32) == t:
            return g
    raise AssertionError(f"no gray of luminance {target!r}")


def _disp(name, kills, color, expect, w=16, h=8, background=None, alpha=None, transparent=False, exposure="auto", tone="linear", bloom=None,
          adapt=1.0, state=(0.0, 0), test=None, **more):
    from rayn_amd.options import Bloom, Display
    n = w * h
    color = np.ascontiguousarray(np.broadcast_to(np.asarray(color, f32), (n, 3))).copy()
    film = {"color": color, "background": background, "alpha": alpha}
    display = Display(exposure=exposure, tone=tone, bloom=None if bloom is None else Bloom(*bloom))
    return Case("display/" + name, "display", kills, w=w, h=h, film=film, transparent=transparent, display=display, adapt=adapt, state=state, expect=expect,
                test=np.asarray([] if test is None else test, np.int64), **more)


def run_display(c, mutant=None):
    return X.display(c.film["color"], c.w, c.h, c.display.to_abi(c.adapt), c.film["background"], c.film["alpha"], c.transparent, c.state, mutant=mutant)


def meter_of(c, mutant=None):
    return X.meter(X.input_color(c.film["color"], c.film["background"], c.transparent), f32, mutant)


QUANT_EDGES = {1: 0x36AA5B87, 64: 0x3D43B081, 128: 0x3E60C9C7, 200: 0x3F160253, 254: 0x3F7DCBEB}  # the smallest d with gamma22(d) * 255 == k


def display_cases():
    out = []
    n = 128
    two = np.full((n, 3), 2.0, f32)  # the controls: a gray of 2, metered

    def film(pixels):
        c = two.copy()
        for q, v in pixels.items():
            c[q] = v
        return c
    # the meter's gate l > 0: N is the number of metered pixels
    g4 = gray_with_luminance(1e-4)
    gate = {"zero": ((0.0, 0.0, 0.0), 0, ("X:meter_ge0",)), "negative_zero": ((-0.0, -0.0, -0.0), 0, ("X:meter_ge0",)),
            "denormal": ((0.0, DENORM, 0.0), 1, ()), "below_zero": ((0.0, -DENORM, 0.0), 0, ()),
            "largest_luminance": ((FMAX, FMAX, FMAX), 1, ()), "one_component_inf": ((1.0, INF, 1.0), 0, ()), "one_component_nan": ((NAN, 1.0, 1.0), 0, ()),
            "floor_at": ((g4,) * 3, 1, ()), "floor_below": ((below(g4),) * 3, 1, ()), "floor_above": ((above(g4),) * 3, 1, ()),
            "floor_far_below": ((2.0 ** -20,) * 3, 1, ("X:no_floor",))}  # one ulp below the floor the logarithm rounds to the same float
    # (floor_at, floor_below and floor_above pin N alone, which the gate already gives: dm_logf rounds the three luminances to ONE
    # float, so whether the floor is applied one ulp below it cannot show in any output; floor_far_below is the case that shows it)
    for tag, (rgb, counts, kills) in gate.items():
        px = [3, 64, 127]
        out.append(_disp(f"meter/{tag}", kills, film({q: rgb for q in px}), dict(N=n - 3 + 3 * counts), test=px, rgb=rgb))
    out.append(_disp("meter/nothing_counts", ("X:meter_ge0",), film({q: (0.0, -0.0, 0.0) if q % 2 else (NAN, 1.0, INF) for q in range(n)}),
                     dict(N=0, e=1.0, state=(0.75, 1)), state=(0.75, 1), test=range(n), all_pixels=True))
    # adaptation: every pixel a gray of 2, m_now = logf(2); the state before holds m = 1e8
    for tag, adapt, state, m, kills in (("adapt_1", 1.0, (1e8, 1), "log2", ("X:adapt_always_blend",)), ("adapt_below_1", float(below(1.0)), (1e8, 1), f32(8.0), ()),  # logf(2) - 1e8 rounds to -1e8; times 1 - 2^-24: -99999992; + 1e8
                                        ("adapt_0", 0.0, (1e8, 1), f32(1e8), ()), ("not_valid", 0.5, (np.nan, 0), "log2", ("X:adapt_always_blend",))):
        out.append(_disp(f"adaptation/{tag}", kills, two, dict(N=n, m=m), adapt=adapt, state=state, test=range(n), all_pixels=True))
    # Reinhard's gate on lx (manual exposure of 1, white 4): off, the pixel keeps v's bits; a gray of 1 becomes (1 + 1/16) / 2
    ctrl = np.ones((n, 3), f32)
    rein = {3: (0.0, 0.0, 0.0), 20: (-0.0, -0.0, -0.0), 37: (0.0, DENORM, 0.0), 64: (INF, 1.0, 1.0), 90: (NAN, 1.0, 1.0), 127: (0.0, -1.0, 0.0)}
    c = ctrl.copy()
    for q, v in rein.items():
        c[q] = v
    d = {q: v for q, v in rein.items()}
    d[0] = (0.53125,) * 3
    out.append(_disp("reinhard/gate", (), c, dict(d=d), exposure=0.0, tone="reinhard", test=sorted(rein)))
    # ACES: rmax(v, 0) gives +0 for -0.0, a negative and a NaN component: d = 0 / 0.14 = +0
    aces = {3: (-0.0, -0.0, -0.0), 64: (-1.0, -3.0e38, -DENORM), 127: (NAN, NAN, NAN)}
    c = ctrl.copy()
    for q, v in aces.items():
        c[q] = v
    one = (f32(1.0) * (f32(2.51) * f32(1.0) + f32(0.03))) / (f32(1.0) * (f32(2.43) * f32(1.0) + f32(0.59)) + f32(0.14))
    d = {q: (0.0, 0.0, 0.0) for q in aces}
    d[0] = (one,) * 3
    out.append(_disp("aces/rmax", (), c, dict(d=d), exposure=0.0, tone="aces", test=sorted(aces)))
    # the bright pass e c - threshold (e = 1, threshold 1, one level): 0 at the threshold, below it and for a colour that is not finite
    dark = film({3: (1.0, below(1.0), 0.5), 64: (INF, NAN, -INF), 127: (1.0, 1.0, 1.0)})
    dark[dark == 2.0] = 1.0
    out.append(_disp("bright/threshold_at_and_below", (), dark, dict(bloom_zero=True), exposure=0.0, bloom=(1.0, 0.5, 1), test=[3, 64, 127]))
    lit = dark.copy()
    lit[64] = (above(1.0), 1.0, 1.0)
    # pixel 64 = (0, 4) has the bright pass 2^-23; level 1 holds 2^-25 at (0, 2); the upsample at (0, 4) is 0.75 * 2^-25 (both x taps
    # are column 0, the y taps rows 1 and 2 with 0.25 and 0.75); the bloom is (2^-23 + 3 * 2^-27) * (0.5 / 2) = 19 * 2^-29
    out.append(_disp("bright/one_ulp_above", (), lit, dict(bloom_value=((64, 0), 19.0 * 2.0 ** -29)), exposure=0.0, bloom=(1.0, 0.5, 1), test=[64]))
    over = dark.copy()
    over[64] = (3.0e38, 1.0, 1.0)  # finite, e c = 2 * 3e38 overflows: the bright pass is +inf, not 0
    out.append(_disp("bright/ec_overflows", ("X:bright_fin_after",), over, dict(bloom_inf=(64, 0)), exposure=1.0, bloom=(1.0, 0.5, 1), test=[64]))
    # quantisation truncates: the smallest d with gamma22(d) * 255 == k gives k, the float below it k - 1 - in all three arms
    edges = np.array(sorted(QUANT_EDGES.values()), np.uint32).view(f32)
    c = np.full((n, 3), 0.5, f32)
    image = {}
    for i, (k, d_bits) in enumerate(sorted(QUANT_EDGES.items())):
        dk = np.array([d_bits], np.uint32).view(f32)[0]
        c[10 + i], c[60 + i] = dk, below(dk)
        image[10 + i], image[60 + i] = k, k - 1
    specials = {100: (1.0, (255, 255)), 101: (above(1.0), (255, 255)), 102: (NAN, (0, 255)), 103: (-1.0, (0, 255)), 104: (-0.0, (0, 0))}
    for q, (v, _) in specials.items():
        c[q] = v
    bg0, a1 = np.zeros((n, 3), f32), np.full(n, 0.5, f32)
    for tag, kw, arm in (("rgba", dict(alpha=a1, transparent=True), 0), ("color_bg", dict(background=bg0), 0), ("color_only", dict(), 1)):
        img = dict(image)
        img.update({q: v[arm] for q, (_, v) in specials.items()})
        out.append(_disp(f"quant/{tag}", ("X:quant_round",), c, dict(image=img), exposure=0.0, test=sorted(img), **kw))
    # up_axis: every level 1 wide (levels = 8 on tiny films), and 5x3 with two levels (t1 = h + 1 clamps on the right and at the bottom,
    # t0 does not).  A constant film of 3 with threshold 1 has the bright pass 2 at every level, every upsample returns 2, and with
    # strength = levels + 1 the bloom is (levels + 1) * 2 exactly; the random film is compared with the restatement
    rng = np.random.default_rng(70)
    for (w, h), levels in (((1, 1), 8), ((2, 1), 8), ((1, 2), 8), ((3, 3), 8), ((5, 3), 2)):
        out.append(_disp(f"up_axis/{w}x{h}/constant", (), np.full((w * h, 3), 3.0, f32), dict(bloom_all=2.0 * (levels + 1)), w=w, h=h, exposure=0.0,
                         bloom=(1.0, float(levels + 1), levels), test=range(w * h), all_pixels=True))
        out.append(_disp(f"up_axis/{w}x{h}/random", (), np.exp(rng.uniform(-2.0, 3.0, (w * h, 3))).astype(f32), dict(), w=w, h=h, exposure=0.0,
                         bloom=(1.0, 0.5, levels), test=range(w * h), all_pixels=True))
    return out


_ALL = []


def all_cases():
    if not _ALL:
        _ALL.extend(progressive_cases() + vdenoise_cases() + denoise_cases() + tvdenoise_cases() + display_cases())
    return _ALL
