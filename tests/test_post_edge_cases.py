"""tests/post_edge_cases.py held to account without a GPU: every case's hand-written outcome holds on the numpy restatements, the compared
quantities ARE the bounds, every case differs from each mutant it names on something under test, every entry of every MUTANTS tuple is
named by a case, the equivalent readings change no case - and the reason the file exists: the inputs of the older GPU tests, replayed
through every mutant, with the number of calls that notice it."""
import itertools

import numpy as np
import pytest

import denoise_np as DN
import denoise_variance_np as VN
import display_np as X
import post_edge_cases as EC
import progressive_cases as PC
import progressive_np as PN
import temporal_cases as TC
import temporal_variance_np as TV
from common import above, below, bits_equal
from denoise_cases import random_film
from display_cases import film as display_film

f32 = np.float32
CASES = EC.all_cases()
IDS = [c.name for c in CASES]


def of(*families):
    cs = [c for c in CASES if c.family in families]
    return pytest.mark.parametrize("c", cs, ids=[c.name for c in cs])


def same(a, b):
    """bit equality of two float32 values or arrays, NaN payloads aside"""
    return bits_equal(np.asarray(a, f32).reshape(-1), np.asarray(b, f32).reshape(-1))


# ---- 1. the hand-written outcomes ----------------------------------------------------------------------------------------------------------

def test_names_are_unique_and_every_case_has_controls():
    assert len(set(IDS)) == len(IDS)
    for c in CASES:
        if c.family == "progressive_wide":
            continue
        under = c.pixels if c.family == "progressive" else c.test
        assert len(under), c.name
        assert len(under) < c.w * c.h or getattr(c, "all_pixels", False) or c.name.startswith(("vatrous/border", "atrous/border")), (c.name, "no control")


def check_tiles(c, epochs, retired, outliers, max_e, what):
    """the hand-written tile outcomes against four per-tile arrays"""
    for k, (n, r, o, e) in c.expect.items():
        got = (int(epochs[k]), int(retired[k]), int(outliers[k]), EC.bits(max_e[k]))
        assert got == (n, r, o, EC.bits(e)), (c.name, what, "tile", k, got, (n, r, o, EC.bits(e)))


@of("progressive")
def test_progressive_outcomes_hold(c):
    st = EC.run_progressive(c)
    check_tiles(c, st.epochs, st.retired, st.outliers, st.max_e, "progressive_np")
    if hasattr(c, "active"):
        assert st.active().tolist() == c.active and list(c.active) == sorted(c.active)
        t = st.totals()
        assert (t["active_tiles"], EC.bits(t["max_e"]), t["outlier_pixels"]) == (c.totals[0], EC.bits(c.totals[1]), c.totals[2])
        lst, count = PN.compact(st.retired)
        assert lst[:count].tolist() == c.active and count == len(c.active)
    for p, v in getattr(c, "mean_color", {}).items():
        assert (st.mean["color"][p] == f32(v)).all(), (c.name, p)


def test_the_wide_tile_does_not_retire():
    c = next(c for c in CASES if c.family == "progressive_wide")
    npix = c.w * c.h
    n, retired, outliers, max_e = c.expect[0]
    assert npix >= 4294968 and outliers == npix and len(PN.tile_rects(c.w, c.h, *c.tile)) == 1
    assert npix * 1000 > 999 * npix and (npix * 1000) % 2 ** 32 == 1736704 <= 999 * npix < 2 ** 32  # the wrap is on the left side only
    assert PN.retires(n, outliers, npix, 2, 999) is False and retired == 0
    assert PN.retires(n, outliers, npix, 2, 999, "u32_products") is True
    # one pixel of the film the device fills: e = 1.0f > 0.5
    st = PN.State(1, 1, (1, 1))
    for g in c.grays:
        PN.accumulate(st, EC.gray_film(1, 1, [g]), **dict(c.params, outlier_permille=0))
    assert st.outliers[0] == 1 and EC.bits(st.max_e[0]) == EC.bits(max_e) == 0x3F800000


@of("vdenoise")
def test_variance_denoiser_outcomes_hold(c):
    col, var, v0 = EC.run_vdenoise(c)
    if hasattr(c, "v0"):
        known = c.v0 != -1
        assert same(v0[known], c.v0[known]) and (np.signbit(v0[known]) == np.signbit(c.v0[known])).all(), (c.name, v0[known], c.v0[known])
        guided = ~np.isnan(c.v0[known])
        assert (np.isnan(var[known]) == ~guided).all()  # nothing overflows: guided on entry is guided at the end
        color = np.asarray(c.color, f32).reshape(-1, 3)
        assert same(col[known][~guided], color[known][~guided])  # a pixel that is not guided passes through
    if hasattr(c, "centre"):
        assert same(col[c.centre], [c.centre_colour] * 3) and same(var[c.centre], c.centre_variance)
    check_weights(c, col)
    check_prefilter(c, col, var)
    if hasattr(c, "keeps"):
        w0 = f32(9.0 / 64.0)
        assert same(var[c.keeps], ((w0 * w0) * v0[c.keeps]) / (w0 * w0))


def check_prefilter(c, col, var):
    for q, v in getattr(c, "variance", {}).items():
        assert same(var[q], v), (c.name, q, var[q], v)
    for q, v in getattr(c, "colour", {}).items():
        assert (col[q] == f32(v)).all(), (c.name, q, col[q])
    for q in getattr(c, "not_guided", []):
        assert np.isnan(var[q])


def check_weights(c, col):
    if hasattr(c, "keeps"):  # every tap has the weight NaN or +0: c' = (9/64 c + 0) / (9/64 + 0)
        w0 = f32(9.0 / 64.0)
        assert same(col[c.keeps], (w0 * np.asarray(c.color, f32).reshape(-1, 3)[c.keeps]) / w0) and np.isfinite(col[c.keeps]).all()
        assert (col[c.positive_zero] == 0).all() and not np.signbit(col[c.positive_zero]).any()


@of("denoise")
def test_denoiser_outcomes_hold(c):
    col = EC.run_denoise(c)
    if hasattr(c, "centre"):
        assert same(col[c.centre], [c.centre_colour] * 3)
    check_weights(c, col)


@of("tvdenoise")
def test_temporal_variance_outcomes_hold(c):
    col, var, v0, k, A = EC.run_tvdenoise(c)
    known = c.v0 != -1
    assert same(v0[known], c.v0[known]) and (np.signbit(v0[known]) == np.signbit(c.v0[known])).all(), (c.name, v0[known], c.v0[known])
    for p, want in getattr(c, "k", {}).items():
        assert k[p] == want, (c.name, p, k[p], want)
    if hasattr(c, "lone"):
        assert EC.bits(var[c.lone]) == EC.bits(c.lone_variance)
    before = c.hist[0]
    assert np.array_equal(A[:, 3].view(np.uint32), before[:, 3].view(np.uint32))  # n' keeps its bits
    if c.beta:
        changed = (A.view(np.uint32) != before.view(np.uint32)).any(axis=1)
        assert not changed[c.keeps].any() and changed[c.takes].all() and same(A[c.takes, :3], col[c.takes])  # beta = 1, one pass: fb = c'
        with np.errstate(over="ignore"):
            assert not np.isfinite((col - c.color)[c.keeps[0]]).all()  # c' - c overflows
    else:
        assert A is before


def _film_pixel_of_image(c, q):
    return c.h - 1 - q // c.w, q % c.w  # the image's rows are top-down


@of("display")
def test_display_outcomes_hold(c, oracle):
    r = EC.run_display(c)
    e = c.expect
    if "N" in e:
        assert EC.meter_of(c)[1] == e["N"], (c.name, EC.meter_of(c)[1])
    if "e" in e:
        assert r["e"] == f32(e["e"])
    if "state" in e:
        assert same(r["state"][0], e["state"][0]) and r["state"][1] == e["state"][1]
    if "m" in e and e["m"] is not None:
        m = X._logf(np.array([2.0], f32), f32)[0] if isinstance(e["m"], str) else e["m"]
        assert same(r["state"][0], m) and r["state"][1] == 1, (c.name, r["state"], m)
    for q, rgb in e.get("d", {}).items():
        assert same(r["d"][q], rgb) and (np.signbit(r["d"][q]) == np.signbit(np.asarray(rgb, f32))).all(), (c.name, q, r["d"][q], rgb)
    for q, v in e.get("image", {}).items():
        y, x = _film_pixel_of_image(c, q)
        assert (r["image"][y, x, :3] == v).all(), (c.name, q, r["image"][y, x], v)
    if e.get("bloom_zero"):
        assert (r["bloom"] == 0).all() and not np.signbit(r["bloom"]).any()
    if "bloom_value" in e:
        assert r["bloom"][e["bloom_value"][0]] == f32(e["bloom_value"][1]), (c.name, r["bloom"][e["bloom_value"][0]])
    if "bloom_inf" in e:
        assert np.isposinf(r["bloom"][e["bloom_inf"]])
    if "bloom_all" in e:
        assert (r["bloom"] == f32(e["bloom_all"])).all(), (c.name, r["bloom"])


# ---- 2. the compared quantities are the bounds ---------------------------------------------------------------------------------------------

def test_the_edges_are_where_the_cases_say(oracle):
    by = {c.name: c for c in CASES}
    # e == 1.0f exactly on the pixels of the outlier cases, and the three targets are 1, one ulp below and one ulp above
    for tag, target in (("at", f32(1.0)), ("below", below(1.0)), ("above", above(1.0))):
        c = by[f"progressive/outlier/target_{tag}"]
        st = EC.run_progressive(c)
        e = PN.e_p(st.mean_y, st.m2, 2, 0.0)
        assert (e[c.e_is_one] == f32(1.0)).all() and f32(c.params["target_error"]) == target
        assert (st.m2[c.e_is_one] == f32(0.5)).all() and (st.mean_y[c.e_is_one] == f32(0.5)).all()
        lum = X.luminance(c.films[1]["color"] + c.films[1]["background"], f32)
        assert (lum[c.e_is_one] == f32(1.0)).all()  # the luminance expression gives the power of two exactly
    assert X.luminance(np.full(3, 2.0 ** 127, f32), f32) == f32(2.0 ** 127)
    # the ragged tile has 128 pixels, the tile of the second-trip cases 300 with the outliers behind the first 256
    c = by["progressive/retire/ragged_tile_7"]
    st = PN.State(c.w, c.h, c.tile)
    assert len(st.pixels_of(1)) == 128 == c.tile_pixels[1] and len(st.rects) == 2 and 6 * 1000 <= 50 * 128 < 7 * 1000 <= 50 * 256
    assert 12 * 1000 <= 50 * 256 < 13 * 1000 and 32 * 1000 == 125 * 256 and 15 * 1000 == 50 * 300
    c = by["progressive/retire/second_trip_15"]
    assert len(PN.State(c.w, c.h, c.tile).pixels_of(0)) == 300 and c.pixels.min() >= 256 and c.pixels.max() == 299
    c = by["progressive/retire/full_tile_13"]
    assert {int(p) >> 6 for p in c.pixels} == {0, 1, 2, 3} and {0, 63} <= {int(p) & 63 for p in c.pixels}
    # n (n - 1) beyond 2^32, its u32 reading, and the single rounding of (float)n
    for count, exact, wrapped in ((65536, 65536 * 65535, 65536 * 65535), (65537, 2 ** 32 + 65536, 65536), (2 ** 24 + 1, 2 ** 48, 2 ** 24)):
        c = by[f"progressive/epochs/crafted_{count}"]
        assert c.fnn == float(exact) and (count * (count - 1)) % 2 ** 32 == wrapped and c.init().epochs[0] == count - 1
    assert f32(2 ** 24 + 1) == f32(2 ** 24) and by["progressive/epochs/crafted_65536"].fnn < 2.0 ** 32
    # the compaction cases have more than one chunk, the second of them three
    assert len(PN.tile_rects(40, 30, 1, 1)) == 1200 > PN.CHUNK and len(PN.tile_rects(50, 41, 1, 1)) == 2050 > 2 * PN.CHUNK
    # the variance pack: v itself is below(0), and 17 wide in 16x8 tiles is one column of tiles
    c = by["vdenoise/pack"]
    assert c.state["m2"][c.below_zero] / f32(2.0) == below(0.0) and len(PN.tile_rects(17, 8, 16, 8)) == 1
    assert 65537 * 65536 > 2 ** 32 and 0.25 * (2.0 ** 32 + 65536.0) == float(f32(0.25 * (2.0 ** 32 + 65536.0)))
    # n' and d of the temporal estimate
    c = by["tvdenoise/nprime"]
    assert {1.0, float(below(1.0)), 4.0, float(below(4.0)), float(above(4.0))} <= set(c.n1[c.test][np.isfinite(c.n1[c.test])].tolist())
    c = by["tvdenoise/d_zero"]
    d = c.mom[c.test, 1] - c.mom[c.test, 0] * c.mom[c.test, 0]
    assert d[0] == 0 and d[1] == above(0.25) - f32(0.25) > 0 and d[2] == below(0.25) - f32(0.25) < 0 and d[3] == 0 and np.signbit(d[3])
    # the stencils are cut on both sides: 2 step + 1 wide
    for name in ("vatrous", "atrous"):
        for step in (1, 2, 4):
            c = by[f"{name}/border/step{step}"]
            assert c.w == c.h == 2 * step + 1 and 1 << (c.iterations - 1) == step
    # the meter's floor: the luminance IS 1e-4f, one ulp below and one above; the gated luminances are +0, -0.0, the denormal and below(0)
    lum = lambda c: X.luminance(np.asarray(c.rgb, f32), f32)
    assert lum(by["display/meter/floor_at"]) == f32(1e-4) and lum(by["display/meter/floor_below"]) == below(1e-4) and lum(by["display/meter/floor_above"]) == above(1e-4)
    z, nz = lum(by["display/meter/zero"]), lum(by["display/meter/negative_zero"])
    assert z == 0 and not np.signbit(z) and nz == 0 and np.signbit(nz)
    assert lum(by["display/meter/denormal"]) == EC.DENORM and lum(by["display/meter/below_zero"]) == -EC.DENORM
    assert np.isfinite(lum(by["display/meter/largest_luminance"]))  # three finite components never give an infinite luminance
    # quantisation: gamma22(d) * 255 is the integer, and one ulp below d it is not reached
    from rayn_amd import image
    for k, d_bits in EC.QUANT_EDGES.items():
        d = np.array([d_bits], np.uint32).view(f32)[0]
        assert image.gamma_corrected(d) * f32(255.0) == f32(k) and image.gamma_corrected(below(d)) * f32(255.0) < f32(k)
        both = oracle.detmath(5, np.array([d, below(d)], f32), np.full(2, f32(1.0) / f32(2.2), f32))  # the pinned dm_powf agrees
        assert same(both, image.gamma_corrected(np.array([d, below(d)], f32)))
    # up_axis: every level of the tiny films is 1 wide or 1 high; 5x3 halves to 3x2 and 2x1
    assert X.level_sizes(3, 3, 8)[-1] == (1, 1) and X.level_sizes(5, 3, 2) == [(5, 3), (3, 2), (2, 1)]


# ---- 3. the mutants ------------------------------------------------------------------------------------------------------------------------

def _result(c, mutant):
    """arrays of a case's result under a mutant, each with the thing under test (pixel or tile) as its first axis"""
    if c.family == "progressive":
        st = EC.run_progressive(c, mutant)
        lst, count = PN.compact(st.retired, mutant)
        tiles = sorted(c.expect)
        return [np.stack([st.epochs, st.retired, st.outliers, st.max_e.view(np.uint32)], axis=1)[tiles].astype(np.uint32).view(f32),
                np.r_[count, lst[:count]].astype(np.uint32).view(f32)]
    if c.family == "vdenoise":
        col, var, _ = EC.run_vdenoise(c, mutant)
        return [col[c.test], var[c.test]]
    if c.family == "denoise":
        return [EC.run_denoise(c, mutant)[c.test]]
    if c.family == "tvdenoise":
        col, var, _, _, A = EC.run_tvdenoise(c, mutant)
        return [col[c.test], var[c.test], A[c.test]]
    r = EC.run_display(c, mutant)
    out = [np.array([r["e"], r["state"][0], r["state"][1]], f32), r["d"][c.test], r["image"].reshape(-1).astype(f32)]
    return out + ([] if r["bloom"] is None else [r["bloom"][c.test]])


def _differs(c, mutant):
    if c.family == "progressive_wide":
        n, _, outliers, _ = c.expect[0]
        return PN.retires(n, outliers, c.w * c.h, 2, 999, mutant) != PN.retires(n, outliers, c.w * c.h, 2, 999)
    return any(a.shape != b.shape or not np.array_equal(np.ascontiguousarray(a).view(np.uint32)[~(np.isnan(a) & np.isnan(b))],
                                                        np.ascontiguousarray(b).view(np.uint32)[~(np.isnan(a) & np.isnan(b))])
               for a, b in zip(_result(c, mutant), _result(c, None)))


KILLS = [(c, k) for c in CASES for k in c.kills]


@pytest.mark.parametrize("c,kill", KILLS, ids=[f"{c.name}-{k}" for c, k in KILLS])
def test_every_case_differs_from_the_mutants_it_names(c, kill, oracle):
    module, mutant = kill.split(":")
    assert mutant in EC.MODULES[module].MUTANTS
    assert _differs(c, mutant), (c.name, kill)


def test_every_mutant_is_named_by_a_case():
    named = {k for c in CASES for k in c.kills}
    every = {f"{m}:{mutant}" for m, mod in EC.MODULES.items() for mutant in mod.MUTANTS}
    assert every - named == set(), sorted(every - named)
    assert named - every == set()
    for name in ("e_ge", "retire_lt", "epochs_gt", "u32_products", "nominal_tile_pixels", "fnn_u32"):
        assert name in PN.MUTANTS
    assert {"v_gt0", "fnn_u32", "border_le", "nan_weight_counts"} <= set(VN.MUTANTS) and {"border_le", "nan_weight_counts"} <= set(DN.MUTANTS)
    assert {"nprime_gt4", "nprime_gt1", "d_ge0"} <= set(TV.MUTANTS) and {"meter_ge0", "no_floor", "adapt_always_blend", "quant_round"} <= set(X.MUTANTS)
    assert PN.EQUIVALENT == ("maxe_ge",) and VN.EQUIVALENT == ("n_ge1",) and X.EQUIVALENT == ("reinhard_ge0",)


def test_the_equivalent_readings_change_no_case(oracle):
    """maxe_ge (progressive_np), n_ge1 (denoise_variance_np) and reinhard_ge0 (display_np): the arguments stand beside their EQUIVALENT
    tuples; not a bit of any case moves, the cases with e = 0, n = 1 and lx = +0 / -0.0 among them"""
    for c in CASES:
        if c.family == "progressive":
            a, b = EC.run_progressive(c), EC.run_progressive(c, "maxe_ge")
            assert np.array_equal(a.max_e.view(np.uint32), b.max_e.view(np.uint32)) and np.array_equal(a.retired, b.retired), c.name
        elif c.family == "vdenoise":
            assert all(same(x, y) for x, y in zip(EC.run_vdenoise(c), EC.run_vdenoise(c, "n_ge1"))), c.name
        elif c.family == "display" and c.display.tone == "reinhard":
            a, b = EC.run_display(c), EC.run_display(c, "reinhard_ge0")
            assert np.array_equal(a["d"].view(np.uint32), b["d"].view(np.uint32)) and np.array_equal(a["image"], b["image"]), c.name
    assert any(c.name == "display/reinhard/gate" for c in CASES) and any(c.name == "progressive/outlier/one_epoch" for c in CASES)
    # n = 1 in the accumulate itself: e is NaN whatever the film holds (m2 is +0 or NaN after one epoch), so n >= 1 reports nothing either
    c = next(c for c in CASES if c.name == "progressive/outlier/one_epoch")
    st = EC.run_progressive(c)
    with np.errstate(all="ignore"):
        e = (np.sqrt(st.m2 / f32(0.0)) / np.abs(st.mean_y)).astype(f32)
    assert np.isnan(e).all() and ((st.m2 == 0) | np.isnan(st.m2)).all() and not np.signbit(st.m2[st.m2 == 0]).any()


# ---- 4. what the older GPU inputs can see --------------------------------------------------------------------------------------------------
# COPIES of the input loops of the older device tests (test_progressive_device.py::test_accumulate_and_compaction_match_the_restatement,
# test_denoise_device.py, test_denoise_variance_device.py, test_temporal_variance_device.py, test_display_device.py): whoever changes a
# loop there changes it here; the call counts asserted below guard the copies.

def _notices(calls, run, mutants):
    """{mutant: the number of calls whose result differs from the statement's in any bit}; run(call, mutant) -> a list of arrays"""
    calls = list(calls)
    want = [run(a, None) for a in calls]
    count = {}
    for m in mutants:
        count[m] = sum(any(not bits_equal(x, y) for x, y in zip(run(a, m), w)) for a, w in zip(calls, want))
    return len(calls), count


def test_what_the_older_progressive_inputs_notice():
    """retired / outliers / max_e after every one of the 105 accumulate calls.  No call notices `e >=` for the outlier, the 32-bit
    products, the nominal tile size, the 32-bit n (n - 1), or a compaction without its carry (no grid has more than 1024 tiles)."""
    import rayn_amd as R
    shapes = [((1, 1), (1, 1)), ((7, 1), (4, 1)), ((17, 13), (8, 8)), ((33, 65), (16, 16)), ((300, 200), (64, 48)), ((300, 200), (16, 16))]
    switches = [dict(), dict(adaptive=False), dict(target_error=0.0, noise_floor=0.0, min_epochs=2, outlier_permille=0),
                dict(target_error=0.3, noise_floor=0.01, min_epochs=3, outlier_permille=500), dict(target_error=0.02, min_epochs=2, outlier_permille=1000),
                dict(target_error=1.0, noise_floor=1.0, min_epochs=2, outlier_permille=1)]
    mutants = (None,) + PN.MUTANTS + PN.EQUIVALENT
    noticed, calls = dict.fromkeys(mutants, 0), 0
    for si, ((w, h), tile) in enumerate(shapes):
        n_tiles = len(PN.tile_rects(w, h, *tile))
        assert n_tiles <= PN.CHUNK
        rng = np.random.default_rng(si)
        for sw_i, sw in enumerate(switches if w * h < 60000 else switches[:3]):
            prog = R.Progressive(**sw)
            kw = dict(target_error=prog.target_error, noise_floor=prog.noise_floor, min_epochs=prog.min_epochs, outlier_permille=prog.outlier_permille,
                      adaptive=prog.adaptive)
            states = {m: PN.State(w, h, tile) for m in mutants}
            for epoch in range(1 + (si + sw_i) % 6):
                film = PC.film(w, h, 100 * si + 10 * sw_i + epoch, special=bool((epoch + sw_i) % 2))
                if epoch % 3 == 2:
                    film = {k: (np.float32(0.5) + np.float32(1e-3) * v).astype(f32) for k, v in film.items()}
                tiles = None
                if epoch % 2 == 1 and n_tiles > 1:
                    tiles = np.sort(rng.choice(n_tiles, max(1, n_tiles // 3), replace=False)).astype(np.uint32)
                calls += 1
                for m, st in states.items():
                    PN.accumulate(st, film, tiles, mutant=m, **kw)
                a = states[None]
                for m, st in states.items():
                    lists = [PN.compact(s.retired, m if s is st else None) for s in (st, a)]
                    noticed[m] += not (np.array_equal(st.retired, a.retired) and np.array_equal(st.outliers, a.outliers) and
                                       np.array_equal(st.max_e.view(np.uint32), a.max_e.view(np.uint32)) and
                                       lists[0][1] == lists[1][1] and np.array_equal(lists[0][0][:lists[0][1]], lists[1][0][:lists[1][1]]))
    print("progressive:", calls, noticed)
    assert calls == 105 and noticed[None] == 0
    for m in ("e_ge", "u32_products", "nominal_tile_pixels", "fnn_u32", "compact_no_carry", "maxe_ge"):
        assert noticed[m] == 0, (m, noticed[m])
    assert (noticed["retire_lt"], noticed["epochs_gt"], noticed["percent"]) == (5, 17, 2)


SIGMAS_D = list(itertools.product((0.0, 0.5), (0.0, 0.4), (0.0, 0.3)))
SIGMAS_V = list(itertools.product((0.0, 4.0), (0.0, 0.4), (0.0, 0.3)))
SPECIAL = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 3.0e38, -3.0e38, 1e-45, -np.nan, 1e30], f32)
# the a-trous replays leave the 300x200 shape of the older tests out: the same random draw, nine times the pixels, minutes on a CPU


def _adversarial_film(w, h, seed, extra=()):
    film = random_film(w, h, seed)
    rng = np.random.default_rng(seed + 100)
    for arr in [film[k] for k in ("color", "normal", "alpha")] + list(extra):
        flat = arr.reshape(-1)
        idx = rng.choice(flat.size, min(flat.size, 4 * SPECIAL.size), replace=False)
        flat[idx] = np.resize(SPECIAL, idx.size)
    film["normal"][rng.choice(w * h, max(1, w * h // 10), replace=False)] = 0.0
    return film


def test_what_the_older_denoise_inputs_notice(oracle):
    """test_denoise_device.py's random and adversarial films (the shapes up to 33x65): 104 calls.  The border reading is noticed (a tap
    one step beyond reads a pixel that differs); a NaN weight needs inf - inf in a guide, which the adversarial films do hold."""
    calls = []
    for si, (w, h) in enumerate([(1, 1), (1, 7), (7, 1), (17, 13), (33, 65)]):
        film = random_film(w, h, si)
        calls += [(film, w, h, L, s) for L, s in [(L, SIGMAS_D[(L + si) % 8]) for L in range(1, 9)] + [(3, s) for s in SIGMAS_D]]
    for seed, (w, h) in enumerate([(1, 1), (7, 1), (17, 13), (33, 65)]):
        film = _adversarial_film(w, h, seed)
        calls += [(film, w, h, L, s) for L, s in [(1, (0.5, 0.4, 0.3)), (4, (0.5, 0.4, 0.3)), (2, (2.0 ** -30, 2.0 ** 30, 0.3)), (3, (2.0 ** 30, 0.0, 2.0 ** -30)),
                                                  (5, (0.0, 0.0, 0.0)), (8, (0.5, 0.0, 0.3))]]
    run = lambda a, m: [DN.atrous(a[0]["color"], a[0]["alpha"], a[0]["normal"], a[1], a[2], a[3], *a[4], mutant=m)]
    n, count = _notices(calls, run, DN.MUTANTS)
    print("denoise:", n, count)
    assert n == 104
    assert (count["border_le"], count["nan_weight_counts"], count["zero_weight_skipped"]) == OLDER["denoise"]


def _random_state(w, h, tile, seed):
    rng = np.random.default_rng(seed + 1000)
    n, t = w * h, len(PN.tile_rects(w, h, *tile))
    m2 = rng.gamma(1.0, 0.05, n).astype(f32)
    m2[rng.choice(n, max(1, n // 16), replace=False)] = 0.0
    epochs = rng.choice(np.array([0, 1, 2, 5, 64], np.uint32), t)
    if t >= 2:
        epochs[rng.choice(t, 2, replace=False)] = (2, 64)
    else:
        epochs[0] = 5
    for _ in range(5):
        rng.normal(size=(n, 3))  # the draws of the planes the denoiser does not read keep the generator where the older test has it
    return {"m2": m2, "epochs": epochs.astype(np.uint32)}


def test_what_the_older_variance_denoiser_inputs_notice(oracle):
    """test_denoise_variance_device.py's synthetic films and states (the shapes up to 50x37).  No call notices the 32-bit n (n - 1): the
    epoch counts stop at 64."""
    calls = []
    shapes = [((1, 1), (1, 1)), ((1, 7), (1, 2)), ((7, 1), (3, 1)), ((17, 13), (16, 16)), ((33, 65), (8, 8)), ((33, 65), (11, 13)), ((50, 37), (16, 16))]
    for si, ((w, h), tile) in enumerate(shapes):
        film, state = random_film(w, h, si), _random_state(w, h, tile, si)
        calls += [(film, state, w, h, tile, L, s) for L, s in [(L, SIGMAS_V[(L + si) % 8]) for L in range(1, 9)] + [(3, s) for s in SIGMAS_V]]
    for seed, ((w, h), tile) in enumerate([((1, 1), (1, 1)), ((7, 1), (3, 1)), ((17, 13), (16, 16)), ((33, 65), (8, 8)), ((50, 37), (16, 16))]):
        state = _random_state(w, h, tile, seed)
        film = _adversarial_film(w, h, seed, extra=(state["m2"],))
        calls += [(film, state, w, h, tile, L, s) for L, s in [(1, (4.0, 0.4, 0.3)), (4, (4.0, 0.4, 0.3)), (2, (2.0 ** -30, 2.0 ** 30, 0.3)),
                                                              (3, (2.0 ** 30, 0.0, 2.0 ** -30)), (5, (0.0, 0.0, 0.0)), (8, (1.0, 0.0, 0.3))]]
    run = lambda a, m: list(VN.denoise(a[0]["color"], a[0]["alpha"], a[0]["normal"], a[1]["m2"], a[1]["epochs"], a[2], a[3], a[4], a[5], *a[6], mutant=m))
    n, count = _notices(calls, run, VN.MUTANTS + VN.EQUIVALENT)
    print("denoise_variance:", n, count)
    assert n == 142 and count["fnn_u32"] == 0 and count["n_ge1"] == 0
    assert (count["v_gt0"], count["border_le"], count["nan_weight_counts"], count["zero_weight_skipped"], count["prefilter_counts_unguided"]) == OLDER["denoise_variance"]


def test_what_the_older_temporal_variance_inputs_notice(oracle):
    """test_temporal_variance_device.py::test_variance_estimate_and_passes_match_the_restatement: 16 calls at 37x23 and 2 at 1x1.  n'
    takes 3.5 and 4.0 but never below(4.0), so `> 4` is noticed through the 4.0 alone; d = -0.0 does not occur."""
    inp = TC.pack_inputs(37, 23, 7)
    calls = [(37, 23, inp, L, s) for L, s in itertools.product((1, 3), SIGMAS_V)]
    one = TC.pack_inputs(1, 1, 3)
    one["color"][:], one["normal"][:], one["alpha"][:], one["obj"][:], one["mom"][:] = (0.5, 0.25, 0.75), (0.0, 0.6, 0.8), 1.0, 1, (0.5, 0.3)
    for n_hist in (1.0, 4.0):
        calls.append((1, 1, dict(one, n1=np.full(1, n_hist, f32)), 2, (4.0, 0.4, 0.3)))
    run = lambda a, m: list(TV.denoise(a[0], a[1], a[2]["color"], a[2]["alpha"], a[2]["normal"], a[2]["obj"], a[2]["n1"], a[2]["mom"], a[3], *a[4], mutant=m))
    n, count = _notices(calls, run, TV.MUTANTS)
    print("temporal_variance:", n, count)
    assert n == 18 and count["d_ge0"] == 0
    assert (count["nprime_gt4"], count["nprime_gt1"]) == OLDER["temporal_variance"]


def test_what_the_older_display_inputs_notice(oracle):
    """test_display_device.py's two sweeps over display_cases.film (every shape, 300x220 included: the one where a metered pixel of luminance 0 could be expected).  The
    meter's gate and floor need three special components in one pixel: of 360 calls 2 notice `l >= 0` (none below 300x220) and 5 the
    missing floor."""
    from rayn_amd.film import Bloom, Display
    shapes = [(1, 1), (1, 7), (7, 1), (17, 13), (33, 65), (255, 1), (256, 1), (257, 1), (300, 220)]
    arms = [(True, True, True), (False, True, False), (False, False, False)]
    combos = list(itertools.product(("linear", "reinhard", "aces"), ("auto", 1.5), (0, 1, 3, 8)))
    disp = lambda tone, exposure, levels: Display(exposure=exposure, tone=tone, bloom=Bloom(0.8, 0.6, levels) if levels else None)

    def film(w, h, seed, arm, adversarial):
        transparent, with_bg, with_alpha = arms[arm]
        color, background, alpha = display_film(w, h, seed, adversarial, with_bg, with_alpha)
        return color, background, alpha, transparent
    calls = []
    for si, (w, h) in enumerate(shapes):
        for i, (tone, exposure, levels) in enumerate(combos):
            arm, adversarial = (i + si) % 3, bool((i // 3 + si) % 2)
            calls.append((w, h, film(w, h, 10 * si + i, arm, adversarial), disp(tone, exposure, levels)))
    for arm, adversarial in itertools.product((0, 1, 2), (False, True)):
        f = film(33, 65, 50 + arm, arm, adversarial)
        calls += [(33, 65, f, disp(*combo)) for combo in combos]

    def run(a, m):
        w, h, (color, background, alpha, transparent), display = a
        r = X.display(color, w, h, display.to_abi(1.0), background, alpha, transparent, mutant=m)
        return [r["d"], r["image"].astype(f32), np.array([r["m"], r["e"]], f32)] + ([] if r["bloom"] is None else [r["bloom"]])
    n, count = _notices(calls, run, X.MUTANTS + X.EQUIVALENT)
    print("display:", n, count)
    assert n == 360 and count["reinhard_ge0"] == 0 and count["adapt_always_blend"] == 0  # every older call has adapt = 1 and a fresh state
    assert (count["meter_ge0"], count["no_floor"], count["quant_round"], count["bright_fin_after"]) == OLDER["display"]


# the counts the replays above measure, beside the zeros asserted in place (the zeros are the gaps the cases close)
OLDER = {"denoise": (79, 10, 4), "denoise_variance": (130, 70, 15, 5, 61), "temporal_variance": (17, 17), "display": (2, 5, 292, 59)}
