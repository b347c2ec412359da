"""tests/reproject_cases.py held to account without a GPU: every case's hand-written outcome holds on the numpy restatements, every case
differs from each mutant it names on a pixel under test, every entry of every MUTANTS tuple is named by a case, the equivalent readings
change no case - and the reason the file exists: on the inputs the older GPU tests feed k_temporal_accumulate, four of the wrong readings
are noticed by no call at all."""
import numpy as np
import pytest

import reproject_cases as RC
import temporal_cases as TC
import temporal_np as T
import temporal_resample_np as TR
from common import bits_equal

f32 = np.float32
CASES = RC.all_cases()
IDS = [c.name for c in CASES]
ACC = [c for c in CASES if c.entry in ("accumulate", "tiny")]


def _same_n(got, want):
    return np.isnan(want) | (got.view(np.uint32) == want.view(np.uint32))


def _blended(out, color):
    return (out.view(np.uint32) != color.view(np.uint32)).any(axis=1)


def _check_accumulate(c, out, hist, what):
    n1 = np.ascontiguousarray(hist[0][:, 3])
    bad = ~_same_n(n1, c.n1)
    assert not bad.any(), (c.name, what, "n'", np.nonzero(bad)[0][:8], n1[bad][:8], c.n1[bad][:8])
    bad = (c.blended != RC.UNKNOWN) & (_blended(np.ascontiguousarray(out, f32), c.color) != (c.blended == 1))
    assert not bad.any(), (c.name, what, "blended", np.nonzero(bad)[0][:8])


# ---- 1. the hand-written outcomes ----------------------------------------------------------------------------------------------------------

def test_names_are_unique_and_every_case_has_pixels_under_test():
    assert len(set(IDS)) == len(IDS)
    for c in CASES:
        assert c.test.any(), c.name
        assert c.entry != "accumulate" or not c.test.all(), (c.name, "no control pixel")


@pytest.mark.parametrize("c", ACC, ids=[c.name for c in ACC])
def test_accumulate_outcomes_hold_on_every_restatement_of_the_accumulate(c):
    """n' and blended as written, on temporal_np, on temporal_resample_np with resample 0 (with and without moments), and on
    temporal_upscale_np at factor 1 without a low camera and confidence - all four the same bits"""
    out, hist = RC.run_accumulate(c)
    _check_accumulate(c, out, hist, "temporal_np")
    for moments in (False, True):
        r = RC.run_resample(c, 0, moments)
        assert bits_equal(r[0], out) and all(bits_equal(a, b) for a, b in zip(r[1][:3], hist[:3])), (c.name, moments)
    planes, _, thist, _ = RC.run_temporal_upscale_1(c)
    assert bits_equal(planes["color"], out) and all(bits_equal(a, b) for a, b in zip(thist[:3], hist[:3])), c.name
    assert np.array_equal(thist[3], hist[3])
    if getattr(c, "not_cubic", False):  # a tiny image never takes the cubic arm
        assert not (RC.run_resample(c, 1)[3] == TR.ARM_CUBIC).any()


@pytest.mark.parametrize("size", ["16x8", "32x16"])
def test_the_edges_are_where_the_cases_say(size):
    """the compared quantities ARE the bounds: te and tol of the depth cases, the dot product of the normal cases, te = +0 and -0, the
    border coordinates, the NaN length behind fminf"""
    by = {c.name: c for c in CASES}
    c = by[f"depth/bound/{size}"]
    ok, fx, fy, te = T.project(c.prev_cam, 0.0, [c.rec[:, 0], c.rec[:, 1], c.rec[:, 2]], c.w, c.h)
    assert ok.all() and (te == f32(4.0)).all() and f32(0.25) * f32(4.0) == f32(1.0)
    xs, ys = np.meshgrid(np.arange(c.w), np.arange(c.h), indexing="xy")
    assert np.array_equal(fx, xs.reshape(-1).astype(f32)) and np.array_equal(fy, ys.reshape(-1).astype(f32))
    d = np.abs(c.prev[1][c.test, 3] - f32(4.0))
    assert sorted(d[np.isfinite(d)].tolist()) == sorted([1.0, float(RC.above(5.0) - f32(4.0)), 1.0, float(f32(4.0) - RC.below(3.0)), float(RC.below(5.0) - f32(4.0)), float(f32(4.0) - RC.above(3.0))])
    c = by[f"normal/floor/{size}"]
    dots = T.dot([c.normal[:, 0], c.normal[:, 1], c.normal[:, 2]], [c.prev[2][:, 0], c.prev[2][:, 1], c.prev[2][:, 2]])[c.test]
    assert {f32(0.8), RC.above(0.8), RC.below(0.8)} <= set(dots[np.isfinite(dots)].tolist()) and c.tp[2] == float(f32(0.8))
    for name in ("projection/ortho", "projection/ortho_negative_zero"):
        c = by[f"{name}/{size}"]
        ok, _, _, te = T.project(c.prev_cam, 0.0, [c.rec[:, 0], c.rec[:, 1], c.rec[:, 2]], c.w, c.h)
        assert (te[c.zero_te] == 0).all() and (np.signbit(te[c.zero_te]) == c.te_sign).all() and not ok[c.zero_te].any(), (name, te[c.zero_te])
    c = by[f"projection/ortho/{size}"]
    _, _, _, te = T.project(c.prev_cam, 0.0, [c.rec[:, 0], c.rec[:, 1], c.rec[:, 2]], c.w, c.h)
    assert te[5 + 3 * c.w] == f32(4.0) - RC.below(4.0) > 0 and te[8 + 3 * c.w] < 0  # one ulp in front of the plane, one behind it
    for kind in ("pinhole", "thin_lens"):
        c = by[f"projection/{kind}/{size}"]
        ok, fx, fy, te = T.project(c.prev_cam, 0.0, [c.rec[:, 0], c.rec[:, 1], c.rec[:, 2]], c.w, c.h)
        z = c.rec[:, 2]
        assert not ok[z == 4].any() and ok[z == RC.below(4.0)].all() and (te[z == RC.below(4.0)] == f32(4.0) - RC.below(4.0)).all()
        assert (fx[ok] == f32(c.w / 2 - 0.5)).all() and (fy[ok] == f32(c.h / 2 - 0.5)).all()
    for c in CASES:
        if c.name.startswith(("border/", "interpolate/border/")) and c.name.endswith(size):
            cam = c.prev_cam if c.entry == "accumulate" else c.ka.camera
            _, fx, fy, _ = T.project(cam, 0.0, [c.rec[:, 0], c.rec[:, 1], c.rec[:, 2]], c.w, c.h)
            want_x, want_y = {float(t) for t, _ in c.targets[0]} | {3.0}, {float(t) for t, _ in c.targets[1]} | {2.0}
            assert set(fx.tolist()) == want_x and set(fy.tolist()) == want_y, (c.name, sorted(set(fx.tolist())), sorted(want_x))
    c = by[f"blend/cap/{size}"]
    W = RC.run_accumulate(c, want_taps=True)[2]
    q = 8 + 5 * c.w
    assert np.isinf(c.prev[0][q, 3]) and (W[[q - 1, q - c.w, q - c.w - 1]] == 1).all()  # the inf length sits on a tap of weight 0: N is NaN
    # the luminance moments of the overflow pixel: the colour blended, y * y overflowed, (y, y2) is stored
    out, hist, mom, _ = RC.run_resample(c, 0, moments=True)
    p = c.moments_overflow
    assert hist[0][p, 3] == 3 and mom[p, 0] > 1e38 and np.isposinf(mom[p, 1])
    # the same projection edges through both keys of the interpolation, the perspective cameras' zc = 0 and one ulp either side included
    for kind in ("pinhole", "thin_lens"):
        c = by[f"interpolate/projection/{kind}/{size}"]
        assert c.perspective and c.ka.camera.kind == c.kb.camera.kind != 2
        z = c.rec[c.test, 2]
        assert {4.0, float(RC.below(4.0)), float(RC.above(4.0))} <= set(z[np.isfinite(z)].tolist())


RESAMPLE = [c for c in CASES if c.entry == "resample"]


@pytest.mark.parametrize("c", RESAMPLE, ids=[c.name for c in RESAMPLE])
def test_catmull_rom_arms_hold(c):
    out, hist, _, arm, raw = RC.run_resample(c, 1, want_unclamped=True)
    known = c.arm != RC.UNKNOWN
    assert np.array_equal(arm[known], c.arm[known]), (c.name, np.nonzero(known & (arm != c.arm))[0][:8])
    assert (arm[c.test] == TR.ARM_CUBIC).any() or "beyond" in c.name
    n1 = np.ascontiguousarray(hist[0][:, 3])
    assert _same_n(n1, c.n1).all(), (c.name, n1[~_same_n(n1, c.n1)])
    if hasattr(c, "resampled"):  # the constant history resamples to exactly lo == hi
        assert (raw[c.test] == f32(c.resampled)).all()
    if hasattr(c, "at_lo"):  # the resampled value IS lo (and hi) of an inner range with lo < hi, and the clamp leaves it there
        inner = lambda p: np.stack([c.prev[0][p + d, 0] for d in (0, 1, c.w, c.w + 1)])
        assert (inner(c.at_lo).min(axis=0) == c.lo).all() and (inner(c.at_lo).max(axis=0) == c.hi).all() and c.lo < c.hi
        assert (inner(c.at_hi).min(axis=0) == c.lo).all() and (inner(c.at_hi).max(axis=0) == c.hi).all()
        assert (raw[c.at_lo] == f32(c.lo)).all() and (raw[c.at_hi] == f32(c.hi)).all()
        for ps, h in ((c.at_lo, f32(c.lo)), (c.at_hi, f32(c.hi))):
            a = (f32(1.0) / hist[0][ps, 3])[:, None]
            assert bits_equal(out[ps], (h + (a * (c.color[ps] - h).astype(f32)).astype(f32)).astype(f32))
    if hasattr(c, "clamped_to"):  # the spike rings, the clamp takes it back
        assert (raw[c.test] != f32(c.clamped_to)).all(axis=1).all()
        a = (f32(1.0) / hist[0][c.test, 3])[:, None]
        h = f32(c.clamped_to)
        assert bits_equal(out[c.test], (h + (a * (c.color[c.test] - h).astype(f32)).astype(f32)).astype(f32))
    # with moments the arms are the same
    assert np.array_equal(RC.run_resample(c, 1, moments=True)[3], arm)


UPSCALE = [c for c in CASES if c.entry == "upscale"]


@pytest.mark.parametrize("c", UPSCALE, ids=[c.name for c in UPSCALE])
def test_upscale_tiers_hold(c):
    planes, weight, tier, _ = RC.run_upscale(c)
    known = c.tier != 0
    assert np.array_equal(tier[known], c.tier[known]), (c.name, np.nonzero(known & (tier != c.tier))[0][:8])
    if getattr(c, "denormal", False):
        assert ((weight > 0) & (weight < np.finfo(f32).tiny)).all()
    if getattr(c, "finite_alpha", False):
        assert np.isfinite(planes["alpha"][c.test]).all() and not np.isfinite(planes["alpha"]).all()
    # the supersampling entry takes the same tier; its confidence is the largest b of the tier that gave the value
    for conf in (False, True):
        info = RC.run_temporal_upscale(c, conf)[3]
        assert np.array_equal(info["tier"], tier)
        if conf and hasattr(c, "conf"):
            assert (info["conf"][c.test] == f32(c.conf)).all()


INTERP = [c for c in CASES if c.entry == "interpolate"]


@pytest.mark.parametrize("c", INTERP, ids=[c.name for c in INTERP])
def test_interpolation_sources_hold(c):
    planes, source = RC.run_interpolate(c)
    assert np.array_equal(source, c.source), (c.name, np.nonzero(source != c.source)[0][:8], source[source != c.source][:8])
    if hasattr(c, "takes_a"):
        for k in ("alpha", "background", "normal"):
            assert bits_equal(planes[k][c.takes_a], np.asarray(c.ka.film[k], f32).reshape(planes[k].shape)[c.takes_a])
    if getattr(c, "finite_alpha", False):
        assert np.isfinite(planes["alpha"][c.test]).all() and not np.isfinite(planes["alpha"]).all()


# ---- 2. the mutants ------------------------------------------------------------------------------------------------------------------------

def _result(c, module, mutant):
    """the arrays of a case's result under one module's restatement, each with the pixel as its first axis"""
    if c.entry in ("accumulate", "tiny"):
        if module == "T":
            out, hist = RC.run_accumulate(c, mutant)
        else:
            planes, _, hist, _ = RC.run_temporal_upscale_1(c, mutant)
            out = planes["color"]
        return [out, hist[0]]
    if c.entry == "resample":
        out, hist = RC.run_resample(c, 1, mutant=mutant)[:2]
        return [out, hist[0]]
    if c.entry == "upscale":
        if module == "U":
            planes, weight, _, _ = RC.run_upscale(c, mutant)
            return list(planes.values()) + [weight]
        planes, weight, hist, _ = RC.run_temporal_upscale(c, True, mutant)
        return list(planes.values()) + [weight, hist[0]]
    planes, source = RC.run_interpolate(c, mutant)
    return list(planes.values()) + [source.view(f32)]


def _differs(c, module, mutant):
    want, got = _result(c, module, None), _result(c, module, mutant)
    return any(not bits_equal(np.ascontiguousarray(a[c.test]), np.ascontiguousarray(b[c.test])) for a, b in zip(got, want))


KILLS = [(c, k) for c in CASES for k in c.kills]


@pytest.mark.parametrize("c,kill", KILLS, ids=[f"{c.name}-{k}" for c, k in KILLS])
def test_every_case_differs_from_the_mutants_it_names(c, kill):
    module, mutant = kill.split(":")
    assert mutant in RC.MODULES[module].MUTANTS
    assert _differs(c, module, mutant), (c.name, kill)


def test_every_mutant_is_named_by_a_case():
    named = {k for c in CASES for k in c.kills}
    every = {f"{m}:{mutant}" for m, mod in RC.MODULES.items() for mutant in mod.MUTANTS}
    assert every - named == set(), sorted(every - named)
    assert named - every == set()


@pytest.mark.parametrize("mutant", T.EQUIVALENT)
def test_the_equivalent_readings_change_no_case(mutant):
    """zc_ge and w_ge (the arguments are in temporal_np's docstring): not a bit of any accumulate case, of the interpolation cases, or of
    the adversarial sweep below moves"""
    for c in ACC:
        want, got = RC.run_accumulate(c), RC.run_accumulate(c, mutant)
        assert bits_equal(got[0], want[0]) and bits_equal(got[1][0], want[1][0]), (c.name, mutant)
    if mutant == "zc_ge":
        assert sum(c.perspective for c in INTERP if hasattr(c, "perspective")) >= 4  # pinhole and thin-lens keys with zc = 0 and +-1 ulp
        for c in INTERP:
            want, got = RC.run_interpolate(c), RC.run_interpolate(c, mutant)
            assert np.array_equal(got[1], want[1]) and all(bits_equal(got[0][k], want[0][k]) for k in want[0])
    assert _sweep_notices(mutant) == 0


# ---- 3. what the older GPU inputs can see --------------------------------------------------------------------------------------------------

_SWEEP = {}


def _sweep_notices(mutant):
    """the number of those calls whose colour or history differs from the statement's in any bit under the mutant"""
    if not _SWEEP:
        _SWEEP["calls"] = list(TC.older_accumulate_calls())
        _SWEEP["want"] = [T.accumulate(*a) for a in _SWEEP["calls"]]
    count = 0
    for a, want in zip(_SWEEP["calls"], _SWEEP["want"]):
        got = T.accumulate(*a, mutant=mutant)
        count += not (bits_equal(got[0], want[0]) and bits_equal(got[1][0], want[1][0]))
    return count


def test_the_older_gpu_inputs_notice_none_of_four_wrong_readings():
    """The finding the cases answer: of the 111 calls behind the two older device tests, some notice `<= tol` read as `<`, `n_tap >= 1` as
    `>` and the normal switch - and not one notices `>= normal_min` read as `>`, `te > 0` as `>=`, or a NaN nh propagating through the cap
    (and none can notice zc_ge: test_the_equivalent_readings_change_no_case).  Every one of those is killed by a case above."""
    assert _sweep_notices(None) == 0 and len(_SWEEP["calls"]) == 111
    assert _sweep_notices("depth_lt") > 0 and _sweep_notices("ntap_gt") > 0 and _sweep_notices("normal_switch_ge") > 0
    for mutant in ("normal_gt", "te_ge", "fmin_is_minimum"):
        assert _sweep_notices(mutant) == 0, mutant
        assert any(f"T:{mutant}" in c.kills for c in CASES)
