"""The rows of tests/sdf_cases.py without a GPU: the oracle's SDF::dist against the numpy statement of it (tests/restatement_np.py) in every bit on every row
under both mul_add policies, and the case generator against what it claims - the finite and distinct shares of the reference distances, what every structured
point group is named for (counted from the statement's own intermediates), and the fast_div == 0 column against a restatement of the window rule."""
import numpy as np
import pytest

import restatement_np as RN
import sdf_cases as SC
from common import bits_equal

BOX_ROWS = [r["name"] for r in SC.ROWS if r["kind"] != "bulb"]  # the statement restates the MandelBox and the sphere SDF, not the Mandelbulb extension


@pytest.fixture(scope="module")
def cases():
    out = {}
    for r in SC.ROWS:
        wd, p, idx = SC.scene(r)
        pts, groups = SC.points(r)
        out[r["name"]] = dict(row=r, wd=wd, p=p, idx=idx, h=wd.hitables[idx], pts=pts, groups=groups)
    return out


@pytest.mark.parametrize("fma", [False, True])
@pytest.mark.parametrize("name", BOX_ROWS)
def test_oracle_dist_equals_the_statement(oracle, cases, name, fma):
    c = cases[name]
    cols = [np.ascontiguousarray(c["pts"][:, k]) for k in range(3)]
    for t0 in c["row"]["t0s"]:
        ref = oracle.sdf_dist(c["h"], c["pts"], fma=fma, t0=t0)
        with RN.fused_policy(fma):
            got = RN.mandelbox_dist(cols, c["h"], np.full(len(c["pts"]), np.float32(t0), np.float32))
        assert bits_equal(got, ref), (name, t0, int((got.view(np.uint32) != ref.view(np.uint32)).sum()))
    if len(c["row"]["t0s"]) > 1:  # the time reaches the distance
        a, b = [oracle.sdf_dist(c["h"], c["pts"], fma=fma, t0=t) for t in c["row"]["t0s"][:2]]
        assert not bits_equal(a, b)
        assert bits_equal(oracle.sdf_dist(c["h"], c["pts"], fma=fma, t0=0.0), oracle.sdf_dist(c["h"], c["pts"], fma=fma))


@pytest.mark.parametrize("name", SC.ROW_NAMES)
def test_reference_distances_are_finite_and_distinct(oracle, cases, name):
    c = cases[name]
    for fma in (False, True):
        ref = oracle.sdf_dist(c["h"], c["pts"], fma=fma, t0=c["row"]["t0s"][-1])
        fin = np.isfinite(ref)
        if c["row"]["nonfinite"]:
            assert fin.mean() < 0.5, "named as an overflow row, yet mostly finite"
            continue
        assert fin.mean() >= 0.99, (name, fin.mean())
        assert len(np.unique(ref[fin].view(np.uint32))) >= 0.95 * fin.sum(), (name, len(np.unique(ref[fin])), int(fin.sum()))
        assert np.isnan(ref[c["groups"]["nan_inf"]][0])  # a NaN component gives a NaN distance


def test_rows_cover_both_sides_of_every_gate():
    E = {r["name"]: r["expect"] for r in SC.ROWS}
    for key in ("fd0", "single", "bulb", "anim"):
        assert {e[key] for e in E.values()} == {True, False}, key
    box = [r for r in SC.ROWS if r["kind"] == "box" and not r["expect"]["fd0"]]
    its = {r["sdf"]["it"] for r in box}
    assert {0, 1, 3, 4, 5, 11, 12, 13, 16} <= its
    assert len(SC.VERDICT_PAIRS) >= 32 and len(set(SC.VERDICT_PAIRS)) == len(SC.VERDICT_PAIRS) and (0.01, 1.9) in SC.VERDICT_PAIRS
    assert len(set(SC.ROW_NAMES)) == len(SC.ROW_NAMES)


def test_generator_pairs_are_the_randomised_parity_tests_draws():
    """the MandelBox the randomised-parity generator builds for seed 3, drawn the long way, has the pair the verdict list holds for it"""
    rng = np.random.default_rng(1003)
    int(rng.integers(17, 49)), int(rng.integers(9, 33)), bool(rng.integers(0, 2)), int(rng.integers(5, 15))
    float(np.float32(rng.uniform(-2.6, -1.7) if rng.integers(0, 2) else rng.uniform(1.8, 2.8)))
    float(np.float32(rng.uniform(0.7, 1.3)))
    mr, fr = float(np.float32(rng.uniform(0.005, 0.6))), float(np.float32(rng.uniform(0.8, 2.2)))
    assert SC.VERDICT_PAIRS[1 + 3] == (mr, fr)
    assert all(0.005 <= a <= 0.6 and 0.8 <= b <= 2.2 for a, b in SC.VERDICT_PAIRS[1:17])


@pytest.mark.parametrize("name", SC.ROW_NAMES)
def test_expected_fast_div_0_is_the_window_rule(cases, name):
    c = cases[name]
    h = c["h"]
    want_fd0 = not (h.sdf_kind == 1 and SC.in_window(h))  # the other SDFs leave the fold constants 0: outside the window
    assert c["row"]["expect"]["fd0"] == want_fd0


def test_verdict_pairs_lie_inside_the_window():
    for a, b in SC.VERDICT_PAIRS:
        wd, _, idx = SC.scene(SC.verdict_row(a, b))
        assert SC.in_window(wd.hitables[idx]), (a, b)


@pytest.mark.parametrize("name", [r["name"] for r in SC.ROWS if r["kind"] == "box"])
def test_structured_groups_do_what_their_names_say(cases, name):
    c = cases[name]
    h, pts, g = c["h"], c["pts"], c["groups"]
    assert g["uniform"] == slice(0, SC.N_UNIFORM) and len(pts) == g["nan_inf"].stop
    assert np.isnan(pts[g["nan_inf"]][0]).any() and np.isinf(pts[g["nan_inf"]][1]).any() and np.isfinite(pts[: g["nan_inf"].start]).all()
    assert (pts[g["origin_axes"]][0] == 0).all() and ((pts[g["origin_axes"]] != 0).sum(1) <= 1).all()
    l = np.float32(h.box_side)
    lf = np.float32(abs(l)) if np.isfinite(l) and l != 0 and abs(l) < 1e6 else np.float32(1.0)
    assert (np.abs(pts[g["far"]]).max(1) > 3.0 * lf).all() and np.abs(pts[g["far"]]).max() <= 105.0 * lf
    assert ((np.abs(pts[g["fold_planes"]]) == lf).sum(1) >= 1).all() and {1, 2, 3} <= set((np.abs(pts[g["fold_planes"]]) == lf).sum(1).tolist())
    lad = np.abs(pts[g["ladder_axis"]]).max(1)
    assert lad.min() == np.float32(2.0 ** -40) and lad.max() == 4.0 and len(pts[g["ladder_diag"]]) == 43
    for fma in (False, True):
        with RN.fused_policy(fma):
            mrs, frs = np.float32(h.min_radius) * np.float32(h.min_radius), np.float32(h.fixed_radius) * np.float32(h.fixed_radius)
            if h.iterations >= 1 and np.isfinite(l) and l > 0 and 0 < mrs:
                for k in ("ladder_axis", "ladder_diag"):  # some lane's denominator is min_radius^2 itself, some lane's is its own r2
                    r2, den, folds = SC.first_fold(pts[g[k]], h)
                    assert (den == mrs).any() and ((den == r2) & (r2 > mrs)).any(), (name, k)
                    if mrs <= frs:
                        assert (folds & (den == mrs)).any()
            if c["row"]["dyadic"]:
                assert min(len(pts[g[k]]) for k in ("r2_eq_frs", "r2_ulp_below_frs", "r2_eq_mrs")) >= 32
                r2, den, folds = SC.first_fold(pts[g["r2_eq_frs"]], h)
                assert (r2 == frs).all() and not folds.any()
                r2, den, folds = SC.first_fold(pts[g["r2_ulp_below_frs"]], h)
                assert (r2 == np.nextafter(frs, np.float32(0))).all() and folds.all() and (den == r2).all()
                r2, den, folds = SC.first_fold(pts[g["r2_eq_mrs"]], h)
                assert (r2 == mrs).all() and (den == mrs).all() and folds.all()


@pytest.mark.parametrize("name", SC.ROW_NAMES)
def test_rays_meet_the_sky_and_the_sdf_where_it_has_a_surface(oracle, cases, name):
    """what the device test's object-id assertion rests on: in the reference the rays of SC.rays() see the sky and - except on the rows named as having no
    surface - the row's SDF, at both depths the device test marches"""
    c = cases[name]
    org, d = SC.rays()
    assert len(org) == 8192 - 13 and np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-6)
    for depth in (0, 2):
        _, obj = oracle.closest_hit(c["wd"], c["p"], depth, org, d)
        ids = set(np.unique(obj).tolist())
        assert 0 in ids and (c["idx"] in ids) == c["row"]["hits_sdf"], (name, depth, sorted(ids))


def test_admissible_arms():
    assert SC.admissible_arms(1, 12, 2) == [(-1, 0), (-1, 1), (-1, 2), (1, 0), (1, 1), (1, 2), (100, 2)]
    assert SC.admissible_arms(1, 5, 2) == [(-1, 0), (-1, 1), (-1, 2), (1, 0), (1, 1), (1, 2)]
    assert SC.admissible_arms(2, 8, 0) == [(-1, 0), (2, 0)] and SC.admissible_arms(0, 0, 0) == [(-1, 0), (0, 0)]
