"""The families of tests/sphere_cases.py without a GPU: the oracle's Sphere::hit and Sphere::occluded (oracle_probe_shading ops 13 and 14) against the numpy
statement (tests/restatement_np.py) in every bit under both mul_add policies; every family against the decision it is named for, counted from the statement's
float32 intermediates; planted mutants of the statement, each of which must change an output of the case set; and the fold worlds' exact ties.

Also held here, on every lane of every family: the device's form of the occlusion test - Sphere::occluded plus the two early-outs of sphere_occluded_dir
(device_core.h), restated in sphere_cases.occ_np(early=True) - equals the literal one, which is the claim the early-outs' comment makes."""
import numpy as np
import pytest

import restatement_np as RN
import sphere_cases as SC
from common import bits_equal

f32 = np.float32
POLICIES = [False, True]


@pytest.fixture(scope="module")
def world():
    return SC.probe_world()


@pytest.fixture(scope="module")
def cases(world):
    wd, _ = world
    return {fma: dict(hit=SC.hit_cases(wd, fma), occ=SC.occ_cases(wd, fma)) for fma in POLICIES}


def _by_family(groups):
    out = {}
    for fam, idx, rec in groups:
        out.setdefault(fam, []).append((idx, rec))
    return out


def _near(x, y, ulps=2):
    return np.abs(SC._ord(x) - SC._ord(y)) <= ulps


# ---- the oracle against the statement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fma", POLICIES)
def test_oracle_hit_equals_the_statement(oracle, world, cases, fma):
    wd, _ = world
    lanes = {}
    for fam, idx, rec in cases[fma]["hit"]:
        h = wd.hitables[idx]
        ref = oracle.probe_shading(wd, 13, idx, rec, fma=fma)[:, 0]
        with RN.fused_policy(fma), np.errstate(all="ignore"):
            got = RN.sphere_hit(h, SC._cols(rec, 0), SC._cols(rec, 3), rec[:, 6].copy(), rec[:, 7].copy())
            own = SC.hit_np(h, rec)
        assert bits_equal(got, ref), (fam, idx, int((got.view(np.uint32) != ref.view(np.uint32)).sum()))
        assert bits_equal(own, ref), (fam, idx)  # the mutable copy the mutants are planted in is the statement
        nan_t = np.isnan(rec[:, 7])
        assert (ref[nan_t] == SC.F32_MAX).all(), (fam, idx)  # the time of a packet whose lane 0 is empty: a miss
        lanes[fam] = lanes.get(fam, 0) + len(rec)
    print("hit lanes per family:", lanes, "total", sum(lanes.values()))
    assert {"H1", "H2", "H2x", "H3", "H4", "H5", "H6"} == set(lanes) and sum(lanes.values()) >= 250000


@pytest.mark.parametrize("fma", POLICIES)
def test_oracle_occluded_equals_the_statement_and_the_early_outs_are_exact(oracle, world, cases, fma):
    wd, _ = world
    lanes, early = {}, 0
    for fam, idx, rec in cases[fma]["occ"]:
        h = wd.hitables[idx]
        ref = oracle.probe_shading(wd, 14, idx, rec, fma=fma)[:, 0]
        with RN.fused_policy(fma), np.errstate(all="ignore"):
            got = RN.sphere_occluded(h, SC._cols(rec, 0), SC._cols(rec, 3), rec[:, 6].copy())
            own, dev = SC.occ_np(h, rec), SC.occ_np(h, rec, early=True)
            p = SC.occ_parts(h, rec)
        assert bits_equal(got, ref), (fam, idx, int((got != ref).sum()))
        assert bits_equal(own, ref), (fam, idx)
        assert bits_equal(dev, ref), (fam, idx, "an early-out of sphere_occluded_dir changes the result", int((dev != ref).sum()))
        early += int(((p["b"] >= 0) | (p["c"] < SC.EARLY_C)).sum())
        nan_t = np.isnan(rec[:, 6])
        assert (ref[nan_t] == 1.0).all(), (fam, idx)  # NaN time: not occluded
        assert set(np.unique(ref).tolist()) <= {0.0, 1.0}
        lanes[fam] = lanes.get(fam, 0) + len(rec)
    print("occlusion lanes per family:", lanes, "total", sum(lanes.values()), "lanes an early-out takes:", early)
    assert {"O1", "O2", "O3", "O4", "O4g", "O4x", "O5", "O6", "O7"} == set(lanes) and sum(lanes.values()) >= 250000 and early > 10000


def test_the_moving_sphere_moves(oracle, world):
    """the lane time reaches the centre: the same ray meets the moving sphere at time 0 and misses it at 0.37; -0.0 is time 0"""
    wd, _ = world
    C = SC._centre_at(wd, SC.MOVING, 0.0)
    rec = SC._rec_hit(np.tile(C - f32([0, 0, 3]), (3, 1)), f32([0, 0, 1]), f32(200.0), f32([0.0, -0.0, 0.37]))
    t = oracle.probe_shading(wd, 13, SC.MOVING, rec)[:, 0]
    assert t[0] < 3.0 and t[0] == t[1] and t[2] == SC.F32_MAX
    for op, n in ((13, 8), (14, 7)):
        for idx in (99, 16):
            with pytest.raises(ValueError):
                oracle.probe_shading(wd, op, idx, np.zeros((1, n), f32))


def test_ops_refuse_a_traced_sdf(oracle):
    wd, _, _ = SC.fold_world("F2")
    for op, n in ((13, 8), (14, 7)):
        with pytest.raises(ValueError):
            oracle.probe_shading(wd, op, 2, np.zeros((1, n), f32))
        oracle.probe_shading(wd, op, 1, np.zeros((1, n), f32))


# ---- each family reaches its target ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fma", POLICIES)
def test_hit_families_reach_their_decisions(world, cases, fma):
    wd, _ = world
    fams = _by_family(cases[fma]["hit"])
    with RN.fused_policy(fma):
        # H1: every sign of the discriminant in at least 1 % of the lanes
        d = np.concatenate([SC.hit_parts(wd.hitables[i], r)["descrim"] for i, r in fams["H1"]])
        share = {k: float(m.mean()) for k, m in (("pos", d > 0), ("zero", d == 0), ("neg", d < 0))}
        print("H1", len(d), share)
        assert min(share.values()) >= 0.01, share
        # H2 (+ H2x): both arms and the miss; the exact threshold from both arms
        arms = dict(t1=0, t2=0, miss=0, t1_eq=0, t2_eq=0)
        for i, r in fams["H2"] + fams["H2x"]:
            p, t = SC.hit_parts(wd.hitables[i], r), SC.hit_np(wd.hitables[i], r)
            hit = t < SC.F32_MAX
            arms["t1"] += int((hit & (t == p["t1"]) & (p["t1"] < p["t2"])).sum())
            arms["t2"] += int((hit & (t == p["t2"]) & ~(p["t1"] > SC.T_HIT)).sum())
            arms["miss"] += int((~hit).sum())
            arms["t1_eq"] += int(((p["t1"] == SC.T_HIT) & (p["descrim"] > 0)).sum())
            arms["t2_eq"] += int(((p["t2"] == SC.T_HIT) & (p["descrim"] > 0) & ~hit).sum())
        print("H2", arms)
        assert min(arms.values()) > 0, arms
        for i, r in fams["H2"]:  # per sphere a unit ray can resolve: the walk crosses the threshold (outcomes on both sides within the walk)
            rad = float(wd.hitables[i].radius)
            if 1e-3 <= rad <= 100.0 and not np.isnan(r[0, 7]):
                p, t = SC.hit_parts(wd.hitables[i], r), SC.hit_np(wd.hitables[i], r)
                took_t1, missed = (t == p["t1"]) & (p["t1"] > SC.T_HIT), t == SC.F32_MAX
                if (p["t1"] > 0).any():  # the origin outside: t1 crosses the threshold - t1 on one side of it, the far root t2 on the other
                    assert took_t1.any() and ((t == p["t2"]) & ~took_t1 & ~missed).any(), (i, rad)
                else:                    # the origin inside: t2 crosses it - a hit on one side, a miss on the other
                    assert (t == p["t2"]).any() and missed.any(), (i, rad)
        # H3: for every base ray, t_max == root hits at that root and t_max == nextbelow(root) does not - for the root the ray is met at (t1 from outside, t2 from inside)
        n_base = 0
        for i, r in fams["H3"]:
            h = wd.hitables[i]
            p, t = SC.hit_parts(h, r), SC.hit_np(h, r)
            blocks = [slice(k * 32, (k + 1) * 32) for k in range(6)]  # t_max = below / at / above t1, then t2
            for lo, hi, key in ((0, 16, "t1"), (16, 32, "t2")):
                base = 0 if key == "t1" else 3
                below, at = blocks[base], blocks[base + 1]
                root = p[key][at][lo:hi]
                assert (root > SC.T_HIT).all() and (p["descrim"][at][lo:hi] > 0).all(), (i, key)
                assert (r[at, 6][lo:hi] == root).all() and (r[below, 6][lo:hi] == SC.nextbelow(root)).all()
                assert (t[at][lo:hi] == root).all(), (i, key, "t_max == root must hit")
                assert (t[below][lo:hi] == SC.F32_MAX).all(), (i, key, "t_max just below the root must miss")
                n_base += hi - lo
            assert (t[192:208] == SC.F32_MAX).all() and (t[208:224] == SC.F32_MAX).all()  # inside: t_max between the roots, and below both
        print("H3 base rays", n_base)
        assert n_base == 32 * len(fams["H3"]) and len(fams["H3"]) >= 9
        # H4: from inside a dome the far root is the hit
        for i, r in fams["H4"]:
            p, t = SC.hit_parts(wd.hitables[i], r), SC.hit_np(wd.hitables[i], r)
            inside = p["c"] < 0  # (1e-3 from the wall of the radius-1e4 dome is below its ulp: some of those starts round onto the wall or past it)
            assert inside.mean() > 0.95 and ((t == p["t2"]) | (t == SC.F32_MAX))[inside].all() and (t == p["t2"]).mean() > 0.95
        assert len(fams["H4"]) == 2
        # H5: the operands the family names are there
        r5 = np.concatenate([r for _, r in fams["H5"]])
        assert np.isnan(r5).any() and np.isinf(r5).any() and (r5[:, 3:6] == 0).all(1).any() and np.signbit(r5[:, 3:6][r5[:, 3:6] == 0]).any()
        assert {0.0, -1.0, float(SC.F32_MAX), float("inf")} <= set(r5[:, 6].tolist())
        big = np.abs(r5[:, 0:3]).max(1)
        assert ((big > 5e18) & (big < 2e19)).any() and ((big > 1.5e19) & (big < 1e20)).any()
        for i, r in fams["H5"]:
            p = SC.hit_parts(wd.hitables[i], r)
            if wd.hitables[i].animated == 0:
                oc0 = [(r[:, c] == f32((wd.hitables[i].center.x, wd.hitables[i].center.y, wd.hitables[i].center.z)[c])) for c in range(3)]
                assert (oc0[0] & oc0[1] & oc0[2]).any() and (oc0[0] & ~oc0[1]).any()
            assert np.isnan(p["descrim"]).any()
        # H6: aimed and arbitrary, hits and misses, unnormalised directions
        for i, r in fams["H6"]:
            t = SC.hit_np(wd.hitables[i], r)
            nrm = np.linalg.norm(r[:, 3:6].astype(np.float64), axis=1)
            assert len(r) == SC.N_RANDOM and (np.abs(nrm - 1) > 0.01).mean() > 0.04
            if float(wd.hitables[i].radius) >= 1e-3 and not np.isnan(r[0, 7]):
                assert 0.05 < (t < SC.F32_MAX).mean() < 1.0, (i, float((t < SC.F32_MAX).mean()))


@pytest.mark.parametrize("fma", POLICIES)
def test_occlusion_families_reach_their_decisions(world, cases, fma):
    wd, _ = world
    fams = _by_family(cases[fma]["occ"])
    with RN.fused_policy(fma):
        # O1: b on both sides of zero and, somewhere, at it
        b = np.concatenate([SC.occ_parts(wd.hitables[i], r)["b"] for i, r in fams["O1"]])
        print("O1", len(b), int((b > 0).sum()), int((b == 0).sum()), int((b < 0).sum()))
        assert (b > 0).mean() > 0.2 and (b < 0).mean() > 0.2 and (b == 0).any()
        for i, r in fams["O1"]:
            bb = SC.occ_parts(wd.hitables[i], r)["b"]
            if len(r) == 64 and not np.isnan(r[0, 6]):  # every walk crosses zero
                assert (bb >= 0).any() and (bb < 0).any(), i
            elif len(r) == 4 and not np.isnan(r[0, 6]):  # the axis-aligned segments give the exact zero
                assert (bb == 0).all(), i
        # O2: for each tiny radius c on both sides of the early-out's constant - where r^2 can reach it: c >= -r^2, so a sphere with r^2 <= 1e-30 has no
        # c < -1e-30 and that side is asserted empty
        for i, r in fams["O2"]:
            h = wd.hitables[i]
            if float(h.radius) > 3e-15:
                continue
            p = SC.occ_parts(h, r)
            r2 = f32(f32(h.radius) * f32(h.radius))
            below, mid = int((p["c"] < SC.EARLY_C).sum()), int(((p["c"] >= SC.EARLY_C) & (p["c"] <= 0)).sum())
            print("O2 radius", float(h.radius), "r^2", float(r2), "c < -1e-30:", below, "-1e-30 <= c <= 0:", mid, "c > 0:", int((p["c"] > 0).sum()))
            assert mid > 0 and (below > 0) == bool(-r2 < SC.EARLY_C), (float(h.radius), below, mid)
            assert (p["c"] > 0).any()
        assert sum(1 for i, _ in fams["O2"] if -f32(f32(wd.hitables[i].radius) ** 2) < SC.EARLY_C and float(wd.hitables[i].radius) <= 3e-15) >= 1
        # O3: b * b underflows
        b = np.concatenate([SC.occ_parts(wd.hitables[i], r)["b"] for i, r in fams["O3"]])
        with np.errstate(all="ignore"):
            assert ((b != 0) & (np.abs(b) < 1e-23) & ((b * b).astype(f32) == 0)).sum() >= 8
        # O4 / O5: both outcomes within 2 ulp of the threshold
        o4 = dict(above=0, at_or_below=0)
        o4["exact"] = 0
        for i, r in fams["O4"] + fams["O4x"]:
            p, occ = SC.occ_parts(wd.hitables[i], r), SC.occ_np(wd.hitables[i], r)
            o4["exact"] += int(((p["t1"] == SC.T_OCC) & (p["descrim"] > 0) & (occ == 1)).sum())
            m = _near(p["t1"], SC.T_OCC) & (p["descrim"] > 0)
            o4["above"] += int((m & (occ == 0)).sum())
            o4["at_or_below"] += int((m & (occ == 1)).sum())
            assert ((occ == 0) == ((SC.RN.smin(p["t1"], p["t2"]) > SC.T_OCC) & (p["t1"] <= p["dist"]) & (p["descrim"] > 0))).all()
        print("O4 within 2 ulp of 0.001:", o4)
        assert min(o4.values()) > 0, o4
        o5 = dict(reaches=0, short=0, exact=0)
        for i, r in fams["O5"]:
            p, occ = SC.occ_parts(wd.hitables[i], r), SC.occ_np(wd.hitables[i], r)
            m = _near(p["dist"], p["t1"]) & (p["t1"] > SC.T_OCC)
            o5["reaches"] += int((m & (occ == 0)).sum())
            o5["short"] += int((m & (occ == 1)).sum())
            o5["exact"] += int((m & (p["dist"] == p["t1"]) & (occ == 0)).sum())
        print("O5 within 2 ulp of dist == t1:", o5)
        assert min(o5.values()) > 0, o5
        # O6: zero-length, non-finite and 1e-30 segments are all "not occluded"
        for i, r in fams["O6"]:
            p = SC.occ_parts(wd.hitables[i], r)
            assert (p["dist"] == 0).any() and np.isnan(p["b"]).any()
            assert ((r[:, 0:3] != r[:, 3:6]).any(1) & (p["dist"] == 0)).any()  # the square of a length of 1e-30 underflows: dist 0 between distinct ends
            assert (SC.occ_np(wd.hitables[i], r) == 1.0).all()
        # O7: a third of the ends on the light proxy; some segments occluded by the spheres a segment of the box can meet
        for i, r in fams["O7"]:
            L = wd.lights[0]
            on = np.abs(np.linalg.norm(r[:, 3:6].astype(np.float64) - [L.pos.x, L.pos.y, L.pos.z], axis=1) - L.rad) < 1e-5
            assert len(r) == SC.N_RANDOM and 0.3 < on.mean() < 0.4
            if 0.1 < float(wd.hitables[i].radius) < 100.0 and not np.isnan(r[0, 6]) and r[0, 6] == 0:
                assert (SC.occ_np(wd.hitables[i], r) == 0).mean() > 0.002, i


# ---- planted mutants ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fma", POLICIES)
@pytest.mark.parametrize("mut", SC.HIT_MUTANTS)
def test_hit_mutant_is_killed(world, cases, fma, mut):
    wd, _ = world
    changed = {}
    with RN.fused_policy(fma):
        for fam, idx, rec in cases[fma]["hit"]:
            a, b = SC.hit_np(wd.hitables[idx], rec), SC.hit_np(wd.hitables[idx], rec, mut=mut)
            changed[fam] = changed.get(fam, 0) + int((a.view(np.uint32) != b.view(np.uint32)).sum())
    print(mut, changed)
    assert sum(changed.values()) > 0, mut


@pytest.mark.parametrize("fma", POLICIES)
@pytest.mark.parametrize("mut", SC.OCC_MUTANTS)
def test_occlusion_mutant_is_killed(world, cases, fma, mut):
    wd, _ = world
    changed = {}
    with RN.fused_policy(fma):
        for fam, idx, rec in cases[fma]["occ"]:
            a, b = SC.occ_np(wd.hitables[idx], rec, early=True), SC.occ_np(wd.hitables[idx], rec, mut=mut, early=True)
            changed[fam] = changed.get(fam, 0) + int((a != b).sum())
    print(mut, changed)
    assert sum(changed.values()) > 0, mut


@pytest.mark.parametrize("fma", POLICIES)
@pytest.mark.parametrize("mut", SC.OCC_EQUIVALENT)
def test_equivalent_early_outs_change_nothing(world, cases, fma, mut):
    """`b >= -1e-6`, `c < 1e-30f` and `c < 0` for the shipped early-outs: no input tells them apart (the argument stands next to sphere_cases.OCC_MUTANTS), and
    no lane of the case set does - the lanes that sit between the shipped constant and the mutant's are counted, so the statement is not empty"""
    wd, _ = world
    between = 0
    with RN.fused_policy(fma):
        for fam, idx, rec in cases[fma]["occ"]:
            h = wd.hitables[idx]
            assert bits_equal(SC.occ_np(h, rec, early=True), SC.occ_np(h, rec, mut=mut, early=True)), (mut, fam, idx)
            p = SC.occ_parts(h, rec)
            if mut.startswith("early_b"):
                between += int(((p["b"] < 0) & (p["b"] >= f32(-1e-6))).sum())
            else:
                between += int(((p["c"] >= SC.EARLY_C) & (p["c"] < (f32(1e-30) if mut == "early_c_1e-30" else f32(0))) & (p["b"] < 0)).sum())
    print(mut, "lanes between the two constants:", between)
    assert between >= 16, (mut, between)


# ---- the fold worlds --------------------------------------------------------------------------------------------------------------------
def _sphere_ties(wd, org, d, rt):
    """rays on which two analytic spheres of different index return the winning distance rt itself: (mask, lowest such index per ray)"""
    n = len(org)
    count, first = np.zeros(n, np.int32), np.full(n, 0xFFFFFFFF, np.uint32)
    for k in range(wd.n_hitables):
        if wd.hitables[k].kind != 0:
            continue
        ts = SC.hit_np(wd.hitables[k], SC._rec_hit(org, d, rt, 0.0))
        eq = (ts == rt) & (ts < SC.F32_MAX)
        first = np.where(eq & (count == 0), np.uint32(k), first)
        count += eq
    return count >= 2, first


@pytest.mark.parametrize("fma", POLICIES)
@pytest.mark.parametrize("name", ["F1", "F2", "F3"])
def test_fold_worlds_hold_exact_sphere_ties(oracle, name, fma):
    wd, p, single = SC.fold_world(name)
    assert sum(1 for k in range(wd.n_hitables) if wd.hitables[k].kind != 0) == {"F1": 0, "F2": 1, "F3": 2}[name] and (single >= 0) == (name == "F2")
    org, d = SC.fold_rays(wd, fma)
    assert len(org) == SC.N_FOLD and SC.N_FOLD % 64 != 0
    for depth in (0, 2):
        rt, robj = oracle.closest_hit(wd, p, depth, org, d, fma=fma)
        with RN.fused_policy(fma):
            tie, first = _sphere_ties(wd, org, d, rt)
        print(name, "depth", depth, "exact sphere-against-sphere ties:", int(tie.sum()), "objects met:", sorted(np.unique(robj).tolist()))
        assert tie.sum() >= 1
        assert (robj[tie] == first[tie]).all(), "the lower index wins a tie"
        met = set(np.unique(robj).tolist())
        assert 0xFFFFFFFF in met and {k for k in range(wd.n_hitables) if wd.hitables[k].kind != 0} <= met
        dup = [k for k in range(1, wd.n_hitables) if wd.hitables[k].kind == 0 and any(
            wd.hitables[j].kind == 0 and wd.hitables[j].radius == wd.hitables[k].radius and wd.hitables[j].center.x == wd.hitables[k].center.x for j in range(k))]
        assert dup and not (met & set(dup)), (dup, met)  # a duplicate at a higher index never wins, also across the SDF
        if name == "F1":
            with RN.fused_policy(fma):
                t, obj, ties = SC.fold_np(wd, p, org, d)
                t2, obj2, _ = SC.fold_np(wd, p, org, d, le=True)
            assert bits_equal(t, rt) and np.array_equal(obj, robj) and ties > 0
            assert (obj != obj2).sum() > 0 and bits_equal(t, t2), "the planted `<=` of the fold must move an object index"


@pytest.mark.parametrize("fma", POLICIES)
@pytest.mark.parametrize("which", ["pre", "post"])
@pytest.mark.parametrize("depth", [0, 2])
def test_sphere_against_sdf_brackets_straddle(oracle, depth, which, fma):
    org, d, side, exact, pairs, (s_lo, s_hi) = SC.sdf_tie_rays(oracle, fma, depth, which)
    print(f"sphere-against-SDF ({which}, depth {depth}, fma {fma}): {pairs} aim pairs, {len(org)} rays, exact ties {exact}")
    assert pairs >= 200 and len(org) >= 2 * pairs
    assert (s_lo >= 0).all() and (s_hi <= 0).all() and (s_lo > 0).any() and (s_hi < 0).any()  # the final bracket: the SDF nearer (or a tie) / the sphere nearer (or a tie)
    wd, p, _ = SC.fold_world("F2")
    rt, robj = oracle.closest_hit(wd, p, depth, org, d, fma=fma)
    si = 1 if which == "pre" else 4
    free = np.isin(robj, [2, si, 5])  # (a few of the rays pass through another sphere of the world on their way)
    assert free.mean() > 0.95, float(free.mean())
    assert set(np.unique(robj[free & (side > 0)]).tolist()) == {2} and set(np.unique(robj[free & (side < 0)]).tolist()) <= {si, 5}
    assert (robj[free & (side == 0)] == (si if which == "pre" else 2)).all()  # an exact tie goes to the lower index: the sphere before the SDF, the SDF before the sphere after it
