"""The reference of the instrumented kernels' counters (oracle/rayn_oracle.cpp, "PER-LANE accounting"), checked without a GPU before the device is held to it
(tests/test_counters_device.py): against the independent numpy restatement per ray, against closed-form anchors, against itself (frame totals = sums of the
per-ray exports over the frame's own rays), and for the conditions each scene of the device tests is there for - so that none of those can pass vacuously.
Every comparison is == on integers."""

import numpy as np
import pytest

import counter_cases as CC
import march_cases as M
import restatement_np as RS

N_RAYS = 5 * 128 + 37  # five periods of the corner classes (march_cases: period 128) and a ragged tail
RAY_SEED, SEG_SEED = 41, 31


def _cols(x):
    return [np.ascontiguousarray(x[:, c]) for c in range(3)]


def restated_closest_hit_evals(wd, p, depth, org, d):
    """HitableStore::add_hits with tests/restatement_np.py, every ray a lane of its own: the evaluations each ray is charged over all TracedSDFs."""
    n = len(org)
    o, dd = _cols(org), _cols(d)
    half_pixel = RS.camera_constants(wd.camera)[4]
    if depth == 0:
        thr_at = (lambda t: np.full(len(t), half_pixel, np.float32)) if wd.camera.kind == 2 else (lambda t: (half_pixel * t).astype(np.float32))
    else:
        k = np.float32(np.float32(np.float32(0.0001) * np.float32(2.0)) * np.float32(depth))
        thr_at = lambda t, k=k: (k * t).astype(np.float32)
    closest = np.full(n, np.float32(np.float32(p.world_radius) * np.float32(2.0)), np.float32)
    evals = np.zeros(n, np.int64)
    t0 = np.zeros(n, np.float32)
    with np.errstate(all="ignore"):
        for i in range(wd.n_hitables):
            h = wd.hitables[i]
            t = RS.sphere_hit(h, o, dd, closest, t0) if h.kind == 0 else RS.sdf_hit(h, o, dd, closest, thr_at, p.sdf_detail_scale, int(p.max_marches), t0, evals=evals)
            closest = np.where(t < closest, t, closest).astype(np.float32)
    return evals


def restated_shadow_evals(wd, p, a, b):
    """A parked segment with tests/restatement_np.py: the TracedSDFs in index order, up to and including the first that occludes."""
    n = len(a)
    aa, bb = _cols(a), _cols(b)
    evals = np.zeros(n, np.int64)
    live = np.ones(n, bool)
    t0 = np.zeros(n, np.float32)
    with np.errstate(all="ignore"):
        for i in range(wd.n_hitables):
            h = wd.hitables[i]
            if h.kind == 0:
                continue
            mine = np.zeros(n, np.int64)
            occ = RS.sdf_occluded(h, aa, bb, p.sdf_detail_scale, int(p.max_vis_marches), t0, evals=mine)
            evals += np.where(live, mine, 0)
            live &= occ != 0
    return evals


# ---- 1. the independent restatement, per ray ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fma", [False, True], ids=["unfused", "fused"])
@pytest.mark.parametrize("budget", [0, 1, 12, None])
@pytest.mark.parametrize("name,depth", [("s1", 0), ("s1", 2), ("s0", 0)])
def test_closest_hit_counts_equal_the_restatement(oracle, name, depth, budget, fma):
    kw = {} if budget is None else {"max_marches": budget}
    wd, p = M.probe_world(name, **kw)
    org, d = M.rays(N_RAYS, RAY_SEED)
    t, obj, ev, it = oracle.closest_hit_counts(wd, p, depth, org, d, fma=fma)
    rt, robj = oracle.closest_hit(wd, p, depth, org, d, fma=fma)
    assert np.array_equal(obj, robj) and M.same_t(t, rt).all()  # the counting entry is the plain one plus two outputs
    with RS.fused_policy(fma):
        mine = restated_closest_hit_evals(wd, p, depth, org, d)
    bad = ev.astype(np.int64) != mine
    assert not bad.any(), M.describe_mismatches(bad, M._RAY_SLOTS, M.RAY_CLASSES)
    sdf = [wd.hitables[k] for k in range(wd.n_hitables) if wd.hitables[k].kind != 0]
    assert len(sdf) == 1 and np.array_equal(it, ev * CC.steps_per_eval(sdf[0]))
    if budget is None:
        assert len(np.unique(ev)) > 20  # marches of many lengths


@pytest.mark.parametrize("fma", [False, True], ids=["unfused", "fused"])
@pytest.mark.parametrize("budget", [0, 1, 5, None])
@pytest.mark.parametrize("name", ["s1", "s0"])
def test_shadow_counts_equal_the_restatement(oracle, name, budget, fma):
    kw = {} if budget is None else {"max_vis_marches": budget}
    wd, p = M.probe_world(name, sdf_only=True, **kw)
    a, b = M.segments(N_RAYS, SEG_SEED)
    vis, ev, it = oracle.shadow_counts(wd, p, a, b, fma=fma)
    assert np.array_equal(vis, oracle.test_occluded(wd, p, a, b, fma=fma))
    with RS.fused_policy(fma):
        mine = restated_shadow_evals(wd, p, a, b)
    bad = ev.astype(np.int64) != mine
    assert not bad.any(), M.describe_mismatches(bad, M._SEG_SLOTS, M.SEG_CLASSES)
    assert np.array_equal(it, ev * CC.steps_per_eval(wd.hitables[0]))
    if budget is None:
        assert len(np.unique(ev)) > 20


def test_shadow_counts_stop_at_the_first_occluding_sdf(oracle):
    """Several TracedSDFs: the per-segment count is the sum over the SDFs in index order up to the first that occludes, each SDF's own count taken from a world
    that holds it alone; the visibility is still the product over all of them."""
    wd, p = M.probe_world("two_sdfs", sdf_only=True)
    a, b = M.segments(4 * N_RAYS, SEG_SEED)
    vis, ev, it = oracle.shadow_counts(wd, p, a, b)
    assert np.array_equal(vis, oracle.test_occluded(wd, p, a, b))
    assert wd.n_hitables == 3
    want_ev, want_it, live = np.zeros(len(a), np.int64), np.zeros(len(a), np.int64), np.ones(len(a), bool)
    stopped_at = np.full(len(a), 3)
    for k in range(3):
        one, _ = M.probe_world("two_sdfs", sdf_only=True)
        one.hitables[0] = wd.hitables[k]
        one.n_hitables = 1
        v1, e1, i1 = oracle.shadow_counts(one, p, a, b)
        want_ev += np.where(live, e1, 0); want_it += np.where(live, i1, 0)
        stopped_at = np.where(live & (v1 == 0), k, stopped_at)
        live &= v1 != 0
    assert np.array_equal(ev, want_ev) and np.array_equal(it, want_it)
    assert np.array_equal(vis == 0, stopped_at < 3)
    assert all((stopped_at == k).sum() > 10 for k in range(4)), np.bincount(stopped_at)  # every exit of the early-out, and segments no SDF occludes


# ---- 2. closed-form anchors ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["s1", "s0", "bulb", "two_sdfs"])
def test_zero_march_budget_costs_one_evaluation_per_sdf(oracle, name):
    wd, p = M.probe_world(name, max_marches=0)
    org, d = M.rays(N_RAYS, RAY_SEED)
    _, _, ev, it = oracle.closest_hit_counts(wd, p, 0, org, d)
    assert (ev == CC.n_sdfs(wd)).all()
    if name != "bulb":
        assert (it == sum(CC.steps_per_eval(wd.hitables[k]) for k in range(wd.n_hitables) if wd.hitables[k].kind != 0)).all()
    wd, p = M.probe_world(name, sdf_only=True, max_vis_marches=0)
    a, b = M.segments(N_RAYS, SEG_SEED)
    vis, ev, _ = oracle.shadow_counts(wd, p, a, b)
    if name == "two_sdfs":
        assert ((ev >= 1) & (ev <= 3)).all() and (ev[vis == 1] == 3).all() and set(np.unique(ev)) == {1, 2, 3}
    else:
        assert (ev == 1).all()


@pytest.mark.parametrize("name", ["s1", "s0", "bulb", "two_sdfs"])
def test_nan_inputs_cost_their_closed_form(oracle, name):
    """A NaN first distance: the ray stops in its first trip (2 evaluations per SDF with a budget, 1 without); the segment enters no trip (1 per SDF, and
    no SDF occludes it, so it reaches them all)."""
    org, d = M.rays(N_RAYS, RAY_SEED)
    nan_ray = M.ray_class(np.arange(N_RAYS)) == M.RAY_CLASSES.index("nan_origin")
    a, b = M.segments(N_RAYS, SEG_SEED)
    nan_seg = M.seg_class(np.arange(N_RAYS)) == M.SEG_CLASSES.index("nan_start")
    assert nan_ray.sum() >= 5 and nan_seg.sum() >= 5
    for budget, per_sdf in ((1, 2), (12, 2), (None, 2), (0, 1)):
        wd, p = M.probe_world(name, **({} if budget is None else {"max_marches": budget}))
        _, _, ev, _ = oracle.closest_hit_counts(wd, p, 2, org, d)
        assert (ev[nan_ray] == per_sdf * CC.n_sdfs(wd)).all(), budget
    for budget in (0, 1, 5, None):
        wd, p = M.probe_world(name, sdf_only=True, **({} if budget is None else {"max_vis_marches": budget}))
        vis, ev, _ = oracle.shadow_counts(wd, p, a, b)
        assert (ev[nan_seg] == wd.n_hitables).all() and (vis[nan_seg] == 1).all(), budget


def test_mandelbulb_orbit_steps(oracle):
    wd, p = M.probe_world("bulb")
    h = [wd.hitables[k] for k in range(wd.n_hitables) if wd.hitables[k].kind != 0][0]
    n_it = int(h.iterations)
    assert h.sdf_kind == 2 and n_it >= 3
    pts = np.array([[0, 0, 0], [20, 0, 0], [np.nan, 0, 0], [0.3, 0.2, 0.1], [1.2, 0.1, 0.0]], np.float32)
    steps = oracle.sdf_steps(h, pts)
    # the origin's orbit turns NaN (0 * inf) and a NaN never bails out; |(20, 0, 0)|^2 leaves the bailout radius in the first step
    assert steps[0] == n_it and steps[1] == 1 and steps[2] == n_it and steps[3] == n_it and 1 <= steps[4] <= n_it
    rng = np.random.default_rng(3)
    cloud = rng.uniform(-1.6, 1.6, (20000, 3)).astype(np.float32)
    s = oracle.sdf_steps(h, cloud)
    assert s.min() >= 1 and s.max() == n_it and len(np.unique(s)) == n_it  # every exit of the loop
    # the steps are those of an orbit restated here in binary32, operation for operation (oracle Mandelbulb::dist)
    assert np.array_equal(s, _bulb_steps(cloud, n_it))
    zero = type(h).from_buffer_copy(h)
    zero.iterations = 0
    assert (oracle.sdf_steps(zero, cloud[:100]) == 0).all()
    # MandelBox: `iterations` whatever the point; sphere SDF: 0
    for name, want in (("s1", None), ("s0", 0)):
        w2, _ = M.probe_world(name, sdf_only=True)
        assert (oracle.sdf_steps(w2.hitables[0], pts) == (int(w2.hitables[0].iterations) if want is None else want)).all()


def _bulb_steps(pts, iterations):
    f = np.float32
    out = np.zeros(len(pts), np.uint32)
    with np.errstate(all="ignore"):
        px, py, pz = (pts[:, c].copy() for c in range(3))
        wx, wy, wz = px.copy(), py.copy(), pz.copy()
        m = wx * wx + wy * wy + wz * wz
        live = np.ones(len(pts), bool)
        for _ in range(iterations):
            out += live
            x, y, z = wx, wy, wz
            x2, y2, z2 = x * x, y * y, z * z
            x4, y4, z4 = x2 * x2, y2 * y2, z2 * z2
            k3 = x2 + z2
            k2 = f(1.0) / np.sqrt(k3 * k3 * k3 * k3 * k3 * k3 * k3)
            k1 = x4 + y4 + z4 - f(6.0) * y2 * z2 - f(6.0) * x2 * y2 + f(2.0) * z2 * x2
            k4 = x2 - y2 + z2
            nx = px + f(64.0) * x * y * z * (x2 - z2) * k4 * (x4 - f(6.0) * x2 * z2 + z4) * k1 * k2
            ny = py + f(-16.0) * y2 * k3 * k4 * k4 + k1 * k1
            nz = pz + f(-8.0) * y * k4 * (x4 * x4 - f(28.0) * x4 * x2 * z2 + f(70.0) * x4 * z4 - f(28.0) * x2 * z2 * z4 + z4 * z4) * k1 * k2
            wx, wy, wz = np.where(live, nx, wx), np.where(live, ny, wy), np.where(live, nz, wz)
            m = np.where(live, wx * wx + wy * wy + wz * wz, m)
            live &= ~(m > f(256.0))
    return out


def test_spheres_only_counts_nothing(oracle):
    wd, p, tabs, film, ctr = CC.frame_reference(oracle, "spheres_only", 3)
    assert CC.n_sdfs(wd) == 0 and ctr.segments > 0
    assert all(v == 0 for v in ctr.lane_counts().values()) and ctr.dist_evals == 0
    org, d = M.rays(N_RAYS, RAY_SEED)
    _, obj, ev, it = oracle.closest_hit_counts(wd, p, 0, org, d)
    assert not ev.any() and not it.any() and (obj != 0xFFFFFFFF).any()


# ---- 3. whole-frame identities on the oracle alone ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,bounces", [("s1", 3), ("s2", 3), ("bulbv", 3), ("two_sdfs", 3)])
def test_frame_tallies_are_the_sums_of_the_per_ray_exports(oracle, name, bounces):
    """One tile at a time (tiles are independent): the rays of depth 0 come from the ray-generation loop, those of depth k + 1 are the rays the integrate calls of
    depth k spawned (oracle.trace_shade records both sides).  extend = sum of closest_hit_counts over exactly these rays; shade_setup = 4 evaluations per valid
    lane whose hit object is a TracedSDF; and oracle.shade_packets(counts=True) on the recorded packets gives the frame's shade and shadow tallies again."""
    wd, p, tabs, _, ctr_all = CC.frame_reference(oracle, name, bounces)
    total = np.zeros(13, np.int64)
    sdf = [k for k in range(wd.n_hitables) if wd.hitables[k].kind != 0]
    rows = (p.height + p.tile_h - 1) // p.tile_h
    for tile in range(oracle.lib().oracle_tile_count(p.width, p.height, p.tile_w, p.tile_h)):
        _, ctr = oracle.render(wd, p, tabs, threads=1, tile_subset=[tile])
        got = ctr.lane_counts()
        total += np.array(list(got.values()), np.int64)
        tx, ty = tile // rows, tile % rows
        x0, y0 = tx * p.tile_w, ty * p.tile_h
        gen = oracle.raygen_tile(wd, p, tabs, x0, y0, min(x0 + p.tile_w, p.width), min(y0 + p.tile_h, p.height))
        sh = oracle.trace_shade(wd, p, tabs, tile)
        org, d = gen["origin"], gen["dir"]
        ev_sum = it_sum = 0
        shade = np.zeros(13, np.int64)
        for depth in range(bounces + 2):
            if len(org) == 0:
                break
            _, _, ev, it = oracle.closest_hit_counts(wd, p, depth, org, d)
            ev_sum += CC.as_u64(ev); it_sum += CC.as_u64(it)
            k = sh["depth"] == depth
            assert k.sum() * 4 >= len(org) > 0  # every ray of these scenes hits something (the sky sphere encloses them)
            assert int(sh["valid"][k].sum()) == len(org)
            st, _, out_f, tally = oracle.shade_packets(wd, p, tabs, depth, sh["obj"][k], sh["valid"][k], sh["sample"][k], sh["lane_f"][k], counts=True)
            assert np.array_equal(st, sh["status"][k])
            shade += np.array(list(tally.values()), np.int64)
            spawned = sh["status"][k] == oracle.SH_SPAWNED
            org, d = sh["out_f"][k][spawned][:, oracle.SHADE_OUT["origin"]], sh["out_f"][k][spawned][:, oracle.SHADE_OUT["dir"]]
        assert (got["evals_extend"], got["iters_extend"]) == (ev_sum, it_sum), tile
        on_sdf = int((sh["valid"] * np.isin(sh["obj"], sdf)[:, None]).sum())
        assert got["evals_shade_setup"] == 4 * on_sdf, tile
        want = np.array(list(got.values()), np.int64)
        want[[0, 3]] = 0  # shade_packets runs no closest hit
        assert np.array_equal(shade, want), (tile, shade, want)
    assert np.array_equal(total, np.array(list(ctr_all.lane_counts().values()), np.int64))  # the threaded frame = the sum of its tiles
    assert ctr_all.dist_evals >= sum(ctr_all.tally[0:3])  # the packet count (x 4 lanes) bounds the lane count from above


@pytest.mark.parametrize("name,bounces", [("s1", 3), ("s2", 3), ("bulbv", 3), ("two_sdfs", 3), ("huge_lights", 3)])
def test_frame_shadow_tallies_are_the_sums_over_the_parked_segments(oracle, name, bounces):
    """The frame's parked shadow jobs as segments (the oracle's job sink), each marched on its own by oracle.shadow_counts - a packet of four equal lanes - against
    the frame's tallies, which charge the lanes of real packets: lanes that stop in different trips, padding lanes, lanes whose sample was elided or blocked."""
    wd, p, tabs, film, ctr_all = CC.frame_reference(oracle, name, bounces)
    film1, ctr, a, b = oracle.render_jobs(wd, p, tabs)
    from common import film_equal_bits
    assert film_equal_bits(film1, film) and ctr.lane_counts() == ctr_all.lane_counts()  # the sink changes nothing
    t = ctr.lane_counts()
    assert len(a) == t["shadow_jobs"] > 0
    vis, ev, it = oracle.shadow_counts(wd, p, a, b)
    assert (CC.as_u64(ev), CC.as_u64(it)) == (t["evals_shadow"], t["iters_shadow"])
    assert 0 < vis.mean() < 1 and len(np.unique(ev)) > 10


def test_camera_time_is_not_needed_by_the_identity_scenes(oracle):
    """closest_hit_counts runs its rays at time 0; the scenes of the identity above hold no closure-sequenced object or camera, so time cannot matter."""
    for name, bounces in (("s1", 3), ("s2", 3), ("bulbv", 3), ("two_sdfs", 3), ("huge_lights", 3)):
        wd = CC.frame_case(name, bounces)[0]
        assert wd.camera.animated == 0 and not any(wd.hitables[k].animated or wd.hitables[k].scale_vel != 0.0 for k in range(wd.n_hitables))


# ---- 4. every scene of the device tests reaches what it is there for -----------------------------------------------------------------------------------------------

def test_case_conditions(oracle):
    t = {(n, b): CC.frame_reference(oracle, n, b)[4].lane_counts() for n, b in CC.FRAMES}
    seg = {(n, b): CC.frame_reference(oracle, n, b)[4].segments for n, b in CC.FRAMES}
    for key in (("s2", 3), ("s2", 8)):
        assert 0 < t[key]["zero_throughput_slots"] < seg[key] and t[key]["elided_shadow_jobs"] > 0 and t[key]["samples_out_of_bounds"] == 0, t[key]
    assert t[("huge_lights", 3)]["samples_out_of_bounds"] > 0 and t[("huge_lights", 3)]["zero_throughput_slots"] > 0
    two = t[("two_sdfs", 3)]
    assert two["jobs_first_sdf_occludes"] > 0 and two["jobs_all_sdfs_marched"] > 0 and two["jobs_first_sdf_occludes"] + two["jobs_all_sdfs_marched"] < two["shadow_jobs"]
    # an analytic sphere between surface and light: NEE samples that pass every other term of the rule and are kept from being jobs by the sphere test alone
    for key in (("anim_spheres", 3), ("s1", 3), ("s2", 3)):
        assert t[key]["sphere_blocked_samples"] > 0, key
    b = t[("bulbv", 3)]
    n_it = [int(h.iterations) for h in CC.frame_case("bulbv", 3)[0].hitables if h.kind != 0 and h.sdf_kind == 2][0]
    for cls in CC.EVAL_KEYS:
        assert b["evals_" + cls] < b["iters_" + cls] < n_it * b["evals_" + cls], (cls, b)
    for key, v in t.items():
        if key[0] != "spheres_only":
            assert v["shadow_jobs"] > 0 and all(v["evals_" + c] > 0 for c in CC.EVAL_KEYS), key
        # a job costs at least one evaluation; a slot on a TracedSDF exactly four
        assert v["evals_shadow"] >= v["shadow_jobs"] and v["evals_shade_setup"] % 4 == 0
    assert t[("s0", 3)]["iters_extend"] == t[("s0", 3)]["iters_shade_setup"] == t[("s0", 3)]["iters_shadow"] == 0
    s1 = t[("s1", 3)]
    assert all(s1["iters_" + c] == 12 * s1["evals_" + c] for c in CC.EVAL_KEYS)  # the shipped MandelBox: 12 folds per evaluation


def test_policies_count_differently_but_consistently(oracle):
    """The fused build marches other distances: its tallies are its own (the device tests compare each policy with its own reference)."""
    a = CC.frame_reference(oracle, "s2", 3)[4].lane_counts()
    b = CC.frame_reference(oracle, "s2", 3, fma=True)[4].lane_counts()
    assert a != b and a["evals_shade_setup"] > 0 and b["iters_extend"] == 12 * b["evals_extend"]
