"""Named scenes for the gates that the VALUES of an uploaded scene decide (build_scene and scene_march_kernels in rayn_amd/csrc/rayn_hip.hip, sdf_dist in
device_core.h), shared by tests/test_sdf_cases.py (the oracle against the numpy statement, and this generator against its own claims; no GPU) and
tests/test_sdf_device.py (the probes, the march kernels and whole films against the oracle).  Plain data and numpy.

A row = (name, what to build, the dispatch it must get, points).  The expected dispatch is written down per row, not computed: test_sdf_cases.py checks the
fast_div == 0 column against a restatement of the window rule; whether an in-window MandelBox gets 1 or 2 is the device's verdict (VERDICT_PAIRS)."""
import numpy as np

import restatement_np as R

f32 = np.float32
RES = (40, 32)
SHIPPED = dict(it=12, side=1.0, mr=0.01, fr=1.9, scale=-2.1)
BUDGET = 0xFFFF  # k_shadow_bulb keeps the march count in 16 bits next to two flags: budgets below this value only


def _row(name, kind="box", fd0=False, single=True, bulb=False, anim=False, t0s=(0.0,), frame=None, nonfinite=False, dyadic=False, hits_sdf=True, **sdf):
    """fd0: the SDF object's fast_div is 0 (otherwise 1 or 2); single: the single-SDF march kernels; bulb: k_shadow_bulb; anim: the kernels carry the packet time;
    nonfinite: a row whose reference distances overflow or are NaN by construction (exempt from the finite share); hits_sdf: some ray of rays() meets the SDF
    in the reference (False where the SDF has no surface to meet: its distance is NaN or never near zero)"""
    spec = dict(SHIPPED)
    spec.update(sdf)
    return dict(name=name, kind=kind, sdf=spec, expect=dict(fd0=fd0, single=single, bulb=bulb, anim=anim), t0s=tuple(t0s), frame=dict(frame or {}),
                nonfinite=nonfinite, dyadic=dyadic, hits_sdf=hits_sdf)


ROWS = [
    # ---- the [2^-60, 2^60] window of min_radius^2, fixed_radius^2 and |box_side|: fast_div 0 against at least 1
    _row("mr_2m30", mr=2.0 ** -30),
    _row("mr_2m31", mr=2.0 ** -31, fd0=True),
    _row("mr_0", mr=0.0, fd0=True),
    # (fixed_radius 2^30 multiplies dr by up to (fixed / min)^2 per iteration: one and two iterations with min_radius 1 keep 99 % of the distances finite)
    _row("fr_2p30_it1", fr=2.0 ** 30, it=1, mr=1.0),
    _row("fr_2p30_it2", fr=2.0 ** 30, it=2, mr=1.0),
    _row("fr_2p30h_it1", fr=float(f32(2.0 ** 30.5)), it=1, mr=1.0, fd0=True),
    _row("fr_2p30h_it2", fr=float(f32(2.0 ** 30.5)), it=2, mr=1.0, fd0=True),
    _row("side_2p60", side=2.0 ** 60),
    _row("side_2p61", side=2.0 ** 61, fd0=True),
    # ---- iteration counts: none, the tail loop alone, by-4 without / with a tail, the unrolled 12, 12 + tail, 12 + by-4
    _row("it0", it=0), _row("it1", it=1), _row("it3", it=3), _row("it4", it=4), _row("it5", it=5), _row("it11", it=11), _row("it12"), _row("it13", it=13),
    _row("it16", it=16),
    # ---- the sphere fold's gate frs_eff: never folds (min > fixed), folds with the quotient 1 (min == fixed); the host gives both div_nr without asking the device
    _row("mr_gt_fr", mr=1.0, fr=0.5),
    _row("mr_eq_fr", mr=1.0, fr=1.0),
    # ---- box sides: no box, no fold (+inf is outside the window), and the two for which clamped(-l, l) is not the median of (p, -l, l)
    _row("side_0", side=0.0),
    _row("side_neg0", side=-0.0, fd0=True),
    _row("side_inf", side=float("inf"), fd0=True),
    _row("side_m1", side=-1.0, fd0=True, hits_sdf=False),
    _row("side_nan", side=float("nan"), fd0=True, nonfinite=True, hits_sdf=False),
    _row("scale_0", scale=0.0),
    _row("scale_vel", scale_vel=4.0, anim=True, t0s=(0.0, 0.37, 1.0)),
    # ---- dyadic fold radii: r2 == fixed_radius^2 and r2 == min_radius^2 can be hit exactly
    _row("dyadic_it5", it=5, mr=0.5, fr=1.0, scale=-2.0, dyadic=True),
    _row("dyadic_it12", mr=0.5, fr=1.0, scale=-2.0, dyadic=True),
    # ---- the other SDFs and scene shapes
    _row("sphere_sdf", kind="sphere", fd0=True),
    _row("bulb_it0", kind="bulb", it=0, fd0=True),
    _row("bulb_it1", kind="bulb", it=1, fd0=True, bulb=True),
    _row("bulb_it8", kind="bulb", it=8, fd0=True, bulb=True),
    _row("bulb_fffe", kind="bulb", it=8, fd0=True, bulb=True, frame=dict(max_marches=BUDGET - 1, max_vis_marches=BUDGET - 1)),
    _row("bulb_marches_ffff", kind="bulb", it=8, fd0=True, frame=dict(max_marches=BUDGET, max_vis_marches=BUDGET - 1)),
    _row("bulb_vis_ffff", kind="bulb", it=8, fd0=True, frame=dict(max_marches=BUDGET - 1, max_vis_marches=BUDGET)),
    _row("two_sdfs", kind="two", single=False),
    _row("anim_spheres", kind="anim", anim=True),
]
ROW_NAMES = [r["name"] for r in ROWS]
BY_NAME = {r["name"]: r for r in ROWS}


def scene(row, sdf_only=False):
    """(world_desc, frame_params, index of the row's SDF object) of a row at RES, 2 samples (8 spp), 3 bounces; sdf_only keeps the TracedSDFs alone (what
    rayn_hip_probe_shadow marches)"""
    import rayn_amd as A
    from rayn_amd import params as P
    from rayn_amd import setup as S
    s, kind = row["sdf"], row["kind"]
    if kind == "bulb":
        cam, world = S.setup(RES, volumes=False, sdf="mandelbulb")
        world.hitables[1].sdf.iterations = s["it"]
    elif kind == "sphere":
        cam, world = S.setup(RES, volumes=False, sdf="sphere")
    else:
        cam, world = S.setup(RES, volumes=False, sdf="mandelbox")
        world.hitables[1] = A.TracedSDF(A.MandelBox(s["it"], A.BoxFold(s["side"]), A.SphereFold(s["mr"], s["fr"]), s["scale"], scale_vel=s.get("scale_vel", 0.0)),
                                        world.hitables[1].material)
        if kind == "two":
            world.hitables.push(A.TracedSDF(A.SphereSDF(0.35), 1, A.vec3(1.4, 0.9, 0.6)))
        elif kind == "anim":
            for i in (2, 3):
                sp = world.hitables[i]
                sp.transform_seq = A.Linear(sp.transform_seq, A.vec3(3.0, -2.0, 1.5))
    if sdf_only:
        keep = [h for h in world.hitables if isinstance(h, A.TracedSDF)]
        world.hitables[:] = keep
    idx = [i for i, h in enumerate(world.hitables) if isinstance(h, A.TracedSDF)][0]
    return world.to_desc(cam), P.frame_params(RES[0], RES[1], 2, 3, **row["frame"]), idx


def in_window(h):
    """the rule behind fast_div != 0 for a MandelBox, restated: both squared radii and the box side inside [2^-60, 2^60], the side not negative (nor -0, nor NaN)"""
    lo, hi = f32(2.0 ** -60), f32(2.0 ** 60)
    mrs, frs, l = f32(h.min_radius) * f32(h.min_radius), f32(h.fixed_radius) * f32(h.fixed_radius), f32(h.box_side)
    return bool(lo <= mrs <= hi and lo <= frs <= hi and 0 <= l <= hi and not np.signbit(l))


# ---- the (min_radius, fixed_radius) pairs whose 1-or-2 verdict the device gives (k_verify_short_div): shipped, the randomised-parity generator's, corners, others
def _generator_pairs(n=16):
    out = []
    for seed in range(n):  # the draws of test_gpu_parity.test_randomised_scene_parity up to the fold radii, in its order
        rng = np.random.default_rng(1000 + seed)
        rng.integers(17, 49), rng.integers(9, 33), rng.integers(0, 2), rng.integers(5, 15)
        rng.uniform(-2.6, -1.7) if rng.integers(0, 2) else rng.uniform(1.8, 2.8)
        rng.uniform(0.7, 1.3)
        out.append((float(f32(rng.uniform(0.005, 0.6))), float(f32(rng.uniform(0.8, 2.2)))))
    return out


VERDICT_PAIRS = ([(0.01, 1.9)] + _generator_pairs()
                 + [(2.0 ** -30, 2.0 ** 30), (2.0 ** -30, 1.9), (0.01, 2.0 ** 30), (2.0 ** -30, float(np.nextafter(f32(2.0 ** -30), f32(1.0)))),
                    (float(np.nextafter(f32(2.0 ** 30), f32(0.0))), 2.0 ** 30)]
                 + [(0.005, 0.8), (0.6, 2.2), (0.005, 2.2), (0.6, 0.8), (0.5, 1.0), (0.1, 1.0), (1.0, 2.0), (0.3, 0.31), (1e-3, 1e3), (1e-6, 1.0), (0.9, 1.1), (0.25, 4.0)])


def verdict_row(mr, fr):
    return _row(f"verdict_{mr!r}_{fr!r}", mr=mr, fr=fr)


# ---- points ----------------------------------------------------------------------------------------------------------------
N_UNIFORM = 4096


def _unit_points(target_of_one, n=64, seed=77):
    """seeded float32 vectors whose mag_sq - under BOTH mul_add policies - is exactly `target_of_one` (1.0, or the float below it)"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(400000, 3))
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)
    v[:6] = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f32)
    cols = [np.ascontiguousarray(v[:, c]) for c in range(3)]
    with R.fused_policy(False):
        a = R.mag_sq(cols)
    with R.fused_policy(True):
        b = R.mag_sq(cols)
    keep = (a == f32(target_of_one)) & (b == f32(target_of_one))
    if target_of_one != 1.0:
        keep[:6] = False
    return v[keep][:n]


def points(row):
    """(pts [n, 3] float32, groups: name -> slice).  4096 seeded uniform points of [-3.5, 3.5]^3, then the structured groups."""
    s = row["sdf"]
    l = f32(s["side"])
    lf = f32(abs(l)) if np.isfinite(l) and l != 0 and abs(l) < 1e6 else f32(1.0)  # where the fold planes are drawn (a finite, moderate stand-in otherwise)
    parts, groups, n = [], {}, 0

    def add(name, a):
        nonlocal n
        a = np.asarray(a, f32).reshape(-1, 3)
        parts.append(a)
        groups[name] = slice(n, n + len(a))
        n += len(a)

    rng = np.random.default_rng(4242)
    add("uniform", rng.uniform(-3.5, 3.5, (N_UNIFORM, 3)))
    ax = np.concatenate([np.eye(3), -np.eye(3)])
    add("origin_axes", np.concatenate([np.zeros((1, 3)), np.array([[-0.0, 0.0, -0.0]]), ax * 0.5, ax * 1.0, ax * 2.5]))
    add("far", rng.uniform(-3.5, 3.5, (64, 3)) * 30.0 * float(lf))
    # 2^-40 .. 2^2: without it no denominator of the sphere fold ever equals a tiny min_radius^2.  (The Mandelbulb estimator underflows to NaN below 2^-14 by
    # construction - 1 / sqrt(k3^7) -, so its ladder has the same 43 rungs between 2^-4 and 2^2.)
    mags = np.exp2(np.linspace(-4, 2, 43)) if row["kind"] == "bulb" else np.exp2(np.arange(-40, 3, dtype=np.float64))
    second = np.array([0, 0, -1.0]) if row["kind"] == "bulb" else np.array([0, -1.0, 0])  # (the Mandelbulb estimator is NaN on the whole y axis, x = z = 0: origin_axes keeps six such points)
    add("ladder_axis", np.concatenate([np.outer(mags, e) for e in (np.array([1.0, 0, 0]), second)]))
    add("ladder_diag", np.outer(mags, np.array([1.0, 1.0, 1.0])))
    pl = rng.uniform(-2.0, 2.0, (96, 3)) * float(lf)
    for i in range(96):  # one, two or three components exactly on a fold plane |p_c| = l, both signs
        for c in range(1 + i % 3):
            pl[i, (i + c) % 3] = float(lf) * (1 if (i >> 2) & 1 else -1)
    add("fold_planes", pl)
    if row["dyadic"]:
        add("r2_eq_frs", _unit_points(1.0))                                    # fixed_radius^2 = 1: r2 == frs exactly, |p_c| <= 1 = l so the box fold is the identity
        add("r2_ulp_below_frs", _unit_points(float(np.nextafter(f32(1.0), f32(0.0)))))
        add("r2_eq_mrs", _unit_points(1.0) * f32(0.5))                         # min_radius^2 = 0.25: halving scales every product exactly
    add("nan_inf", [[np.nan, 0.3, 0.2], [0.3, np.inf, 0.2]])
    return np.ascontiguousarray(np.concatenate(parts).astype(f32)), groups


def first_fold(pts, h):
    """The sphere fold's operands in iteration 1 of the MandelBox h, from the statement's own primitives: (r2 after the box fold, the denominator
    max(min_radius^2, r2), folds = r2 < fixed_radius^2), per point, under the policy in force."""
    l, mrs, frs = f32(h.box_side), f32(f32(h.min_radius) * f32(h.min_radius)), f32(f32(h.fixed_radius) * f32(h.fixed_radius))
    p = [np.ascontiguousarray(pts[:, c]) for c in range(3)]
    with np.errstate(all="ignore"):
        q = [R.mul_add(R.smin(R.smax(p[c], -l), l), f32(2.0), (-p[c]).astype(f32)) for c in range(3)]
        r2 = R.mag_sq(q)
        den = R.smax(np.full_like(r2, mrs), r2)
        return r2, den, r2 < frs


AIMED = 256


def rays(n=8192 - 13):
    """origins and unit directions as test_gpu_parity.test_closest_hit_bit_exact builds them (half from the shipped camera position towards the scene)"""
    rnd = lambda k, lo, hi, seed: np.random.default_rng(seed).uniform(lo, hi, k).astype(f32)
    org = rnd(3 * n, -3.0, 3.0, 11).reshape(-1, 3)
    org[: n // 2] = np.array([-1.0125, 0.45, 4.5], f32)
    d = rnd(3 * n, -1.0, 1.0, 12).reshape(-1, 3)
    d[: n // 2] = -org[: n // 2] + rnd(3 * (n // 2), -1.5, 1.5, 13).reshape(-1, 3)
    d[-AIMED:] = -org[-AIMED:]  # the last rays aim at the SDF's centre: the only way to meet a set as thin as |p| = 0 (no iterations, scale 0)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(f32)
    return org, d


def segments(n=8192 - 13):
    rnd = lambda k, seed: np.random.default_rng(seed).uniform(-2.0, 2.0, k).astype(f32)
    return rnd(3 * n, 21).reshape(-1, 3), rnd(3 * n, 22).reshape(-1, 3)


def admissible_arms(h_kind, iterations, own_fast_div):
    """every (sdfk, fast_div) rayn_hip_probe_sdf_dist_as accepts for an object: the generic and the per-kind instantiation in the own arm and every lower
    one, plus the 12-iteration short-division instantiation where the object qualifies"""
    arms = [(k, fd) for k in (-1, h_kind) for fd in range(own_fast_div + 1)]
    if h_kind == 1 and own_fast_div == 2 and iterations == 12:
        arms.append((100, 2))
    return arms
