"""Worlds and case families that put the analytic Sphere's two functions - sphere_hit and sphere_occluded_dir of rayn_amd/csrc/device_core.h, restating
src/sphere.rs:24-72 - and the hitable fold around them (src/hitable.rs:177-198) ON their decisions: descrim > 0, t > 0.0001 and t <= t_max, the choice between
the roots, min(t1, t2) > 0.001 and t1 <= dist, the two early-outs of the device's occlusion test, and the strict `<` of the fold.  Shared by
tests/test_sphere_cases.py (the oracle against the numpy statement, every family against what it claims, planted mutants; no GPU) and
tests/test_sphere_device.py (the device against the oracle).  Plain numpy and deterministic; every family is built under a stated mul_add policy, because the
roots a `t_max == root` case names differ between the two builds.

"Bit-walk": one coordinate stepped through consecutive float bit patterns around the stated place - 64 consecutive ones, and the same 64 steps at strides 16
and 256 where the decision may lie further from the float32 construction than 32 patterns."""
import numpy as np

import restatement_np as RN

f32 = np.float32
F32_MAX = np.finfo(f32).max
T_HIT = f32(0.0001)  # src/sphere.rs: Sphere::hit's near threshold
T_OCC = f32(0.001)   # Sphere::occluded's
EARLY_C = f32(-1e-30)  # sphere_occluded_dir's second early-out
TINY_RADII = (1e-16, 1e-15, 3e-15)  # r^2 below, at and above 1e-30
RADII = TINY_RADII + (1e-3, 0.15, 0.45, 1.0, 100.0, 1e4)
MOVING = len(RADII)  # index of the sphere with the closure centre
MOVING_TIMES = (0.0, -0.0, 0.37, 1.0, float("nan"))  # NaN: packet_time of a packet whose lane 0 is empty
N_RANDOM = 1 << 14  # H6 / O7 lanes per (sphere, time)


# ---- float helpers -------------------------------------------------------------------------------------------------------------
def _ord(x):
    """float32 -> int64, monotonic over the floats, -0 and +0 adjacent (0 and 1)"""
    b = np.asarray(x, f32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b + 1)


def _unord(k):
    k = np.asarray(k, np.int64)
    b = np.where(k >= 1, k - 1, 0x80000000 | (-k))
    return b.astype(np.uint32).view(f32)


def walk(x, count=64, stride=1):
    """`count` floats around x, `stride` bit patterns apart, x itself among them"""
    return _unord(int(_ord(f32(x))) + (np.arange(count, dtype=np.int64) - count // 2) * stride)


def nextbelow(x):
    return np.nextafter(f32(x), f32(-np.inf))


def nextabove(x):
    return np.nextafter(f32(x), f32(np.inf))


def _frame(seed):
    """a seeded orthonormal frame (float64) that is not axis-aligned"""
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    return q[:, 0], q[:, 1], q[:, 2]


def _unit(rng, n):
    g = rng.standard_normal((n, 3))
    return g / np.linalg.norm(g, axis=1, keepdims=True)


def _cols(a, k=0):
    return [np.ascontiguousarray(a[:, k + c]) for c in range(3)]


# ---- the per-lane probe world ----------------------------------------------------------------------------------------------------
def centre_of(i):
    """non-dyadic centres; a tiny sphere's centre is of its radius' size, so that points k * r from it are representable; the 1e-3 sphere's likewise (H2's exact
    t == 0.0001 needs roots on a grid as fine as 0.0001's own)"""
    r = RADII[i] if i < len(RADII) else 0.45
    if r <= 1e-3:
        return np.array([1.3 * r, -0.7 * r, 2.1 * r], f32)
    if r >= 100.0:
        return np.array([0.013, -0.021, 0.017], f32) if r == 100.0 else np.array([1.7, -2.3, 0.9], f32)
    return np.array([0.3 + 0.37 * i, -0.7 + 0.11 * i, 1.1 - 0.23 * i], f32)


MOVING_VEL = np.array([300.0, -200.0, 150.0], f32)


def probe_world():
    """(world_desc, frame_params): the nine radii of RADII as constant spheres, then one radius-0.45 sphere with a Linear centre of large velocity"""
    import rayn_amd as A
    from rayn_amd import params as P
    mats = A.MaterialStore()
    mats.add_material(A.Sky(A.Srgb(0.3, 0.4, 0.6), A.Srgb(0.01, 0.015, 0.03)))
    mats.add_material(A.Lambertian(A.Srgb(0.8, 0.3, 0.2)))
    hit = A.HitableStore()
    for i, r in enumerate(RADII):
        hit.push(A.Sphere(centre_of(i), r, 0 if r >= 100.0 else 1))
    hit.push(A.Sphere(A.Linear(centre_of(MOVING), MOVING_VEL), 0.45, 1))
    cams = A.CameraStore()
    cam = cams.add_camera(A.PinholeCamera((16.0, 16.0), 60.0, A.vec3(0, 0, 3), A.vec3(0, 0, 0), A.vec3(0, 1, 0)))
    world = A.World(hit, [A.SphereLight(A.vec3(-0.3, 0.2, 1.9), 0.15, A.Srgb(1.0, 1.0, 1.0))], mats, cams, A.VolumeParams(None, None))
    return world.to_desc(cam), P.frame_params(16, 16, 1, 1)


def targets():
    """[(sphere index, lane time)]: every constant sphere at time 0, the moving one at each of MOVING_TIMES"""
    return [(i, 0.0) for i in range(len(RADII))] + [(MOVING, t) for t in MOVING_TIMES]


def _centre_at(wd, idx, t):
    """the sphere's centre at lane time t as the statement computes it (float32); at t = NaN the cases are laid out around the centre at 0"""
    t = 0.0 if t != t else t
    c = RN.sphere_center(wd.hitables[idx], np.full(1, f32(t), f32))
    return np.array([c[0][0], c[1][0], c[2][0]], f32)


# ---- the statement with its intermediates, and the mutants ------------------------------------------------------------------------
def hit_parts(h, rec):
    """Sphere::hit's float32 intermediates for records [n, 8] (o, d, t_max, t0) from the statement's primitives, under the policy in force"""
    with np.errstate(all="ignore"):
        oc = RN.vsub(_cols(rec, 0), RN.sphere_center(h, np.ascontiguousarray(rec[:, 7])))
        b = RN.dot(oc, _cols(rec, 3))
        c = (RN.mag_sq(oc) - f32(f32(h.radius) * f32(h.radius))).astype(f32)
        descrim = ((b * b).astype(f32) - c).astype(f32)
        ds = np.sqrt(descrim).astype(f32)
        return dict(b=b, c=c, descrim=descrim, t1=((-b) - ds).astype(f32), t2=((-b) + ds).astype(f32), t_max=np.ascontiguousarray(rec[:, 6]))


HIT_MUTANTS = ("t1_lt_tmax", "t2_lt_tmax", "ge_near", "near_0.001", "descrim_ge", "take_t1_unchecked")


def hit_np(h, rec, mut=None):
    """Sphere::hit (src/sphere.rs:48-72) from hit_parts; mut names one planted change"""
    p = hit_parts(h, rec)
    t1, t2, tm = p["t1"], p["t2"], p["t_max"]
    near = f32(0.001) if mut == "near_0.001" else T_HIT
    gt = (lambda t: t >= near) if mut == "ge_near" else (lambda t: t > near)
    with np.errstate(all="ignore"):
        pos = p["descrim"] >= 0 if mut == "descrim_ge" else p["descrim"] > 0
        t1v = gt(t1) & ((t1 < tm) if mut == "t1_lt_tmax" else (t1 <= tm)) & pos
        t2v = gt(t2) & ((t2 < tm) if mut == "t2_lt_tmax" else (t2 <= tm)) & pos
        take = (t1 < t2) if mut == "take_t1_unchecked" else (t1 < t2) & t1v
    return np.where(t1v | t2v, np.where(take, t1, t2), F32_MAX).astype(f32)


def occ_parts(h, rec):
    """Sphere::occluded's float32 intermediates for records [n, 7] (a, b, t0)"""
    with np.errstate(all="ignore"):
        a = _cols(rec, 0)
        dirv = RN.vsub(_cols(rec, 3), a)
        dist = RN.mag(dirv)
        dirv = RN.vdiv(dirv, dist)
        oc = RN.vsub(a, RN.sphere_center(h, np.ascontiguousarray(rec[:, 6])))
        b = RN.dot(oc, dirv)
        c = (RN.mag_sq(oc) - f32(f32(h.radius) * f32(h.radius))).astype(f32)
        descrim = ((b * b).astype(f32) - c).astype(f32)
        ds = np.sqrt(descrim).astype(f32)
        return dict(dist=dist, b=b, c=c, descrim=descrim, t1=((-b) - ds).astype(f32), t2=((-b) + ds).astype(f32))


# Planted changes of the occlusion test that some segment can tell from the original.  The early-outs are the DEVICE's (sphere_occluded_dir), so their mutants are
# applied to the device form (early=True).  Not listed, because no input can tell them from the shipped code:
#   * early-out `c < 0` or `c <= 0` for `c < -1e-30f`: with b < 0 and c <= 0, descrim = fl(fl(b*b) - c) >= fl(b*b), so sqrt >= |b| and t1 <= 0;
#   * early-out `c < 1e-30f`: with 0 <= c < 1e-30 an occluding t1 > 0.001 needs -b > 0.001, so b*b > 1e-6 and fl(b*b - c) == fl(b*b), whose root is |b|: t1 == 0;
#   * early-out `b >= -1e-6` (any bound down to -0.001f): sqrt >= 0 gives t1 = fl(-b - sqrt) <= -b <= 0.001, which fails `min(t1, t2) > 0.001`.
# test_sphere_cases.py asserts the last two do NOT change an output of the case set, and kills the nearest changes that are not exact instead:
# `b >= -0.0011f` and `c < 1.2e-6f` (a grazing segment 0.00108 before its closest approach to the 1e-3 sphere, family O4g).
OCC_MUTANTS = ("near_0.0001", "t1_lt_dist", "t2_le_dist", "early_b_-0.0011", "early_c_1.2e-6")
OCC_EQUIVALENT = ("early_b_-1e-6", "early_c_1e-30", "early_c_0")


def occ_np(h, rec, mut=None, early=False):
    """Sphere::occluded (src/sphere.rs:24-46), 0 occluded / 1 not; early=True adds sphere_occluded_dir's two early-outs (device_core.h); mut = one planted change"""
    p = occ_parts(h, rec)
    t1, t2 = p["t1"], p["t2"]
    near = f32(0.0001) if mut == "near_0.0001" else T_OCC
    with np.errstate(all="ignore"):
        far = (t1 < p["dist"]) if mut == "t1_lt_dist" else (t2 <= p["dist"]) if mut == "t2_le_dist" else (t1 <= p["dist"])
        valid = (RN.smin(t1, t2) > near) & far & (p["descrim"] > 0)
        if early or (mut or "").startswith("early"):
            b_lim = {"early_b_-0.0011": f32(-0.0011), "early_b_-1e-6": f32(-1e-6)}.get(mut, f32(0.0))
            c_lim = {"early_c_1.2e-6": f32(1.2e-6), "early_c_1e-30": f32(1e-30), "early_c_0": f32(0.0)}.get(mut, EARLY_C)
            valid &= ~((p["b"] >= b_lim) | (p["c"] < c_lim))
    return np.where(valid, f32(0.0), f32(1.0)).astype(f32)


# ---- hit families ----------------------------------------------------------------------------------------------------------------
def _rec_hit(o, d, t_max, t0):
    o, d = np.atleast_2d(np.asarray(o, f32)), np.atleast_2d(np.asarray(d, f32))
    n = max(len(o), len(d), np.size(t_max))
    out = np.empty((n, 8), f32)
    out[:, 0:3], out[:, 3:6], out[:, 6], out[:, 7] = o, d, t_max, t0
    return out


def _walk_coord(base, k, **kw):
    """copies of the point `base` with coordinate k bit-walked"""
    w = walk(base[k], **kw)
    out = np.tile(np.asarray(base, f32), (len(w), 1))
    out[:, k] = w
    return out


STRIDES = (1, 16, 256)


def hit_cases(wd, fma):
    """[(family, sphere index, records [n, 8])] under the mul_add policy `fma`"""
    out = []
    with RN.fused_policy(fma):
        for ti, (idx, t0) in enumerate(targets()):
            h = wd.hitables[idx]
            C, r = _centre_at(wd, idx, t0).astype(np.float64), float(f32(h.radius))
            u, v, w = _frame(500 + ti)
            rng = np.random.default_rng(9000 + ti)
            tm = f32(200.0)
            add = lambda fam, rec: out.append((fam, idx, np.ascontiguousarray(rec, f32)))
            # H1: the impact parameter across r, from a near and a far start
            for L in (2.0 * r, 1000.0 * r):
                base = (C + v * r - u * L).astype(f32)
                k = int(np.argmax(np.abs(v)))
                add("H1", np.concatenate([_rec_hit(_walk_coord(base, k, stride=s), u.astype(f32), tm, t0) for s in STRIDES]))
            # H2: t1 across 0.0001 (origin outside, ray along -n), t2 across it (origin just inside, ray along +n); n = w
            k = int(np.argmax(np.abs(w)))
            for sign, dvec in ((1.0, -w), (-1.0, w)):
                base = (C + w * (r + sign * 1e-4)).astype(f32)
                add("H2", np.concatenate([_rec_hit(_walk_coord(base, k, stride=s), dvec.astype(f32), tm, t0) for s in STRIDES]))
            # H3: t_max at, just below and just above each root of 16 rays from outside and 16 from inside; inside also between the roots and below both.  Only
            # where a root can be valid: no unit ray resolves a sphere of radius <= 3e-15 from 0.0001 away, so the tiny spheres have no base rays
            if r >= 1e-3 and t0 == t0:
                dirs = _unit(rng, 32)
                aim = C + _unit(rng, 32) * r * rng.uniform(0.0, 0.8, (32, 1))
                start = np.where(np.arange(32)[:, None] < 16, aim - dirs * 3.0 * r, C + _unit(rng, 32) * r * rng.uniform(0.05, 0.8, (32, 1)))
                base = _rec_hit(start, dirs, tm, t0)
                p = hit_parts(h, base)
                rows = []
                for root in (p["t1"], p["t2"]):
                    for tmx in (nextbelow(root), root, nextabove(root)):
                        rows.append(_rec_hit(base[:, 0:3], base[:, 3:6], tmx, t0))
                mid = ((p["t1"].astype(np.float64) + p["t2"]) * 0.5).astype(f32)
                rows += [_rec_hit(base[16:, 0:3], base[16:, 3:6], mid[16:], t0), _rec_hit(base[16:, 0:3], base[16:, 3:6], (p["t1"][16:] * f32(2.0)).astype(f32), t0)]
                add("H3", np.concatenate(rows))
            # H4: origins anywhere inside the two domes, the centre and 1e-3 from the wall included
            if r >= 100.0:
                n4 = 4096
                org = C + _unit(rng, n4) * r * np.cbrt(rng.uniform(0.0, 1.0, (n4, 1)))
                org[:64] = C
                org[64:512] = C + _unit(rng, 448) * (r - 1e-3)
                add("H4", _rec_hit(org, _unit(rng, n4), f32(2.0 * r + 7.0), t0))
            # H5: degenerate operands
            base = _rec_hit((C - u * 3.0 * max(r, 1e-3)), u, tm, t0)[0]
            rows = [base.copy() for _ in range(3)]
            rows[0][3:6] = 0.0
            rows[1][3:6] *= f32(2.0 ** 10)
            rows[2][3:6] *= f32(2.0 ** -10)
            for bad in (np.inf, -np.inf, np.nan):
                for slot in range(7):
                    row = base.copy()
                    row[slot] = bad
                    rows.append(row)
            for tmx in (0.0, -1.0, F32_MAX, np.inf):
                for b2 in (base, _rec_hit(C + w * 0.5 * r, v, tm, t0)[0]):
                    row = b2.copy()
                    row[6] = tmx
                    rows.append(row)
            for big in (1e19, 3e19):
                rows.append(_rec_hit(u * big, -u, F32_MAX, t0)[0])
            Cf = C.astype(f32)
            for mask in range(8):  # o - centre is +0 in every subset of the components, against every axis direction with every sign of zero
                o = np.where([(mask >> c) & 1 for c in range(3)], Cf, (C + u * 2.0 * max(r, 1e-3)).astype(f32))
                for d in _axis_dirs():
                    rows.append(_rec_hit(o, d, tm, t0)[0])
            add("H5", np.array(rows, f32))
            # H6: random - half aimed at the sphere, half arbitrary, 1/16 with unnormalised directions
            n6 = N_RANDOM
            scale = max(r, 1e-3) if r < 100.0 else 1.0
            org = C + _unit(rng, n6) * scale * np.exp2(rng.uniform(-1.0, 4.0, (n6, 1)))
            if r >= 100.0:
                org = C + rng.uniform(-3.0, 3.0, (n6, 3))
            d = _unit(rng, n6)
            aim = C + _unit(rng, n6 // 2) * r * rng.uniform(0.0, 1.2, (n6 // 2, 1)) - org[: n6 // 2]
            d[: n6 // 2] = aim / np.maximum(np.linalg.norm(aim, axis=1, keepdims=True), 1e-300)
            d[:: 16] *= np.exp2(rng.uniform(-10, 10, (len(d[::16]), 1)))
            far = 200.0 if r < 100.0 else 2.5 * r  # (the fold starts at 2 * world_radius; a dome's wall lies further than that from its inside)
            add("H6", _rec_hit(org, d, np.where(rng.random(n6) < 0.25, rng.uniform(0.0, 8.0 * scale if r < 100.0 else far, n6), far), t0))
        # H2x: exact t == 0.0001.  A root of a walk above lies on a grid coarser than 0.0001's own ulp (|b| and the square root are both above 2^-13), so a walk
        # steps over the threshold without landing on it.  Near the 1e-3 sphere both terms can be made smaller than 2^-13: unit rays (dx, 1, 0) with |dx| < 2e-4
        # (1 + dx^2 rounds to 1), from an origin on the x axis through the centre - inside, half chord 0.0001, for t2; outside, 0.00012 before a half chord of
        # 0.00002, for t1 - and dx solved by bisection on the statement's root so that it equals 0.0001 + j ulp, j = -2 .. 2
        i3 = RADII.index(1e-3)
        h, C = wd.hitables[i3], _centre_at(wd, i3, 0.0)
        r = float(f32(h.radius))
        for key, x, y in (("t2", np.sqrt(r * r - 1e-8), 0.0), ("t1", np.sqrt(r * r - 4e-10), -1.2e-4)):
            o = np.tile(C, (64, 1))
            o[:, 0] = walk(f32(float(C[0]) + x), count=64)
            o[:, 1] = f32(float(C[1]) + y)
            root = lambda dx: hit_parts(h, _rec_hit(o, np.stack([dx.astype(f32), np.ones(64, f32), np.zeros(64, f32)], 1), f32(200.0), 0.0))[key].astype(np.float64)
            rising = root(np.full(64, 2e-4)) > root(np.full(64, -2e-4))
            for j in range(-2, 3):
                target = float(_unord(_ord(T_HIT) + j))
                lo, hi = np.full(64, -2e-4), np.full(64, 2e-4)
                for _ in range(48):
                    mid = 0.5 * (lo + hi)
                    ge = (root(mid) >= target) == rising
                    lo, hi = np.where(ge, lo, mid), np.where(ge, mid, hi)
                for dx in (lo, hi):
                    out.append(("H2x", i3, _rec_hit(o, np.stack([dx.astype(f32), np.ones(64, f32), np.zeros(64, f32)], 1), f32(200.0), 0.0)))
    return out


def _axis_dirs():
    """axis-aligned unit vectors with every sign of zero in the other components"""
    out = []
    for ax in range(3):
        for s in (1.0, -1.0):
            for z0 in (0.0, -0.0):
                for z1 in (0.0, -0.0):
                    v = [z0, z1]
                    v.insert(ax, s)
                    out.append(v)
    return np.array(out, f32)


# ---- occlusion families ------------------------------------------------------------------------------------------------------------
def _rec_occ(a, b, t0):
    a, b = np.atleast_2d(np.asarray(a, f32)), np.atleast_2d(np.asarray(b, f32))
    n = max(len(a), len(b))
    out = np.empty((n, 7), f32)
    out[:, 0:3], out[:, 3:6], out[:, 6] = a, b, t0
    return out


def occ_cases(wd, fma):
    """[(family, sphere index, records [n, 7])] under the mul_add policy `fma`"""
    out = []
    light = wd.lights[0]
    Lpos, Lrad = np.array([light.pos.x, light.pos.y, light.pos.z]), float(light.rad)
    with RN.fused_policy(fma):
        for ti, (idx, t0) in enumerate(targets()):
            h = wd.hitables[idx]
            C, r = _centre_at(wd, idx, t0).astype(np.float64), float(f32(h.radius))
            u, v, w = _frame(700 + ti)
            rng = np.random.default_rng(9500 + ti)
            ext = max(r, 1e-3)
            add = lambda fam, rec: out.append((fam, idx, np.ascontiguousarray(rec, f32)))
            # O1: dot(oc, dir) across +-0 - the start on the plane through the centre perpendicular to the segment, inside, on and outside the sphere
            k = int(np.argmax(np.abs(u)))
            for q in (0.5 * r, r, 2.0 * r):
                a = _walk_coord((C + v * q).astype(f32), k)
                add("O1", _rec_occ(a, a.astype(np.float64) + u * 4.0 * ext, t0))
                ax = (C.astype(f32) + f32([q, 0, 0])).astype(f32)  # and b == 0 exactly: the start beside the centre along x, the segment along +-y and +-z
                ends = np.tile(ax, (4, 1))
                ends[0, 1], ends[1, 1], ends[2, 2], ends[3, 2] = ax[1] + f32(4 * ext), ax[1] - f32(4 * ext), ax[2] + f32(4 * ext), ax[2] - f32(4 * ext)
                add("O1", _rec_occ(ax, ends, t0))
            # O2: the start at the centre, on the surface and within 4 ulp of it; for the tiny radii also k * r from the centre
            ends = [C + u * 4.0 * ext, C - u * 4.0 * ext, C + w * 4.0 * ext]
            starts = [C.astype(f32)]
            for n_ in (u, -u, v, w):
                s = (C + n_ * r).astype(f32)
                kk = int(np.argmax(np.abs(n_)))
                starts += list(_walk_coord(s, kk, count=9))
            if r <= 3e-15:
                eps = float(np.finfo(f32).eps)
                for kf in (0.0, 0.5, 1.0 - eps, 1.0, 1.0 + eps):
                    for n_ in (u, -u, v, w, np.array([1.0, 0, 0]), np.array([0, -1.0, 0])):
                        starts.append((C + n_ * (kf * r)).astype(f32))
            starts = np.array(starts, f32)
            add("O2", np.concatenate([_rec_occ(starts, e, t0) for e in ends]))
            # O3: |b| < 1e-23 with |c| tiny: b * b underflows.  Start 1e-24 off the perpendicular plane, at 0, 0.5, 1 and 1.5 radii (radii this small only)
            if r <= 3e-15:
                rows = []
                for q in (0.0, 0.5, 1.0, 1.5):
                    for off in (1e-24, -1e-24, 3e-27, -3e-27):
                        a = C + v * (q * r) + u * off
                        rows.append(_rec_occ(a, a + u * 1.0, t0)[0])
                add("O3", np.array(rows, f32))
            # O4: the start outside, its distance walked so that t1 crosses 0.001; the segment ends beyond the sphere
            k = int(np.argmax(np.abs(w)))
            base = (C + w * (r + 1e-3)).astype(f32)
            a = np.concatenate([_walk_coord(base, k, stride=s) for s in STRIDES])
            add("O4", _rec_occ(a, C - w * (r + 4.0 * ext), t0))
            # O5: the end walked along the segment so that dist crosses t1 (4096 consecutive patterns: exact equality is reached where dist takes every float)
            for j in range(4):
                d = _unit(rng, 1)[0]
                a = (C - d * (r + rng.uniform(0.01, 2.0) * ext) + np.cross(d, u) * 0.3 * r).astype(f32)
                t1 = occ_parts(h, _rec_occ(a, a.astype(np.float64) + d * 8.0 * ext, t0))["t1"][0]
                if not (np.isfinite(t1) and t1 > 0):
                    continue
                kk = int(np.argmax(np.abs(d)))
                e = _walk_coord((a.astype(np.float64) + d * float(t1)).astype(f32), kk, count=4096)
                add("O5", _rec_occ(a, e, t0))
            # O6: a == b, non-finite ends, segments 1e-30 long
            a0 = (C - u * 2.0 * ext).astype(f32)
            rows = [_rec_occ(a0, a0, t0)[0], _rec_occ(C, C, t0)[0], _rec_occ(a0, a0.astype(np.float64) + u * 1e-30, t0)[0],
                    _rec_occ(np.zeros(3), u * 1e-30, t0)[0], _rec_occ(u * 1e-30, -u * 1e-30, t0)[0]]  # (1e-30 squared underflows: dist 0 between distinct ends)
            for bad in (np.inf, -np.inf, np.nan):
                for slot in range(6):
                    row = _rec_occ(a0, C + u * 2.0 * ext, t0)[0]
                    row[slot] = bad
                    rows.append(row)
            add("O6", np.array(rows, f32))
            # O7: random segments of the box [-3, 3]^3 around the sphere's neighbourhood; for one third the end lies on the light proxy, as NEE produces
            n7 = N_RANDOM
            shift = C if ext <= 1.0 else 0.0
            sc = ext if r < 0.1 else 1.0  # a sphere far smaller than the box is met by no segment of it: shrink the box with the sphere
            a = shift + rng.uniform(-3.0, 3.0, (n7, 3)) * sc
            b = shift + rng.uniform(-3.0, 3.0, (n7, 3)) * sc
            b[::3] = Lpos + _unit(rng, len(b[::3])) * Lrad
            add("O7", _rec_occ(a, b, t0))
        # O4g: the grazing segment the non-exact early-out mutants are told by: 0.00108 before its closest approach to the 1e-3 sphere, half chord 3e-5
        i3 = RADII.index(1e-3)
        C, r = _centre_at(wd, i3, 0.0).astype(np.float64), float(f32(wd.hitables[i3].radius))
        rows = []
        for s in range(32):
            u, v, w = _frame(800 + s)
            a = C + v * np.sqrt(r * r - 9e-10) - u * 0.00108
            rows.append(_rec_occ(a, a + u * 0.01, 0.0)[0])
        out.append(("O4g", i3, np.array(rows, f32)))
        # O4x: t1 on the threshold itself.  Near the 1e-3 sphere t1 and 0.001 share one binade: the start 0.00102 before a half chord of 0.00002, the segment
        # along +y exactly (so b = -(the start's y offset)), and the start's y walked through 64 consecutive floats - one ulp of t1 per step - for 64 chords
        h = wd.hitables[i3]
        Cf = _centre_at(wd, i3, 0.0)
        xs = walk(f32(float(Cf[0]) + np.sqrt(r * r - 4e-10)), count=64)
        a0 = np.stack([xs, np.full(64, f32(float(Cf[1]) - 1.02e-3), f32), np.full(64, Cf[2], f32)], 1)
        p0 = occ_parts(h, _rec_occ(a0, a0 + f32([0, 0.01, 0]), 0.0))
        half = np.sqrt(p0["descrim"].astype(np.float64))  # the half chord of each x, as the statement sees it
        ys = np.stack([walk(f32(float(Cf[1]) - (float(T_OCC) + hc)), count=64) for hc in half])
        a = np.stack([np.repeat(xs, 64), ys.ravel(), np.full(4096, Cf[2], f32)], 1)
        e = a.copy()
        e[:, 1] = (a[:, 1] + f32(0.01)).astype(f32)
        out.append(("O4x", i3, _rec_occ(a, e, 0.0)))
    return out


# ---- fold worlds --------------------------------------------------------------------------------------------------------------------
SPH = dict(A=((-0.9, 0.31, 0.2), 0.45), B=((0.33, -0.21, 0.13), 0.3), C=((0.07, 0.41, 0.17), 0.25), D=((0.6, 0.9, -0.5), 0.2))
SDF1 = ((0.05, 0.02, -0.03), 0.35)   # overlaps B (before it in F2) and C (after it)
SDF2 = ((-0.2, -0.9, 0.4), 0.3)
N_FOLD = 49999  # rays per fold world (not a multiple of 64), the tie rays not counted


def fold_world(name):
    """(world_desc, frame_params, expected single_sdf index): F1 spheres only; F2 [A, B, SphereSDF, A' (= A), C, C+] with C+ = C one ulp of radius up;
    F3 two SDFs with spheres between and after them"""
    import rayn_amd as A
    from rayn_amd import params as P
    mats = A.MaterialStore()
    mats.add_material(A.Sky(A.Srgb(0.3, 0.4, 0.6), A.Srgb(0.01, 0.015, 0.03)))
    mats.add_material(A.Lambertian(A.Srgb(0.8, 0.3, 0.2)))
    sp = lambda k, up=False: A.Sphere(np.array(SPH[k][0], f32), float(nextabove(SPH[k][1]) if up else f32(SPH[k][1])), 1)
    sdf = lambda s: A.TracedSDF(A.SphereSDF(s[1]), 1, np.array(s[0], f32))
    hit = A.HitableStore()
    order = {"F1": ["A", "B", "A", "C", "C+", "D", "D"], "F2": ["A", "B", SDF1, "A", "C", "C+"], "F3": ["A", SDF1, "B", "A", SDF2, "C", "C+", "D"],
             "F2_sdf_only": [SDF1]}[name]
    for k in order:
        hit.push(sdf(k) if isinstance(k, tuple) else sp(k[0], up=k.endswith("+")))
    cams = A.CameraStore()
    cam = cams.add_camera(A.PinholeCamera((16.0, 16.0), 60.0, A.vec3(0, 0, 3), A.vec3(0, 0, 0), A.vec3(0, 1, 0)))
    world = A.World(hit, [A.SphereLight(A.vec3(-0.3, 0.2, 1.9), 0.15, A.Srgb(1.0, 1.0, 1.0))], mats, cams, A.VolumeParams(None, None))
    return world.to_desc(cam), P.frame_params(16, 16, 1, 2), {"F1": -1, "F2": 2, "F3": -1, "F2_sdf_only": 0}[name]


def fold_rays(wd, fma):
    """(origins, directions) [N_FOLD, 3] for a fold world: per analytic sphere the families H1, H2 and H4-like starts inside it, rays through each sphere's
    centre from seeded directions (the duplicates are met by every one of them), and random rays"""
    org, dirs = [], []
    with RN.fused_policy(fma):
        for i in range(wd.n_hitables):
            h = wd.hitables[i]
            C = np.array([h.center.x, h.center.y, h.center.z], np.float64)
            r = float(f32(h.radius)) if h.kind == 0 else float(f32(h.sdf_radius))
            rng = np.random.default_rng(4000 + i)
            for s in range(4):
                u, v, w = _frame(4100 + 10 * i + s)
                for L in (2.0 * r, 1000.0 * r):  # H1
                    base = (C + v * r - u * L).astype(f32)
                    o = np.concatenate([_walk_coord(base, int(np.argmax(np.abs(v))), stride=st) for st in STRIDES])
                    org.append(o), dirs.append(np.tile(u.astype(f32), (len(o), 1)))
                for sign, dvec in ((1.0, -w), (-1.0, w)):  # H2
                    o = np.concatenate([_walk_coord((C + w * (r + sign * 1e-4)).astype(f32), int(np.argmax(np.abs(w))), stride=st) for st in STRIDES])
                    org.append(o), dirs.append(np.tile(dvec.astype(f32), (len(o), 1)))
            n = 1024
            d = _unit(rng, n)  # through the sphere, from outside and (H4) from inside
            aim = C + _unit(rng, n) * r * rng.uniform(0.0, 1.0, (n, 1))
            start = np.where(np.arange(n)[:, None] < n // 2, aim - d * rng.uniform(1.0, 4.0, (n, 1)), C + _unit(rng, n) * r * rng.uniform(0.0, 0.999, (n, 1)))
            org.append(start.astype(f32)), dirs.append(d.astype(f32))
    org, dirs = np.concatenate(org), np.concatenate(dirs)
    rng = np.random.default_rng(4999)
    n = N_FOLD - len(org)
    assert n > 8192, n
    o = rng.uniform(-3.0, 3.0, (n, 3))
    d = _unit(rng, n)
    d[: n // 2] = rng.uniform(-1.0, 1.0, (n // 2, 3)) - o[: n // 2]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(np.concatenate([org, o.astype(f32)])), np.ascontiguousarray(np.concatenate([dirs, d.astype(f32)]))


def fold_np(wd, p, org, dirs, le=False):
    """HitableStore::add_hits' fold (src/hitable.rs:177-198) over a world of analytic spheres at ray time 0: (t, object index, number of exact ties met);
    le=True plants `<=` for the strict `<`"""
    n = len(org)
    closest = np.full(n, f32(p.world_radius * 2.0), f32)
    obj = np.full(n, 0xFFFFFFFF, np.uint32)
    ties = 0
    for k in range(wd.n_hitables):
        h = wd.hitables[k]
        assert h.kind == 0
        rec = _rec_hit(org, dirs, closest, 0.0)
        ts = hit_np(h, rec)
        ties += int(((ts == closest) & (obj != 0xFFFFFFFF)).sum())
        take = (ts <= closest) if le else (ts < closest)
        closest = np.where(take, ts, closest).astype(f32)
        obj = np.where(take, np.uint32(k), obj)
    return closest, obj, ties


def sdf_tie_rays(oracle, fma, depth, which, n=256, levels=40):
    """Rays of world F2 whose sphere hit and SDF hit are as close as float32 directions allow.  which = "post": sphere C (after the SDF) against the SDF; "pre":
    sphere B (before it).  Per ray an aim point is bisected across the circle in which the two surfaces meet until the sphere's t (the statement's, t_max 200) and
    the SDF's (the oracle's closest hit in the SDF-only world, at `depth`) change order; the last two brackets are kept.
    -> (origins, directions, sign of t_sphere - t_sdf per ray, number of exact ties among the rays, number of aim-point pairs whose first bracket straddled,
    (sign at the final bracket's SDF-side end, sign at its sphere-side end) of those pairs)"""
    wd, p, _ = fold_world("F2")
    wds, ps, _ = fold_world("F2_sdf_only")
    si = 1 if which == "pre" else 4
    h = wd.hitables[si]
    Cs, rs = np.array([h.center.x, h.center.y, h.center.z]), float(f32(h.radius))
    Cd, rd = np.array(SDF1[0], f32).astype(np.float64), float(f32(SDF1[1]))
    axis = Cs - Cd
    D = np.linalg.norm(axis)
    axis /= D
    x = (D * D + rd * rd - rs * rs) / (2 * D)  # the circle's plane, its radius
    rho = np.sqrt(rd * rd - x * x)
    rng = np.random.default_rng(6000 + depth + (100 if which == "pre" else 0))
    e1 = np.cross(axis, [0.3, 0.5, 0.8])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(axis, e1)
    phi = rng.uniform(0, 2 * np.pi, n)
    X = Cd + axis * x + rho * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2)
    outward = (X - (Cd + axis * x)) / rho
    o = (X + (outward + 0.3 * _unit(rng, n)) * rng.uniform(1.5, 3.0, (n, 1))).astype(f32)

    def diff(s):
        d = X + axis * s[:, None] - o
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
        with RN.fused_policy(fma):
            ts = hit_np(h, _rec_hit(o, d, f32(200.0), 0.0))
        td, _ = oracle.closest_hit(wds, ps, depth, o, d, fma=fma)
        return d, ts.astype(np.float64) - td.astype(np.float64)

    lo, hi = np.full(n, -0.05), np.full(n, 0.05)  # aim towards the SDF's side / the sphere's side of the circle
    _, flo = diff(lo)
    _, fhi = diff(hi)
    ok = (flo > 0) & (fhi < 0)  # SDF nearer at lo, sphere nearer at hi
    for s_ in (lo, hi):  # and nothing else of the world in front of either
        _, obj = oracle.closest_hit(wd, p, depth, o, diff(s_)[0], fma=fma)
        ok &= np.isin(obj, [2, si, 5])
    keep = []
    for _ in range(levels):
        mid = 0.5 * (lo + hi)
        dm, fm = diff(mid)
        keep.append((dm, fm))
        up = fm > 0
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    dl, fl_ = diff(lo)
    dh, fh = diff(hi)
    ds_ = [dl, dh] + [k[0] for k in keep[-2:]] + [k[0] for k in keep]
    fs = [fl_, fh] + [k[1] for k in keep[-2:]] + [k[1] for k in keep]
    sel = [ok, ok, ok, ok] + [ok & (f == 0) for _, f in keep]  # the final bracket, the one before it, and every exact tie met on the way
    O = np.concatenate([o[m] for m in sel])
    Dd = np.concatenate([d[m] for d, m in zip(ds_, sel)])
    F = np.concatenate([f[m] for f, m in zip(fs, sel)])
    _, first = np.unique(np.concatenate([O, Dd], 1).view(np.uint32), axis=0, return_index=True)  # a converged bisection repeats its ray
    first.sort()
    O, Dd, F = O[first], Dd[first], F[first]
    return np.ascontiguousarray(O), np.ascontiguousarray(Dd), np.sign(F), int((F == 0).sum()), int(ok.sum()), (np.sign(fl_[ok]), np.sign(fh[ok]))
