"""Per-lane probes of the shading half of the path: camera rays, the sampling maps, the BSDFs, sphere-light and equi-angular volume
sampling, the light pick and the filter importance sampler (rayn_hip_probe_shading, op table in include/rayn_hip.h) against the
oracle's own functions (oracle_probe_shading), bit for bit, under both mul_add policies.  Films reach a small part of these functions'
input space; the edge sets below target the places where the device code (div_by_mag, rcp_sqrt_rn, dmf_* fast paths, compares for
max / min) and the oracle (4-wide IEEE code) differ in form.  The CPU test gives the oracle's side a second opinion from
tests/restatement_np.py on the same inputs."""
import ctypes as C

import numpy as np
import pytest

from common import bits_equal
from oracle.oracle_py import SHADING_IN, SHADING_OUT

f32 = np.float32
N_RANDOM = 1 << 18  # random lanes per op and policy
ONE_MINUS = f32(1.0 - 2.0 ** -24)
SAMPLE_EDGES = np.array([0.0, 0.5, 0.25, 0.75, ONE_MINUS, 2.0 ** -24, 0.5 - 2.0 ** -25, 0.5 + 2.0 ** -24, 1e-6, 0.999995], f32)
ROUGHNESS = [0.0, 1e-3, 0.4, 0.6, 1.0, -0.5, 1.5]  # through Dielectric.new_remap: exponents 301, ~300, 39.88, 8.68, 1, 1519.75, 19.75
LIGHT_RADII = [1e-3, 3e-3, 0.01, 0.05, 0.15, 0.5, 1.0, 2.0, 5.0, 10.0]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
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


def _dirs(rng, n):
    """normalised float32 Gaussians; 1/16 scaled off unit length, 1/32 axis-aligned with signed zeros"""
    g = rng.standard_normal((n, 3)).astype(f32)
    v = (g / np.sqrt((g * g).sum(1, dtype=f32))[:, None]).astype(f32)
    k = n // 16
    v[:k] *= np.exp2(rng.uniform(-10, 10, (k, 1))).astype(f32)
    ax = _axis_dirs()
    m = n // 32
    v[k:k + m] = ax[rng.integers(0, len(ax), m)]
    return v


def _u(rng, n, k=1):
    return rng.random((n, k), dtype=f32)


def _grid(*cols):
    """every combination of the given value lists, one row each"""
    mesh = np.meshgrid(*[np.asarray(c, f32) for c in cols], indexing="ij")
    return np.stack([m.ravel() for m in mesh], 1).astype(f32)


def _probe_world(camera=None):
    """(world_desc, frame_params) of the probe scene: 16 materials (every kind; Lambertian albedo 0 and > 1; Dielectric at every roughness
    of ROUGHNESS, albedo 0 and > 1) and 16 sphere lights (radius 1e-3 .. 10), one upload for a whole sweep."""
    import rayn_amd as R
    from rayn_amd import params as P
    mats = R.MaterialStore()
    mats.add_material(R.Sky(R.Srgb(0.3, 0.4, 0.6), R.Srgb(0.01, 0.015, 0.03)))
    mats.add_material(R.Emissive.new_splat(R.Srgb(2.5, 0.0, 3e38)))
    mats.add_material(R.Lambertian(R.Srgb(0.0, 0.0, 0.0)))
    mats.add_material(R.Lambertian(R.Srgb(3.0, 1.5, 7.0)))
    mats.add_material(R.Lambertian(R.Srgb(0.8, 0.3, 0.2)))
    for r in ROUGHNESS:
        mats.add_material(R.Dielectric.new_remap(R.Srgb(0.2, 0.3, 0.4), r))
    mats.add_material(R.Dielectric.new_remap(R.Srgb(0.0, 0.0, 0.0), 0.25))
    mats.add_material(R.Dielectric.new_remap(R.Srgb(4.0, 2.0, 9.0), 0.8))
    mats.add_material(R.Dielectric.new_remap(R.Srgb(0.7, 0.7, 0.7), 0.05))
    assert len(mats) == 15
    mats.add_material(R.Emissive.new_splat(R.Srgb(0.0, 0.0, 0.0)))
    lights = []
    for i, r in enumerate(LIGHT_RADII):  # exactly representable positions: rays through a centre are exact
        lights.append(R.SphereLight(R.vec3(1.25 * (i % 3) - 1.0, -2.5 + 0.5 * i, 0.75), r, R.Srgb(40.0, 20.0, 10.0)))
    lights.append(R.SphereLight(R.vec3(0.0, 0.0, 0.0), 1.0, R.Srgb(1.0, 1.0, 1.0)))
    lights.append(R.SphereLight(R.vec3(100.0, -50.0, 25.0), 3.0, R.Srgb(1.0, 1.0, 1.0)))
    lights.append(R.SphereLight(R.vec3(-0.3, 0.2, 1.9), 0.15, R.Srgb(1.0, 1.0, 1.0)))
    lights.append(R.SphereLight(R.vec3(1e-3, 2e-3, -1e-3), 1e-3, R.Srgb(1.0, 1.0, 1.0)))
    lights.append(R.SphereLight(R.vec3(0.5, 0.5, 0.5), 0.25, R.Srgb(1.0, 1.0, 1.0)))
    lights.append(R.SphereLight(R.vec3(-4.0, 8.0, -2.0), 7.5, R.Srgb(1.0, 1.0, 1.0)))
    assert len(lights) == 16
    hit = R.HitableStore()
    hit.push(R.Sphere(R.vec3(0.0, 0.0, 0.0), 100.0, 0))
    cams = R.CameraStore()
    cam = cams.add_camera(camera if camera is not None else R.PinholeCamera((16.0, 16.0), 60.0, R.vec3(0, 0, 3), R.vec3(0, 0, 0), R.vec3(0, 1, 0)))
    world = R.World(hit, lights, mats, cams, R.VolumeParams(None, None))
    return world.to_desc(cam), P.frame_params(16, 16, 1, 1)


MAT_SKY, MAT_EMISSIVE = 0, 1
MAT_SCATTER = list(range(2, 15))  # Lambertian and Dielectric


def _cameras(rng):
    """every camera kind x every `animated` bit, random fov / aspect, `up` not orthogonal to the view direction, thin-lens aperture 0 on
    some; plus a degenerate `up` parallel to the view direction"""
    import rayn_amd as R
    out = []
    for kind in range(3):
        for anim in range(16):
            res = (float(rng.integers(1, 400)), float(rng.integers(1, 400)))
            o = rng.uniform(-5, 5, 3).astype(f32)
            at = rng.uniform(-1, 1, 3).astype(f32)
            up = (rng.uniform(-1, 1, 3) + np.array([0, 1.5, 0])).astype(f32)
            fo = rng.uniform(-2, 2, 3).astype(f32)
            seq = lambda v, bit: R.Linear(v, rng.uniform(-3, 3, 3).astype(f32)) if anim >> bit & 1 else v
            if kind == 0:
                c = R.PinholeCamera(res, float(f32(rng.uniform(1, 170))), seq(o, 0), seq(at, 1), seq(up, 2))
            elif kind == 1:
                ap = 0.0 if anim % 3 == 0 else float(f32(rng.uniform(0.001, 0.5)))
                c = R.ThinLensCamera(res, float(f32(rng.uniform(1, 170))), ap, seq(o, 0), seq(at, 1), seq(up, 2), seq(fo, 3))
            else:
                c = R.OrthographicCamera(res, float(f32(rng.uniform(0.01, 20))), seq(o, 0), seq(at, 1), seq(up, 2))
            out.append(c)
    out.append(R.PinholeCamera((32.0, 16.0), 45.0, R.vec3(0, 0, 3), R.vec3(0, 0, 0), R.vec3(0, 0, 1)))
    out.append(R.OrthographicCamera((16.0, 32.0), 2.0, R.vec3(0, 3, 0), R.vec3(0, 0, 0), R.vec3(0, 1, 0)))
    return out


def _groups(op, rng, n_random):
    """[(world_desc, frame_params, index, records, aux)] of one op: random lanes over the whole domain + the explicit edge set"""
    from oracle import oracle_py as O
    wd, p = _probe_world()
    se = SAMPLE_EDGES
    if op == 0:
        cams = _cameras(rng)
        per = max(4, (n_random // len(cams)) // 4 * 4)
        out = []
        for cam in cams:
            cwd, cp = _probe_world(cam)
            uv = np.concatenate([_u(rng, per, 2), _grid([0.0, 0.5, 1.0, ONE_MINUS], [0.0, 0.5, 1.0, ONE_MINUS])])
            lens = np.concatenate([_u(rng, per, 2), _grid(se[:4], se[:4])])
            n = len(uv)
            t0 = np.repeat(rng.uniform(-1.0, 2.0, (n + 3) // 4).astype(f32), 4)[:n, None]  # one t0 per packet of four lanes
            out.append((cwd, cp, 0, np.concatenate([uv, lens, t0], 1), None))
        return out
    if op in (1, 2):
        edge = _grid(np.concatenate([se, [1.0, 0.0]]), np.concatenate([se, [1.0, 0.0]]))
        return [(wd, p, 0, np.concatenate([_u(rng, n_random, 2), edge]), None)]
    if op == 3:
        import rayn_amd as R
        powers = np.array([R.Dielectric.new_remap(R.Srgb(0, 0, 0), r).exponent for r in ROUGHNESS] + [2.0, 1e4], f32)
        rnd = np.concatenate([_u(rng, n_random, 2), rng.choice(np.concatenate([powers, rng.uniform(1, 302, 64).astype(f32)]), (n_random, 1))], 1)
        return [(wd, p, 0, np.concatenate([rnd, _grid(se, se, powers)]), None)]
    if op == 4:
        ax = _axis_dirs()
        edge = np.array([[0, 0, -1], [0, 0, 1], [0.6, 0.8, 0], [0.6, 0.8, -0.0], [-0.6, 0.8, -0.0], [0, -0.0, -1], [1e-20, 1e-20, -1],
                         [0.6, 0, -0.8], [np.nan, 0, 1], [0, 0, np.nan], [0, 0, 0], [0, 0, -0.0], [3.0, 4.0, -0.0]], f32)
        return [(wd, p, 0, np.concatenate([_dirs(rng, n_random), ax, edge]), None)]
    if op == 5:
        rnd = np.concatenate([_u(rng, n_random), np.where(rng.random((n_random, 1)) < 0.5, f32(0.04), _u(rng, n_random))], 1)
        edge = _grid([0.0, -0.0, 1.0, 1e-8, ONE_MINUS, 0.5, 2.0 ** -24], [0.04, 0.0, 1.0, 0.5])
        return [(wd, p, 0, np.concatenate([rnd, edge]), None)]
    if op in (6, 7, 8):
        idx = [i for i in range(16) if i != MAT_SKY] if op == 6 else (list(range(16)) if op == 7 else MAT_SCATTER)
        per = n_random // len(idx)
        ax = _axis_dirs()
        out = []
        for i in idx:
            if op == 7:
                edge = np.concatenate([ax, np.array([[0, 1, 0], [0, -1, 0], [0, 1e-30, 0], [0, np.inf, 0], [0, np.nan, 0]], f32)])
                out.append((wd, p, i, np.concatenate([_dirs(rng, per), edge]), None))
                continue
            nrm = _dirs(rng, per)
            a0 = _dirs(rng, per)
            if op == 6:
                a1 = _dirs(rng, per)
                k = per // 16
                a1[:k] = -a0[:k]   # wi = -wo: the half vector is 0 / 0
                a0[k:2 * k] = nrm[k:2 * k]  # arg0 = n
                a1[2 * k:3 * k] = nrm[2 * k:3 * k]
                rnd = np.concatenate([a0, a1, nrm], 1)
                e = [np.concatenate([x, y, z]) for x in ax[::3] for y in ax[::3] for z in ax[::3]]  # includes wi = -wo, wo = n, wo = -n
                out.append((wd, p, i, np.concatenate([rnd, np.array(e, f32)]), None))
            else:
                k = per // 16
                a0[:k] = nrm[:k]      # wo = normal
                a0[k:2 * k] = -nrm[k:2 * k]
                rnd = np.concatenate([a0, nrm, _u(rng, per, 5)], 1)
                eu = _grid(se[:5], se[:5], se[:5], se[:5])  # u0..u3 on the sample edges
                nsel = np.concatenate([ax, np.array([[0, 0, -1], [0.6, 0, -0.8], [0.6, 0.8, 0]], f32)])
                rows = []
                for j, nv in enumerate(nsel):
                    wo = nsel[(j * 7 + 3) % len(nsel)]
                    blk = np.concatenate([np.tile(wo, (len(eu), 1)), np.tile(nv, (len(eu), 1)), np.full((len(eu), 1), se[j % len(se)], f32), eu], 1)
                    rows.append(blk[rng.choice(len(blk), 96, replace=False)])
                    rows.append(np.concatenate([nv, nv, [0.5], se[:4]])[None].astype(f32))
                    rows.append(np.concatenate([-nv, nv, [0.0], se[4:8]])[None].astype(f32))
                out.append((wd, p, i, np.concatenate([rnd] + rows), None))
        return out
    if op == 9:
        per = n_random // 16
        out = []
        for i in range(16):
            L = wd.lights[i]
            pos, rad = np.array([L.pos.x, L.pos.y, L.pos.z], f32), f32(L.rad)
            d = _dirs(rng, per)
            dist = (rad * np.exp2(rng.uniform(-1, 12, (per, 1)))).astype(f32)
            pts = (pos + d * dist).astype(f32)
            rnd = np.concatenate([_u(rng, per, 2), pts], 1)
            ax = _axis_dirs()[::4]
            special = np.concatenate([pos + ax * rad, pos + ax * (rad * f32(0.5)), pos[None], pos + ax * (rad * f32(1e4)),
                                      pos + _dirs(rng, 8) * rad]).astype(f32)  # on, inside, at the centre of, far from the light
            uu = _grid(se, se)
            edge = np.concatenate([np.repeat(uu, len(special), 0), np.tile(special, (len(uu), 1))], 1)
            out.append((wd, p, i, np.concatenate([rnd, edge]), None))
        return out
    if op == 10:
        per = n_random // 16
        out = []
        for i in range(16):
            L = wd.lights[i]
            pos, rad = np.array([L.pos.x, L.pos.y, L.pos.z], f32), f32(L.rad)
            ro = (pos + _dirs(rng, per) * (rad * np.exp2(rng.uniform(-2, 8, (per, 1))))).astype(f32)
            rd = _dirs(rng, per)
            md = np.exp2(rng.uniform(-8, 8, (per, 1))).astype(f32)
            rnd = np.concatenate([_u(rng, per), ro, rd, md], 1)
            rows = []
            for ax in _axis_dirs()[::4]:
                for s in se:  # a ray through the centre (d = 0), with max_distance == delta and others; a ray starting at the centre
                    for md_ in (4.0, 8.0, 2.0, 0.0):
                        rows.append(np.concatenate([[s], pos - 4 * ax, ax, [md_]]))
                    rows.append(np.concatenate([[s], pos + np.roll(ax, 1) * 0.5 - 4 * ax, ax, [4.0]]))  # off-centre, max_distance == delta
                    rows.append(np.concatenate([[s], pos, ax, [1.0]]))
            out.append((wd, p, i, np.concatenate([rnd, np.array(rows, f32)]), None))
        return out
    if op == 11:
        out = []
        for nl in range(1, 17):
            below = [np.nextafter(f32(k) / f32(nl), f32(0)) for k in range(1, nl + 1)]
            at = [f32(k) / f32(nl) for k in range(nl)]
            edge = np.array(below + at + [0.0, -0.0, 1.0, ONE_MINUS, 1.5, 2.0, 1e10, 5e9, np.inf, -np.inf, np.nan, -1.0, -1e-30, 3e38], f32)
            out.append((wd, p, nl, np.concatenate([_u(rng, n_random // 16)[:, 0], edge])[:, None], None))
        return out
    if op == 12:
        u = np.concatenate([_u(rng, n_random // 2)[:, 0], np.array([0.0, 0.5, ONE_MINUS, 2.0 ** -24, 0.25, 0.75, 5e-6, 4e-6, 0.999995, 0.999996,
                                                                     1.0, -0.0, np.nan, np.inf, -np.inf, -1.0, 2.0, 0.5 - 2.0 ** -25], f32)])[:, None]
        out = []
        for kind, radius, prm in ((0, 1.5, (0.0, 0.0)), (2, 2.0, (1.0 / 3.0, 1.0 / 3.0))):
            fis = O.build_tables(4, 1, 2, 1, 1, 1, filter_kind=kind, filter_radius=radius, filter_params=prm)[3]
            out.append((wd, p, 0, u, fis))
        return out
    raise ValueError(op)


def _report(op, index, inp, got, ref):
    g, r = np.ascontiguousarray(got, f32), np.ascontiguousarray(ref, f32)
    bad = ~((g.view(np.uint32) == r.view(np.uint32)) | (np.isnan(g) & np.isnan(r)))
    rows = np.nonzero(bad.any(1))[0]
    i = rows[0]
    hx = lambda v: " ".join(f"{x:08x}" for x in np.asarray(v, f32).view(np.uint32))
    return (f"op {op} index {index}: {len(rows)} of {len(g)} lanes differ; first lane {i}\n  in  {inp[i].tolist()}\n"
            f"  dev {g[i].tolist()} [{hx(g[i])}]\n  ref {r[i].tolist()} [{hx(r[i])}]")


def _device(gpu_ctx, p, op, index, inp, aux):
    from rayn_amd._lib import lib
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    inp = np.ascontiguousarray(inp, f32)
    out = np.zeros((len(inp), SHADING_OUT[op]), f32)
    a = None if aux is None else np.ascontiguousarray(aux, f32)
    rc = lib().rayn_hip_probe_shading(gpu_ctx.h, C.byref(p), op, index, fp(inp), fp(out), None if a is None else fp(a), len(inp))
    assert rc == 0, gpu_ctx.last_error()
    return out


# ---- GPU: device against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("op", list(range(13)))
def test_shading_probe_bit_exact(gpu_ctx, oracle, op, fma):
    rng = np.random.default_rng(100 + op)
    gpu_ctx.set_fma_policy(fma)
    try:
        last = None
        for wd, p, index, inp, aux in _groups(op, rng, N_RANDOM):
            assert inp.shape[1] == SHADING_IN[op]
            if wd is not last:
                gpu_ctx.upload_world(wd)
                last = wd
            got = _device(gpu_ctx, p, op, index, inp, aux)
            ref = oracle.probe_shading(wd, op, index, inp, aux, fma=bool(fma))
            assert bits_equal(got, ref), _report(op, index, inp, got, ref)
    finally:
        gpu_ctx.set_fma_policy(0)


@pytest.mark.gpu
def test_shading_probe_rejects_unprobed_paths(gpu_ctx, oracle):
    """Sky's f panics in the reference and Sky / Emissive never scatter: both sides refuse those ops instead of inventing a result.  The sphere ops 13 / 14
    refuse an index that names no hitable (this world has one); that they refuse a TracedSDF is tests/test_sphere_device.py's part."""
    from rayn_amd._lib import lib
    wd, p = _probe_world()
    gpu_ctx.upload_world(wd)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    buf = np.zeros(64, f32)
    for op, index in ((6, MAT_SKY), (8, MAT_SKY), (8, MAT_EMISSIVE), (6, 16), (9, 16), (10, 16), (11, 0), (13, 1), (14, 1), (13, 16), (14, 16), (15, 0)):
        assert lib().rayn_hip_probe_shading(gpu_ctx.h, C.byref(p), op, index, fp(buf), fp(buf), None, 1) != 0, (op, index)
        assert len(gpu_ctx.last_error()) > 10, (op, index)
        if op < 15:
            with pytest.raises(ValueError):
                oracle.probe_shading(wd, op, index, buf[:SHADING_IN[op]], None)
    assert lib().rayn_hip_probe_shading(gpu_ctx.h, C.byref(p), 12, 0, fp(buf), fp(buf), None, 1) != 0  # op 12 needs the table


@pytest.mark.gpu
def test_mandelbulb_logf_bit_exact(gpu_ctx, oracle):
    """Probe op 14 of rayn_hip_probe_detmath (dmf_logf, the Mandelbulb estimator's logarithm as the kernels evaluate it: table + short
    polynomial + rounding-safety test) against the oracle's rayn_detmath.h logarithm: 2 M log-uniform arguments over [1e-30, 1e30], a dense
    band around 1 and the special values."""
    from rayn_amd._lib import lib
    rng = np.random.default_rng(14)
    n = 2_000_000
    a = np.exp(rng.uniform(np.log(1e-30), np.log(1e30), n)).astype(f32)
    a[: n // 8] = (1.0 + rng.uniform(-1e-3, 1e-3, n // 8)).astype(f32)
    a[n // 8: n // 8 + 65536] = (np.arange(-32768, 32768, dtype=np.int64) + 0x3F800000).astype(np.uint32).view(f32)  # every float next to 1
    special = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 3e38, -3e38, 88.0, -87.0, 1e4, -1e4, 1e-45,
                        np.finfo(f32).max, np.finfo(f32).tiny, 256.0, 2.0, 0.5], f32)
    a[-special.size:] = special
    out = np.zeros_like(a)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    assert lib().rayn_hip_probe_detmath(gpu_ctx.h, 14, fp(a), fp(a), fp(out), a.size) == 0
    ref = oracle.detmath(6, a)
    bad = ~((out.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(out) & np.isnan(ref)))
    assert not bad.any(), f"{int(bad.sum())} arguments differ, first {a[bad][0]!r}: {out[bad][0]!r} vs {ref[bad][0]!r}"


# ---- CPU: the oracle's side against the numpy restatement ----------------------------------------------------------------------
def _restated(op, wd, index, x):
    """tests/restatement_np.py's version of an op (unfused policy): [n, SHADING_OUT[op]]"""
    import restatement_np as RN
    c = lambda k: x[:, k].copy()
    v3 = lambda k: [c(k), c(k + 1), c(k + 2)]
    n = len(x)
    if op == 1:
        r = list(RN.concentric_circle_map(c(0), c(1)))
    elif op == 2:
        r = RN.cosine_weighted_in_hemisphere(c(0), c(1))
    elif op == 3:
        r = RN.cosine_power_weighted(c(0), c(1), c(2))
    elif op == 4:
        m = RN.onb(v3(0))
        r = m[0] + m[1] + m[2]
    elif op == 5:
        r = [RN.f_schlick(c(0), c(1))]
    elif op == 6:
        r = RN.bsdf_f(wd.materials[index], v3(0), v3(3), v3(6))
    elif op == 7:
        r = RN.bsdf_le(wd.materials[index], v3(0), n)
    elif op == 8:
        nrm = v3(3)
        wi, f, pdf = RN.bsdf_scatter(wd.materials[index], v3(0), nrm, RN.onb(nrm), c(6), [c(7), c(8), c(9), c(10)])
        r = wi + f + [pdf]
    elif op == 9:
        pt, pdf = RN.light_sample(wd.lights[index], c(0), c(1), v3(2))
        r = pt + [pdf]
    elif op == 10:
        r = list(RN.light_sample_volume(wd.lights[index], c(0), v3(1), v3(4), c(7)))
    else:
        raise ValueError(op)
    return np.stack([np.broadcast_to(np.asarray(v, f32), (n,)) for v in r], 1)


@pytest.mark.parametrize("op", list(range(1, 11)))
def test_oracle_shading_second_restatement(oracle, op):
    """The oracle's shading functions (unfused policy) against tests/restatement_np.py, which shares no code with it, on the same edge
    sets as the device test plus random lanes.  restatement_np's transcendentals are binary64 rounded once to binary32: equal to the
    correctly rounded rayn_detmath.h results except next to a rounding tie."""
    rng = np.random.default_rng(100 + op)
    for wd, p, index, inp, aux in _groups(op, rng, 1 << 14):
        if op == 6 and index not in MAT_SCATTER:
            continue  # restatement_np states f for Lambertian and Dielectric only
        ref = oracle.probe_shading(wd, op, index, inp, aux)
        with np.errstate(all="ignore"):
            got = _restated(op, wd, index, inp)
        assert bits_equal(got, ref), _report(op, index, inp, got, ref)
