"""numpy restatement of the preview integrator (rayn_hip_preview_device; the definition is in include/rayn_hip.h), binary32 operation by
operation, and the scenes and cases its tests share.  It is built on the CPU oracle's closest_hit (through temporal_np's G-buffer), sdf_dist
(the tetrahedron normal) and test_occluded, and on restatement_np's onb, cosine_weighted_in_hemisphere, fract, normalized and signum; it
shares no code with rayn_amd/csrc/preview.hip, and tests/test_preview_device.py compares the two bit for bit.  TEST INFRASTRUCTURE: nothing
under rayn_amd/ imports this.

Definition, for pixel p = x + y * width (bottom-up rows), all f32 under the mul_add policy where restatement_np's functions honour it:
  1. primary hit = the G-buffer pass: record (P, t), object; every closure time is time_start (the world frozen there);
  2. background = a miss or a hit on a Sky material: colour 0, alpha 0, normal 0, ao 1; everything else is a surface with alpha 1;
  3. n: Sphere normalized(P - center), offset 0; TracedSDF hps = max(0.0001, detail_scale * thr_at(t)), the tetrahedron normal of the SDF at
     P - center with epsilon hps, offset hps;
  4. wo = -d, nf = n * signum(dot(n, wo));
  5. k = 0..K-1: u = fract(s[k].x + r_p), v = fract(s[k].y + r_p), l = cosine_weighted_in_hemisphere(u, v), w = onb(nf) * l,
     a = P + nf * offset, b = a + w * radius, vis_k = test_occluded(a, b);
  6. ao = count(vis_k == 1) / K, hl = ambient + (1 - ambient) * max(0, dot(nf, wo)), colour = ao * hl."""
import numpy as np

import restatement_np as R
import temporal_np as T
from restatement_np import f32

MAT_SKY = 2  # RAYN_MAT_SKY


def _cols(a):
    a = np.ascontiguousarray(a, f32).reshape(-1, 3)
    return [a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()]


def _rows(v):
    return np.stack([np.asarray(c, f32) for c in v], axis=1).astype(f32)


def _center(h, n):
    return R.splat((h.center.x, h.center.y, h.center.z), n)


def preview(oracle, wd, p, samples, scramble, radius, ambient, fma=False):
    """The preview of world wd under the frame parameters p: `samples` (K, 2) float32, `scramble` (n,) float32 or None, f32 radius and
    ambient.  -> dict: color (n, 3), alpha (n,), normal (n, 3), ao (n,), records (n, 4), object (n,) - the entry's outputs - and, for the
    coverage conditions, surface (n,) bool, vis (n, K) float32 (rows of background pixels are 1), sphere_stop / sdf_stop (n, K) bool:
    the AO ray was stopped by an analytic sphere / only by a TracedSDF."""
    samples = np.ascontiguousarray(samples, f32).reshape(-1, 2)
    K = len(samples)
    radius, ambient = f32(radius), f32(ambient)
    org, dirs = T.pixel_centre_rays(oracle, wd, p, fma)
    fw = T.frozen_world(wd, p.time_start)
    t, obj = oracle.closest_hit(fw, p, 0, org, dirs, fma=fma)
    rec, obj = T.gbuffer_assemble(org, dirs, t, obj)
    n = len(obj)
    hit = obj != T.MISS
    sky = np.array([hit[i] and wd.materials[wd.hitables[int(obj[i])].material].kind == MAT_SKY for i in range(n)], bool)
    surface = hit & ~sky
    out = {"records": rec, "object": obj, "surface": surface, "color": np.zeros((n, 3), f32), "alpha": surface.astype(f32), "normal": np.zeros((n, 3), f32),
           "ao": np.ones(n, f32), "vis": np.ones((n, K), f32), "sphere_stop": np.zeros((n, K), bool), "sdf_stop": np.zeros((n, K), bool)}
    sel = np.flatnonzero(surface)
    if len(sel) == 0:
        return out
    m = len(sel)
    half_pixel = R.camera_constants(wd.camera)[4]
    with R.fused_policy(fma), np.errstate(all="ignore"):
        P, ht, hobj = _cols(rec[sel, :3]), rec[sel, 3].copy(), obj[sel]
        wo = R.vneg(_cols(dirs[sel]))
        nrm = [np.zeros(m, f32) for _ in range(3)]
        offset = np.zeros(m, f32)
        for i in range(fw.n_hitables):
            s = np.flatnonzero(hobj == i)
            if len(s) == 0:
                continue
            h = fw.hitables[i]
            ps = R.vsub([P[c][s] for c in range(3)], _center(h, len(s)))
            if h.kind == 0:  # src/sphere.rs:73-86
                nn = R.normalized(ps)
                ob = np.zeros(len(s), f32)
            else:  # src/sdf.rs:85-101 + sdfu normals_fast
                thr = np.full(len(s), half_pixel, f32) if wd.camera.kind == 2 else (half_pixel * ht[s]).astype(f32)
                ob = R.smax(np.full(len(s), f32(0.0001), f32), (f32(p.sdf_detail_scale) * thr).astype(f32))
                gsum = None
                for kx, ky, kz in ((1, -1, -1), (-1, -1, 1), (-1, 1, -1), (1, 1, 1)):
                    kv = [np.full(len(s), f32(kx), f32), np.full(len(s), f32(ky), f32), np.full(len(s), f32(kz), f32)]
                    d = oracle.sdf_dist(h, _rows(R.vadd(ps, R.vscale(kv, ob))), fma=fma)
                    term = R.vscale(kv, d)
                    gsum = term if gsum is None else R.vadd(gsum, term)
                nn = R.normalized(gsum)
            for c in range(3):
                nrm[c][s] = nn[c]
            offset[s] = ob
        nf = R.vscale(nrm, R.signum(R.dot(nrm, wo)))
        basis = R.onb(nf)
        a = R.vadd(P, R.vscale(nf, offset))
        r_p = np.zeros(m, f32) if scramble is None else np.ascontiguousarray(scramble, f32).reshape(-1)[sel]
        spheres = [fw.hitables[i] for i in range(fw.n_hitables) if fw.hitables[i].kind == 0]
        zero_t = np.zeros(m, f32)
        count = np.zeros(m, np.uint32)
        for k in range(K):
            u, v = R.fract((samples[k, 0] + r_p).astype(f32)), R.fract((samples[k, 1] + r_p).astype(f32))
            l = R.cosine_weighted_in_hemisphere(u, v)
            w = R.mat_vec(basis, l)
            b = R.vadd(a, R.vscale(w, radius))
            vis = oracle.test_occluded(fw, p, _rows(a), _rows(b), fma=fma)
            by_sphere = np.zeros(m, bool)
            for h in spheres:
                by_sphere |= R.sphere_occluded(h, a, b, zero_t) == 0
            out["vis"][sel, k] = vis
            out["sphere_stop"][sel, k] = by_sphere
            out["sdf_stop"][sel, k] = (vis == 0) & ~by_sphere
            count += (vis == 1).astype(np.uint32)
        ao = (count.astype(f32) / f32(K)).astype(f32)
        hl = (ambient + ((f32(1.0) - ambient) * R.smax(np.zeros(m, f32), R.dot(nf, wo))).astype(f32)).astype(f32)
        col = (ao * hl).astype(f32)
    out["color"][sel] = col[:, None]
    out["normal"][sel] = _rows(nf)
    out["ao"][sel] = ao
    return out


def ao_inputs(samples, scramble, sel):
    """The (u, v) pairs (m * K, 2) step 5 feeds to cosine_weighted_in_hemisphere for the pixels `sel`: what the sampling-map checks run on."""
    samples = np.ascontiguousarray(samples, f32).reshape(-1, 2)
    r_p = np.zeros(len(sel), f32) if scramble is None else np.ascontiguousarray(scramble, f32).reshape(-1)[sel]
    u = np.stack([R.fract((samples[k, 0] + r_p).astype(f32)) for k in range(len(samples))], axis=1)
    v = np.stack([R.fract((samples[k, 1] + r_p).astype(f32)) for k in range(len(samples))], axis=1)
    return np.stack([u.reshape(-1), v.reshape(-1)], axis=1).astype(f32)


def coverage(ref, has_sdf):
    """The fractions the coverage conditions are about: surface pixels, occluded and visible surface AO rays, and the numbers of rays a
    sphere / a TracedSDF stopped."""
    s = ref["surface"]
    vis = ref["vis"][s]
    return {"surface": float(s.mean()), "background": float((~s).mean()), "occluded": float((vis == 0).mean()) if vis.size else 0.0,
            "visible": float((vis == 1).mean()) if vis.size else 0.0, "sphere_stop": int(ref["sphere_stop"].sum()), "sdf_stop": int(ref["sdf_stop"].sum()),
            "has_sdf": bool(has_sdf)}


def check_coverage(ref, has_sdf):
    """Assert the coverage conditions on a restatement result: at least 5 % surface and 5 % background pixels, at least 5 % occluded and 5 %
    visible surface AO rays and, in a scene with a TracedSDF, at least one ray stopped by a sphere and one by an SDF."""
    c = coverage(ref, has_sdf)
    assert c["surface"] >= 0.05 and c["background"] >= 0.05, c
    assert c["occluded"] >= 0.05 and c["visible"] >= 0.05, c
    if has_sdf:
        assert c["sphere_stop"] >= 1 and c["sdf_stop"] >= 1, c
    return c


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------
# Not built on scenes.scene: the resting sphere, the morphing scale and the Mandelbulb's orthographic size make other world descriptions.
def scene(name, res, camera="pinhole", moving=False):
    """(world description, world, camera handle).  spheres: no TracedSDF - a sphere resting on a ground sphere with a smaller one resting
    against it, under the sky dome; s1: the shipped MandelBox; bulb: the Mandelbulb; multi: MandelBox + a sphere SDF; every SDF scene gets
    an analytic sphere resting against the fractal, so that AO rays meet both kinds.  moving: the camera drifts, the SDF (s1: its scale
    too) and the resting sphere move."""
    import rayn_amd as A
    from rayn_amd import setup as S
    from rayn_amd.scene import Linear, OrthographicCamera, Sphere, ThinLensCamera, TracedSDF, SphereSDF, MandelBox
    if name == "spheres":
        cam, world = S.setup_s0(res)
        grey = world.hitables[1].material
        del world.hitables[1]  # the sphere SDF
        world.hitables.push(Sphere(A.vec3(0.0, 0.0, 0.0), 1.2, grey))
        world.hitables.push(Sphere(A.vec3(0.0, -51.2, 0.0), 50.0, grey))
        world.hitables.push(Sphere(A.vec3(-1.2, -0.6, 1.3), 0.6, grey))
    else:
        cam, world = S.SCENES["s1" if name == "multi" else name](res)
        grey = next(h.material for h in world.hitables if isinstance(h, TracedSDF))
        if name == "multi":
            world.hitables.push(TracedSDF(SphereSDF(0.6), grey, A.vec3(1.4, 0.9, 0.3)))
        world.hitables.push(Sphere(A.vec3(*RESTING[name][:3]), RESTING[name][3], grey))
    c = world.cameras.get(cam)
    rs = (float(res[0]), float(res[1]))
    if camera == "thin":
        world.cameras[cam] = ThinLensCamera(rs, 55.0, 0.08, c.origin, c.at, c.up, A.vec3(0.2, 0.1, 0.0))
    elif camera == "ortho":
        world.cameras[cam] = OrthographicCamera(rs, 3.5 if name != "bulb" else 2.6, c.origin, c.at, c.up)
    if moving:
        c = world.cameras.get(cam)
        c.origin = Linear(c.origin, A.vec3(0.9, -0.3, 0.15))
        c.at = Linear(c.at, A.vec3(0.1, 0.2, 0.0))
        for h in world.hitables:
            if isinstance(h, TracedSDF) and h.transform_seq is None:
                h.transform_seq = Linear(A.vec3(0.0, 0.0, 0.0), A.vec3(-0.6, 0.45, 0.3))
                if isinstance(h.sdf, MandelBox):
                    h.sdf.scale_vel = 0.2  # the fractal morphs too
        k = len(world.hitables) - 1
        world.hitables[k].transform_seq = Linear(world.hitables[k].transform_seq, A.vec3(-0.6, 0.45, 0.3))
    return world.to_desc(cam), world, cam


# the analytic sphere (x, y, z, radius) that rests against each SDF scene's fractal, towards the camera
RESTING = {"s0": (-0.55, 0.35, 1.2, 0.3), "s1": (-0.6, 0.45, 1.35, 0.3), "bulb": (-0.45, 0.3, 1.05, 0.25), "multi": (-0.6, 0.45, 1.35, 0.3)}


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
# (id, scene, camera, moving, (w, h), K, mul_add policy, AO radius, time range or None, scramble?, optional outputs?)
# Cameras and radii were chosen on the CPU so that this restatement alone meets the coverage conditions (check_coverage).  The spheres-only
# scene has no TracedSDF and drops the two conditions about rays stopped in SDF scenes.
CASES = [
    ("spheres-pinhole-k4", "spheres", "pinhole", False, (48, 32), 4, 0, 0.8, None, True, True),
    ("spheres-ortho-k1-bare", "spheres", "ortho", False, (40, 24), 1, 1, 0.8, None, False, False),
    ("box-pinhole-k8", "s1", "pinhole", False, (64, 40), 8, 0, 0.3, None, True, True),
    ("box-thin-k4-fma", "s1", "thin", False, (37, 23), 4, 1, 0.3, None, True, True),
    ("box-pinhole-k8-bare", "s1", "pinhole", False, (37, 23), 8, 0, 0.3, None, False, False),
    ("box-pinhole-k64", "s1", "pinhole", False, (16, 16), 64, 0, 0.3, None, True, True),
    ("bulb-ortho-k4", "bulb", "ortho", False, (40, 24), 4, 0, 0.3, None, True, True),
    ("bulb-pinhole-k1-fma", "bulb", "pinhole", False, (48, 32), 1, 1, 0.3, None, True, True),
    ("multi-thin-k8", "multi", "thin", False, (37, 23), 8, 0, 0.3, None, True, True),
    ("multi-ortho-k4-fma", "multi", "ortho", False, (40, 24), 4, 1, 0.3, None, True, True),
    ("moving-pinhole-k4", "s1", "pinhole", True, (40, 24), 4, 0, 0.3, (0.375, 0.4), True, True),
    ("moving-thin-k4-fma", "s1", "thin", True, (40, 24), 4, 1, 0.3, (-1.25, -1.0), True, True),
]
FRAME = 3  # the frame whose default tables (rayn_amd.film.preview_tables) the cases use
AMBIENT = 0.3


def case_inputs(case):
    """(world description, frame parameters, samples (K, 2), scramble or None) of a case"""
    import rayn_amd as A
    from rayn_amd import film as F
    _, name, camera, moving, (w, h), K, _, _, time_range, with_scramble, _ = case
    wd, _, _ = scene(name, (w, h), camera, moving)
    p = A.frame_params(w, h, 1, 0, frame=FRAME, time_range=time_range)
    samples, scramble = F.preview_tables(K, FRAME, w, h)
    return wd, p, samples, scramble if with_scramble else None


_REFERENCES = {}


def case_reference(oracle, case):
    """The restatement's result of a case, computed once per process and shared read-only by the tests that need it"""
    if case[0] not in _REFERENCES:
        wd, p, samples, scramble = case_inputs(case)
        ref = preview(oracle, wd, p, samples, scramble, case[7], AMBIENT, fma=bool(case[6]))
        for v in ref.values():
            v.setflags(write=False)
        _REFERENCES[case[0]] = ref
    return _REFERENCES[case[0]]
