"""Inputs of the shade-stage probe (rayn_hip_probe_shade), shared by tests/test_shade.py (CPU: the oracle's packet entry against the renderer it wraps, and
every case against the condition it names) and tests/test_shade_device.py (the product kernels against the oracle).  Plain numpy + the CPU oracle; importing
this module needs no GPU.

A case is a list of 4-lane packets of ONE depth of one scene, in the oracle's form (oracle_py.shade_packets): obj [n], valid / sample / pix [n, 4],
lane_f [n, 4, 15].  RECORDED cases are the integrate calls of one 8 x 8 tile as oracle_py.trace_shade saw them; MUTATED cases are a recorded depth with one
named change; `shapes` and `second_trip` cut or tile a recorded depth to a slot count.  to_pool() turns a case into the probe's form: the binned queue
(slot 4k + i = lane i of packet k, padded to whole 64-slot groups) over a pool whose order is a seeded shuffle, unrelated to the slot order, with a few
records nothing refers to.  compare() checks what the probe returned against the oracle's outputs, word for word."""
import functools

import numpy as np

from oracle.oracle_py import SH_BACKGROUND, SH_COLOR, SH_INVALID, SH_SPAWNED, SHADE_IN, SHADE_OUT

SENTINEL = 0xC0FFEE5A   # as a float -7.997..: no result of a case, and not a NaN
INVALID = 0xFFFFFFFF
TERM_NONE = 0xFF
W = H = 16              # film of the recorded scenes: 2 x 2 tiles of 8 x 8
TILE = 8
TILE_INDEX = 1          # column-major: x0 = 0, y0 = 8
SAMPLES = 2             # x 4 lanes = 8 paths per pixel
BOUNCES = 4
EXTRA_RECORDS = 5       # pool records no ref names
F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------------------ scenes

def _ship(volumes=True, sdf="mandelbox"):
    from rayn_amd import setup as S
    return S.setup((W, H), volumes=volumes, sdf=sdf)


def _build_world(name):
    """(camera handle, World, frame-parameter overrides) of a scene tag"""
    import rayn_amd as R
    from rayn_amd.scene import VolumeParams
    kw = {}
    if name in ("ship", "ship_b0", "ship_vm4"):            # the shipped MandelBox scene with volume: 5 lights, VM 2, the per-light volume memo on
        cam, world = _ship()
        if name == "ship_b0":
            kw["max_bounces"] = 0
        if name == "ship_vm4":
            kw["volume_marches"] = 4
    elif name == "s1":                                      # the same without volume: ns = 4
        cam, world = _ship(volumes=False)
    elif name == "spheres_only":                            # no TracedSDF: no job list, no march
        cam, world = _ship(volumes=False)
        del world.hitables[1]
    elif name == "bulbv":                                   # the Mandelbulb with volume: k_shadow_bulb
        cam, world = _ship(sdf="mandelbulb")
    elif name == "two_sdfs":                                # two further TracedSDFs: the generic k_shadow
        cam, world = _ship(volumes=False)
        world.hitables.insert(1, R.TracedSDF(R.SphereSDF(0.35), 1))
        world.hitables.push(R.TracedSDF(R.MandelBox(6, R.BoxFold(1.0), R.SphereFold(0.5, 1.0), -2.0), 1))
    elif name == "anim_spheres":                            # moving light proxies and a moving diffuse ball: the packet time comes from lane 0
        cam, world = _ship(volumes=False)
        for i in (2, 3, 4):
            s = world.hitables[i]
            s.transform_seq = R.Linear(s.transform_seq, R.vec3(3.0, -2.0, 1.5))
        ball = world.materials.add_material(R.Lambertian(R.Srgb(0.7, 0.6, 0.5)))
        world.hitables.push(R.Sphere(R.Linear(R.vec3(-0.6, 0.1, 1.9), R.vec3(9.0, 3.0, 0.0)), 0.45, ball))
    elif name == "lights8":                                 # 8 lights at VM 2: more lights than the memo holds
        cam, world = _ship()
        for k in range(3):
            world.lights.append(R.SphereLight(R.vec3(-1.5 + 1.5 * k, 1.8, -0.4 + 0.7 * k), 0.1 + 0.05 * k, R.Srgb(9.0, 6.0 + k, 3.0)))
    elif name == "lights3_vm4":                             # 3 lights at VM 4
        cam, world = _ship()
        world.lights = world.lights[:3]
        kw["volume_marches"] = 4
    elif name == "no_lights_vol":                           # 0 lights with a scattering volume
        cam, world = _ship()
        world.lights = []
    elif name in ("bound_at", "bound_above"):               # zero_thr_bounds: no extinction, so a volume sample's x is Le * 1/(4 pi) * 1 and the bound sees Le itself
        cam, world = _ship()
        world.volume_params = VolumeParams(0.25, None)
        e = float(F32(2.0) ** 60)
        for L in world.lights:
            L.emission = R.Srgb(e, e, e)
        if name == "bound_above":
            world.lights[1].emission = R.Srgb(float(np.nextafter(F32(e), F32(np.inf))), e, e)
    elif name == "far_open":                                # zero_thr_bounds, pdf side: no sky sphere (so a far sample point is not occluded analytically), no extinction,
        cam, world = _ship()                                # and every light 2^62 away with radius 2^63: it contains every sample point, so its own pdf is the constant
        world.volume_params = VolumeParams(0.25, None)      # 1 / (2 pi), and equi-angular sampling towards it is uniform along the segment: |pdf| = 1 / (2 pi t)
        del world.hitables[0]
        far = float(F32(2.0) ** 62)
        for L, pos in zip(world.lights, ((far, 0, 0), (-far, 0, 0), (0, far, 0), (0, -far, 0), (0, 0, far))):
            L.pos, L.rad = R.vec3(*pos), float(F32(2.0) ** 63)
    elif name == "huge_lights":                             # tests/test_gpu_parity.py's "huge_lights": one light of absurd power and size next to an over-bright dielectric
        cam, world = _ship()
        world.lights[1].emission = R.Srgb(3.3e38, 1e38, 3e37)
        world.lights[1].rad = 0.9
        world.materials[1] = R.Dielectric.new_remap(R.Srgb(3.0, 3.0, 3.0), 0.6)
    elif name == "ball":                                    # grazing: a diffuse ball and two tiny lights, one on the tangent plane of its top point (at smaller x,
        cam, world = _ship(volumes=False)                   # larger z) and one on that of its bottom point (at smaller x and smaller z); no volume
        m = world.materials.add_material(R.Lambertian(R.Srgb(0.7, 0.6, 0.5)))
        world.hitables.push(R.Sphere(R.vec3(*BALL_C), BALL_R, m))
        world.lights = [R.SphereLight(R.vec3(BALL_C[0] - 1.5, BALL_C[1] + BALL_R, BALL_C[2] + 0.75), float(F32(2.0) ** -60), R.Srgb(30.0, 20.0, 10.0)),
                        R.SphereLight(R.vec3(BALL_C[0] - 1.5, BALL_C[1] - BALL_R, BALL_C[2] - 0.75), float(F32(2.0) ** -60), R.Srgb(10.0, 20.0, 30.0))]
    else:
        raise ValueError(name)
    return cam, world, kw


BALL_C, BALL_R = (0.5, 0.5, 2.0), 0.25  # exactly representable, so the points C +- (0, R, 0) (y = 0.75 and 0.25) and their normals (0, +-1, 0) are exact


@functools.lru_cache(maxsize=None)
def scene(name):
    """{wd, p, tabs, ns, n_lights} of a scene tag; the tables are the reference's (oracle build, unfused: they are inputs to both sides)"""
    from oracle import oracle_py
    from rayn_amd import params as P
    cam, world, kw = _build_world(name)
    kw = dict({"max_bounces": BOUNCES}, **kw)
    p = P.frame_params(W, H, SAMPLES, tile_size=(TILE, TILE), **kw)
    tabs = oracle_py.build_tables(4 * p.samples, p.max_bounces, p.volume_marches, p.frame, p.width, p.height)
    wd = world.to_desc(cam)
    return {"name": name, "wd": wd, "p": p, "tabs": tabs, "ns": 4 + (4 * p.volume_marches if wd.has_scattering else 0), "n_lights": len(world.lights),
            "receives": [type(world.materials[h.material]).__name__ not in ("Sky", "Emissive") for h in world.hitables]}


RECORDED_SCENES = ("ship", "s1", "spheres_only", "bulbv", "two_sdfs", "anim_spheres", "lights8", "lights3_vm4", "no_lights_vol", "ship_b0")
SDF_SCENES = tuple(n for n in RECORDED_SCENES if n not in ("spheres_only", "no_lights_vol"))  # a TracedSDF and a light: the shade stage parks shadow segments
SHADOW_KERNEL = {"ship": "k_shadow1", "s1": "k_shadow1", "spheres_only": "none", "bulbv": "k_shadow_bulb", "two_sdfs": "k_shadow", "anim_spheres": "k_shadow1",
                 "lights8": "k_shadow1", "lights3_vm4": "k_shadow1", "no_lights_vol": "k_shadow1", "ship_b0": "k_shadow1"}


@functools.lru_cache(maxsize=None)
def trace(name, fma=False):
    """oracle_py.trace_shade of the recorded tile of a scene, + pix [n, 4] = the film pixel index of every lane (0 on an invalid one)"""
    from oracle import oracle_py
    sc = scene(name)
    tr = oracle_py.trace_shade(sc["wd"], sc["p"], sc["tabs"], TILE_INDEX, fma=fma)
    rows = H // TILE
    x0, y0 = (TILE_INDEX // rows) * TILE, (TILE_INDEX % rows) * TILE
    tr["pix"] = np.where(tr["valid"] != 0, (x0 + tr["tcx"]) + (y0 + tr["tcy"]) * W, 0).astype(np.uint32)
    tr["origin"] = (x0, y0)
    return tr


def recorded(name, depth, fma=False):
    """the packets of one depth of a recorded scene as a case (arrays are copies: mutations do not reach the trace)"""
    tr = trace(name, fma)
    m = tr["depth"] == depth
    return {"scene": name, "depth": depth, "obj": tr["obj"][m].copy(), "valid": tr["valid"][m] != 0, "sample": tr["sample"][m].copy(), "pix": tr["pix"][m].copy(),
            "lane_f": tr["lane_f"][m].copy()}


def recorded_outputs(name, depth, fma=False):
    tr = trace(name, fma)
    m = tr["depth"] == depth
    return tr["status"][m], tr["aov"][m], tr["out_f"][m]


def depths(name):
    return sorted(set(trace(name)["depth"].tolist()))


def expect(case, fma=False):
    """(status, aov, out_f) of the oracle for a case"""
    from oracle import oracle_py
    sc = scene(case["scene"])
    return oracle_py.shade_packets(sc["wd"], sc["p"], sc["tabs"], case["depth"], case["obj"], case["valid"], case["sample"], case["lane_f"], fma=fma)


def expect_tally(case, fma=False, tile_to=None):
    """The oracle's per-lane accounting of a case (dict over oracle_py.TALLY_KEYS): normal and shadow evaluations with their fold / orbit steps, the three
    elision counters, the parked shadow jobs.  tile_to = the slot count to_pool() repeats the packets to (slot j = lane j % 4 of packet (j // 4) % n): the tally
    of each unique packet times how often the tiling holds it."""
    from oracle import oracle_py
    sc = scene(case["scene"])
    run = lambda sl: oracle_py.shade_packets(sc["wd"], sc["p"], sc["tabs"], case["depth"], case["obj"][sl], case["valid"][sl], case["sample"][sl], case["lane_f"][sl],
                                             fma=fma, counts=True)[3]
    n = len(case["obj"])
    if tile_to is None:
        return run(slice(0, n))
    times = np.bincount(np.arange(tile_to // 4) % n, minlength=n)
    total = dict.fromkeys(oracle_py.TALLY_KEYS, 0)
    for k in range(n):
        for key, v in run(slice(k, k + 1)).items():
            total[key] += int(times[k]) * v
    return total


# ------------------------------------------------------------------------------------------------------------------------------ mutated cases

def _take(case, idx, **change):
    idx = np.asarray(idx)
    out = dict(case, **{k: case[k][idx].copy() for k in ("obj", "valid", "sample", "pix", "lane_f")})
    out.update(change)
    return out


def _on(case, scene_name):
    """the same packets shown to another world (objects must mean the same there)"""
    return dict(case, scene=scene_name)


def _set_thr(case, packets, value):
    lf = case["lane_f"]
    for k in np.flatnonzero(packets):
        lf[k, case["valid"][k], SHADE_IN["throughput"]] = value


def special_lane_case(base, component_value, field):
    """the named special value in ONE component of `field`, on lane k % 4 of packet k (the lanes 0..3 in turn) and component (k // 4) % 3, where that lane is valid"""
    c = _take(base, np.arange(len(base["obj"])))
    sl = SHADE_IN[field]
    hit = np.zeros(c["valid"].shape, bool)
    for k in range(len(c["obj"])):
        i = k % 4
        if c["valid"][k, i]:
            c["lane_f"][k, i, sl.start + (k // 4) % 3] = component_value
            hit[k, i] = True
    c["marked"] = hit
    return c


def _receiving(case):
    return np.asarray(scene(case["scene"])["receives"])[case["obj"]]


def build(name):
    """a mutated / shaped case by name; `marked` [n, 4] (where present) = the lanes the named change touched"""
    if name == "zero_thr_huge_lights":
        # tests/test_gpu_parity.py's "huge_lights" with every throughput exactly 0 and the shading points (hit t = 0) scattered 0.3 to 1.3 radii-ish around the
        # huge light (radius 0.9): where x = Le * f * tr divided by the pdf overflows, inf * 0 = NaN reaches the radiance - such a sample fails the elision's
        # bounds and is tested and marched as ever
        c = recorded("ship", 1)
        _set_thr(c, np.ones(len(c["obj"]), bool), 0.0)
        L = scene("huge_lights")["wd"].lights[1]
        pos = np.array([L.pos.x, L.pos.y, L.pos.z], F32)
        rng = np.random.default_rng(3)
        for k in range(len(c["obj"])):
            for i in np.flatnonzero(c["valid"][k]):
                off = rng.normal(size=3)
                off *= rng.uniform(0.3, 1.3) / np.linalg.norm(off)
                c["lane_f"][k, i, SHADE_IN["origin"]] = pos + off.astype(F32)
                c["lane_f"][k, i, SHADE_IN["t"]] = 0.0
        c["marked"] = c["valid"].copy()
        return _on(c, "huge_lights")
    if name in ("zero_thr", "zero_thr_all"):
        c = recorded("ship", 2)
        pk = np.ones(len(c["obj"]), bool) if name == "zero_thr_all" else np.arange(len(c["obj"])) % 2 == 1
        _set_thr(c, pk, 0.0)
        c["marked"] = c["valid"] & pk[:, None]
        return c
    if name in ("zero_thr_bound_at", "zero_thr_bound_above"):
        # sky hits only (the sky receives no light: volume NEE alone), throughput exactly 0, no extinction.  bound_at: every |Le| is exactly 2^60, so every
        # volume sample lies inside the elision's bounds; bound_above: one component of one light is the next float above 2^60.
        c = recorded("ship", 1)
        c = _take(c, np.flatnonzero(~_receiving(c) & (c["obj"] == 0)))
        _set_thr(c, np.ones(len(c["obj"]), bool), 0.0)
        c["marked"] = c["valid"].copy()
        return _on(c, "bound_at" if name == "zero_thr_bound_at" else "bound_above")
    if name in ("zero_thr_pdf_above", "zero_thr_pdf_below"):
        # the same rays as hits of an emissive sphere (no surface NEE either) in "far_open", where |pdf| = 1 / (2 pi t) within a tenth: the hit distance puts it
        # in the middle of the binade above 2^-60 (2^-59.5: elided) or of the one below (2^-60.5: tested, and marched where no sphere is in the way)
        c = recorded("ship", 1)
        c = _take(c, np.flatnonzero(~_receiving(c) & (c["obj"] == 0)))
        c["obj"][:] = 1
        _set_thr(c, np.ones(len(c["obj"]), bool), 0.0)
        c["marked"] = c["valid"].copy()
        t = F32(2.0 ** (59.5 if name == "zero_thr_pdf_above" else 60.5) / (2.0 * np.pi))
        c["lane_f"][:, :, SHADE_IN["t"]] = np.where(c["valid"], t, c["lane_f"][:, :, SHADE_IN["t"]])
        return _on(c, "far_open")
    if name == "nan_thr":
        return special_lane_case(recorded("ship", 2), np.nan, "throughput")
    if name == "inf_thr":
        return special_lane_case(recorded("ship", 2), np.inf, "throughput")
    if name == "inf_rad":
        return special_lane_case(recorded("ship", 2), np.inf, "radiance")
    if name == "denormal_thr":
        return special_lane_case(recorded("ship", 2), F32(1e-42), "throughput")
    if name == "neg_t":  # the Mandelbulb's inside exit: a negative hit distance, and with it a negative equi-angular pdf
        c = recorded("bulbv", 1)
        lane = (np.arange(len(c["obj"]))[:, None] * 4 + np.arange(4)[None, :])
        hit = c["valid"] & (lane % 4 == (lane // 4) % 4) & (c["obj"] == 1)[:, None]
        c["lane_f"][hit, SHADE_IN["t"]] = -np.abs(c["lane_f"][hit, SHADE_IN["t"]])  # (some recorded hits of the bulb are negative already)
        c["marked"] = hit
        return c
    if name == "in_light":
        # hit t = 0 puts the shading point at the origin exactly: at a light's centre, on its surface, inside it - per packet in turn, over the lights in turn
        c = recorded("ship", 1)
        sc = scene("ship")
        hit = np.zeros(c["valid"].shape, bool)
        for k in range(len(c["obj"])):
            L = sc["wd"].lights[(k // 3) % sc["n_lights"]]
            pos, rad = np.array([L.pos.x, L.pos.y, L.pos.z], F32), F32(L.rad)
            where = (pos, pos + np.array([rad, 0, 0], F32), pos + np.array([0, rad * F32(0.5), 0], F32))[k % 3]
            for i in np.flatnonzero(c["valid"][k]):
                c["lane_f"][k, i, SHADE_IN["origin"]] = where
                c["lane_f"][k, i, SHADE_IN["t"]] = 0.0
                hit[k, i] = True
        c["marked"] = hit
        return c
    if name == "grazing":
        # The lights have radius 2^-60, so every sample of one is its centre.  Even packets hit the TOP point of the ball from above: normal (+0, 1, +0), and
        # light 0 on that tangent plane gives wi = (neg, +0, pos): dot(normal, wi) = -0 + +0 + +0 = +0 exactly.  Odd packets hit the BOTTOM point from below:
        # normal (+0, -1, +0), and light 1 on that plane gives wi = (neg, +0, neg): every product is -0, and so is the sum, fused or not.  The other light of
        # each point lies behind the surface (dot < 0).  Every lane comes in at another angle.
        sc = scene("ball")
        ball = len(sc["receives"]) - 1
        base = recorded("s1", 0)
        c = _take(base, np.arange(min(24, len(base["obj"]))))
        rng = np.random.default_rng(5)
        c["obj"][:] = ball
        c["bottom"] = np.arange(len(c["obj"])) % 2 == 1
        for k in range(len(c["obj"])):
            up = F32(-1.0) if c["bottom"][k] else F32(1.0)
            point = np.array(BALL_C, F32) + np.array([0, up * F32(BALL_R), 0], F32)
            c["valid"][k] &= np.array([True, k % 3 != 0, k % 3 == 2, k % 5 == 0])  # lane 0 stays a real hit; 1 to 4 valid lanes
            for i in range(4):
                d = np.array([rng.uniform(-0.6, 0.6), -up, rng.uniform(-0.6, 0.6)], F32)
                d /= F32(np.sqrt((d.astype(np.float64) ** 2).sum()))
                c["lane_f"][k, i, SHADE_IN["dir"]] = d
                c["lane_f"][k, i, SHADE_IN["origin"]] = point  # t = 0: point_at = dir * 0 + origin = the point exactly
                c["lane_f"][k, i, SHADE_IN["t"]] = 0.0
                c["lane_f"][k, i, SHADE_IN["radiance"]] = rng.uniform(0, 1, 3).astype(F32)
                c["lane_f"][k, i, SHADE_IN["throughput"]] = rng.uniform(0.1, 1, 3).astype(F32)
        c["lane_f"][~c["valid"]] = np.nan
        c["lane_f"][~c["valid"], SHADE_IN["radiance"]] = 0
        c["lane_f"][~c["valid"], SHADE_IN["throughput"]] = 0
        c["lane_f"][~c["valid"], SHADE_IN["t"]] = 0
        c["lane_f"][~c["valid"], SHADE_IN["scramble"]] = 0
        c["sample"][~c["valid"]] = 0
        c["pix"][~c["valid"]] = 0
        c["marked"] = c["valid"].copy()
        return _on(c, "ball")
    if name == "far":  # rho_t = 0.035: exp(-rho_t t) is denormal for t = 2700 (e^-94.5) and 0 for t = 3200 (e^-112), alternating per packet
        c = recorded("ship", 1)
        t = np.where(np.arange(len(c["obj"])) % 2 == 0, F32(2700.0), F32(3200.0))
        c["lane_f"][:, :, SHADE_IN["t"]] = np.where(c["valid"], t[:, None], c["lane_f"][:, :, SHADE_IN["t"]])
        c["marked"] = c["valid"] & (t == F32(3200.0))[:, None]
        return c
    if name.startswith("roulette_d"):  # the states of depth 2 shown at depths 2, 3 and max_bounces with component_max(throughput) of 0, 0.5, exactly 1 and 4
        c = recorded("ship", 2)
        c["depth"] = int(name[len("roulette_d"):])
        top = np.array([0.0, 0.5, 1.0, 4.0], F32)[np.arange(len(c["obj"])) % 4]
        for k in range(len(c["obj"])):
            c["lane_f"][k, c["valid"][k], SHADE_IN["throughput"]] = np.array([top[k] * F32(0.25), top[k], top[k] * F32(0.5)], F32)
        c["cmax"] = top
        return c
    if name in ("bins", "bins_dark_wave"):
        # no volume, so a wave fetches its random numbers only when one of its 16 packets receives light.  bins: 5 sky packets, then receiving ones, then
        # emissive ones, then receiving ones again: the waves hold the end of a sky / emissive bin and the start of a receiving one; trailing lanes of every
        # third packet are padding (1, 2 or 3 valid lanes).  bins_dark_wave: a whole wave of sky packets in front of a mixed one.
        base = recorded("s1", 0)
        recv = _receiving(base)
        sky, lit, emis = np.flatnonzero(base["obj"] == 0), np.flatnonzero(recv), np.flatnonzero(~recv & (base["obj"] != 0))
        assert len(sky) >= 16 and len(lit) >= 30 and len(emis) >= 2, (len(sky), len(lit), len(emis))
        if name == "bins":
            order = np.concatenate([sky[:5], lit[:14], emis[:2], sky[5:8], lit[14:30]])
        else:
            order = np.concatenate([sky[:16], sky[:3], lit[:9], emis[:2], lit[9:11]])
        c = _take(base, order)
        for k in range(len(c["obj"])):
            if k % 3 == 0:
                keep = 1 + (k // 3) % 3
                drop = np.arange(4) >= keep
                c["valid"][k, drop] = False
                c["lane_f"][k, drop] = np.nan
                for f in ("radiance", "throughput", "t", "scramble"):
                    c["lane_f"][k, drop, SHADE_IN[f]] = 0
                c["sample"][k, drop] = 0
                c["pix"][k, drop] = 0
        return c
    raise ValueError(name)


MUTATED = ("zero_thr", "zero_thr_all", "zero_thr_huge_lights", "zero_thr_bound_at", "zero_thr_bound_above", "zero_thr_pdf_above", "zero_thr_pdf_below", "nan_thr", "inf_thr", "inf_rad", "denormal_thr", "neg_t", "in_light",
           "grazing", "far", "roulette_d2", "roulette_d3", f"roulette_d{BOUNCES}", "bins", "bins_dark_wave")
SHAPES = [(n, ms, nc) for n in (64, 256, 320, 1024) for ms in (0, 4096) for nc in (0, 192)]  # n_slots, max_slots - n_slots, nee_cap - n_slots


def fit(case, n_slots, tail_packets=2):
    """the case cut to n_slots / 4 packets, or - when it has fewer - repeated cyclically up to n_slots / 4 - tail_packets, which leaves padding packets at the end"""
    n = len(case["obj"])
    want = n_slots // 4
    idx = np.arange(want) if n >= want else np.arange(want - tail_packets) % n
    return _take(case, idx, n_slots=n_slots)


def second_trip_slots(stream_blocks, list_ids_per_block, ns, finish_threads=256):
    """the smallest multiple of 64 for which ns * n_slots exceeds what one trip of k_shadow_list's full grid scans - which also exceeds one trip of k_shade_finish"""
    n = (stream_blocks * list_ids_per_block) // ns + 1
    n = (n + 63) // 64 * 64
    assert ns * n > stream_blocks * list_ids_per_block and n > stream_blocks * finish_threads
    return n


def second_trip_base():
    """the unique packets of second_trip: one recorded depth of the shipped volume scene at VM 4 (ns = 20)"""
    return recorded("ship_vm4", 1)


# ------------------------------------------------------------------------------------------------------------------------------ pool form

def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def to_pool(case, seed=7, extra=EXTRA_RECORDS, tile_to=None):
    """-> dict(ref [n_slots], geo0 / geo1 / col0 / col1 [n_pool, 4], slot [n_valid], lane [n_valid, 2] = (packet, lane) of every referenced record's slot,
    P [n_valid], free [extra]).  tile_to = a slot count the packets are repeated to (second_trip: slot j holds lane j % 4 of packet (j // 4) % n)."""
    n = len(case["obj"])
    if tile_to is None:
        n_slots = case.get("n_slots", (4 * n + 63) // 64 * 64)
        pk = np.arange(n)
    else:
        n_slots = tile_to
        pk = np.arange(tile_to // 4) % n
    assert 4 * len(pk) <= n_slots and n_slots % 64 == 0
    valid = case["valid"][pk]
    kk, ii = np.nonzero(valid)               # slot order
    slot = (4 * kk + ii).astype(np.uint32)
    src_k = pk[kk]
    n_valid = len(slot)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n_valid + extra).astype(np.uint32)
    P, free = perm[:n_valid], perm[n_valid:]
    ref = np.full(n_slots, INVALID, np.uint32)
    ref[slot] = P
    lf = case["lane_f"][src_k, ii]           # [n_valid, 15]
    recs = {k: np.zeros((n_valid + extra, 4), F32) for k in ("geo0", "geo1", "col0", "col1")}
    word = (case["obj"][src_k].astype(np.uint32) | (case["sample"][src_k, ii].astype(np.uint32) << 8))
    recs["geo0"][P, :3] = lf[:, SHADE_IN["origin"]]
    recs["geo0"][P, 3] = lf[:, 3]
    recs["geo1"][P, :2] = lf[:, 4:6]
    recs["geo1"][P, 2] = lf[:, SHADE_IN["t"]]
    recs["geo1"].view(np.uint32)[P, 3] = word
    recs["col0"][P, :3] = lf[:, SHADE_IN["radiance"]]
    recs["col0"][P, 3] = lf[:, 11]
    recs["col1"][P, :2] = lf[:, 12:14]
    recs["col1"].view(np.uint32)[P, 2] = case["pix"][src_k, ii]
    recs["col1"][P, 3] = lf[:, SHADE_IN["time"]]
    for k in recs:                           # records nothing refers to: arbitrary words the stage must leave alone
        recs[k].view(np.uint32)[free] = rng.integers(0, 1 << 32, (extra, 4), dtype=np.uint64).astype(np.uint32)
    return dict(recs, ref=ref, slot=slot, P=P, free=free, packet=src_k, lane=ii, n_slots=n_slots)


def from_pool(pool, scramble):
    """the packets a pool form holds (the inverse of to_pool, up to the records of invalid lanes): obj, valid, sample, pix [n, 4] and lane_f [n, 4, 15]"""
    ref = pool["ref"]
    n = len(ref) // 4
    valid = (ref != INVALID).reshape(n, 4)
    P = np.where(ref == INVALID, 0, ref)
    g0, g1, c0, c1 = (pool[k][P] for k in ("geo0", "geo1", "col0", "col1"))
    word, pix = g1.view(np.uint32)[:, 3], c1.view(np.uint32)[:, 2]
    lf = np.zeros((4 * n, 15), F32)
    lf[:, 0:3] = g0[:, :3]; lf[:, 3] = g0[:, 3]; lf[:, 4:6] = g1[:, :2]; lf[:, 6] = g1[:, 2]; lf[:, 7] = c1[:, 3]
    lf[:, 8:11] = c0[:, :3]; lf[:, 11] = c0[:, 3]; lf[:, 12:14] = c1[:, :2]; lf[:, 14] = scramble[pix]
    obj = (word & 0xFF).reshape(n, 4)
    return {"obj": obj, "valid": valid, "sample": (word >> 8).reshape(n, 4), "pix": pix.reshape(n, 4), "lane_f": lf.reshape(n, 4, 15)}


# ------------------------------------------------------------------------------------------------------------------------------ comparison

def _same(a, b):
    """bit equality of float32 arrays; two NaNs are equal whatever their sign or payload (tests/common.py: bits_equal)"""
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def compare(name, case, pool, got, want, sentinel=SENTINEL, limit=8):
    """Every word the contract names, probe against oracle.  -> (number of differing words, messages for the first `limit`: case, slot, lane of the packet,
    output word, both bit patterns)."""
    status, aov, out_f = want
    k, i, P, slot = pool["packet"], pool["lane"], pool["P"], pool["slot"]
    depth = case["depth"]
    st = status[k, i]
    of = out_f[k, i]
    bad = []  # (slot array, word name, got bits, want bits)

    def chk(word, g, w, where=None, exact=False):
        g, w = np.asarray(g), np.asarray(w)
        ne = (g != w) if exact else ~_same(g.astype(F32, copy=False), w.astype(F32, copy=False))
        if where is not None:
            ne &= where
        idx = np.flatnonzero(ne)
        if len(idx):
            gb = g if exact else _bits(g)
            wb = w if exact else _bits(np.broadcast_to(w, g.shape))
            bad.append((slot[idx], word, gb[idx], np.broadcast_to(wb, gb.shape)[idx]))

    assert (st != SH_INVALID).all(), "the oracle left a valid lane without a status"
    spawned, term = st == SH_SPAWNED, st != SH_SPAWNED
    # status: the survivor ballot and the termination record
    alive_want = np.zeros(pool["n_slots"] // 64, np.uint64)
    np.bitwise_or.at(alive_want, slot[spawned] >> 6, np.uint64(1) << (slot[spawned] & 63).astype(np.uint64))
    groups = np.arange(len(alive_want))
    ne = np.flatnonzero(got["alive_mask"] != alive_want)
    if len(ne):
        bad.append((groups[ne] * 64, "alive_mask (slot = first of the group)", got["alive_mask"][ne], alive_want[ne]))
    cnt_want = np.array([bin(int(m)).count("1") for m in alive_want], np.uint8)
    ne = np.flatnonzero(got["bgrp_cnt"] != cnt_want)
    if len(ne):
        bad.append((groups[ne] * 64, "bgrp_cnt (slot = first of the group)", got["bgrp_cnt"][ne], cnt_want[ne]))
    info_want = np.where(spawned, TERM_NONE, depth | np.where(st == SH_BACKGROUND, 0x80, 0)).astype(np.uint8)
    chk("term_info", got["term_info"][P], info_want, exact=True)
    chk("term_key", got["term_key"][P], np.where(spawned, np.uint32(sentinel), slot), exact=True)
    # radiance of every lane
    for c in range(3):
        chk(f"radiance.{'rgb'[c]}", got["col0"][P, c], of[:, c])
    # spawned lanes: the new ray, with hit_t, the object / sample word, the pixel index and the time unchanged
    g_thr = np.stack([got["col0"][P, 3], got["col1"][P, 0], got["col1"][P, 1]], 1)
    g_dir = np.stack([got["geo0"][P, 3], got["geo1"][P, 0], got["geo1"][P, 1]], 1)
    for c in range(3):
        chk(f"throughput.{'rgb'[c]}", g_thr[:, c], of[:, 3 + c], spawned)
        chk(f"origin.{'xyz'[c]}", got["geo0"][P, c], of[:, 6 + c], spawned)
        chk(f"dir.{'xyz'[c]}", g_dir[:, c], of[:, 9 + c], spawned)
    chk("hit_t (unchanged)", _bits(got["geo1"][P, 2]), _bits(pool["geo1"][P, 2]), exact=True)
    chk("object | sample word (unchanged)", _bits(got["geo1"][P, 3]), _bits(pool["geo1"][P, 3]), exact=True)
    chk("pixel index (unchanged)", _bits(got["col1"][P, 2]), _bits(pool["col1"][P, 2]), exact=True)
    chk("time (unchanged)", _bits(got["col1"][P, 3]), _bits(pool["col1"][P, 3]), exact=True)
    # the aov record: present exactly where the oracle emitted Alpha + WorldNormal
    has = aov[k, i] != 0
    g_aov = _bits(got["aov"][P])
    for c in range(3):
        chk(f"aov.{'xyz'[c]}", got["aov"][P, c], of[:, 12 + c], has)
        chk(f"aov.{'xyz'[c]} (sentinel)", g_aov[:, c], np.uint32(sentinel), ~has, exact=True)
    chk("aov.object", g_aov[:, 3], np.where(has, case["obj"][k], np.uint32(sentinel)).astype(np.uint32), exact=True)
    # pool records no ref names
    free = pool["free"]
    for key in ("geo0", "geo1", "col0", "col1"):
        ne = np.flatnonzero((_bits(got[key][free]) != _bits(pool[key][free])).any(1))
        if len(ne):
            bad.append((np.full(len(ne), INVALID, np.uint32), f"{key} of unreferenced pool record {free[ne].tolist()}", _bits(got[key][free][ne])[:, 0], _bits(pool[key][free][ne])[:, 0]))
    for key, fill in (("aov", sentinel), ("term_key", sentinel), ("term_info", TERM_NONE)):
        g = got[key][free]
        g = _bits(g).reshape(len(free), -1) if g.dtype == F32 else g.reshape(len(free), -1)
        ne = np.flatnonzero((g != fill).any(1))
        if len(ne):
            bad.append((np.full(len(ne), INVALID, np.uint32), f"{key} of unreferenced pool record {free[ne].tolist()}", g[ne][:, 0], np.full(len(ne), fill)))
    total = sum(len(b[0]) for b in bad)
    msgs = []
    for slots, word, gb, wb in bad:
        for s, g, w in zip(slots, gb, wb):
            if len(msgs) < limit:
                msgs.append(f"{name}: slot {int(s)} lane {int(s) % 4} {word}: got 0x{int(g):08x} want 0x{int(w):08x}")
    return total, msgs
