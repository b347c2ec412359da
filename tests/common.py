"""Shared scene/config helpers for the tests (BASELINE.json configs scaled to oracle-sized cases)."""
import numpy as np

from rayn_amd import params as P
from rayn_amd import setup as S


def case(name, width, height, samples, bounces, **kw):
    """Returns (world_desc, frame_params).  name: s0 (sphere SDF), s1 (MandelBox), s2 (MandelBox + volume), s3 (MandelBox, moving camera), ship (setup::setup() as shipped = s2)."""
    cam, world = S.SCENES[name]((width, height))
    return world.to_desc(cam), P.frame_params(width, height, samples, bounces, **kw)


def above(v):
    """the next float32 above v"""
    return np.nextafter(np.float32(v), np.float32(np.inf))


def below(v):
    """the next float32 below v"""
    return np.nextafter(np.float32(v), np.float32(-np.inf))


def film_l2(a, b):
    """max over pixels of the per-pixel L2 distance over all 10 film floats (the north_star metric,
    applied to every channel)."""
    d2 = ((a["color"].astype(np.float64) - b["color"]) ** 2).sum(-1) + ((a["background"].astype(np.float64) - b["background"]) ** 2).sum(-1) \
        + ((a["normal"].astype(np.float64) - b["normal"]) ** 2).sum(-1) + (a["alpha"].astype(np.float64) - b["alpha"]) ** 2
    return float(np.sqrt(d2).max())


def bits_equal(x, y):
    """Bit equality of float32 arrays; two NaNs compare equal whatever their sign/payload (IEEE 754 leaves the
    NaN an invalid operation produces unspecified: x86 makes 0xFFC00000, gfx950 0x7FC00000)."""
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    both_nan = np.isnan(x) & np.isnan(y)
    return x.shape == y.shape and bool(np.all((x.view(np.uint32) == y.view(np.uint32)) | both_nan))


def film_equal_bits(a, b):
    return all(bits_equal(a[k], b[k]) for k in ("color", "alpha", "background", "normal"))


def randomise_materials(world, rng, seed):
    """Random shading parameters for a scene of rayn_amd.setup.setup(): the SDF's material (Lambertian or Dielectric, roughness in [0, 1] with
    the ends 0 and 1 forced on every third seed, albedo incl. 0 and > 1), the emission of the light proxies, the sky colours, and 1 to
    RAYN_MAX_LIGHTS sphere lights of random radius and emission (the shipped ones first, further ones at random positions)."""
    import rayn_amd as R
    from rayn_amd import _abi
    f = lambda lo, hi, k=3: rng.uniform(lo, hi, k).astype(np.float32)
    srgb = lambda v: R.Srgb(*[float(x) for x in v])
    albedo = np.zeros(3, np.float32) if rng.integers(0, 6) == 0 else f(0.0, 1.3)
    if seed % 3 == 0:
        mat = R.Dielectric.new_remap(srgb(albedo), float(seed % 2))
    elif rng.integers(0, 3) == 0:
        mat = R.Lambertian(srgb(albedo))
    else:
        mat = R.Dielectric.new_remap(srgb(albedo), float(np.float32(rng.uniform(0.0, 1.0))))
    sdf_mats = {h.material for h in world.hitables if isinstance(h, R.TracedSDF)}
    for i, m in enumerate(world.materials):
        if i in sdf_mats:
            world.materials[i] = mat
        elif isinstance(m, R.Sky):
            world.materials[i] = R.Sky(srgb(f(0.0, 1.5)), srgb(f(0.0, 0.4)))
        elif isinstance(m, R.Emissive):
            world.materials[i] = R.Emissive.new_splat(srgb(f(0.0, 8.0)))
    nl = int(rng.integers(1, _abi.MAX_LIGHTS + 1))
    lights = list(world.lights[:nl])
    while len(lights) < nl:
        lights.append(R.SphereLight(f(-2.5, 2.5), 0.15, srgb(f(0.0, 1.0))))
    for L in lights:
        L.rad = float(np.float32(np.exp(rng.uniform(np.log(0.01), np.log(0.8)))))
        L.emission = srgb(f(0.0, 60.0))
    world.lights = lights
