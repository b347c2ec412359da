"""k_shade_setup's per-light volume memo and the sphere list of its inline occlusion tests against the CPU oracle, bit for bit, on small films
of scenes chosen so that every arm of the kernel runs:
  * the volume memo (equi-angular distance, pdf and transmittance per light in LDS) serves up to VOL_MEMO_LIGHTS = 7 lights and is off above
    that, or when the scene has at least as many lights as volume samples (n_lights >= 4 * volume_marches);
  * the occlusion tests iterate DScene::sphere_mask: no analytic sphere besides the sky, the full 15 next to the SDF, moving spheres."""
import numpy as np
import pytest

from common import film_equal_bits

pytestmark = pytest.mark.gpu
W, H, SAMPLES, BOUNCES = 32, 32, 2, 3


def _scene(kind):
    """(world_desc, volume_marches) of one arm; every scene is the shipped MandelBox scene with the volume on"""
    import rayn_amd as R
    from rayn_amd import setup as S
    cam_h, world = S.setup((W, H), volumes=True, sdf="mandelbox")
    vm = S.VOLUME_MARCHES_PER_SAMPLE
    assert vm == 2 and len(world.lights) == 5
    if kind.startswith("lights"):
        n, _, marches = kind[6:].partition("_vm")
        n = int(n)
        rng = np.random.default_rng(100 + n)
        lights = list(world.lights[:n])
        while len(lights) < n:
            pos = rng.uniform(-2.5, 2.5, 3).astype(np.float32)
            lights.append(R.SphereLight(pos, 0.15, R.Srgb(*[float(x) for x in rng.uniform(2.0, 30.0, 3)])))
        world.lights = lights
        if marches:
            vm = int(marches)
    elif kind == "no_spheres":  # the sky dome and the fractal: the sphere list holds the sky alone
        del world.hitables[2:]
    elif kind == "max_spheres":  # RAYN_MAX_HITABLES = 16: the sky, the SDF and 14 spheres
        mats = [world.materials.add_material(R.Lambertian(R.Srgb(0.8, 0.3, 0.2))), world.materials.add_material(R.Dielectric.new_remap(R.Srgb(0.3, 0.6, 0.3), 0.4))]
        k = 0
        while len(world.hitables) < 16:
            a = 0.7 * k
            world.hitables.push(R.Sphere(R.vec3(1.9 * np.cos(a), -1.1 + 0.25 * k, 1.9 * np.sin(a)), 0.22 + 0.02 * k, mats[k % 2]))
            k += 1
    elif kind == "anim_spheres":  # the packet time enters sphere_center
        for i in (2, 3, 4):
            s = world.hitables[i]
            s.transform_seq = R.Linear(s.transform_seq, R.vec3(3.0, -2.0, 1.5))
        ball = world.materials.add_material(R.Lambertian(R.Srgb(0.7, 0.6, 0.5)))
        world.hitables.push(R.Sphere(R.Linear(R.vec3(-1.6, -0.4, 1.9), R.vec3(9.0, 3.0, 0.0)), 0.3, ball))
    elif kind != "shipped":
        raise ValueError(kind)
    return world.to_desc(cam_h), vm


# lights1: every pick repeats; shipped: 5 lights; lights7: the largest memo; lights8: 8 lights for 4 * 2 volume samples, the memo is off by its own
# condition (volume_marches is 2..4, so that condition needs at least 8 lights); lights16: RAYN_MAX_LIGHTS; lights8_vm3: fewer lights than the 12
# volume samples but above VOL_MEMO_LIGHTS, off by the limit alone; lights3_vm4: the memo at the largest march count
KINDS = ["lights1", "shipped", "lights7", "lights8", "lights16", "lights8_vm3", "lights3_vm4", "no_spheres", "max_spheres", "anim_spheres"]


@pytest.mark.parametrize("kind,fma", [(k, False) for k in KINDS] + [("shipped", True)])
def test_setup_memo_film_bits(gpu_ctx, oracle, kind, fma):
    from rayn_amd import params as P
    wd, vm = _scene(kind)
    p = P.frame_params(W, H, SAMPLES, BOUNCES, volume_marches=vm)
    tabs = oracle.build_tables(4 * p.samples, p.max_bounces, p.volume_marches, p.frame, p.width, p.height)
    ref, ctr = oracle.render(wd, p, tabs, fma=fma)
    gpu_ctx.upload_world(wd)
    gpu_ctx.set_fma_policy(1 if fma else 0)
    try:
        out = gpu_ctx.render_host(p, tabs)
        st = gpu_ctx.stats()
    finally:
        gpu_ctx.set_fma_policy(0)
    assert st["paths"] == ctr.paths and st["segments"] == ctr.segments
    assert film_equal_bits(out, ref)
    assert np.abs(ref["color"]).sum() > 0
