"""The scene builders the tests share.  TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this.
(tests/preview_np.py keeps a builder of its own: its scenes differ for real.)"""
import numpy as np


def scene(name, res, camera="pinhole", moving=False):
    """(world description, world, camera handle) of a test scene: s0 sphere SDF, s1 MandelBox, bulb Mandelbulb, multi = MandelBox + sphere SDF;
    moving: the camera's origin and `at` drift, the fractal and one light proxy sphere translate."""
    import rayn_amd as R
    from rayn_amd import setup as S
    from rayn_amd.scene import Linear, OrthographicCamera, Sphere, SphereSDF, ThinLensCamera, TracedSDF
    cam, world = S.SCENES["s1" if name == "multi" else name](res)
    if name == "multi":
        world.hitables.push(TracedSDF(SphereSDF(0.6), 1, R.vec3(1.4, 0.9, 0.3)))
    c = world.cameras.get(cam)
    rs = (float(res[0]), float(res[1]))
    if camera == "thin":
        world.cameras[cam] = ThinLensCamera(rs, 55.0, 0.08, c.origin, c.at, c.up, R.vec3(0.2, 0.1, 0.0))
    elif camera == "ortho":
        world.cameras[cam] = OrthographicCamera(rs, 3.5, c.origin, c.at, c.up)
    if moving:
        c = world.cameras.get(cam)
        c.origin = Linear(c.origin, R.vec3(0.9, -0.3, 0.15))
        c.at = Linear(c.at, R.vec3(0.1, 0.2, 0.0))
        for h in world.hitables:
            if isinstance(h, TracedSDF) and h.transform_seq is None:
                h.transform_seq = Linear(R.vec3(0.0, 0.0, 0.0), R.vec3(-0.6, 0.45, 0.3))
        k = next(i for i, h in enumerate(world.hitables) if isinstance(h, Sphere) and h.radius < 1.0)
        world.hitables[k].transform_seq = Linear(world.hitables[k].transform_seq, R.vec3(0.5, 0.25, -0.4))
    return world.to_desc(cam), world, cam


def moving_scene(w, h):
    """(world, camera handle) of temporal_np.DefaultsCase's scene at another size: the shipped scene under a camera whose origin moves"""
    import rayn_amd as R
    from rayn_amd import setup as S
    from rayn_amd.scene import Linear
    cam, world = S.setup((w, h))
    c = world.cameras.get(cam)
    c.origin = Linear(c.origin, R.vec3(0.9, -0.3, 0.15))
    return world, cam


# ---- the rest of the closed set (SURVEY.md section 8 f/N4): cameras, Lambertian, Box filter, odd scenes ----
def custom_scene(kind, res):
    """(camera handle, World) of one of the closed-set test scenes"""
    import rayn_amd as R
    from rayn_amd import setup as S
    from rayn_amd.scene import _mul
    cam_h, world = S.setup(res, volumes=(kind == "thinlens_volume"), sdf="mandelbox")
    resf = (float(res[0]), float(res[1]))
    origin = _mul(R.vec3(-0.45, 0.2, 2.0), 2.25)
    if kind in ("thinlens", "thinlens_volume"):
        world.cameras = R.CameraStore()
        cam_h = world.cameras.add_camera(R.ThinLensCamera(resf, 50.0, 0.08, origin, R.vec3(0, 0, 0), R.vec3(0, 1, 0), R.vec3(0.2, 0.1, 0.9)))
    elif kind == "ortho":
        world.cameras = R.CameraStore()
        cam_h = world.cameras.add_camera(R.OrthographicCamera(resf, 11.0 / 4.0, R.vec3(9.5, -3.5, 9.5), R.vec3(0.0, 0.8, 0.0), R.vec3(0, 1, 0)))
    elif kind == "anim_pinhole":  # camera motion blur: origin and up are closures |t| base + vel*t (lane-0 time quirk)
        world.cameras = R.CameraStore()
        cam_h = world.cameras.add_camera(R.PinholeCamera(resf, 60.0, R.Linear(origin, R.vec3(6.0, -2.0, 1.0)), R.vec3(0, 0, 0),
                                                         R.Linear(R.vec3(0, 1, 0), R.vec3(2.0, 0.0, 0.0))))
    elif kind == "anim_thinlens":
        world.cameras = R.CameraStore()
        cam_h = world.cameras.add_camera(R.ThinLensCamera(resf, 50.0, 0.05, origin, R.Linear(R.vec3(0, 0, 0), R.vec3(1.0, 2.0, 0.0)), R.vec3(0, 1, 0),
                                                          R.Linear(R.vec3(0.2, 0.1, 0.9), R.vec3(0.0, 0.0, -4.0))))
    elif kind == "anim_spheres":  # closure transform_seq on Spheres: motion-blurred light proxies + a moving diffuse ball
        for i in (2, 3, 4):
            s = world.hitables[i]
            s.transform_seq = R.Linear(s.transform_seq, R.vec3(3.0, -2.0, 1.5))
        ball = world.materials.add_material(R.Lambertian(R.Srgb(0.7, 0.6, 0.5)))
        world.hitables.push(R.Sphere(R.Linear(R.vec3(-1.6, -0.4, 1.9), R.vec3(9.0, 3.0, 0.0)), 0.3, ball))
    elif kind == "lambertian":
        world.materials[1] = R.Lambertian(R.Srgb(0.6, 0.3, 0.2))
    elif kind == "no_lights":
        world.lights = []
    elif kind == "spheres_only":
        del world.hitables[1]
    elif kind == "two_sdfs":
        # a second TracedSDF (sphere SDF) after the MandelBox + one before it: exercises the multi-SDF march paths
        world.hitables.insert(1, R.TracedSDF(R.SphereSDF(0.35), 1))
        world.hitables.push(R.TracedSDF(R.MandelBox(6, R.BoxFold(1.0), R.SphereFold(0.5, 1.0), -2.0), 1))
    elif kind == "offset_sdf":  # EXTENSION: TracedSDF with a constant origin (the SDF's frame is translated)
        world.hitables[1].transform_seq = R.vec3(0.35, -0.2, 0.15)
    elif kind == "moving_sdf":  # EXTENSION: TracedSDF origin as the closure |t| base + vel*t (motion-blurred fractal), volume on
        cam_h, world = S.setup(res, volumes=True, sdf="mandelbox")
        world.hitables[1].transform_seq = R.Linear(R.vec3(0.1, 0.0, -0.05), R.vec3(-4.0, 3.0, 2.0))
    elif kind == "moving_two_sdfs":  # both SDFs of a multi-SDF scene move differently (generic march kernels)
        world.hitables.insert(1, R.TracedSDF(R.SphereSDF(0.35), 1, R.Linear(R.vec3(1.4, 0.9, 0.6), R.vec3(0.0, -6.0, 0.0))))
        world.hitables[2].transform_seq = R.Linear(R.vec3(0.0, 0.0, 0.0), R.vec3(3.0, 0.0, -2.0))
    elif kind == "moving_bulb":
        cam_h, world = S.setup_bulb(res)
        world.hitables[1].transform_seq = R.Linear(R.vec3(0.0, 0.05, 0.0), R.vec3(2.0, -1.0, 0.5))
    elif kind == "morphing_box":  # EXTENSION: MandelBox scale as the closure |t| scale + scale_vel*t (single-SDF fast-path kernels), volume on
        cam_h, world = S.setup(res, volumes=True, sdf="mandelbox")
        world.hitables[1].sdf.scale_vel = 4.0
    elif kind == "morphing_two_sdfs":  # ... in a multi-SDF scene (generic march kernels), together with a moving origin
        world.hitables.push(R.TracedSDF(R.MandelBox(7, R.BoxFold(1.0), R.SphereFold(0.5, 1.0), -2.0, scale_vel=-3.0), 1,
                                        R.Linear(R.vec3(0.3, 0.0, 0.0), R.vec3(0.0, 2.0, 0.0))))
        world.hitables[1].sdf.scale_vel = 2.5
    elif kind == "full_house":  # RAYN_MAX_HITABLES = 16 objects: every class of the bin histogram / scan / scatter is populated (ids 0..15)
        mats = [world.materials.add_material(R.Lambertian(R.Srgb(0.8, 0.3, 0.2))), world.materials.add_material(R.Dielectric.new_remap(R.Srgb(0.3, 0.6, 0.3), 0.4)),
                world.materials.add_material(R.Emissive.new_splat(R.Srgb(2.0, 1.5, 1.0)))]
        k = 0
        while len(world.hitables) < 16:
            a = 0.7 * k
            world.hitables.push(R.Sphere(R.vec3(1.9 * np.cos(a), -1.1 + 0.25 * k, 1.9 * np.sin(a)), 0.22 + 0.02 * k, mats[k % 3]))
            k += 1
    elif kind == "lambert_sdf_sphere":
        world.hitables[1] = R.TracedSDF(R.SphereSDF(1.0), world.materials.add_material(R.Lambertian(R.Srgb(0.5, 0.5, 0.5))))
    elif kind == "huge_lights":
        # r6 (zero-throughput NEE elision, k_shade_setup): one light of absurd power and size next to an over-bright dielectric, volume on.  Close to that light
        # pdf < 1 and x = Le * f * tr lies within a factor 1/pdf of FLT_MAX, so (x * occluded) / pdf is +inf for a VISIBLE sample and 0 for an occluded one;
        # on a segment whose throughput is exactly 0 the reference then adds inf * 0 = NaN (src/integrator.rs:91-92) or nothing - the march outcome reaches
        # the film, the sample fails the elision's bounds (|x| <= 2^60) and must be tested and marched like any other.
        cam_h, world = S.setup(res, volumes=True, sdf="mandelbox")
        world.lights[1].emission = R.Srgb(3.3e38, 1e38, 3e37)
        world.lights[1].rad = 0.9
        world.materials[1] = R.Dielectric.new_remap(R.Srgb(3.0, 3.0, 3.0), 0.6)
    else:
        raise ValueError(kind)
    return cam_h, world


def custom_world(kind, res):
    cam_h, world = custom_scene(kind, res)
    return world.to_desc(cam_h)
