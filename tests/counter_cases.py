"""Scenes, sizes and reference tallies shared by tests/test_counters.py (no GPU: the reference is checked first) and tests/test_counters_device.py (the instrumented
kernels are then held to it with ==).  Plain numpy + the CPU oracle; importing this module needs no GPU.

What is counted (oracle/rayn_oracle.cpp, "PER-LANE accounting"): an SDF evaluation is charged to a lane while the lane holds a ray and has not stopped - the
closest hit of every valid ray against every TracedSDF, four evaluations per valid slot whose hit object is a TracedSDF, and the occlusion march of every PARKED
shadow segment against the TracedSDFs in index order up to the first that occludes; plus the fold / orbit steps those evaluations ran, the parked segments, and the
three counters of the zero-throughput elision.  All of it is a deterministic function of the scene and the rays."""
import numpy as np

FRAME_W, FRAME_H, FRAME_SAMPLES = 40, 24, 1   # 4 spp: 3 840 paths in 6 tiles of 16 x 16 (two of them partial)
# (scene, max_bounces): the scenes of the whole-frame tests; s2 also at the depth of the elision test, where roulette and the zero throughputs are at work
FRAMES = [("s1", 3), ("s2", 3), ("s2", 8), ("s0", 3), ("bulbv", 3), ("two_sdfs", 3), ("anim_spheres", 3), ("spheres_only", 3), ("huge_lights", 3)]
EVAL_KEYS = ("extend", "shade_setup", "shadow")
ELISION_KEYS = ("zero_throughput_slots", "elided_shadow_jobs", "samples_out_of_bounds")


def frame_case(name, bounces):
    """(world_desc, frame_params) of a whole-frame case: a rayn_amd.setup.SCENES tag or one of the closed-set scenes of tests/test_gpu_parity.py"""
    from rayn_amd import params as P
    from rayn_amd import setup as S
    from common import case
    if name in S.SCENES:
        return case(name, FRAME_W, FRAME_H, FRAME_SAMPLES, bounces)
    from scenes import custom_world
    return custom_world(name, (FRAME_W, FRAME_H)), P.frame_params(FRAME_W, FRAME_H, FRAME_SAMPLES, bounces)


_frames = {}


def frame_reference(oracle, name, bounces, fma=False):
    """(wd, p, tables, film, counters) of a whole-frame case; the oracle renders once per (scene, bounces, policy)."""
    key = (name, bounces, bool(fma))
    if key not in _frames:
        wd, p = frame_case(name, bounces)
        tabs = oracle.build_tables(4 * p.samples, p.max_bounces, p.volume_marches, p.frame, p.width, p.height, fma=fma)
        film, ctr = oracle.render(wd, p, tabs, fma=fma)
        _frames[key] = (wd, p, tabs, film, ctr)
    return _frames[key]


def expected(ctr):
    """What a counting context must report for the frame of `ctr` (oracle Counters): eval_counts, sdf_iterations, elision_counts as the dicts
    rayn_amd.Context returns them, and rayn_stats.shadow_jobs."""
    ev, it, el, jobs = ctr.device_counts()
    return dict(zip(EVAL_KEYS, ev)), dict(zip(EVAL_KEYS, it)), dict(zip(ELISION_KEYS, el)), jobs


def n_sdfs(wd):
    return sum(1 for k in range(wd.n_hitables) if wd.hitables[k].kind != 0)


def steps_per_eval(h):
    """Fold steps of one evaluation of a MandelBox / sphere SDF (a Mandelbulb's depend on the point)."""
    assert h.kind != 0 and h.sdf_kind in (0, 1)
    return int(h.iterations) if h.sdf_kind == 1 else 0


def as_u64(x):
    return int(np.asarray(x, np.uint64).sum())
