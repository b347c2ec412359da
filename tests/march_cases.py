"""Inputs and helpers for the steady-state tests of the persistent march kernels (tests/test_march_steady_device.py; checked without a GPU by
tests/test_march_cases.py).  Plain numpy + the CPU oracle; importing this module needs no GPU.

k_extend1, k_shadow1 and k_shadow_bulb run in one of two modes, decided per queue chunk: the steady state (every lane hoards a spare ray, or K rays), and the
endgame (one ray per lane, fetched only when the lane is idle) once fewer than ENDGAME_ENTRIES entries (x K in k_shadow_bulb) remain.  A probe of a few
ten thousand rays only ever runs the endgame; steady_n() gives the size from which a launch runs the steady state, the generators fill that many entries with
ordinary rays and the corner classes of tests/test_march_step.py mixed through them, and the threaded oracle helpers make the reference affordable."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

WINDOW = 2048       # every corner class occurs in every WINDOW consecutive entries; i % WINDOW names the class of entry i
CORNER_STRIDE = 8   # entry i is a corner entry iff i % CORNER_STRIDE == CORNER_PHASE: one in eight, so every 64-entry fetch of a wave holds eight of them
CORNER_PHASE = 3
CLASS_SLOTS = 16    # the corner entries cycle through a table of 16 class slots: period 8 * 16 = 128 entries, which divides WINDOW

# shadow segments (start a, end b); the classes of tests/test_march_step.py::_segments
SEG_CLASSES = ("nan_start", "inf_start", "far_start", "zero_length", "end_inside", "neg_zero_start", "neg_zero_end", "nan_end", "near_coincident")
_SEG_SLOTS = (0, 1, 2, 3, 4, 4, 5, 6, 7, 8, 2, 3, 4, 8, 0, 4)
# rays (origin, direction); the classes of tests/test_march_step.py::test_closest_hit_march_test_cases
RAY_CLASSES = ("nan_origin", "inf_origin", "nan_dir", "far_origin", "zero_dir", "neg_zero_origin")
_RAY_SLOTS = (0, 1, 2, 3, 3, 4, 5, 3, 0, 2, 3, 4, 5, 1, 3, 3)
assert len(_SEG_SLOTS) == len(_RAY_SLOTS) == CLASS_SLOTS and WINDOW % (CORNER_STRIDE * CLASS_SLOTS) == 0
assert set(_SEG_SLOTS) == set(range(len(SEG_CLASSES))) and set(_RAY_SLOTS) == set(range(len(RAY_CLASSES)))


def steady_n(chunk, endgame, blocks, k=1, extra_chunks=0):
    """Entries with which one launch of a persistent march kernel (grid of `blocks` blocks of 4 waves, K = k rays per lane) fetches the first
    1 + extra_chunks chunks of every wave in steady state.

    The queue head only moves by atomicAdd(head, CHUNK): the j-th chunk handed out (j = 0, 1, ..) starts at base = j * chunk, whichever wave takes it, and the
    kernel's `endgame = n - base < ENDGAME_ENTRIES * K` puts the wave that took it into the endgame iff n - j * chunk < k * endgame.  The grid holds
    waves = 4 * blocks waves (stride_grid caps it at `blocks`, and n / 256 > blocks here), and a wave's first act is a fetch.  With
        n = k * endgame + waves * chunk * (1 + extra_chunks) + tail,   tail = 3 * 64 + 37 > 0
    every chunk j < waves * (1 + extra_chunks) has n - j * chunk >= k * endgame + tail: the first waves * (1 + extra_chunks) hand-outs - one round of first
    fetches of the whole grid, and extra_chunks further rounds - are all steady-state ones, in whatever order the waves arrive.  (A wave that runs ahead of the
    others takes a later chunk than its turn; the count of steady-state chunks does not depend on who takes them.)  A steady-state wave fetches for all 64 lanes
    at once (a spare per lane), so its first chunk of 256 is four bulk fetches, each promoted while the previous rays still march.
    The tail is odd: 37 entries past three whole 64-groups, so the queue ends in padding entries (extend: INVALID up to the next multiple of 64) and the
    last chunk is a partial one."""
    waves = 4 * blocks
    return k * endgame + waves * chunk * (1 + extra_chunks) + 3 * 64 + 37


def corner_class(i, slots):
    """Class number of entry i under a slot table (_SEG_SLOTS / _RAY_SLOTS), -1 for an ordinary entry.  Works on arrays."""
    i = np.asarray(i, dtype=np.int64)
    cls = np.asarray(slots, dtype=np.int64)[(i // CORNER_STRIDE) % CLASS_SLOTS]
    return np.where(i % CORNER_STRIDE == CORNER_PHASE, cls, -1)


def seg_class(i):
    return corner_class(i, _SEG_SLOTS)


def ray_class(i):
    return corner_class(i, _RAY_SLOTS)


_inputs = {}


def _f32(rng, lo, hi, shape):
    return rng.uniform(lo, hi, shape).astype(np.float32)


def segments(n, seed):
    """(start, end), float32 [n, 3], read-only.  Ordinary segments as in test_occluded_bit_exact (both ends uniform in [-2, 2]^3) with one entry in eight
    replaced by a corner class (SEG_CLASSES), cycling with period 128."""
    key = ("seg", n, seed)
    if key not in _inputs:
        rng = np.random.default_rng(seed)
        a = _f32(rng, -2.0, 2.0, (n, 3))
        b = _f32(rng, -2.0, 2.0, (n, 3))
        noise = _f32(rng, -1e-5, 1e-5, (n, 3))
        c = seg_class(np.arange(n))
        m = lambda name: c == SEG_CLASSES.index(name)
        a[m("nan_start"), 0] = np.nan                                # a NaN FIRST distance
        a[m("inf_start"), 1] = np.inf
        a[m("far_start")] *= np.float32(40.0)                        # the first distance exceeds the segment
        b[m("zero_length")] = a[m("zero_length")]                    # NaN direction: NaN LATER distances
        b[m("end_inside")] *= np.float32(0.05)                       # the end lies inside the set
        a[m("neg_zero_start")] = np.float32(-0.0)
        b[m("neg_zero_end")] = np.float32(-0.0)
        b[m("nan_end"), 2] = np.nan
        a[m("near_coincident")] = b[m("near_coincident")] + noise[m("near_coincident")]
        a.setflags(write=False); b.setflags(write=False)
        _inputs[key] = (a, b)
    return _inputs[key]


def rays(n, seed):
    """(origin, direction), float32 [n, 3], read-only.  Ordinary rays as in test_closest_hit_bit_exact (half of them from the shipped camera position towards
    the scene, half from random origins in [-3, 3]^3 in random directions; unit directions), the two kinds mixed at random so that every wave holds long and
    short marches side by side, with one entry in eight replaced by a corner class (RAY_CLASSES), cycling with period 128."""
    key = ("ray", n, seed)
    if key not in _inputs:
        rng = np.random.default_rng(seed)
        org = _f32(rng, -3.0, 3.0, (n, 3))
        d = _f32(rng, -1.0, 1.0, (n, 3))
        cam = rng.random(n) < 0.5
        org[cam] = np.array([-1.0125, 0.45, 4.5], np.float32)        # the shipped camera position
        d[cam] = -org[cam] + _f32(rng, -1.5, 1.5, (int(cam.sum()), 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
        c = ray_class(np.arange(n))
        m = lambda name: c == RAY_CLASSES.index(name)
        org[m("nan_origin"), 0] = np.nan                             # a NaN first distance
        org[m("inf_origin"), 2] = np.inf
        d[m("nan_dir"), 1] = np.nan                                  # NaN later distances
        org[m("far_origin")] *= np.float32(30.0)
        d[m("zero_dir")] = np.float32(0.0)
        org[m("neg_zero_origin")] = np.float32(-0.0)
        org.setflags(write=False); d.setflags(write=False)
        _inputs[key] = (org, d)
    return _inputs[key]


def cpus():
    """Worker threads for the oracle: the CPUs this process may run on, 16 at the most (never the machine's CPU count)."""
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _blocks(n, parts):
    edges = np.linspace(0, n, parts + 1).astype(np.int64)
    return [(int(lo), int(hi)) for lo, hi in zip(edges[:-1], edges[1:]) if hi > lo]


def oracle_closest_hit_mt(oracle, wd, p, depth, org, d, threads=None):
    """oracle.closest_hit over contiguous blocks of the rays on a thread pool.  Every oracle entry builds its own World from (wd, p) and ctypes releases the GIL
    for the call, so the blocks are independent; a ray's result does not depend on its neighbours."""
    n = len(org)
    parts = _blocks(n, 4 * (threads or cpus()))
    t = np.empty(n, np.float32)
    obj = np.empty(n, np.uint32)

    def run(r):
        lo, hi = r
        t[lo:hi], obj[lo:hi] = oracle.closest_hit(wd, p, depth, org[lo:hi], d[lo:hi])
    with ThreadPoolExecutor(threads or cpus()) as ex:
        list(ex.map(run, parts))
    return t, obj


def oracle_test_occluded_mt(oracle, wd, p, a, b, threads=None):
    """oracle.test_occluded over contiguous blocks of the segments on a thread pool (see oracle_closest_hit_mt)."""
    n = len(a)
    parts = _blocks(n, 4 * (threads or cpus()))
    out = np.empty(n, np.float32)

    def run(r):
        lo, hi = r
        out[lo:hi] = oracle.test_occluded(wd, p, a[lo:hi], b[lo:hi])
    with ThreadPoolExecutor(threads or cpus()) as ex:
        list(ex.map(run, parts))
    return out


def oracle_closest_hit_counts_mt(oracle, wd, p, depth, org, d, threads=None, fma=False):
    """oracle.closest_hit_counts over contiguous blocks of the rays on a thread pool (see oracle_closest_hit_mt): (t, obj, evals, steps) per ray."""
    n = len(org)
    parts = _blocks(n, 4 * (threads or cpus()))
    t = np.empty(n, np.float32)
    obj, ev, it = (np.empty(n, np.uint32) for _ in range(3))

    def run(r):
        lo, hi = r
        t[lo:hi], obj[lo:hi], ev[lo:hi], it[lo:hi] = oracle.closest_hit_counts(wd, p, depth, org[lo:hi], d[lo:hi], fma=fma)
    with ThreadPoolExecutor(threads or cpus()) as ex:
        list(ex.map(run, parts))
    return t, obj, ev, it


def oracle_shadow_counts_mt(oracle, wd, p, a, b, threads=None, fma=False):
    """oracle.shadow_counts over contiguous blocks of the segments on a thread pool: (visibility, evals, steps) per segment."""
    n = len(a)
    parts = _blocks(n, 4 * (threads or cpus()))
    out = np.empty(n, np.float32)
    ev, it = np.empty(n, np.uint32), np.empty(n, np.uint32)

    def run(r):
        lo, hi = r
        out[lo:hi], ev[lo:hi], it[lo:hi] = oracle.shadow_counts(wd, p, a[lo:hi], b[lo:hi], fma=fma)
    with ThreadPoolExecutor(threads or cpus()) as ex:
        list(ex.map(run, parts))
    return out, ev, it


def probe_world(name, sdf_only=False, **kw):
    """(world_desc, frame_params) of a probe scene: a rayn_amd.setup.SCENES tag, "two_sdfs" (two further TracedSDFs: the generic kernels) or "offset_sdf" /
    "moving_sdf" (tests/test_gpu_parity.py: a TracedSDF whose origin is a constant / a closure of time - the probes run at time 0); sdf_only drops the
    analytic spheres, as rayn_hip_probe_shadow marches the TracedSDF factors only; kw = frame parameters (march budgets)."""
    import rayn_amd as R
    from rayn_amd import params as P
    from rayn_amd import setup as S
    if name == "two_sdfs":
        cam, world = S.setup((64, 64), volumes=False, sdf="mandelbox")  # test_gpu_parity's "two_sdfs": a sphere SDF before the MandelBox, a second MandelBox after it
        world.hitables.insert(1, R.TracedSDF(R.SphereSDF(0.35), 1))
        world.hitables.push(R.TracedSDF(R.MandelBox(6, R.BoxFold(1.0), R.SphereFold(0.5, 1.0), -2.0), 1))
    elif name in S.SCENES:
        cam, world = S.SCENES[name]((64, 64))
    else:
        from scenes import custom_scene
        cam, world = custom_scene(name, (64, 64))
    if sdf_only:
        world.hitables[:] = [h for h in world.hitables if isinstance(h, R.TracedSDF)]
    return world.to_desc(cam), P.frame_params(64, 64, 1, 3, **kw)


_results = {}


def clear():
    """Drop the cached inputs and oracle results (some hundred MB at the sizes of the GPU tests)."""
    _inputs.clear()
    _results.clear()


def _key(kind, name, kw, seed, n, extra=()):
    return (kind, name, tuple(sorted(kw.items())), seed, n) + tuple(extra)


def occluded_case(oracle, name, kw, seed, n, fma=False):
    """(wd, p, a, b, ref) for rayn_hip_probe_shadow on segments(n, seed) of scene `name`; the oracle runs once per (scene, params, seed, n, policy), and the
    same call leaves the per-segment counts for occluded_counts()."""
    wd, p = probe_world(name, sdf_only=True, **kw)
    a, b = segments(n, seed)
    key = _key("occ", name, kw, seed, n, (bool(fma),))
    if key not in _results:
        ref, ev, it = oracle_shadow_counts_mt(oracle, wd, p, a, b, fma=fma)
        for x in (ref, ev, it):
            x.setflags(write=False)
        _results[key] = (ref, ev, it)
    return wd, p, a, b, _results[key][0]


def occluded_counts(name, kw, seed, n, fma=False):
    """(evaluations, fold / orbit steps) the instrumented shadow-march kernel must report for occluded_case(...): the sums of the oracle's per-segment counts"""
    _, ev, it = _results[_key("occ", name, kw, seed, n, (bool(fma),))]
    return int(ev.sum(dtype=np.uint64)), int(it.sum(dtype=np.uint64))


def closest_hit_case(oracle, name, depth, kw, seed, n, fma=False):
    """(wd, p, org, d, ref_t, ref_obj) for rayn_hip_probe_extend on rays(n, seed) of scene `name`; the oracle runs once per (scene, params, depth, seed, n,
    policy), and the same call leaves the per-ray counts for closest_hit_counts()."""
    wd, p = probe_world(name, **kw)
    org, d = rays(n, seed)
    key = _key("hit", name, kw, seed, n, (depth, bool(fma)))
    if key not in _results:
        res = oracle_closest_hit_counts_mt(oracle, wd, p, depth, org, d, fma=fma)
        for x in res:
            x.setflags(write=False)
        _results[key] = res
    return (wd, p, org, d) + _results[key][:2]


def closest_hit_counts(name, depth, kw, seed, n, fma=False):
    """(evaluations, fold / orbit steps) the instrumented extend kernel must report for closest_hit_case(...): the sums of the oracle's per-ray counts"""
    _, _, ev, it = _results[_key("hit", name, kw, seed, n, (depth, bool(fma)))]
    return int(ev.sum(dtype=np.uint64)), int(it.sum(dtype=np.uint64))


def counted(ctx, fn, *args):
    """fn(ctx, *args) through the instrumented instantiations (rayn_hip_set_profiling's count_evals; the probes then report into the context's counters):
    (result, eval_counts, sdf_iterations, elision_counts, stage_slots).  Counting is off again afterwards, whatever happens."""
    ctx.set_profiling(False, True)
    try:
        out = fn(ctx, *args)
        return out, ctx.eval_counts(), ctx.sdf_iterations(), ctx.elision_counts(), ctx.stage_slots()
    finally:
        ctx.set_profiling(False, False)


def same_t(t, rt):
    """Per-ray equality of hit distances as bit patterns; two NaNs are equal whatever their sign or payload (tests/common.py: bits_equal)."""
    return (t.view(np.uint32) == rt.view(np.uint32)) | (np.isnan(t) & np.isnan(rt))


def _fp(x):
    return x.ctypes.data_as(C.POINTER(C.c_float))


def march_limits(ctx):
    """(chunk, endgame_entries, persistent_blocks, bulb_rays) of the library and the context's tuning: rayn_hip_probe_march_limits."""
    from rayn_amd._lib import lib
    v = [C.c_uint32() for _ in range(4)]
    rc = lib().rayn_hip_probe_march_limits(ctx.h, *[C.byref(x) for x in v])
    assert rc == 0, rc
    return tuple(int(x.value) for x in v)


def probe_shadow(ctx, p, a, b):
    from rayn_amd._lib import lib
    out = np.zeros(len(a), np.float32)
    assert lib().rayn_hip_probe_shadow(ctx.h, C.byref(p), _fp(a), _fp(b), _fp(out), len(a)) == 0, ctx.last_error()
    return out


def probe_extend(ctx, p, depth, org, d):
    from rayn_amd._lib import lib
    t = np.zeros(len(org), np.float32)
    obj = np.zeros(len(org), np.uint32)
    assert lib().rayn_hip_probe_extend(ctx.h, C.byref(p), depth, _fp(org), _fp(d), _fp(t), obj.ctypes.data_as(C.POINTER(C.c_uint32)), len(org)) == 0, ctx.last_error()
    return t, obj


def describe_mismatches(bad, slots, names):
    """Text for an assertion message: how many entries disagree, the first few indices, and their split over the corner classes (i % WINDOW names the class)."""
    idx = np.flatnonzero(bad)
    if len(idx) == 0:
        return "no mismatches"
    c = corner_class(idx, slots)
    split = {"ordinary": int((c < 0).sum())}
    split.update({names[k]: int((c == k).sum()) for k in range(len(names)) if (c == k).any()})
    return f"{len(idx)} of {len(bad)} entries differ; first {idx[:8].tolist()} (i % {WINDOW}: {(idx[:8] % WINDOW).tolist()}); by class {split}"
