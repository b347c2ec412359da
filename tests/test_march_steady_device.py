"""The persistent march kernels (k_extend1, k_shadow1, k_shadow_bulb) in their STEADY STATE - spare rays prefetched and promoted while the lane marches, PREFETCH_MIN,
K rays per lane, orbits carried across rounds - against the CPU oracle, bit for bit, on queues sized from the library's own thresholds
(rayn_hip_probe_march_limits -> march_cases.steady_n).  Every other direct comparison of these kernels (test_closest_hit_bit_exact, test_occluded_bit_exact,
tests/test_march_step.py, the two tuning-variant film tests) stays below ENDGAME_ENTRIES and so runs the endgame only: one ray per lane, no spares.

Inputs: march_cases.rays / segments - ordinary rays with the corner classes of tests/test_march_step.py (NaN / infinite / far / zero-length / signed zero) spread
through the whole queue, one entry in eight, so that every wave meets them while it holds spares.  On a mismatch the message names the classes: i % 2048.
Everything is compared exactly: hit distances as bit patterns (NaN equal to NaN), objects and visibility as values.  No tolerance anywhere."""
import contextlib

import numpy as np
import pytest

import march_cases as M
from common import bits_equal, film_equal_bits

pytestmark = pytest.mark.gpu
SEG_SEED, RAY_SEED = 31, 41
TUNED_BLOCKS = 64   # 256 waves: steady_n(.., extra_chunks=3) gives every wave of a tuned context four steady-state chunks at a third of the default context's n
TUNED_EXTRA = 3


@contextlib.contextmanager
def tuned_ctx(monkeypatch, env):
    """One extra context on cuda:0 under RAYN_HIP_ENV_TUNING=1 with `env` and 64 persistent blocks; closed (and the variables removed) on exit."""
    import rayn_amd
    env = dict(env, RAYN_HIP_PERSISTENT_BLOCKS=str(TUNED_BLOCKS))
    monkeypatch.setenv("RAYN_HIP_ENV_TUNING", "1")  # the library reads its tuning variables only under this opt-in, at context creation
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = rayn_amd.Context(0)
    try:
        assert M.march_limits(ctx)[2] == TUNED_BLOCKS
        yield ctx
    finally:
        ctx.close()
        for k in env:
            monkeypatch.delenv(k)
        monkeypatch.delenv("RAYN_HIP_ENV_TUNING")


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    """The inputs and oracle results are shared by the tests of this file (march_cases' cache) and dropped after the last one."""
    yield
    M.clear()


def _n(ctx, k=1, tuned=False):
    chunk, endgame, blocks, _ = M.march_limits(ctx)
    assert blocks == (TUNED_BLOCKS if tuned else 2048)
    n = M.steady_n(chunk, endgame, blocks, k, TUNED_EXTRA if tuned else 0)
    assert n - 4 * blocks * chunk * (1 + (TUNED_EXTRA if tuned else 0)) > k * endgame  # (the sizing rule, restated on the library's constants)
    return n


def check_shadow(ctx, oracle, name, kw, n):
    wd, p, a, b, ref = M.occluded_case(oracle, name, kw, SEG_SEED, n)
    ctx.upload_world(wd)
    out = M.probe_shadow(ctx, p, a, b)
    bad = out != ref
    print(name, kw, "n", n, "mismatches", int(bad.sum()), "occluded share", 1.0 - float(ref.mean()))
    assert not bad.any(), M.describe_mismatches(bad, M._SEG_SLOTS, M.SEG_CLASSES)
    return out


def check_shadow_counted(ctx, oracle, name, kw, n):
    """check_shadow + ONE launch of the instrumented instantiation on the same segments: the same visibility, and evaluations / fold or orbit steps equal to the
    sums of the per-segment counts the oracle call of check_shadow left (march_cases.occluded_counts).  In steady state a lane holds a spare segment while its
    current one has ended, or K - 1 further ones: an evaluation charged to a lane without a current segment, or an orbit carried into the next round and charged
    twice, shows here and at no smaller size.  The stage slots of k_shadow_bulb depend on which wave wins which chunk: inequalities."""
    out = check_shadow(ctx, oracle, name, kw, n)
    wd, p, a, b, _ = M.occluded_case(oracle, name, kw, SEG_SEED, n)
    got, ev, it, el, slots = M.counted(ctx, M.probe_shadow, p, a, b)
    want_ev, want_it = M.occluded_counts(name, kw, SEG_SEED, n)
    print(name, "counted: evals", ev, "iterations", it, "want", want_ev, want_it, "slots", slots)
    assert np.array_equal(got, out)
    assert ev == {"extend": 0, "shade_setup": 0, "shadow": want_ev} and it == {"extend": 0, "shade_setup": 0, "shadow": want_it}
    assert not any(el.values())
    if name == "bulb":
        assert slots["shadow_orbit"] % 64 == 0 and slots["shadow_epilogue"] % 64 == 0 and it["shadow"] <= slots["shadow_orbit"] and ev["shadow"] <= slots["shadow_epilogue"]
    else:
        assert not any(slots.values())


def check_extend(ctx, oracle, name, depth, kw, n):
    wd, p, org, d, rt, robj = M.closest_hit_case(oracle, name, depth, kw, RAY_SEED, n)
    ctx.upload_world(wd)
    t, obj = M.probe_extend(ctx, p, depth, org, d)
    bad_obj, bad_t = obj != robj, ~M.same_t(t, rt)
    print(name, depth, kw, "n", n, "object mismatches", int(bad_obj.sum()), "t mismatches", int(bad_t.sum()))
    assert not bad_obj.any(), "objects: " + M.describe_mismatches(bad_obj, M._RAY_SLOTS, M.RAY_CLASSES)
    assert not bad_t.any(), "t: " + M.describe_mismatches(bad_t, M._RAY_SLOTS, M.RAY_CLASSES)
    return t, obj


def check_extend_counted(ctx, oracle, name, depth, kw, n):
    """check_extend + ONE launch of the instrumented instantiation on the same rays (see check_shadow_counted; the INVALID padding entries at the queue's end
    and the NaN / far corner classes are in it)."""
    t, obj = check_extend(ctx, oracle, name, depth, kw, n)
    wd, p, org, d, _, _ = M.closest_hit_case(oracle, name, depth, kw, RAY_SEED, n)
    (ct, cobj), ev, it, el, slots = M.counted(ctx, M.probe_extend, p, depth, org, d)
    want_ev, want_it = M.closest_hit_counts(name, depth, kw, RAY_SEED, n)
    print(name, depth, "counted: evals", ev, "iterations", it, "want", want_ev, want_it)
    assert np.array_equal(cobj, obj) and np.array_equal(ct.view(np.uint32), t.view(np.uint32))
    assert ev == {"extend": want_ev, "shade_setup": 0, "shadow": 0} and it == {"extend": want_it, "shade_setup": 0, "shadow": 0}
    assert not any(el.values()) and not any(slots.values())


# ---- a. the default context: 2 048 persistent blocks, default thresholds ----------------------------------------------------------------------

def test_limits_probe(gpu_ctx):
    chunk, endgame, blocks, bulb_rays = M.march_limits(gpu_ctx)
    assert chunk > 0 and chunk % 64 == 0 and endgame > 40021  # the older probe tests (<= 40 021 entries) are endgame tests
    assert blocks == 2048 and bulb_rays == 3                  # Tuning's defaults: the shared context is never tuned


@pytest.mark.parametrize("name,depth", [("s1", 0), ("s1", 2), ("s0", 0), ("bulb", 0)])
def test_extend_steady_default(gpu_ctx, oracle, name, depth):
    """k_extend1 (MandelBox in its shipped-shape instantiation, sphere SDF, Mandelbulb) with every wave of the full grid fetching in steady state."""
    (check_extend_counted if (name, depth) == ("s1", 0) else check_extend)(gpu_ctx, oracle, name, depth, {}, _n(gpu_ctx))  # + k_extend1<true, -1> in steady state


@pytest.mark.parametrize("name", ["s1", "s0", "bulb"])
def test_shadow_steady_default(gpu_ctx, oracle, name):
    """k_shadow1 (MandelBox, sphere SDF) and k_shadow_bulb (three rays per lane: its threshold is 3 x ENDGAME_ENTRIES) on the full grid."""
    k = M.march_limits(gpu_ctx)[3] if name == "bulb" else 1
    (check_shadow_counted if name in ("s1", "bulb") else check_shadow)(gpu_ctx, oracle, name, {}, _n(gpu_ctx, k))  # + k_shadow1<true, -1> / k_shadow_bulb<true, K, STEPS>


# ---- b. tuned contexts, one at a time ---------------------------------------------------------------------------------------------------------------

EXTEND_ENVS = [{"RAYN_HIP_PREFETCH_EXTEND": "1"}, {"RAYN_HIP_PREFETCH_EXTEND": "64"}, {"RAYN_HIP_SDF_TEMPLATES": "0"}, {"RAYN_HIP_BOX12S": "0"}]
SHADOW_ENVS = [{"RAYN_HIP_PREFETCH_SHADOW": "1"}, {"RAYN_HIP_PREFETCH_SHADOW": "64"}, {"RAYN_HIP_SDF_TEMPLATES": "0"}]
# the five shapes of test_bulb_march_kernel_variants_are_invisible
BULB_ENVS = [{"RAYN_HIP_BULB_RAYS": "2", "RAYN_HIP_BULB_STEPS": "2"}, {"RAYN_HIP_BULB_RAYS": "4", "RAYN_HIP_BULB_ORBIT_MIN": "0", "RAYN_HIP_BULB_STEPS": "1"},
             {"RAYN_HIP_BULB_RAYS": "3", "RAYN_HIP_BULB_ORBIT_MIN": "63", "RAYN_HIP_BULB_PREFETCH": "1", "RAYN_HIP_BULB_STEPS": "1"},
             {"RAYN_HIP_BULB_RAYS": "2", "RAYN_HIP_BULB_STEPS": "1"}, {"RAYN_HIP_BULB_RAYS": "4", "RAYN_HIP_BULB_STEPS": "2", "RAYN_HIP_BULB_PREFETCH": "200"}]
_id = lambda env: ",".join(f"{k[9:]}={v}" for k, v in env.items()) if isinstance(env, dict) else None


@pytest.mark.parametrize("name", ["s1", "bulb"])
@pytest.mark.parametrize("env", EXTEND_ENVS, ids=_id)
def test_extend_steady_variants(oracle, monkeypatch, env, name):
    """k_extend1: fetch as soon as one lane lacks a spare / only when all do; the instantiation that reads the SDF kind from the object; the per-kind MandelBox one."""
    with tuned_ctx(monkeypatch, env) as ctx:
        check_extend(ctx, oracle, name, 0, {}, _n(ctx, 1, tuned=True))


@pytest.mark.parametrize("name", ["s1", "s0"])
@pytest.mark.parametrize("env", SHADOW_ENVS, ids=_id)
def test_shadow1_steady_variants(oracle, monkeypatch, env, name):
    with tuned_ctx(monkeypatch, env) as ctx:
        check_shadow(ctx, oracle, name, {}, _n(ctx, 1, tuned=True))


def test_shadow1_mandelbulb_instantiation_steady(oracle, monkeypatch):
    """RAYN_HIP_BULB_PATH=0: the Mandelbulb scene through k_shadow1 (one ray per lane + a spare: the threshold is 1 x ENDGAME_ENTRIES)."""
    with tuned_ctx(monkeypatch, {"RAYN_HIP_BULB_PATH": "0"}) as ctx:
        check_shadow(ctx, oracle, "bulb", {}, _n(ctx, 1, tuned=True))


@pytest.mark.parametrize("env", BULB_ENVS, ids=_id)
def test_shadow_bulb_steady_variants(oracle, monkeypatch, env):
    """k_shadow_bulb with 2 / 3 / 4 rays per lane (each with its own K in the sizing), one or two orbit steps per trip, drain-everything and carry-almost-everything
    rounds, eager and lazy refill."""
    with tuned_ctx(monkeypatch, env) as ctx:
        k = M.march_limits(ctx)[3]
        assert k == int(env["RAYN_HIP_BULB_RAYS"])
        check_shadow(ctx, oracle, "bulb", {}, _n(ctx, k, tuned=True))


def test_generic_extend_at_size(oracle, monkeypatch):
    """k_extend (RAYN_HIP_FAST_PATH=0; no endgame of its own) with the eager refill, at the same n."""
    with tuned_ctx(monkeypatch, {"RAYN_HIP_FAST_PATH": "0", "RAYN_HIP_REFILL_EXTEND": "1"}) as ctx:
        check_extend(ctx, oracle, "s1", 0, {}, _n(ctx, 1, tuned=True))


def test_generic_shadow_at_size(oracle, monkeypatch):
    """k_shadow on a scene of several TracedSDFs, at the same n."""
    with tuned_ctx(monkeypatch, {}) as ctx:
        check_shadow(ctx, oracle, "two_sdfs", {}, _n(ctx, 1, tuned=True))


# ---- b2. the queue's end at a chunk boundary --------------------------------------------------------------------------------------------------------
# Every size above puts the end of the queue deep inside a chunk.  Here: one lane; one 64-group minus / plus one entry; exactly one chunk of 256, one short and
# one more (a second wave claims a chunk of ONE entry, every further wave of the grid finds the queue exhausted at its first claim with nothing in hand); two
# chunks plus one.  All endgame launches (n < ENDGAME_ENTRIES): what varies is the cursor's window arithmetic, which is the same in both modes.
EDGE_N = [1, 63, 64, 65, 255, 256, 257, 513]


@pytest.mark.parametrize("n", EDGE_N)
@pytest.mark.parametrize("kernel", ["k_extend1", "k_extend1_bulb", "k_extend"])
def test_extend_queue_edges(gpu_ctx, oracle, monkeypatch, kernel, n):
    assert M.march_limits(gpu_ctx)[0] == 256  # the sizes above are written for this CHUNK
    if kernel == "k_extend":
        with tuned_ctx(monkeypatch, {"RAYN_HIP_FAST_PATH": "0"}) as ctx:
            check_extend(ctx, oracle, "s1", 0, {}, n)
    else:
        check_extend(gpu_ctx, oracle, "bulb" if kernel == "k_extend1_bulb" else "s1", 0, {}, n)


@pytest.mark.parametrize("n", EDGE_N)
@pytest.mark.parametrize("name", ["s1", "bulb", "two_sdfs"])
def test_shadow_queue_edges(gpu_ctx, oracle, name, n):
    """k_shadow1, k_shadow_bulb (default K and STEPS) and k_shadow (a scene of several TracedSDFs)."""
    assert M.march_limits(gpu_ctx)[0] == 256
    check_shadow(gpu_ctx, oracle, name, {}, n)


# ---- c. march budgets in steady state ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,budget", [("s1", 0), ("s1", 1), ("s1", 5), ("bulb", 0), ("bulb", 1), ("bulb", 5)])
def test_shadow_budgets_steady(oracle, monkeypatch, name, budget):
    with tuned_ctx(monkeypatch, {}) as ctx:
        k = M.march_limits(ctx)[3] if name == "bulb" else 1
        check_shadow(ctx, oracle, name, {"max_vis_marches": budget}, _n(ctx, k, tuned=True))


@pytest.mark.parametrize("name,depth,budget", [("s1", 2, 0), ("s1", 0, 1), ("s1", 2, 12), ("bulb", 0, 9)])
def test_extend_budgets_steady(oracle, monkeypatch, name, depth, budget):
    with tuned_ctx(monkeypatch, {}) as ctx:
        check_extend(ctx, oracle, name, depth, {"max_marches": budget}, _n(ctx, 1, tuned=True))


# ---- d. the whole path at size: packet times, INVALID tile-tail entries inside the queue, the counting instantiations ----------------------------------

FILM_W = FILM_H = 256
# x 4 = spp: 1.0 M / 3.9 M paths (>= 2 x ENDGAME_ENTRIES, under the 2^22 that would bring in a second worker).  The bulb fills less of the view and has no central
# light: about 1.5 shadow jobs per path over the three depths, against the 3 x 3 x ENDGAME_ENTRIES = 4.7 M the proof below needs at three rays per lane.
FILM_SAMPLES = {"s3": 4, "bulbm": 15}
FILM_BOUNCES = 2
FILM_ENVS = {"s3": [{}, {"RAYN_HIP_PREFETCH_EXTEND": "1", "RAYN_HIP_PREFETCH_SHADOW": "64"}],
             "bulbm": [{}, {"RAYN_HIP_PREFETCH_EXTEND": "64"}, {"RAYN_HIP_BULB_RAYS": "2", "RAYN_HIP_BULB_STEPS": "1", "RAYN_HIP_BULB_ORBIT_MIN": "0"}]}


def _shadow_reached_steady_state(st, k, endgame, bounces, what):
    """Pigeonhole: more shadow jobs than (max_bounces + 1) launches could hold below the threshold -> at least one launch of the shadow kernel exceeded it."""
    print(what, "paths", st["paths"], "shadow_jobs", st["shadow_jobs"], "needed >", (bounces + 1) * k * endgame, "batches", st["batches"])
    assert st["batches"] == 1
    assert st["paths"] >= 2 * endgame
    assert st["shadow_jobs"] > (bounces + 1) * k * endgame


@pytest.mark.parametrize("name", ["s3", "bulbm"])
def test_whole_path_at_size(gpu_ctx, oracle, monkeypatch, name):
    """One film of >= 2 x ENDGAME_ENTRIES paths in ONE batch on one worker (s3: moving camera and fractal; bulbm: moving camera and bulb): a spread sample of
    whole tiles against the oracle (tiles are independent), every tuned context's whole film against the default context's, and the counting kernels' film."""
    import rayn_amd
    from rayn_amd import params as P
    cam, world = rayn_amd.setup.SCENES[name]((FILM_W, FILM_H))
    wd = world.to_desc(cam)
    p = P.frame_params(FILM_W, FILM_H, FILM_SAMPLES[name], FILM_BOUNCES)
    tabs = oracle.build_tables(4 * p.samples, p.max_bounces, p.volume_marches, p.frame, p.width, p.height)
    _, endgame, _, bulb_rays = M.march_limits(gpu_ctx)
    gpu_ctx.upload_world(wd)
    film = gpu_ctx.render_host(p, tabs)
    _shadow_reached_steady_state(gpu_ctx.stats(), bulb_rays if name == "bulbm" else 1, endgame, FILM_BOUNCES, f"{name} default")
    rows = FILM_H // p.tile_h
    n_tiles = (FILM_W // p.tile_w) * rows
    subset = np.unique(np.linspace(0, n_tiles - 1, 32).astype(np.uint32))
    ref, ctr = oracle.render(wd, p, tabs, threads=M.cpus(), tile_subset=subset)
    for t in subset:
        tx, ty = int(t) // rows, int(t) % rows  # reference tile order: column-major
        sl = (slice(ty * p.tile_h, (ty + 1) * p.tile_h), slice(tx * p.tile_w, (tx + 1) * p.tile_w))
        for ch in ("color", "alpha", "background", "normal"):
            assert bits_equal(film[ch][sl], ref[ch][sl]), (name, int(t), ch)
    assert len(np.unique(film["alpha"])) > 2  # fractal and sky both in view
    # the counting instantiations (k_extend1<true, -1>, k_shadow1<true, -1> / k_shadow_bulb<true, K, STEPS>) at size
    gpu_ctx.set_profiling(False, True)
    try:
        counted = gpu_ctx.render_host(p, tabs)
        ev, it, slots = gpu_ctx.eval_counts(), gpu_ctx.sdf_iterations(), gpu_ctx.stage_slots()
    finally:
        gpu_ctx.set_profiling(False, False)
    assert film_equal_bits(counted, film)
    print(name, "evals", ev, "iterations", it, "slots", slots)
    assert all(v > 0 for v in ev.values())
    if name == "bulbm":
        assert 0 < it["shadow"] <= slots["shadow_orbit"] and 0 < ev["shadow"] <= slots["shadow_epilogue"], (ev, it, slots)
    # the counters exactly, where the oracle was run: the sampled tiles alone (tiles are independent), counted, against the tallies of the same oracle call
    gpu_ctx.set_tile_subset(subset)
    gpu_ctx.set_profiling(False, True)
    try:
        gpu_ctx.render_host(p, tabs)
        sub = (list(gpu_ctx.eval_counts().values()), list(gpu_ctx.sdf_iterations().values()), list(gpu_ctx.elision_counts().values()), gpu_ctx.stats()["shadow_jobs"])
    finally:
        gpu_ctx.set_profiling(False, False)
        gpu_ctx.set_tile_subset(None)
    print(name, "sampled tiles: counted", sub, "oracle", ctr.device_counts())
    assert sub == ctr.device_counts()
    assert all(0 < sub[0][k] < v for k, v in enumerate(ev.values()))
    for env in FILM_ENVS[name]:
        with tuned_ctx(monkeypatch, env) as ctx:
            ctx.upload_world(wd)
            out = ctx.render_host(p, tabs)
            st = ctx.stats()
            k = M.march_limits(ctx)[3] if name == "bulbm" else 1
        _shadow_reached_steady_state(st, k, endgame, FILM_BOUNCES, f"{name} {env}")
        assert film_equal_bits(out, film), env
