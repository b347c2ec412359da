"""The counters of the instrumented (COUNT = true) kernel instantiations - rayn_hip_get_eval_counts, _sdf_iterations, _elision_counts, and rayn_stats.shadow_jobs -
against the CPU oracle's per-lane accounting (oracle/rayn_oracle.cpp; checked on its own by tests/test_counters.py), with == on integers and no tolerance
anywhere.  None of these numbers can reach the film, so the bit-exact film tests say nothing about them; every roofline figure of the project is one of them
times a price.

a. the march kernels one launch at a time through the probes (which run the instrumented instantiation while count_evals is on and report into the context's
   counters): each scene-selected kernel, march budgets 0 / 1 / default, depths 0 and 2, both mul_add policies, the generic kernels forced onto a single-SDF
   scene, the Mandelbulb through k_shadow1, and the five shapes of k_shadow_bulb.  n = 40 021 is not a multiple of 64 (padding entries in the queue) and runs
   the endgame only; the steady state is tests/test_march_steady_device.py's.
c. the shade stage through rayn_hip_probe_shade on the cases of tests/shade_cases.py.
d. whole frames, also in several batches on two workers and on a two-entry context.
The stage slots of k_shadow_bulb (rayn_hip_get_stage_slots) are NOT pinned: they count the executions of the kernel's two stages per wave, which depend on which
wave wins which chunk of the queue.  They stay what they can be: multiples of 64 that bound the orbit steps and the evaluations from above."""
import contextlib

import numpy as np
import pytest

import counter_cases as CC
import march_cases as M
import shade_cases as SC
from common import film_equal_bits

pytestmark = pytest.mark.gpu
N = 40021
SEG_SEED, RAY_SEED = 31, 41
MARCH_SCENES = ("s1", "s0", "bulb", "two_sdfs", "moving_sdf")  # k_extend1 / k_shadow1 on the MandelBox and the sphere SDF, k_shadow_bulb, the generic kernels, an animated origin
ZERO3 = dict.fromkeys(CC.EVAL_KEYS, 0)


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    M.clear()


@contextlib.contextmanager
def policy(ctx, fma):
    ctx.set_fma_policy(fma)
    try:
        yield
    finally:
        ctx.set_fma_policy(0)


@contextlib.contextmanager
def env_ctx(monkeypatch, env):
    """one extra context on cuda:0 under RAYN_HIP_ENV_TUNING=1 with `env`; closed (and the variables removed) on exit"""
    import rayn_amd
    monkeypatch.setenv("RAYN_HIP_ENV_TUNING", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = rayn_amd.Context(0)
    try:
        yield ctx
    finally:
        ctx.close()
        for k in env:
            monkeypatch.delenv(k)
        monkeypatch.delenv("RAYN_HIP_ENV_TUNING")


def _stage_slots_bound(slots, ev, it):
    """what can be said of rayn_hip_get_stage_slots (see the module text)"""
    assert slots["shadow_orbit"] % 64 == 0 and slots["shadow_epilogue"] % 64 == 0
    assert it["shadow"] <= slots["shadow_orbit"] and ev["shadow"] <= slots["shadow_epilogue"], (ev, it, slots)


# ---- a. the march kernels through the probes ---------------------------------------------------------------------------------------------------------------------

def extend_counts(ctx, oracle, name, depth, kw, fma=0):
    wd, p, org, d, rt, robj = M.closest_hit_case(oracle, name, depth, kw, RAY_SEED, N, fma=bool(fma))
    want_ev, want_it = M.closest_hit_counts(name, depth, kw, RAY_SEED, N, fma=bool(fma))
    ctx.upload_world(wd)
    with policy(ctx, fma):
        t, obj = M.probe_extend(ctx, p, depth, org, d)
        (ct, cobj), ev, it, el, slots = M.counted(ctx, M.probe_extend, p, depth, org, d)
    print("extend", name, depth, kw, fma, "evals", ev, "iterations", it, "want", want_ev, want_it)
    assert np.array_equal(cobj, obj) and np.array_equal(ct.view(np.uint32), t.view(np.uint32))   # the counted launch against the uncounted one, bit for bit
    assert np.array_equal(obj, robj) and M.same_t(t, rt).all()                                   # and both against the oracle
    assert ev == dict(ZERO3, extend=want_ev), (ev, want_ev)
    assert it == dict(ZERO3, extend=want_it), (it, want_it)
    assert not any(el.values()) and not any(slots.values())
    return want_ev, want_it


def shadow_counts(ctx, oracle, name, kw, fma=0, bulb_kernel=False):
    wd, p, a, b, ref = M.occluded_case(oracle, name, kw, SEG_SEED, N, fma=bool(fma))
    want_ev, want_it = M.occluded_counts(name, kw, SEG_SEED, N, fma=bool(fma))
    ctx.upload_world(wd)
    with policy(ctx, fma):
        out = M.probe_shadow(ctx, p, a, b)
        got, ev, it, el, slots = M.counted(ctx, M.probe_shadow, p, a, b)
    print("shadow", name, kw, fma, "evals", ev, "iterations", it, "want", want_ev, want_it, "slots", slots)
    assert np.array_equal(got, out) and np.array_equal(out, ref)
    assert ev == dict(ZERO3, shadow=want_ev), (ev, want_ev)
    assert it == dict(ZERO3, shadow=want_it), (it, want_it)
    assert not any(el.values())
    if bulb_kernel:
        _stage_slots_bound(slots, ev, it)
        assert slots["shadow_epilogue"] > 0
    else:
        assert not any(slots.values())  # only k_shadow_bulb has stages
    return want_ev, want_it


def _kw(key, budget):
    return {} if budget is None else {key: budget}


@pytest.mark.parametrize("fma", [0, 1], ids=["unfused", "fused"])  # each kernel set against the oracle built with the same mul_add policy
@pytest.mark.parametrize("budget", [0, 1, None])
@pytest.mark.parametrize("depth", [0, 2])
@pytest.mark.parametrize("name", MARCH_SCENES)
def test_extend_counts(gpu_ctx, oracle, name, depth, budget, fma):
    ev, it = extend_counts(gpu_ctx, oracle, name, depth, _kw("max_marches", budget), fma=fma)
    wd = M.probe_world(name)[0]
    if budget == 0:
        assert ev == N * CC.n_sdfs(wd)  # anchor: one evaluation per valid ray and TracedSDF - and none for the 43 padding entries
    if name == "bulb" and budget is None:
        assert ev < it < 8 * ev  # early exits of the orbit at work


@pytest.mark.parametrize("fma", [0, 1], ids=["unfused", "fused"])
@pytest.mark.parametrize("budget", [0, 1, 5, None])
@pytest.mark.parametrize("name", MARCH_SCENES)
def test_shadow_counts(gpu_ctx, oracle, name, budget, fma):
    ev, _ = shadow_counts(gpu_ctx, oracle, name, _kw("max_vis_marches", budget), fma=fma, bulb_kernel=name == "bulb")
    if budget == 0 and name != "two_sdfs":
        assert ev == N


def test_generic_kernels_on_a_single_sdf_scene(oracle, monkeypatch):
    """RAYN_HIP_FAST_PATH=0: k_extend<true> / k_shadow<true> where the default context runs k_extend1 / k_shadow1 - the same counts"""
    with env_ctx(monkeypatch, {"RAYN_HIP_FAST_PATH": "0"}) as ctx:
        for name in ("s1", "bulb"):
            extend_counts(ctx, oracle, name, 0, {})
            extend_counts(ctx, oracle, name, 2, {"max_marches": 1})
            shadow_counts(ctx, oracle, name, {})
            shadow_counts(ctx, oracle, name, {"max_vis_marches": 5})


def test_mandelbulb_through_k_shadow1(oracle, monkeypatch):
    with env_ctx(monkeypatch, {"RAYN_HIP_BULB_PATH": "0"}) as ctx:
        for budget in (0, 1, 5, None):
            shadow_counts(ctx, oracle, "bulb", _kw("max_vis_marches", budget))


# the five shapes of test_bulb_march_kernel_variants_are_invisible: K = 2 / 3 / 4 rays per lane, one or two orbit steps per trip, ORBIT_MIN 0 and 63 (every orbit
# drained in its round / almost every orbit carried into the next: the carry-over extremes)
BULB_ENVS = [{"RAYN_HIP_BULB_RAYS": "2", "RAYN_HIP_BULB_STEPS": "2"}, {"RAYN_HIP_BULB_RAYS": "4", "RAYN_HIP_BULB_ORBIT_MIN": "0", "RAYN_HIP_BULB_STEPS": "1"},
             {"RAYN_HIP_BULB_RAYS": "3", "RAYN_HIP_BULB_ORBIT_MIN": "63", "RAYN_HIP_BULB_PREFETCH": "1", "RAYN_HIP_BULB_STEPS": "1"},
             {"RAYN_HIP_BULB_RAYS": "2", "RAYN_HIP_BULB_STEPS": "1"}, {"RAYN_HIP_BULB_RAYS": "4", "RAYN_HIP_BULB_STEPS": "2", "RAYN_HIP_BULB_PREFETCH": "200"}]


@pytest.mark.parametrize("env", BULB_ENVS, ids=lambda env: ",".join(f"{k[9:]}={v}" for k, v in env.items()))
def test_shadow_bulb_shapes(oracle, monkeypatch, env):
    with env_ctx(monkeypatch, env) as ctx:
        assert M.march_limits(ctx)[3] == int(env["RAYN_HIP_BULB_RAYS"])
        for budget in (1, 5, None):
            shadow_counts(ctx, oracle, "bulb", _kw("max_vis_marches", budget), bulb_kernel=True)


# ---- c. the shade stage ------------------------------------------------------------------------------------------------------------------------------------------

NEE_EXTRA = 192
OUT_WORDS = ("geo0", "geo1", "col0", "col1", "aov", "term_key", "term_info", "alive_mask", "bgrp_cnt")


def shade_counts(ctx, name, case, fma, tile_to=None):
    """the case through the product instantiations and through the instrumented ones: the same outputs, word for word, and every counter equal to the tally of
    the oracle's integrate on the same packets.  tile_to: the packets repeated to that many slots (slot j = lane j % 4 of packet (j // 4) % n)."""
    sc = SC.scene(case["scene"])
    pool = SC.to_pool(case, tile_to=tile_to)
    n = pool["n_slots"]
    want = SC.expect_tally(case, bool(fma), tile_to)
    args = (sc["p"], sc["tabs"], case["depth"], pool["ref"], pool["geo0"], pool["geo1"], pool["col0"], pool["col1"])
    kw = dict(max_slots=n, nee_cap=n + NEE_EXTRA, sentinel=SC.SENTINEL)
    ctx.upload_world(sc["wd"])
    with policy(ctx, fma):
        _, plain = ctx.probe_shade(*args, **kw)
        (_, got), ev, it, el, slots = M.counted(ctx, lambda c: c.probe_shade(*args, **kw))
    print(f"{name} policy {fma}: n_slots {n} job_count {got['job_count']} evals {ev} iterations {it} elision {el} want {want}")
    for k in OUT_WORDS:
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(plain[k]).view(np.uint8)), (name, k)
    assert got["shadow_kernel"] == plain["shadow_kernel"]
    assert plain["job_count"] == plain["shadow_jobs"] == got["job_count"] == got["shadow_jobs"] == want["shadow_jobs"], (plain["job_count"], got["job_count"], want)
    assert ev == {"extend": 0, "shade_setup": want["evals_shade_setup"], "shadow": want["evals_shadow"]}, (ev, want)
    assert it == {"extend": 0, "shade_setup": want["iters_shade_setup"], "shadow": want["iters_shadow"]}, (it, want)
    assert el == {k: want[k] for k in CC.ELISION_KEYS}, (el, want)
    if got["shadow_kernel"] == "k_shadow_bulb" and got["job_count"]:
        _stage_slots_bound(slots, ev, it)
    else:
        assert not any(slots.values())
    return want


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("name", SC.RECORDED_SCENES)
def test_shade_recorded_depths(gpu_ctx, oracle, name, fma):
    total = np.zeros(13, np.int64)
    for d in SC.depths(name):
        total += np.array(list(shade_counts(gpu_ctx, f"{name} depth {d}", SC.recorded(name, d, bool(fma)), fma).values()), np.int64)
    t = dict(zip(oracle.TALLY_KEYS, total.tolist()))
    if name in SC.SDF_SCENES:
        assert t["shadow_jobs"] > 0 and t["evals_shade_setup"] > 0 and t["evals_shadow"] >= t["shadow_jobs"]
    else:
        assert t["shadow_jobs"] == 0 and t["evals_shadow"] == 0


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("name", SC.MUTATED)
def test_shade_mutated(gpu_ctx, oracle, name, fma):
    t = shade_counts(gpu_ctx, name, SC.build(name), fma)
    if name in ("zero_thr_all", "zero_thr_bound_at", "zero_thr_pdf_above"):   # inside the bounds: every sample of every slot elided
        assert t["shadow_jobs"] == 0 and t["zero_throughput_slots"] > 0 and t["samples_out_of_bounds"] == 0
    if name in ("zero_thr_bound_above", "zero_thr_pdf_below", "zero_thr_huge_lights"):  # the other side of each bound
        assert t["samples_out_of_bounds"] > 0 and t["zero_throughput_slots"] > 0
    if name == "zero_thr":
        assert t["elided_shadow_jobs"] > 0 and t["shadow_jobs"] > 0


def test_shade_second_trip(gpu_ctx, oracle):
    """k_shadow_list in the second trip of its grid-stride loop (tests/test_shade_device.py::test_second_trip's size): a job the list dropped or wrote twice
    changes job_count and the shadow evaluations"""
    blocks, ids, _ = gpu_ctx.probe_shade_limits()
    base = SC.second_trip_base()
    n = SC.second_trip_slots(blocks, ids, SC.scene(base["scene"])["ns"])
    t = shade_counts(gpu_ctx, "second_trip", base, 0, tile_to=n)
    assert t["shadow_jobs"] > 0


# ---- d. whole frames ---------------------------------------------------------------------------------------------------------------------------------------------

def _ten(ctx):
    return ctx.eval_counts(), ctx.sdf_iterations(), ctx.elision_counts(), ctx.stats()["shadow_jobs"]


def _counted_frame(ctx, wd, p, tabs):
    ctx.upload_world(wd)
    ctx.set_profiling(False, True)
    try:
        film = ctx.render_host(p, tabs)
        return film, _ten(ctx), ctx.stage_slots(), ctx.stats()
    finally:
        ctx.set_profiling(False, False)


@pytest.mark.parametrize("name,bounces", CC.FRAMES)
def test_frame_counts(gpu_ctx, oracle, name, bounces):
    wd, p, tabs, ref, ctr = CC.frame_reference(oracle, name, bounces)
    want = CC.expected(ctr)
    film, ten, slots, st = _counted_frame(gpu_ctx, wd, p, tabs)
    print(name, bounces, "got", ten, "slots", slots)
    assert film_equal_bits(film, ref) and st["segments"] == ctr.segments and st["batches"] == 1
    assert ten == want, (ten, want)
    if name == "bulbv":
        _stage_slots_bound(slots, ten[0], ten[1])
    else:
        assert not any(slots.values())
    plain = gpu_ctx.render_host(p, tabs)  # the product kernels park the same jobs
    assert film_equal_bits(plain, ref) and gpu_ctx.stats()["shadow_jobs"] == want[3]
    # several batches on two workers: the counters are summed over workers and batches
    gpu_ctx.set_workers(2, 0)
    gpu_ctx.set_batch_paths(4096)
    try:
        film2, ten2, _, st2 = _counted_frame(gpu_ctx, wd, p, tabs)
    finally:
        gpu_ctx.set_workers(2)
        gpu_ctx.set_batch_paths(1 << 28)
    assert st2["batches"] > 1, st2
    assert film_equal_bits(film2, ref) and ten2 == want, (ten2, want)


@pytest.fixture(scope="module")
def two_entry_ctx():
    import rayn_amd
    ctx = rayn_amd.Context([0, 0])
    yield ctx
    ctx.close()


@pytest.mark.parametrize("name,bounces", CC.FRAMES)
def test_frame_counts_two_entries(two_entry_ctx, oracle, name, bounces):
    """Context([0, 0]): the tiles are dealt to two entries on the same GPU and the counters are summed over the peers"""
    wd, p, tabs, ref, ctr = CC.frame_reference(oracle, name, bounces)
    film, ten, _, st = _counted_frame(two_entry_ctx, wd, p, tabs)
    assert film_equal_bits(film, ref) and st["segments"] == ctr.segments
    assert ten == CC.expected(ctr), (ten, CC.expected(ctr))


def test_frame_counts_fused_policy(gpu_ctx, oracle):
    wd, p, tabs, ref, ctr = CC.frame_reference(oracle, "s2", 3, fma=True)
    with policy(gpu_ctx, 1):
        film, ten, _, st = _counted_frame(gpu_ctx, wd, p, tabs)
    assert film_equal_bits(film, ref) and ten == CC.expected(ctr), (ten, CC.expected(ctr))
