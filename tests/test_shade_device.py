"""The shade stage (launch_shade: k_shade_setup, k_shadow_list, the scene's shadow-march kernel, k_shade_finish) through rayn_hip_probe_shade against the CPU
oracle's Integrator::integrate on the same packets (oracle_py.shade_packets), bit for bit, on the cases of tests/shade_cases.py: every depth of one recorded
tile of ten scenes (each shadow-march kernel, the LDS memo on and off, VM 2 and 4, no lights, packet times from lane 0), and recorded depths with one named
change - exact-zero, NaN, infinite and denormal throughputs, the elision bounds from both sides, negative hit distances, shading points inside lights, lights
on the tangent planes of a sphere (dot(normal, wi) exactly +0 and -0), underflowing transmittance, the roulette at depths 2 / 3 / max_bounces, waves that straddle bins - in a pool whose order is unrelated to
the slot order, with a plane stride that is not the slot count.  A mismatch names the case, the slot, the lane of the packet, the output word and both bit
patterns.  Both kernel sets (mul_add policy 0 and 1) are compared with the oracle built the same way."""
import ctypes as C

import numpy as np
import pytest

import shade_cases as SC

pytestmark = pytest.mark.gpu

INVALID_ARG = -1
NEE_EXTRA = 192  # the plane stride of the NEE records is deliberately not the slot count


def run(ctx, name, case, fma, max_extra=0, nee_extra=NEE_EXTRA, tile_to=None):
    sc = SC.scene(case["scene"])
    pool = SC.to_pool(case, tile_to=tile_to)
    want = SC.expect(case, bool(fma))
    n = pool["n_slots"]
    ctx.upload_world(sc["wd"])
    ctx.set_fma_policy(fma)
    try:
        _, got = ctx.probe_shade(sc["p"], sc["tabs"], case["depth"], pool["ref"], pool["geo0"], pool["geo1"], pool["col0"], pool["col1"],
                                 max_slots=n + max_extra, nee_cap=n + nee_extra, sentinel=SC.SENTINEL)
    finally:
        ctx.set_fma_policy(0)
    total, msgs = SC.compare(name, case, pool, got, want)
    print(f"{name} policy {fma}: n_slots {n} max_slots {n + max_extra} nee_cap {n + nee_extra} valid lanes {len(pool['P'])} shadow kernel {got['shadow_kernel']} "
          f"job_count {got['job_count']} differing words {total}")
    assert total == 0, msgs
    # the parked segments are the oracle's count exactly (its restatement of the parking rule, per lane: tests/test_counters.py)
    assert got["shadow_jobs"] == got["job_count"] == SC.expect_tally(case, bool(fma), tile_to)["shadow_jobs"] <= sc["ns"] * n
    return got


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("name", SC.RECORDED_SCENES)
def test_recorded_tile_every_depth(gpu_ctx, oracle, name, fma):
    """the film's own states, shown to the shade stage alone"""
    jobs = 0
    for d in SC.depths(name):
        got = run(gpu_ctx, f"{name} depth {d}", SC.recorded(name, d, bool(fma)), fma)
        assert got["shadow_kernel"] == SC.SHADOW_KERNEL[name]
        jobs += got["job_count"]
        if d == 0 and name in SC.SDF_SCENES:
            assert got["job_count"] > 0
    if name in ("spheres_only", "no_lights_vol"):
        assert jobs == 0


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("name", SC.MUTATED)
def test_mutated_case(gpu_ctx, oracle, name, fma):
    got = run(gpu_ctx, name, SC.build(name), fma)
    if name in ("zero_thr_all", "zero_thr_bound_at", "zero_thr_pdf_above"):   # every NEE sample lies inside the elision's bounds: nothing is parked, and the radiance still matched
        assert got["job_count"] == 0
    if name in ("zero_thr", "zero_thr_huge_lights", "zero_thr_bound_above", "zero_thr_pdf_below"):  # the untouched packets / |x| above 2^60 / |pdf| below 2^-60: tested and marched as ever
        assert got["job_count"] > 0


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("n_slots,max_extra,nee_extra", SC.SHAPES)
def test_shapes(gpu_ctx, oracle, n_slots, max_extra, nee_extra, fma):
    """one recorded depth cut (64, 256, 320) or repeated (1024) to a slot count, with the grids and the plane stride at and above it"""
    case = SC.fit(SC.recorded("ship", 0), n_slots)
    run(gpu_ctx, f"shape {n_slots}+{max_extra}+{nee_extra}", case, fma, max_extra, nee_extra)


@pytest.mark.parametrize("fma", [0, 1])
def test_second_trip(gpu_ctx, oracle, fma):
    """k_shadow_list and k_shade_finish in the second trip of their grid-stride loops: the unique packets of one recorded depth (VM 4: ns = 20) repeated to the
    smallest slot count whose ns * n_slots exceeds what one trip of the full grid scans, both sizes from the library"""
    blocks, ids, setup_threads = gpu_ctx.probe_shade_limits()
    base = SC.second_trip_base()
    ns = SC.scene(base["scene"])["ns"]
    n = SC.second_trip_slots(blocks, ids, ns)
    assert ns * n > blocks * ids and n > blocks * 256 and n > setup_threads
    per_slot = 12 * 4 + 2 * (ns - 3) * 4 + ns * 4 + ns + 8 + 4 + 4 + 12 + 1 + ns * 4 + ns * 24  # the NEE records and the job list (kernels.h: Nee)
    print(f"second_trip: stream_blocks {blocks} ids per block trip {ids} ns {ns} -> n_slots {n}, about {(per_slot + 4 + 7 * 16) * n / 2**30:.2f} GiB of device memory")
    got = run(gpu_ctx, "second_trip", base, fma, tile_to=n)
    assert got["job_count"] > 0


# ---- what the probe refuses ------------------------------------------------------------------------------------------------------------------------

def _raw(ctx, sc, depth_, pool, **ov):
    """the C entry with every argument replaceable by name -> (rc, outputs)"""
    from rayn_amd._lib import lib
    n_pool = pool["geo0"].shape[0]
    out = {k: np.zeros((n_pool, 4), np.float32) for k in ("out_geo0", "out_geo1", "out_col0", "out_col1", "out_aov")}
    out.update(out_term_key=np.zeros(n_pool, np.uint32), out_term_info=np.zeros(n_pool, np.uint8), out_alive=np.zeros(max(pool["n_slots"] // 64, 1), np.uint64),
               out_cnt=np.zeros(max(pool["n_slots"] // 64, 1), np.uint8), out_jobs=np.zeros(3, np.uint64))
    s1, s2, scr, fis = sc["tabs"]
    a = dict(p=sc["p"], s1=s1, s2=s2, scr=scr, fis=fis, depth=depth_, n_slots=pool["n_slots"], max_slots=pool["n_slots"], nee_cap=pool["n_slots"] + NEE_EXTRA,
             ref=pool["ref"], n_pool=n_pool, geo0=pool["geo0"], geo1=pool["geo1"], col0=pool["col0"], col1=pool["col1"], sentinel=SC.SENTINEL, **out)
    a.update(ov)
    types = {np.dtype(np.float32): C.c_float, np.dtype(np.uint32): C.c_uint32, np.dtype(np.uint8): C.c_uint8, np.dtype(np.uint64): C.c_uint64}
    ptr = lambda x: None if x is None else np.ascontiguousarray(x).ctypes.data_as(C.POINTER(types[np.asarray(x).dtype]))
    args = [C.byref(a["p"])] + [ptr(a[k]) if k not in ("depth", "n_slots", "max_slots", "nee_cap", "n_pool", "sentinel") else int(a[k])
                                for k in ("s1", "s2", "scr", "fis", "depth", "n_slots", "max_slots", "nee_cap", "ref", "n_pool", "geo0", "geo1", "col0", "col1", "sentinel",
                                          "out_geo0", "out_geo1", "out_col0", "out_col1", "out_aov", "out_term_key", "out_term_info", "out_alive", "out_cnt", "out_jobs")]
    rc = lib().rayn_hip_probe_shade(ctx.h, *args)
    return rc, {k: v for k, v in a.items() if k.startswith("out_") and v is not None}


def _with(arr, index, value, view=None):
    a = arr.copy()
    (a.view(view) if view else a)[index] = value
    return a


def _refusals():
    """name -> function(case pool, scene) -> the overrides of one refused call"""
    def first_packet_with(pool, n_valid):
        v = (pool["ref"] != SC.INVALID).reshape(-1, 4)
        return int(np.flatnonzero(v.sum(1) >= n_valid)[0])

    def two_objects(pool, sc):
        k = first_packet_with(pool, 2)
        P = pool["ref"][4 * k + 1]
        word = pool["geo1"].view(np.uint32)[P, 3]
        return {"geo1": _with(pool["geo1"], (P, 3), (word & ~np.uint32(0xFF)) | ((word & 0xFF) ^ 1), np.uint32)}

    def lane0_invalid(pool, sc):
        k = first_packet_with(pool, 2)
        return {"ref": _with(pool["ref"], 4 * k, SC.INVALID)}

    def word_of_first(pool, key, col, value):
        P = pool["ref"][0]
        return {key: _with(pool[key], (P, col), value, np.uint32)}

    return {
        "null_ref": lambda pool, sc: {"ref": None},
        "null_record": lambda pool, sc: {"geo1": None},
        "null_table": lambda pool, sc: {"s2": None},
        "null_output": lambda pool, sc: {"out_aov": None},
        "n_slots_0": lambda pool, sc: {"n_slots": 0},
        "n_slots_not_64": lambda pool, sc: {"n_slots": pool["n_slots"] - 32},
        "max_slots_below": lambda pool, sc: {"max_slots": pool["n_slots"] - 64},
        "nee_cap_below": lambda pool, sc: {"nee_cap": pool["n_slots"] - 1},
        "ids_beyond_32_bits": lambda pool, sc: {"nee_cap": -(-(1 << 32) // sc["ns"])},
        "ref_beyond_pool": lambda pool, sc: {"ref": _with(pool["ref"], 5, pool["geo0"].shape[0])},
        "ref_twice": lambda pool, sc: {"ref": _with(pool["ref"], 5, pool["ref"][4])},
        "lane0_invalid": lane0_invalid,
        "two_objects_in_a_packet": two_objects,
        "object_beyond_hitables": lambda pool, sc: word_of_first(pool, "geo1", 3, sc["wd"].n_hitables),
        "sample_beyond_spp": lambda pool, sc: word_of_first(pool, "geo1", 3, (4 * sc["p"].samples) << 8),
        "pixel_beyond_film": lambda pool, sc: word_of_first(pool, "col1", 2, sc["p"].width * sc["p"].height),
        "depth_above_max_bounces": lambda pool, sc: {"depth": sc["p"].max_bounces + 1},
    }


@pytest.mark.parametrize("what", list(_refusals()))
def test_probe_refuses(gpu_ctx, oracle, what):
    """what the kernels could not index, or what their stated preconditions exclude (rayn_hip.h), one at a time on an otherwise valid case"""
    case = SC.recorded("ship", 1)
    sc = SC.scene("ship")
    pool = SC.to_pool(case)
    assert (pool["ref"][:8] != SC.INVALID).all()
    gpu_ctx.upload_world(sc["wd"])
    rc, out = _raw(gpu_ctx, sc, 1, pool, **_refusals()[what](pool, sc))
    assert rc == INVALID_ARG, (what, rc, gpu_ctx.last_error())
    assert all((v == 0).all() for v in out.values()), "a refused call wrote its outputs"
    rc, _ = _raw(gpu_ctx, sc, 1, pool)
    assert rc == 0, gpu_ctx.last_error()
