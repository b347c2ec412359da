"""The ray-generation stage (k_pack_tables, k_batch_setup, k_raygen through their product launchers) through rayn_hip_probe_raygen against the CPU oracle's
export of the ray-gen loop its films are made of (oracle_py.raygen_tile), word for word, on the cases of tests/raygen_cases.py: clamped and non-square
tiles, tile lists whose pool order is not their list order, 1280 tiles in one launch, 256 / 320 / 1024 groups in one tile, 16384 spp, tiles at the far
ends of long films; caller-built tables whose sums with the scramble are exactly 1, negative, -0, subnormal, at least 2^23, infinite or NaN; the filter's
inverse CDF at u = 0.5, at both ends and at exact integer indices; static and animated cameras of every kind under offset, zero and negative time ranges;
the thin lens's own sample set; the packed sample records at every volume_marches the ABI takes and depth 120.  Besides the rays: the pool's initial
state, the padding rule (a padding slot is marked empty and nothing else is written), term_key untouched, nothing written at or beyond n_pool, the group
tables and the control words.  Both kernel sets (mul_add policy 0 and 1) are compared with the oracle built the same way."""
import ctypes as C

import numpy as np
import pytest

import raygen_cases as RC
import raygen_np as RN

pytestmark = pytest.mark.gpu

INVALID_ARG = -1
S = RN.SENTINEL


def run(ctx, name, fma):
    c = RC.get(name)
    ctx.upload_world(c["wd"])
    ctx.set_fma_policy(fma)
    try:
        _, got = ctx.probe_raygen(c["p"], c["tabs"], c["tiles"], c["n_pool"], surplus=RN.SURPLUS, sentinel=S)
    finally:
        ctx.set_fma_policy(0)
    want = RN.reference(c, rays=list(RC.oracle_rays(name, fma)))
    d = RN.differing(got, want)
    m = RC.measure(c)
    print(f"{name} policy {fma}: n_pool {c['n_pool']} tiles {m['tiles']} groups per tile {m['groups_per_tile']} padding share {m['padding_share']} "
          f"u == 0.5 {m['u_half']} index 510 {m['index_510']} index 0 {m['index_0']} t == 0 {m['t_zero']} NaN sums {m['nan_sums']} inf sums {m['inf_sums']} "
          f"ctl {got['ctl']} differing words {d}")
    return c, got, want, d


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("name", RC.NAMES)
def test_case(gpu_ctx, oracle, name, fma):
    c, got, want, d = run(gpu_ctx, name, fma)
    seen = {k: v for k, v in d.items() if c["only"] is None or k in c["only"]}
    assert not any(seen.values()), (name, fma, seen)
    n_pool = c["n_pool"]
    u32 = lambda k: RN.words(got[k])
    # the control words: the queue is the whole pool, padding included (kernels.h: q_valid counts the padding slots after ray generation)
    assert got["ctl"]["q_groups"] == n_pool // 64 and got["ctl"]["head_extend"] == 0 and got["ctl"]["q_valid"] == n_pool
    assert all(got["ctl"][k] == S for k in RN.CTL if k not in ("q_groups", "q_valid", "head_extend"))
    # a padding slot: marked empty, nothing else written
    pad = want["padding"]
    for k in ("geo0", "geo1", "col0", "col1"):
        assert (u32(k)[pad] == S).all(), k
    assert (got["q"][pad] == RN.INVALID).all() and (got["term_info"][pad] == RN.TERM_NONE).all() and pad.sum() == n_pool - want["path"].sum()
    assert (u32("aov")[pad] == np.array([0, 0, 0, RN.OBJ_NONE], np.uint32)).all()
    # term_key is not written by this stage; nothing is written at or beyond n_pool, in any buffer
    assert (got["term_key"] == S).all()
    for k in RN.PLANES:
        assert (u32(k)[n_pool:] == S).all(), k
    assert (got["q"][n_pool:] == S).all() and (got["term_info"][n_pool:] == S & 0xFF).all() and (got["pgrp_tile"][n_pool // 64:] == S).all()
    nt = len(c["tiles"])
    assert (got["tgb"][nt:] == S).all() and (got["tgc"][nt:] == S).all() and (RN.words(got["records_surplus"]) == S).all()


# ---- what the probe refuses ------------------------------------------------------------------------------------------------------------------------

def _raw(ctx, c, **ov):
    """the C entry with every argument replaceable by name -> (rc, outputs)"""
    from rayn_amd._lib import lib
    n_pool, surplus = ov.get("n_pool", c["n_pool"]), ov.get("surplus", RN.SURPLUS)
    NP, nt = c["n_pool"] + 4096, len(c["tiles"])  # generous: no argument of a refused call sizes them
    p = c["p"]
    stride = 8 + 12 + 8 * 4
    out = {k: np.zeros((NP, 4), np.float32) for k in ("out_geo0", "out_geo1", "out_col0", "out_col1", "out_aov")}
    out.update(out_term_key=np.zeros(NP, np.uint32), out_term_info=np.zeros(NP, np.uint8), out_q=np.zeros(NP, np.uint32), out_pgrp=np.zeros(NP // 64, np.uint32),
               out_tgb=np.zeros(nt + 2, np.uint32), out_tgc=np.zeros(nt + 2, np.uint32), out_ctl=np.zeros(8, np.uint32),
               out_records=np.zeros((p.max_bounces + 1) * 4 * p.samples * stride + 64, np.float32))
    s1, s2, scr, fis = c["tabs"]
    a = dict(p=p, s1=s1, n_s1=s1.size, s2=s2, n_s2=s2.size, scr=scr, n_scr=scr.size, fis=fis, n_tiles=nt, tiles=c["tiles"], n_pool=n_pool, surplus=surplus, sentinel=S, **out)
    a.update(ov)
    types = {np.dtype(np.float32): C.c_float, np.dtype(np.uint32): C.c_uint32, np.dtype(np.uint8): C.c_uint8}
    ptr = lambda x: None if x is None else np.ascontiguousarray(x).ctypes.data_as(C.POINTER(types[np.asarray(x).dtype]))
    scalars = ("n_s1", "n_s2", "n_scr", "n_tiles", "n_pool", "surplus", "sentinel")
    order = ("s1", "n_s1", "s2", "n_s2", "scr", "n_scr", "fis", "n_tiles", "tiles", "n_pool", "surplus", "sentinel", "out_geo0", "out_geo1", "out_col0", "out_col1",
             "out_aov", "out_term_key", "out_term_info", "out_q", "out_pgrp", "out_tgb", "out_tgc", "out_ctl", "out_records")
    keep = [np.ascontiguousarray(a[k]) if k not in scalars and a[k] is not None else a[k] for k in order]
    args = [C.byref(a["p"])] + [int(v) if k in scalars else ptr(v) for k, v in zip(order, keep)]
    rc = lib().rayn_hip_probe_raygen(ctx.h, *args)
    return rc, {k: v for k, v in zip(order, keep) if k.startswith("out_") and v is not None}


def _p(c, **kw):
    p = type(c["p"]).from_buffer_copy(c["p"])
    for k, v in kw.items():
        setattr(p, k, v)
    return {"p": p}


def _tile(c, t, col, value):
    tiles = c["tiles"].copy()
    tiles[t, col] = value
    return {"tiles": tiles}


def _refusals():
    """name -> function(case) -> the overrides of one refused call.  The case is `permuted`: 8 tiles in a 30 x 17 film at spp 4"""
    def swapped_bases(c):  # two unequal tiles exchange their pool_base: the longer one now runs into its neighbour (overlap), the shorter leaves a gap
        tiles, by = c["tiles"].copy(), np.argsort(c["tiles"][:, 4])
        a, b = [int(k) for k in by[1:3]]  # neighbours in the pool, of 1 and 5 groups
        assert (tiles[a, 5] + 63) // 64 != (tiles[b, 5] + 63) // 64
        tiles[a, 4], tiles[b, 4] = c["tiles"][b, 4], c["tiles"][a, 4]
        return {"tiles": tiles}

    def gap(c):  # a tile from the middle of the pool dropped: its groups belong to nobody
        by = np.argsort(c["tiles"][:, 4])
        keep = np.delete(by, 3)
        return {"tiles": c["tiles"][np.sort(keep)], "n_tiles": len(keep)}

    def beyond(c):  # the pool one group short of the last tile's segment
        return {"n_pool": c["n_pool"] - 64}

    return {
        "null_table": lambda c: {"s2": None},
        "null_scramble": lambda c: {"scr": None},
        "null_tiles": lambda c: {"tiles": None},
        "null_output": lambda c: {"out_aov": None},
        "null_records": lambda c: {"out_records": None},
        "volume_marches_0": lambda c: _p(c, volume_marches=0),
        "volume_marches_1": lambda c: _p(c, volume_marches=1),
        "volume_marches_5": lambda c: _p(c, volume_marches=5),
        "max_bounces_121": lambda c: _p(c, max_bounces=121),
        "samples_0": lambda c: _p(c, samples=0),
        "samples_4097": lambda c: _p(c, samples=4097),
        "tables_of_another_depth": lambda c: _p(c, max_bounces=c["p"].max_bounces + 1),
        "tables_of_another_spp": lambda c: _p(c, samples=c["p"].samples + 1),
        "samples_1d_short": lambda c: {"n_s1": c["tabs"][0].size - 1},
        "samples_2d_long": lambda c: {"n_s2": c["tabs"][1].size + 2},
        "scramble_of_another_film": lambda c: {"n_scr": c["tabs"][2].size - c["p"].width},
        "film_wider_than_scramble": lambda c: _p(c, width=c["p"].width + 1),
        "n_tiles_0": lambda c: {"n_tiles": 0},
        "n_pool_0": lambda c: {"n_pool": 0},
        "n_pool_not_64": lambda c: {"n_pool": c["n_pool"] + 32},
        "n_pool_beyond_the_tiles": lambda c: {"n_pool": c["n_pool"] + 64},
        "n_pool_short": beyond,
        "surplus_64": lambda c: {"surplus": 64},
        "surplus_not_64": lambda c: {"surplus": 160},
        "sentinel_invalid": lambda c: {"sentinel": 0xFFFFFFFF},
        "sentinel_is_a_slot": lambda c: {"sentinel": c["n_pool"] - 1},
        "sentinel_low_byte_ff": lambda c: {"sentinel": 0xC0FFEEFF},
        "tile_without_pixels": lambda c: _tile(c, 2, 2, 0),
        "tile_of_1025_pixels": lambda c: {"tiles": np.array([[0, 0, 41, 25, 0, 41 * 25 * 4, 0, 0]], np.uint32), "n_tiles": 1, "n_pool": 4160, **_p(c, width=41, height=25),
                                          "scr": np.zeros(41 * 25, np.float32), "n_scr": 41 * 25},
        "tile_beyond_the_right_edge": lambda c: _tile(c, 7, 0, c["p"].width - int(c["tiles"][7, 2]) + 1),
        "tile_beyond_the_top_edge": lambda c: _tile(c, 4, 1, c["p"].height - int(c["tiles"][4, 3]) + 1),
        "tile_x0_wraps": lambda c: _tile(c, 0, 0, 0xFFFFFFFF),
        "n_paths_one_more": lambda c: _tile(c, 3, 5, int(c["tiles"][3, 5]) + 1),
        "n_paths_of_another_spp": lambda c: _tile(c, 3, 5, int(c["tiles"][3, 5]) * 2),
        "pool_base_not_64": lambda c: _tile(c, 1, 4, int(c["tiles"][1, 4]) + 32),
        "segments_overlap_and_gap": swapped_bases,
        "segments_leave_a_gap": gap,
        "same_tile_twice": lambda c: {"tiles": np.concatenate([c["tiles"], c["tiles"][:1]]), "n_tiles": len(c["tiles"]) + 1},
    }


@pytest.mark.parametrize("what", list(_refusals()))
def test_probe_refuses(gpu_ctx, oracle, what):
    """what the kernels could not index (rayn_hip.h), one violated precondition at a time on an otherwise valid case: the call is refused, its outputs stay
    untouched, and the same context then runs the case"""
    c = RC.get("permuted")
    gpu_ctx.upload_world(c["wd"])
    rc, out = _raw(gpu_ctx, c, **_refusals()[what](c))
    assert rc == INVALID_ARG, (what, rc, gpu_ctx.last_error())
    assert all((v == 0).all() for v in out.values()), "a refused call wrote its outputs"
    rc, out = _raw(gpu_ctx, c)
    assert rc == 0, gpu_ctx.last_error()
    want = RN.reference(c, rays=list(RC.oracle_rays("permuted", 0)))
    NP = c["n_pool"] + RN.SURPLUS
    assert np.array_equal(out["out_q"][:NP], want["q"]) and np.array_equal(out["out_pgrp"][:NP // 64], want["pgrp_tile"])
    assert np.array_equal(RN.words(out["out_geo0"])[:NP][want["path"]], want["geo0"][want["path"]])
