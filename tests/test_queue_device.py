"""The queue stages of the depth loop (k_group_hist, k_scan_tile, k_tile_prefix, k_bin_scatter, k_compact_scatter) through rayn_hip_probe_queue against
the numpy stable partition of tests/queue_np.py, word for word, on the cases of tests/queue_cases.py: more than 1024 tiles, more than 512 groups in a
tile, second grid-stride trips, the corner populations and the overflow guard - shapes no film of the fast suite reaches.  Both kernel sets
(mul_add policy 0 and 1) hold their own copy of these kernels, so every case runs under both."""
import ctypes as C
import functools

import numpy as np
import pytest

import queue_cases as QC
import queue_np as QN
from common import case as film_case, film_equal_bits

pytestmark = pytest.mark.gpu

SENTINEL = 0xC0FFEE00 | 0x5A  # neither INVALID nor a reference of any case
SMALL = QC.small_cases()
OVERFLOW = QC.overflow_cases()


@functools.lru_cache(maxsize=None)
def _named(name):
    """a case and its numpy statement, computed once and shared by both policies"""
    for c in SMALL + [c for c, _ in OVERFLOW]:
        if c["name"] == name:
            return c, QN.reference(c)
    c = getattr(QC, name)()
    return c, QN.reference(c)


def run_probe(ctx, case, ref):
    from rayn_amd._lib import lib
    n_tiles, n = case["tile_groups"].size, case["q"].size
    backed = lambda a: a if a.size else np.zeros(1, a.dtype)[:0]  # an empty array still hands a valid pointer over
    q, obj, survive = backed(case["q"]), backed(case["obj"]), backed(case["survive"])
    slots = ref["out_slots"]
    got = {"bq": np.zeros(slots, np.uint32), "qn": np.zeros(slots, np.uint32), "tile": np.zeros((n_tiles, 5), np.uint32),
           "cls_cnt": np.zeros((n_tiles, QN.NC), np.uint32), "cls_base": np.zeros((n_tiles, QN.NC), np.uint32), "ctl": np.array(case["ctl0"], np.uint64)}
    up, bp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)))
    rc = lib().rayn_hip_probe_queue(ctx.h, case["nclass"], n_tiles, up(case["tile_groups"]), up(q), bp(obj), bp(survive), case["n_refs"], ref["cap_bin"],
                                    ref["cap_repack"], case["bounds"] * n, case["bounds"] * ref["need_b"] * 64, SENTINEL, slots, up(got["bq"]), up(got["qn"]),
                                    up(got["tile"]), up(got["cls_cnt"]), up(got["cls_base"]), got["ctl"].ctypes.data_as(C.POINTER(C.c_uint64)))
    assert rc == 0, ctx.last_error()
    return got


def check_queue(got, want, what):
    """the stage's slots [0, groups * 64) equal the statement (so each is written, with a reference or INVALID); every slot beyond keeps the sentinel"""
    assert np.array_equal(got[:want.size], want), (what, np.flatnonzero(got[:want.size] != want)[:8].tolist())
    assert (got[want.size:] == SENTINEL).all(), (what, "stray write", (want.size + np.flatnonzero(got[want.size:] != SENTINEL)[:8]).tolist())
    assert not (want == SENTINEL).any()


def check(ctx, name, fma):
    case, ref = _named(name)
    ctx.set_fma_policy(fma)
    try:
        got = run_probe(ctx, case, ref)
    finally:
        ctx.set_fma_policy(0)
    print(name, fma, dict(zip(QN.CTL, got["ctl"].tolist())))
    assert dict(zip(QN.CTL, got["ctl"].tolist())) == dict(zip(QN.CTL, ref["ctl"].tolist()))  # sizes, flag, and counters advanced by exactly the statement's sums
    check_queue(got["bq"], ref["bq"], "binned queue")
    check_queue(got["qn"], ref["qn"], "next queue")
    # the bin stage's per-tile results are written before the guard decides; the repack's only mean something when both stages ran
    for k in ("cls_cnt", "cls_base"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["tile"][:, [0, 1, 4]], ref["tile"][:, [0, 1, 4]])
    if ref["ok_b"]:
        assert np.array_equal(got["tile"][:, 2:4], ref["tile"][:, 2:4])
    return got, ref


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("name", [c["name"] for c in SMALL])
def test_queue_stages_match_the_stable_partition(gpu_ctx, name, fma):
    check(gpu_ctx, name, fma)


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("name", ["big5m", "big17m"])
def test_queue_stages_second_grid_stride_trip(gpu_ctx, name, fma):
    """big5m: k_bin_scatter and k_compact_scatter go round their grid-stride loop twice; big17m: k_group_hist too"""
    check(gpu_ctx, name, fma)


@pytest.mark.parametrize("fma", [0, 1])
def test_overflow_guard(gpu_ctx, fma):
    """A stage whose output is one group larger than its queue sets its bit, reports size 0 and writes nothing - and neither does any later stage; a
    queue of exactly the needed size is filled without a flag; the next call on the same context is unaffected."""
    for case, stage in OVERFLOW:
        got, ref = check(gpu_ctx, case["name"], fma)
        ctl = dict(zip(QN.CTL, got["ctl"].tolist()))
        if stage is None:
            assert ctl["overflow"] == 0 and ctl["b_groups"] == ref["need_b"] == ref["cap_bin"] and ctl["q_groups"] == ref["need_q"] > 0
            assert (got["bq"][:ref["need_b"] * 64] != SENTINEL).all() and (got["qn"][:ref["need_q"] * 64] != SENTINEL).all()
            continue
        assert ctl["overflow"] == 1 << stage
        assert ctl["q_groups"] == 0 and ctl["q_valid"] == 0 and (got["qn"] == SENTINEL).all()
        if stage == 0:
            assert ctl["b_groups"] == 0 and ctl["b_valid"] == 0 and (got["bq"] == SENTINEL).all()
        else:
            assert ctl["b_groups"] == ref["need_b"] and (got["bq"][:ref["need_b"] * 64] != SENTINEL).all()
        check(gpu_ctx, "tiles1025", fma)  # a normal case right after the refused one


def test_probe_rejects_what_the_kernels_could_not_index(gpu_ctx):
    case, ref = _named("residues")
    for change in ({"nclass": 0}, {"nclass": 17}, {"nclass": 3}, {"n_refs": 100}):
        bad = dict(case, **change)
        with pytest.raises(AssertionError):
            run_probe(gpu_ctx, bad, ref)
    short = dict(ref, out_slots=ref["out_slots"] - 5 * 64)
    with pytest.raises(AssertionError):
        run_probe(gpu_ctx, case, short)
    check(gpu_ctx, "residues", 0)


def test_film_with_more_than_1024_tiles_in_one_batch(gpu_ctx, oracle):
    """s1 at 80x64 in 2x2 tiles: 1280 tiles and 20 480 paths in ONE batch, so k_batch_setup, k_raygen, the queue stages and the resolve all see a tile
    count beyond one trip of k_tile_prefix - bit-identical to the oracle."""
    wd, p = film_case("s1", 80, 64, 1, 2, tile_size=(2, 2))
    tabs = oracle.build_tables(4 * p.samples, p.max_bounces, p.volume_marches, p.frame, p.width, p.height)
    ref, ctr = oracle.render(wd, p, tabs)
    gpu_ctx.upload_world(wd)
    gpu_ctx.set_workers(1)  # one worker: the whole share is one batch
    try:
        out = gpu_ctx.render_host(p, tabs)
        st = gpu_ctx.stats()
    finally:
        gpu_ctx.set_workers(2)
    assert st["batches"] == 1 and st["tiles"] == 1280 and st["paths"] == 20480 == ctr.paths
    assert st["segments"] == ctr.segments
    assert film_equal_bits(out, ref)
