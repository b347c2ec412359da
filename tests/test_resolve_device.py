"""The film resolve (k_resolve_reg<1|2|4|8>, k_resolve_blk<128|256|512, 8>, k_resolve_huge) through rayn_hip_probe_resolve against the serial-sum
statement of tests/resolve_np.py, bit for bit in all four planes, on the cases of tests/resolve_cases.py: every launch boundary of launch_resolve from
both sides, depths up to 120, slots and offsets at the ends of their key fields, reversed / sorted / one-pair-out-of-order inputs, dropped samples,
empty pixels, several depth-0 objects, -0.0 / subnormal / infinite / NaN values, 1024-pixel, non-square and packed tiles and a grid wider than the
tiles - keys the renderer never hands the resolve in the films of the suite.  Every word of a pixel no tile owns must still hold the sentinel.
Both kernel sets (mul_add policy 0 and 1) hold their own copy of the resolve, so every case runs under both."""
import ctypes as C
import functools

import numpy as np
import pytest

import resolve_cases as RC
import resolve_np as RN
from common import bits_equal

pytestmark = pytest.mark.gpu

SENTINEL = 0xC0FFEE5A  # as a float -7.997..: no sum of a case, and not a NaN (bits_equal lets any NaN pass for another)


@functools.lru_cache(maxsize=None)
def _statement(name):
    """computed once per case and shared by both policies"""
    return RN.reference(RC.get(name), SENTINEL)


def run_probe(ctx, case, **change):
    """-> (rc, planes); `change` replaces fields of the case (the rejection test)"""
    from rayn_amd._lib import lib
    c = dict(case, **change)
    N = c["out_pixels"]
    got = {k: np.zeros((N, ch) if ch > 1 else N, np.float32) for k, ch in RN.PLANES}
    fp, up, bp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)))
    hist = None if c["base_hist"] is None else up(np.ascontiguousarray(c["base_hist"], np.uint32))
    arrays = [np.ascontiguousarray(c[k], t) for k, t in (("tiles", np.uint32), ("term_info", np.uint8), ("term_key", np.uint32), ("col0", np.float32),
                                                         ("aov", np.float32), ("obj", np.uint32))]
    tiles, info, key, col0, aov, obj = arrays
    assert info.size == key.size == obj.size == c["n_paths"] and col0.shape == aov.shape == (c["n_paths"], 3)
    rc = lib().rayn_hip_probe_resolve(ctx.h, c["width"], c["spp"], tiles.shape[0], up(tiles), c["max_tile_pixels"], c["n_paths"], bp(info), up(key), fp(col0),
                                      fp(aov), up(obj), hist, c["hist_stride"], c["n_depths"], SENTINEL, N, fp(got["color"]), fp(got["alpha"]),
                                      fp(got["background"]), fp(got["normal"]))
    return rc, got


def check(ctx, name, fma):
    case, want = RC.get(name), _statement(name)
    ctx.set_fma_policy(fma)
    try:
        rc, got = run_probe(ctx, case)
    finally:
        ctx.set_fma_policy(0)
    assert rc == 0, ctx.last_error()
    own = want["owned"]
    for k, _ in RN.PLANES:
        g, w = got[k], want[k]
        bad = np.flatnonzero((g.view(np.uint32) != w.view(np.uint32)).reshape(g.shape[0], -1).any(axis=1))
        print(name, fma, RN.family(case["spp"]), k, "pixels differing in bits:", bad.size, "of", int(own.sum()))
        assert bits_equal(g[own], w[own]), (k, bad[:8].tolist())
        assert (g[~own].view(np.uint32) == SENTINEL).all(), (k, "a pixel no tile owns was written", np.flatnonzero((g.view(np.uint32) != SENTINEL).reshape(g.shape[0], -1).any(axis=1) & ~own)[:8].tolist())


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("name", RC.NAMES)
def test_resolve_matches_the_serial_sum(gpu_ctx, name, fma):
    check(gpu_ctx, name, fma)


def test_probe_rejects_what_the_kernels_could_not_index(gpu_ctx):
    """every precondition rayn_hip.h lists, one at a time, on otherwise valid cases - then a normal case on the same context"""
    INVALID_ARG = -1
    reg, blk = RC.get("random_256"), RC.get("random_1024")

    def tiles_with(case, t, word, value):
        a = case["tiles"].copy()
        a[t, word] = value
        return a

    def path_with(case, field, i, value):
        a = case[field].copy()
        a[i] = value
        return a

    P0 = int(reg["tiles"][1, 4])                # first path of tile 1 of the reg case
    B0 = int(blk["tiles"][1, 4])
    d0 = int(blk["term_info"][B0] & 0x7F)
    base = int(blk["base_hist"][d0, 1])
    live = np.flatnonzero(reg["term_info"][P0:P0 + 256] != 0xFF)
    bad = [
        (reg, {"spp": 0}), (reg, {"spp": 254}), (reg, {"spp": 16388}),                                   # spp out of range
        (reg, {"tiles": tiles_with(reg, 2, 2, 300), "max_tile_pixels": 4096}),                           # 300 x 4 pixels > MAX_TILE_PIXELS
        (reg, {"max_tile_pixels": 19}),                                                                  # a 20-pixel tile in a 19-wide grid
        (reg, {"tiles": tiles_with(reg, 2, 4, reg["n_paths"] - 20 * 256 + 1)}),                          # the last path is one beyond the arrays
        (reg, {"tiles": tiles_with(reg, 3, 1, 8)}),                                                      # rows 8..12 of a 12-row film
        (reg, {"out_pixels": 23 * 9}),                                                                   # the film ends above the last row of tile 2
        (reg, {"tiles": tiles_with(reg, 1, 0, 1)}),                                                      # tile 1 moved onto tile 0: two owners of a pixel
        (RC.get("packed_256"), {"out_pixels": 50}),                                                      # packed: 51 pixels in 50
        (reg, {"term_info": path_with(reg, "term_info", P0 + 5, 121)}), (reg, {"term_info": path_with(reg, "term_info", P0 + 5, 0x80 | 126)}),  # depth > MAX_BOUNCES
        (reg, {"obj": path_with(reg, "obj", P0 + 7, 0x100)}), (reg, {"obj": path_with(reg, "obj", P0 + 7, 0xFFFFFFFF)}),  # neither below 0xFF nor OBJ_NONE
        (blk, {"term_key": path_with(blk, "term_key", B0, base - 1)}),                                   # a slot below its base_hist entry
        (blk, {"term_key": path_with(blk, "term_key", B0, base + (1 << 25))}),                           # an offset of 2^25
        (reg, {"term_info": path_with(reg, "term_info", P0 + live[1], reg["term_info"][P0 + live[0]]),   # two samples of one pixel with equal (depth, slot)
               "term_key": path_with(reg, "term_key", P0 + live[1], reg["term_key"][P0 + live[0]])}),
    ]
    for case, change in bad:
        rc, got = run_probe(gpu_ctx, case, **change)
        assert rc == INVALID_ARG, (list(change), rc)
        assert all((g == 0).all() for g in got.values()), "a refused call wrote its outputs"
    assert blk["term_info"][B0] != 0xFF and base > 0
    for name in ("random_256", "random_1024"):
        check(gpu_ctx, name, 0)
