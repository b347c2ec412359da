"""Seeded inputs of the queue-stage probe (rayn_hip_probe_queue), shared by tests/test_queue.py (numpy statement against a naive loop, properties, and
the check that every edge below is really in the list) and tests/test_queue_device.py (the kernels).  A case is a dict:
    name, nclass, tile_groups [n_tiles] (64-entry groups per tile, tiles back to back), q [n] (reference, or INVALID for a padding entry), obj [n] (class
    byte, or OBJ_NONE), survive [n_refs], n_refs, ctl0 (start values of the control block, order queue_np.CTL), bounds (factor on the actual counts
    for max_entries / max_slots), cap_bin_delta / cap_repack_delta (None: ample; else cap_groups = the stage's need + delta).

What the shapes are for (rayn_amd/csrc/kernels.hip): k_tile_prefix walks the tiles 1024 at a time; k_scan_tile walks a tile's groups 512 at a time;
k_bin_scatter / k_compact_scatter take a second grid-stride trip after 2048 * 256 * 8 slots and k_group_hist after 2048 * 256 * 2 16-byte pieces.

Time of queue_np.reference on the two large cases, measured on the CPU (one core): big5m (5.2 M entries) 0.7 s, big17m (17.0 M entries) 2.5 s;
building their inputs costs under 0.1 s each.  Every other case is a few milliseconds."""
import numpy as np

from queue_np import INVALID, OBJ_NONE

# non-zero start values, so that a counter which is set instead of advanced (or a head that is not reset) shows; shaded_slots starts above 2^32
CTL0 = (0, 0, 0xB0B0, 0xB1B1, 0, 1000, (2 << 32) + 5, 3000, 4000, 77, 88, 99)
SCATTER_TRIP = 2048 * 256 * 8   # slots of one grid-stride trip of k_bin_scatter / k_compact_scatter
HIST_TRIP = 2048 * 256 * 2 * 16  # entries of one grid-stride trip of k_group_hist


def _finish(name, nclass, tile_groups, obj, q, survive, bounds=1, cap_bin_delta=None, cap_repack_delta=None):
    obj = np.ascontiguousarray(obj, np.uint8)
    q = np.ascontiguousarray(q, np.uint32)
    obj[q == INVALID] = OBJ_NONE  # a padding entry carries no object
    ctl0 = list(CTL0)
    ctl0[1] = int((q != INVALID).sum())
    return {"name": name, "nclass": nclass, "tile_groups": np.ascontiguousarray(tile_groups, np.uint32), "q": q, "obj": obj,
            "survive": np.ascontiguousarray(survive, np.uint8), "n_refs": int(q.size), "ctl0": tuple(ctl0), "bounds": bounds,
            "cap_bin_delta": cap_bin_delta, "cap_repack_delta": cap_repack_delta}


def _refs(n, tile_groups, rng, tail_pad=True):
    """references = a bijection of the entry index (so that order is checkable); the last few entries of every tile are padding (INVALID)"""
    q = (np.arange(n, dtype=np.uint32) ^ np.uint32(0x2A))
    if tail_pad:
        end = np.cumsum(np.asarray(tile_groups, np.int64) * 64)
        for e, g in zip(end, tile_groups):
            if g:
                q[e - int(rng.integers(0, 64)):e] = INVALID
    return q


def make(name, nclass, tile_groups, seed, weights=None, none=0.1, survive=0.5, tail_pad=True, **kw):
    """random classes with the given weights (default: uniform), a fraction `none` of misses, a fraction `survive` of survivors"""
    rng = np.random.default_rng(seed)
    tile_groups = np.asarray(tile_groups, np.int64)
    n = int(tile_groups.sum()) * 64
    w = np.ones(nclass) if weights is None else np.asarray(weights, float)
    obj = rng.choice(nclass, n, p=w / w.sum()).astype(np.uint8)
    obj[rng.random(n) < none] = OBJ_NONE
    q = _refs(n, tile_groups, rng, tail_pad)
    sv = (rng.random(n) < survive).astype(np.uint8) if 0 < survive < 1 else np.full(n, int(survive), np.uint8)
    return _finish(name, nclass, tile_groups, obj, q, sv, **kw)


def _tiles(n_tiles, seed):
    """0 to 3 groups per tile, with empty tiles at the start, in the middle and at the end"""
    tg = np.random.default_rng(seed).integers(0, 4, n_tiles)
    if n_tiles == 1:
        tg[:] = 2
    elif n_tiles == 2:
        tg[:] = (0, 3)
    else:
        tg[0] = tg[n_tiles // 2] = tg[-1] = 0
        tg[1] = 3
    return tg


def _residues():
    """one tile whose four class counts are 4, 5, 6, 7 (every residue mod 4), a second whose counts are 0, 1, 2, 3"""
    rng = np.random.default_rng(40)
    obj = np.full(128, OBJ_NONE, np.uint8)
    obj[:22] = np.repeat([0, 1, 2, 3], [4, 5, 6, 7])
    obj[64:70] = np.repeat([1, 2, 3], [1, 2, 3])
    obj[:64] = rng.permutation(obj[:64])
    obj[64:] = rng.permutation(obj[64:])
    return _finish("residues", 4, [1, 1], obj, _refs(128, [1, 1], rng, False), rng.integers(0, 2, 128))


def _exact_survivors():
    """tile 0 leaves exactly 64 survivors, tile 1 exactly 128 (no tail padding in the next queue), tile 2 exactly 1"""
    rng = np.random.default_rng(41)
    tg = [3, 4, 2]
    n = 64 * 9
    obj = rng.integers(0, 5, n).astype(np.uint8)
    q = _refs(n, tg, rng, False)
    sv = np.zeros(n, np.uint8)
    for lo, hi, k in ((0, 192, 64), (192, 448, 128), (448, 576, 1)):
        sv[q[lo + rng.choice(hi - lo, k, replace=False)]] = 1
    return _finish("exact_survivors", 5, tg, obj, q, sv)


def _big(name, nclass, pattern_groups, reps, seed, none):
    """np.tile of a pattern of whole tiles: the numpy statement's cost per entry stays a few passes over the arrays"""
    rng = np.random.default_rng(seed)
    pg = np.asarray(pattern_groups, np.int64)
    m = int(pg.sum()) * 64
    obj = rng.integers(0, nclass, m).astype(np.uint8)
    obj[rng.random(m) < none] = OBJ_NONE
    obj[:64] = 0  # a whole group of one class
    tg = np.tile(pg, reps)
    n = m * reps
    q = np.arange(n, dtype=np.uint32) ^ np.uint32(0x2A)
    return _finish(name, nclass, tg, np.tile(obj, reps), q, np.tile((rng.random(m) < 0.7).astype(np.uint8), reps), bounds=1)


def small_cases():
    """every case but the two large ones, in a fixed order"""
    out = []
    for i, (n_tiles, nclass) in enumerate([(1, 1), (2, 2), (1023, 4), (1024, 5), (1025, 13), (2049, 16), (3100, 2)]):
        out.append(make(f"tiles{n_tiles}", nclass, _tiles(n_tiles, 10 + i), 20 + i, bounds=2 if n_tiles in (1025, 3100) else 1))
    out.append(make("groups_per_tile", 13, [1, 63, 64, 65, 511, 512, 513, 1100], 30, survive=0.6))
    out.append(make("groups_per_tile_c1", 1, [513, 0, 1100, 512], 31, none=0.02, survive=0.9, bounds=2))
    out.append(make("one_class", 4, [2, 0, 5, 1], 32, weights=[0, 0, 1, 0], none=0.0, tail_pad=False))           # groups of 64 equal bytes, classes 0, 1, 3 empty
    out.append(make("sparse_classes", 13, [3, 1, 0, 7], 33, weights=[0, 1, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 1]))    # empty classes between populated ones
    out.append(make("full_house16", 16, [4, 2, 9, 0, 1], 34, none=0.05))
    out.append(_residues())
    out.append(make("none40", 5, [3, 2, 0, 6, 1], 35, none=0.4))
    out.append(make("all_none", 4, [2, 0, 3], 36, none=1.0))                                                    # no live entry: every tile's group count falls to 0
    out.append(make("survive_all", 4, [3, 0, 2, 5], 37, survive=1))
    out.append(make("survive_none", 4, [3, 0, 2, 5], 38, survive=0))
    out.append(_exact_survivors())
    out.append(make("no_groups", 2, [0, 0, 0], 39, bounds=1))                                                   # an actual count of 0 groups
    return out


def overflow_cases():
    """(case, stage) with the stage's cap one group short of the need, and the bin stage with its cap exactly at the need (stage None: no overflow)"""
    tg = _tiles(1025, 50)
    return [(make("overflow_bin", 5, tg, 51, cap_bin_delta=-1), 0), (make("overflow_repack", 5, tg, 51, cap_repack_delta=-1), 1),
            (make("cap_bin_exact", 5, tg, 51, cap_bin_delta=0), None), (make("cap_both_exact", 5, tg, 51, cap_bin_delta=0, cap_repack_delta=0), None)]


def big5m():
    """>= 5 M entries in 3-to-24-group tiles: k_bin_scatter and k_compact_scatter take a second grid-stride trip"""
    return _big("big5m", 4, [16, 0, 24, 3, 8, 13], 1280, 60, 0.05)  # 64 groups = 4096 entries per pattern


def big17m():
    """2048 * 256 * 2 * 16 entries plus a tail: k_group_hist takes a second grid-stride trip (two classes keep the numpy statement cheap)"""
    return _big("big17m", 2, [16, 0, 40, 8], 4150, 61, 0.05)
