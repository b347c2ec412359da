"""The two queue stages of one depth, stated in numpy from their definition (not from the kernels).

Bin: for tile k in order, the tile's segment of the binned queue starts at 64 x the sum of ceil(total_j / 64) over the earlier tiles; inside it, for class c
ascending, the references of the tile's entries with obj == c in queue order, then INVALID up to a multiple of 4; then INVALID up to a multiple of 64.
Repack: the same with one class and pad 1 over the survivors of the tile's binned segment in slot order.  Group ranges, class counts and bases, base_hist
and the control block's sizes and counters follow from the same sums.  A stage whose output needs more groups than its cap writes nothing, reports size 0
and sets its bit of the sticky overflow flag; every later stage is then empty too.

Shared by tests/test_queue.py (CPU: against a naive loop, and the properties) and tests/test_queue_device.py (the kernels through rayn_hip_probe_queue)."""
import numpy as np

INVALID = 0xFFFFFFFF
OBJ_NONE = 0xFF
NC = 16  # SCAN_NC_BIN: the row length of tile_cls_cnt / tile_cls_base
CTL = ("q_groups", "q_valid", "b_groups", "b_valid", "overflow", "segments", "shaded_slots", "entries_sum", "next_sum", "job_count", "head_shadow", "head_extend")


def pack(n_tiles, nclass, pad, tile, cls, ref):
    """Stable partition of the items (tile[i], cls[i], ref[i]), given in queue order with tile non-decreasing, into per-tile segments of class bins.
    Returns (queue, per-tile group begin, per-tile group count, cnt [n_tiles, nclass], bin base [n_tiles, nclass])."""
    cnt = np.bincount(tile * nclass + cls, minlength=n_tiles * nclass).reshape(n_tiles, nclass)
    padded = -(-cnt // pad) * pad
    groups = -(-padded.sum(1) // 64)
    begin = np.cumsum(groups) - groups
    base = begin[:, None] * 64 + np.cumsum(padded, 1) - padded
    out = np.full(int(groups.sum()) * 64, INVALID, np.uint32)
    earlier = np.cumsum(cnt, 0) - cnt  # items of class c in earlier tiles
    for c in range(nclass):
        i = np.flatnonzero(cls == c)  # queue order, and tile-major because the tiles lie back to back
        t = tile[i]
        out[base[t, c] + np.arange(i.size) - earlier[t, c]] = ref[i]
    return out, begin, groups, cnt, base


def reference(case):
    """Everything rayn_hip_probe_queue returns for the case, as a dict.  'bq' / 'qn' hold only the slots the stage owns (groups * 64; empty after an
    overflow): the slots beyond keep the caller's sentinel.  'need_b' / 'need_q' are the groups the stages need, 'cap_bin' / 'cap_repack' / 'out_slots'
    what the case asks the probe for: a cap is need + its delta, or the whole output buffer (need_b + 4 groups) where the case gives no delta."""
    tg = np.asarray(case["tile_groups"], np.int64)
    n_tiles, nclass = tg.size, case["nclass"]
    q, obj, survive = case["q"], case["obj"], case["survive"]
    tile = np.repeat(np.arange(n_tiles), tg * 64)
    live = obj != OBJ_NONE
    bq, b_begin, b_groups, cnt, base = pack(n_tiles, nclass, 4, tile[live], obj[live].astype(np.int64), q[live])
    slot_tile = np.repeat(np.arange(n_tiles), b_groups * 64)
    alive = bq != INVALID
    alive[alive] = survive[bq[alive]] != 0
    qn, q_begin, q_groups, scnt, _ = pack(n_tiles, 1, 1, slot_tile[alive], np.zeros(int(alive.sum()), np.int64), bq[alive])
    need_b, need_q = int(b_groups.sum()), int(q_groups.sum())
    out_groups = need_b + 4
    cap_bin = out_groups if case.get("cap_bin_delta") is None else need_b + case["cap_bin_delta"]
    cap_repack = out_groups if case.get("cap_repack_delta") is None else need_q + case["cap_repack_delta"]
    ctl = dict(zip(CTL, case["ctl0"]))
    ctl["q_groups"] = int(tg.sum())
    none = np.zeros(0, np.uint32)
    # bin stage
    if need_b > cap_bin:
        ctl["overflow"] |= 1
    ok_b = ctl["overflow"] == 0
    ctl["entries_sum"] += ctl["q_groups"] * 64
    ctl["b_groups"], ctl["b_valid"] = (need_b, int(cnt.sum())) if ok_b else (0, 0)
    ctl["segments"] += ctl["b_valid"]
    ctl["shaded_slots"] += ctl["b_groups"] * 64
    ctl["job_count"] = ctl["head_shadow"] = 0
    # repack stage (after a refused bin stage nothing was binned; its k_tile_prefix then sees the bin stage's totals, which cap_repack >= need_b covers)
    if ok_b and need_q > cap_repack:
        ctl["overflow"] |= 2
    ok_q = ctl["overflow"] == 0
    ctl["q_groups"], ctl["q_valid"] = (need_q, int(scnt.sum())) if ok_q else (0, 0)
    ctl["next_sum"] += ctl["q_groups"] * 64
    ctl["head_extend"] = 0
    cls_cnt = np.zeros((n_tiles, NC), np.uint32)
    cls_base = np.zeros((n_tiles, NC), np.uint32)
    cls_cnt[:, :nclass], cls_base[:, :nclass] = cnt, base
    tile_out = np.stack([b_begin, b_groups, q_begin, q_groups, b_begin * 64], 1).astype(np.uint32)
    return {"bq": bq if ok_b else none, "qn": qn if ok_q else none, "tile": tile_out, "cls_cnt": cls_cnt, "cls_base": cls_base,
            "ctl": np.array([ctl[k] for k in CTL], np.uint64), "need_b": need_b, "need_q": need_q, "cap_bin": cap_bin, "cap_repack": cap_repack,
            "out_slots": out_groups * 64, "ok_b": ok_b, "ok_q": ok_q}
