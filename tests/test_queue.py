"""The numpy statement of the queue stages (tests/queue_np.py) against a deliberately naive loop over entries, the properties every binned / repacked
queue must have, and the check that the case list (tests/queue_cases.py) really holds every edge the device test (tests/test_queue_device.py) is
there for - so that a later edit cannot silently thin it.  No GPU."""
import functools

import numpy as np
import pytest

import queue_cases as QC
import queue_np as QN
from queue_np import INVALID, OBJ_NONE

SMALL = QC.small_cases()
OVERFLOW = QC.overflow_cases()
ALL_SMALL = SMALL + [c for c, _ in OVERFLOW]


@functools.lru_cache(maxsize=None)
def big(name):
    case = getattr(QC, name)()
    return case, QN.reference(case)


def naive(case):
    """entry by entry, list by list: (binned queue, next queue, per-tile rows, cls_cnt, cls_base) with ample caps"""
    nclass = case["nclass"]
    q, obj, survive = case["q"].tolist(), case["obj"].tolist(), case["survive"].tolist()
    bq, qn, rows, cnts, bases, e = [], [], [], [], [], 0
    for g in case["tile_groups"].tolist():
        bins = [[] for _ in range(nclass)]
        for i in range(e, e + 64 * g):
            if obj[i] != OBJ_NONE:
                bins[obj[i]].append(q[i])
        e += 64 * g
        b_begin, seg, cnt, base = len(bq) // 64, [], [0] * QN.NC, [0] * QN.NC
        for c in range(nclass):
            cnt[c], base[c] = len(bins[c]), len(bq) + len(seg)
            seg += bins[c]
            while len(seg) % 4:
                seg.append(INVALID)
        while len(seg) % 64:
            seg.append(INVALID)
        bq += seg
        nxt = [r for r in seg if r != INVALID and survive[r]]
        while len(nxt) % 64:
            nxt.append(INVALID)
        rows.append([b_begin, len(seg) // 64, len(qn) // 64, len(nxt) // 64, b_begin * 64])
        qn += nxt
        cnts.append(cnt)
        bases.append(base)
    return bq, qn, rows, cnts, bases


@pytest.mark.parametrize("case", ALL_SMALL, ids=lambda c: c["name"])
def test_numpy_statement_matches_the_naive_loop(case):
    bq, qn, rows, cnts, bases = naive(case)
    ample = dict(case, cap_bin_delta=None, cap_repack_delta=None)
    ref = QN.reference(ample)
    assert ref["bq"].tolist() == bq and ref["qn"].tolist() == qn
    assert ref["tile"].tolist() == rows and ref["cls_cnt"].tolist() == cnts and ref["cls_base"].tolist() == bases
    ctl, c0 = dict(zip(QN.CTL, ref["ctl"].tolist())), dict(zip(QN.CTL, case["ctl0"]))
    hits, surv = sum(r != INVALID for r in bq), sum(r != INVALID for r in qn)
    assert ctl == {"q_groups": len(qn) // 64, "q_valid": surv, "b_groups": len(bq) // 64, "b_valid": hits, "overflow": 0, "segments": c0["segments"] + hits,
                   "shaded_slots": c0["shaded_slots"] + len(bq), "entries_sum": c0["entries_sum"] + len(case["q"]), "next_sum": c0["next_sum"] + len(qn),
                   "job_count": 0, "head_shadow": 0, "head_extend": 0}
    assert ref["need_b"] == len(bq) // 64 and ref["need_q"] == len(qn) // 64 and ref["out_slots"] >= len(bq) + 256


def check_properties(case, ref):
    """each live reference once in the binned queue, each survivor once in the next queue, queue order inside (tile, class), one class per 4-slot packet,
    64-aligned segments"""
    q, obj, survive, nclass = case["q"], case["obj"], case["survive"], case["nclass"]
    bq, qn, rows = ref["bq"], ref["qn"], ref["tile"].astype(np.int64)
    n_tiles = rows.shape[0]
    live = obj != OBJ_NONE
    assert not (q[live] == INVALID).any()
    entry_of = np.full(case["n_refs"], -1, np.int64)  # references are unique: reference -> queue position
    entry_of[q[q != INVALID]] = np.flatnonzero(q != INVALID)
    entry_tile = np.repeat(np.arange(n_tiles), case["tile_groups"].astype(np.int64) * 64)
    # segments: back to back, whole groups
    assert (rows[:, 0] == np.cumsum(rows[:, 1]) - rows[:, 1]).all() and (rows[:, 2] == np.cumsum(rows[:, 3]) - rows[:, 3]).all()
    assert bq.size == rows[:, 1].sum() * 64 and qn.size == rows[:, 3].sum() * 64 and (rows[:, 4] == rows[:, 0] * 64).all()
    slot_tile = np.repeat(np.arange(n_tiles), rows[:, 1] * 64)
    vb = bq != INVALID
    want = np.zeros(case["n_refs"], np.int64)
    want[q[live]] = 1
    assert np.array_equal(np.bincount(bq[vb], minlength=case["n_refs"]), want)  # exactly the live references, once each
    assert np.array_equal(entry_tile[entry_of[bq[vb]]], slot_tile[vb])  # in their own tile's segment
    # inside a tile: class-major, queue order inside a class
    key = (slot_tile[vb] * nclass + obj[entry_of[bq[vb]]]) * (1 << 32) + entry_of[bq[vb]]
    assert (np.diff(key) > 0).all()
    # a 4-slot packet holds one class, its INVALID slots at the end
    pk = bq.reshape(-1, 4)
    pv = pk != INVALID
    assert (pv[:, :-1] >= pv[:, 1:]).all()
    slot_cls = np.full(bq.size, 255, np.int64)
    slot_cls[vb] = obj[entry_of[bq[vb]]]
    pc = slot_cls.reshape(-1, 4)
    assert ((pc == pc[:, :1]) | ~pv).all()
    # next queue: exactly the survivors, in slot order of the tile's binned segment, no padding but the tail
    alive = vb.copy()
    alive[vb] = survive[bq[vb]] != 0
    vq = qn != INVALID
    next_tile = np.repeat(np.arange(n_tiles), rows[:, 3] * 64)
    assert np.array_equal(qn[vq], bq[alive]) and np.array_equal(next_tile[vq], slot_tile[alive])
    per_tile = np.bincount(slot_tile[alive], minlength=n_tiles)
    assert (rows[:, 3] == -(-per_tile // 64)).all()
    for k in np.flatnonzero(rows[:, 3]):
        seg = vq[rows[k, 2] * 64:(rows[k, 2] + rows[k, 3]) * 64]
        assert seg[:per_tile[k]].all() and not seg[per_tile[k]:].any()


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c["name"])
def test_properties(case):
    check_properties(case, QN.reference(case))


@pytest.mark.parametrize("name", ["big5m", "big17m"])
def test_properties_of_the_large_cases(name):
    check_properties(*big(name))


def test_overflow_statement():
    for case, stage in OVERFLOW:
        ref = QN.reference(case)
        ctl = dict(zip(QN.CTL, ref["ctl"].tolist()))
        assert ctl["overflow"] == (0 if stage is None else 1 << stage), case["name"]
        assert ref["need_b"] > 1024 and ref["need_q"] > 64  # more than one trip of k_tile_prefix feeds the comparison
        if stage == 0:
            assert ref["cap_bin"] == ref["need_b"] - 1 and ref["cap_repack"] >= ref["need_b"]
            assert ref["bq"].size == ref["qn"].size == 0 and ctl["b_groups"] == ctl["b_valid"] == ctl["q_groups"] == ctl["q_valid"] == 0
        elif stage == 1:
            assert ref["cap_repack"] == ref["need_q"] - 1 and ref["bq"].size == ref["need_b"] * 64 and ref["qn"].size == 0
            assert ctl["b_groups"] == ref["need_b"] and ctl["q_groups"] == ctl["q_valid"] == 0
        else:
            assert ref["cap_bin"] == ref["need_b"] and ref["bq"].size == ref["need_b"] * 64 and ref["qn"].size == ref["need_q"] * 64


def test_the_case_list_holds_every_edge():
    cases = SMALL + [big("big5m")[0], big("big17m")[0]]
    refs = {c["name"]: (QN.reference(c) if not c["name"].startswith("big") else big(c["name"])[1]) for c in cases}
    by = {c["name"]: c for c in cases}
    assert len(by) == len(cases)
    # tiles: the trip length of k_tile_prefix and both sides of it, empty tiles at the start, in the middle and at the end
    assert {c["tile_groups"].size for c in cases} >= {1, 2, 1023, 1024, 1025, 2049, 3100}
    for n in (1023, 1024, 1025, 2049, 3100):
        tg = by[f"tiles{n}"]["tile_groups"]
        assert tg[0] == 0 and tg[-1] == 0 and (tg[1:-1] == 0).any() and tg.max() == 3 and set(tg.tolist()) == {0, 1, 2, 3}
    # groups per tile: the trip length of k_scan_tile (512) and both sides of it, more than two trips, and the wave width
    assert set(by["groups_per_tile"]["tile_groups"].tolist()) >= {1, 63, 64, 65, 511, 512, 513, 1100}
    assert {c["nclass"] for c in cases} >= {1, 2, 4, 5, 13, 16}
    assert by["groups_per_tile"]["nclass"] > 4 and by["groups_per_tile_c1"]["nclass"] == 1  # a wave that owns several classes, and three idle waves
    # populations
    hist = lambda c: np.stack([(c["obj"].reshape(-1, 64) == k).sum(1) for k in range(c["nclass"])], 1)  # per group and class
    assert (hist(by["one_class"])[:, 2] == 64).all() and (hist(by["one_class"])[:, [0, 1, 3]] == 0).all()
    assert (hist(big("big5m")[0]) == 64).any()
    pop = refs["sparse_classes"]["cls_cnt"].sum(0) > 0
    assert pop[:13].tolist() == [False, True, False, False, False, True, False, False, False, False, False, False, True]
    cnt = refs["residues"]["cls_cnt"][:, :4]
    assert cnt.tolist() == [[4, 5, 6, 7], [0, 1, 2, 3]]
    assert (refs["full_house16"]["cls_cnt"].sum(0) > 0).all()
    real = by["none40"]["q"] != INVALID
    assert 0.36 < (by["none40"]["obj"][real] == OBJ_NONE).mean() < 0.44
    assert (by["all_none"]["obj"] == OBJ_NONE).all() and by["all_none"]["q"].size > 0 and refs["all_none"]["need_b"] == 0
    # a tile whose group count has fallen to 0 after a repack, next to tiles that keep theirs
    assert any(((r["tile"][:, 1] > 0) & (r["tile"][:, 3] == 0)).any() and (r["tile"][:, 3] > 0).any() for r in refs.values())
    # survivors
    assert refs["survive_all"]["ctl"][1] == refs["survive_all"]["ctl"][3] > 0 and refs["survive_none"]["ctl"][1] == 0 < refs["survive_none"]["ctl"][3]
    assert any(0.4 < r["ctl"][1] / max(1, r["ctl"][3]) < 0.6 for r in refs.values())
    ex = refs["exact_survivors"]
    assert (ex["qn"].reshape(-1, 64) != INVALID).sum(1).tolist() == [64, 64, 64, 1] and ex["tile"][:, 3].tolist() == [1, 2, 1]
    # bounds
    assert {c["bounds"] for c in cases} >= {1, 2} and by["no_groups"]["q"].size == 0 and by["no_groups"]["tile_groups"].size == 3
    # the grid-stride trips
    b5, b17 = big("big5m"), big("big17m")
    assert b5[0]["q"].size >= 5_000_000 and b5[1]["need_b"] * 64 > QC.SCATTER_TRIP + 64 * 1024
    assert b17[0]["q"].size >= QC.HIST_TRIP + 64 * 1024 and b17[0]["q"].size % QC.HIST_TRIP != 0
    assert b5[0]["tile_groups"].size > 1024 and b17[0]["tile_groups"].size > 1024
    # overflow: each stage one group short, the bin stage exactly at its need
    assert sorted((s, c["cap_bin_delta"], c["cap_repack_delta"]) for c, s in OVERFLOW if s is not None) == [(0, -1, None), (1, None, -1)]
    assert any(s is None and c["cap_bin_delta"] == 0 for c, s in OVERFLOW)
