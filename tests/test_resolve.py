"""CPU checks of the film-resolve statement (tests/resolve_np.py) and of the cases the device test runs (tests/resolve_cases.py):
  - the statement equals a plain loop over np.float32 scalars, bit for bit, on every case of at most 256 spp;
  - every case tells the wrong resolves it names (resolve_np.MUTANTS) from the right one, and every mutant is named by a case of every kernel family it
    can occur in;
  - for the order mutants, a case named to kill one whose every pixel has at least 64 terms in the sums concerned differs in at least 80 % of those
    (pixel, channel) sums.  Two kinds of case are exempt and only have to differ (resolve_cases: weak): the order of a pair_* case is sample order
    but for ONE transposition of neighbours, which changes about 5 % of the sums at 64 terms - hence 51 pixels and six channels per case; and in a
    values_* case three pixels in five hold only -0.0, only subnormals (their sums are exact) or both infinities (NaN whatever the order);
  - the cases are what their names say: geometry, launch boundaries, the preconditions rayn_hip_probe_resolve checks."""
import numpy as np
import pytest

import resolve_cases as RC
import resolve_np as RN
from common import bits_equal

SENTINEL = 0xC0FFEE5A
SMALL = [n for n in RC.NAMES if RC.get(n)["spp"] <= 256]


def loop_reference(case):
    """Tile::add_sample as a loop: one np.float32 accumulator per channel, samples visited in sorted order, terms of another sum skipped"""
    spp, n = case["spp"], np.float32(case["spp"])
    N = case["out_pixels"]
    out = {"color": np.zeros((N, 3), np.float32), "alpha": np.zeros(N, np.float32), "background": np.zeros((N, 3), np.float32),
           "normal": np.zeros((N, 3), np.float32), "owned": np.zeros(N, bool)}
    info, key, obj = case["term_info"].tolist(), case["term_key"].tolist(), case["obj"].tolist()
    col, aov = case["col0"], case["aov"]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for _t, _lpix, P0, fi in RN.tile_pixels(case):
            live = sorted((info[P0 + i] & 0x7F, key[P0 + i], i) for i in range(spp) if info[P0 + i] != 0xFF)
            hits = sorted((obj[P0 + i], i) for i in range(spp) if obj[P0 + i] != 0xFF)
            for c in range(3):
                acc = [np.float32(0.0), np.float32(0.0)]
                for _d, _s, i in live:
                    acc[info[P0 + i] >> 7] = acc[info[P0 + i] >> 7] + col[P0 + i, c]
                a = np.float32(0.0)
                for _o, i in hits:
                    a = a + aov[P0 + i, c]
                out["color"][fi, c], out["background"][fi, c], out["normal"][fi, c] = acc[0] / n, acc[1] / n, a / n
            out["alpha"][fi] = np.float32(len(hits)) / n
            assert not out["owned"][fi]
            out["owned"][fi] = True
    return out


@pytest.mark.parametrize("name", SMALL)
def test_statement_equals_the_plain_loop(name):
    case = RC.get(name)
    want, got = loop_reference(case), RN.reference(case, SENTINEL)
    own = want["owned"]
    assert np.array_equal(own, got["owned"])
    for k, _ in RN.PLANES:
        assert bits_equal(got[k][own], want[k][own]), k
        assert (got[k][~own].view(np.uint32) == SENTINEL).all(), k


def differing(a, b, plane):
    """fraction of the (pixel, channel) words of a plane that differ, over the pixels either film owns (planes padded to a common size)"""
    N = max(a["owned"].size, b["owned"].size)
    pad = lambda x: np.concatenate([x.reshape(x.shape[0], -1), np.zeros((N - x.shape[0], x.reshape(x.shape[0], -1).shape[1]), x.dtype)])
    x, y = pad(a[plane]).view(np.uint32), pad(b[plane]).view(np.uint32)
    own = pad(a["owned"])[:, 0] | pad(b["owned"])[:, 0]
    nan = np.isnan(x.view(np.float32)) & np.isnan(y.view(np.float32))
    return float(((x != y) & ~nan)[own].mean())


def min_terms(case, mutant):
    """the fewest terms any pixel has in the sums an order mutant reorders"""
    _px, _col, is_c, is_b, _nrm, has = RN.pixel_terms(case)
    if mutant == "normal_sample_order":
        return int(has.sum(axis=1).min())
    return int((is_c | is_b).sum(axis=1).min())


@pytest.mark.parametrize("name", RC.NAMES)
def test_case_kills_the_wrong_resolves_it_names(name):
    case = RC.get(name)
    right = RN.reference(case, SENTINEL)
    assert case["kills"], "a case that can tell nothing apart"
    for m in case["kills"]:
        wrong = RN.reference(case, SENTINEL, mutant=m)
        d = {k: differing(right, wrong, k) for k, _ in RN.PLANES}
        print(name, m, d)
        assert max(d.values()) > 0.0, (name, m)
        if m in RN.ORDER_MUTANTS and not case["weak"] and min_terms(case, m) >= 64:
            # Color and Background share one order; a pixel's flagged and unflagged terms both move, so count the channel pairs in which either sum changed
            if m == "normal_sample_order":
                frac = d["normal"]
            else:
                frac = float(((right["color"].view(np.uint32) != wrong["color"].view(np.uint32))
                              | (right["background"].view(np.uint32) != wrong["background"].view(np.uint32)))[right["owned"]].mean())
            assert frac >= 0.8, (name, m, frac)


def test_every_mutant_is_killed_in_every_family():
    """per kernel family (reg at 256, blk at 1024 and 4096, huge at 4400) each wrong resolve is named by some case; signed_key32 exists only in blk, where a
    depth >= 64 case names it"""
    for spp in RC.FAMILY_SPP:
        named = {m for n in RC.NAMES if RC.get(n)["spp"] == spp for m in RC.get(n)["kills"]}
        want = set(RN.MUTANTS) - (set() if RC.is_blk(spp) else {"signed_key32"})
        assert named == want, (spp, want - named)
        if RC.is_blk(spp):
            assert "signed_key32" in RC.get("deep_%d" % spp)["kills"]


def test_spp_grid_reaches_every_variant_from_both_sides():
    assert [RC.get("spp%d" % s)["spp"] for s in RC.SPP_GRID] == list(RC.SPP_GRID)
    fam = [RN.family(s) for s in RC.SPP_GRID]
    assert set(fam) == {"reg<1>", "reg<2>", "reg<4>", "reg<8>", "blk<128,8>", "blk<256,8>", "blk<512,8>", "huge"}
    for edge in (64, 128, 256, 512, 1024, 2048, 4096):
        assert edge in RC.SPP_GRID and edge + 4 in RC.SPP_GRID and RN.family(edge) != RN.family(edge + 4)
    assert all(s % 4 == 0 for s in RC.SPP_GRID)


@pytest.mark.parametrize("name", RC.NAMES)
def test_case_is_well_formed(name):
    """what rayn_hip_probe_resolve checks, and what the issue asks of every case: >= 48 pixels in >= 3 unequal tiles (8 at 16384 spp), non-contiguous in the
    pool, inside a film they do not cover (unless packed)"""
    c = RC.get(name)
    spp, tiles = c["spp"], c["tiles"].tolist()
    px = RN.tile_pixels(c)
    assert len(tiles) >= 3 and len(px) >= (8 if spp == 16384 else 48)
    assert len({(t[2], t[3]) for t in tiles}) >= 3 and ({(3, 2), (1, 5)} <= {(t[2], t[3]) for t in tiles} or spp == 16384 or name == "tile1024_spp4" or name.startswith("wide_grid"))
    spans = sorted((t[4], t[4] + t[2] * t[3] * spp) for t in tiles)
    assert spans[0][0] > 0 and all(a[1] < b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= c["n_paths"]
    assert [t[4] for t in tiles] != sorted(t[4] for t in tiles)
    fi = [p[3] for p in px]
    assert len(set(fi)) == len(fi) and max(fi) < c["out_pixels"] and all(t[2] * t[3] <= c["max_tile_pixels"] for t in tiles)
    assert (len(fi) == c["out_pixels"]) == bool(tiles[0][7])
    info, key, obj = c["term_info"], c["term_key"], c["obj"]
    assert ((obj < 0xFF) | (obj == 0xFF)).all()
    for t, _lpix, P0, _fi in px:
        live = info[P0:P0 + spp] != 0xFF
        d = (info[P0:P0 + spp] & 0x7F)[live].astype(np.int64)
        s = key[P0:P0 + spp][live].astype(np.int64)
        assert (d <= 120).all() and np.unique((d << 32) | s).size == d.size
        if RC.is_blk(spp):
            off = s - c["base_hist"][d, t].astype(np.int64)
            assert (off >= 0).all() and (off < (1 << 25)).all() and (c["base_hist"][d, t] != 0).all()


def test_cases_are_what_their_names_say():
    for spp in RC.FAMILY_SPP:
        nt = RC.block_threads(spp)
        c = RC.get("deep_%d" % spp)
        assert set(np.unique(c["term_info"][RC.Layout(spp).idx] & 0x7F).tolist()) == {0, 63, 64, 119, 120}
        c = RC.get("none30_%d" % spp)
        assert 0.25 < (c["term_info"][RC.Layout(spp).idx] == 0xFF).mean() < 0.35
        for nm, at in (("pair_lane", 37), ("pair_wave", 63)) + ((("pair_reg", nt - 1),) if nt > 64 else ()):
            c = RC.get("%s_%d" % (nm, spp))
            k = np.where(c["term_info"][RC.Layout(spp).idx] != 0xFF, c["term_key"][RC.Layout(spp).idx].astype(np.int64), 1 << 40)  # dropped samples sort last
            down = np.diff(k, axis=1) < 0
            assert (down.sum(axis=1) == 1).all() and down[:, at].all()
            assert ((k < 1 << 40).sum(axis=1) == spp).sum() == 17  # one pixel in three keeps the whole chain
        c = RC.get("sorted_sky_%d" % spp)
        assert (np.diff(c["term_key"][RC.Layout(spp).idx].astype(np.int64), axis=1) > 0).all() and (c["term_info"][RC.Layout(spp).idx] == 0x80).all()
        c = RC.get("mixed0_%d" % spp)
        assert set(np.unique(c["term_info"][RC.Layout(spp).idx]).tolist()) == {0x00, 0x80}
        c = RC.get("empty_%d" % spp)
        r = RN.reference(c)
        live = (c["term_info"][RC.Layout(spp).idx] != 0xFF).any(axis=1)
        hit = (c["obj"][RC.Layout(spp).idx] != 0xFF).any(axis=1)
        assert (~live).sum() == 8 and (~hit).sum() == 8 and (~live & ~hit).sum() == 4 and (r["alpha"][r["owned"]] == 0).sum() == 8
        if RC.is_blk(spp):
            c = RC.get("offset_top_%d" % spp)
            L = RC.Layout(spp)
            d = (c["term_info"][L.idx] & 0x7F).astype(np.int64)
            off = c["term_key"][L.idx].astype(np.int64) - c["base_hist"][d, L.tile_of[:, None]].astype(np.int64)
            assert (off.min(axis=1) == 0).all() and (off.max(axis=1) == (1 << 25) - 1).all()
            assert np.unique(c["base_hist"][:17, :4]).size == 17 * 4 and (c["base_hist"] >> 31).any()
        else:
            c = RC.get("slot_bit31_%d" % spp)
            k = c["term_key"][RC.Layout(spp).idx]
            assert (k.max(axis=1) == 0xFFFFFFFF).all() and 0.4 < (k >> 31).mean() < 0.6
        c = RC.get("values_%d" % spp)
        r = RN.reference(c)
        own = np.flatnonzero(r["owned"])
        planes = np.concatenate([r["color"], r["background"], r["normal"]], axis=1)[own]
        assert own.size == 51  # (film order is not tile_pixels order: the pixels are told apart by content)
        assert np.isnan(planes).any(axis=1).sum() >= 10 + 1           # the +Inf .. -Inf pixels and the NaN pixels
        sub = (np.abs(planes) < 2.0 ** -126) & (planes != 0)
        assert sub.any(axis=1).sum() >= 10                              # subnormal sums stay subnormal (and non-zero)
        assert (planes.view(np.uint32) == 0).all(axis=1).sum() >= 10    # only -0.0: every sum is +0.0
    c = RC.get("tile1024_spp4")
    assert c["spp"] == 4 and (32, 32) in {(t[2], t[3]) for t in c["tiles"].tolist()} and c["max_tile_pixels"] == 1024
    for spp in RC.FAMILY_SPP:
        c = RC.get("wide_grid_%d" % spp)
        assert c["max_tile_pixels"] == 1024 and (5, 3) in {(t[2], t[3]) for t in c["tiles"].tolist()}
        c = RC.get("packed_%d" % spp)
        assert c["tiles"][:, 7].all() and c["out_pixels"] == 51
    c = RC.get("uncovered_256")
    assert not c["tiles"][:, 7].any() and (~RN.reference(c)["owned"]).sum() == 23 * 12 - 51
    assert len(RN.tile_pixels(RC.get("spp16384"))) == 8 and max(RC.get(n)["n_paths"] for n in RC.NAMES) < 51 * 4400 + 64  # 8 x 16384 and 51 x 4400 paths are the largest inputs
