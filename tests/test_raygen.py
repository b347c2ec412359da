"""CPU checks of the ray-generation statement (tests/raygen_np.py), of the oracle's export of its ray-gen loop (oracle_raygen_tile) and of the cases the
device test runs (tests/raygen_cases.py):
  - the export and the numpy statement agree in every bit of everything the probe returns, on every case, under both mul_add policies;
  - the export's (pixel, sample) order is the order in which the film's own tile closure hands its rays on (trace_tile's depth-0 entries);
  - the cases are what their names say - the counts of paths at the filter's and the sampler's edges, the padding share, the groups per tile are measured
    here and printed;
  - every case tells the wrong statements it names (raygen_np.MUTANTS) from the right one, every mutant is named by some case, and a case that names the
    time or the lens mutant differs from it in at least 10 % of its paths."""
import numpy as np
import pytest

import raygen_cases as RC
import raygen_np as RN
from common import bits_equal

f32 = np.float32


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("name", RC.NAMES)
def test_export_equals_the_statement(oracle, name, fma):
    c = RC.get(name)
    rays = RC.oracle_rays(name, fma)
    for t, r in enumerate(rays):  # the export's own words: its loop order is the slot order
        xs, ys, s = RN.slot_paths(c, t)
        lx, ly, ls = RN.loop_paths(c, t)
        assert np.array_equal(xs, lx) and np.array_equal(ys, ly) and np.array_equal(s, ls)
        assert np.array_equal(r["pixel"], (xs + ys * int(c["p"].width)).astype(np.uint32)) and np.array_equal(r["sample"], s.astype(np.uint32))
        mine = RN.tile_rays(c, t, bool(fma))
        for k in ("origin", "dir", "time"):
            assert bits_equal(r[k], mine[k]), (name, t, k)
    d = RN.differing(RN.reference(c, rays=list(rays)), RN.reference(c, fma=bool(fma)))
    print(name, fma, d)
    assert not any(d.values()), d


def test_fused_policy_is_stated():
    """the two policies differ where a mul_add rounds (normalized, cross, concentric_circle_map): the comparison above is one per policy, not one twice"""
    c = RC.get("anim_thin_lens_15")
    assert RN.changed_paths(RN.reference(c), RN.reference(c, fma=True)) > 0.2
    a, cc = f32(1.0 + 2.0 ** -12), f32(-(1.0 + 2.0 ** -11))  # a * a = 1 + 2^-11 + 2^-24: the last term is lost when the product is rounded
    assert RN.RS.fma32(a, a, cc) == f32(2.0 ** -24) and f32(a * a + cc) == 0


def test_export_order_is_the_films(oracle):
    """trace_tile records every packet the film's tile closure shades; at depth 0 those are the ray-gen rays, binned by hit object in insertion order"""
    c = RC.get("edge_50x37")
    for k in (0, 5):
        x0, y0, ew, eh = [int(v) for v in c["tiles"][k][:4]]
        r = RC.oracle_rays("edge_50x37", 0)[k]
        tr = oracle.trace_tile(c["wd"], c["p"], c["tabs"], k)
        d0 = (tr["depth"] == 0) & (tr["valid"] == 1)
        assert d0.sum() == len(r["pixel"]) == ew * eh * RN.spp_of(c)  # the scene is closed: every ray hits something
        pix = (x0 + tr["px"][d0].astype(np.int64)) + (y0 + tr["py"][d0].astype(np.int64)) * int(c["p"].width)
        key = pix * 65536 + tr["sample"][d0]
        order = {int(v): i for i, v in enumerate(r["pixel"].astype(np.int64) * 65536 + r["sample"])}
        assert len(order) == len(key) == len(set(key.tolist()))
        at = np.array([order[int(v)] for v in key])
        for o in np.unique(tr["obj"][d0]):
            assert (np.diff(at[tr["obj"][d0] == o]) > 0).all(), (k, o)


@pytest.mark.parametrize("name", RC.NAMES)
def test_case_is_well_formed(name):
    """what rayn_hip_probe_raygen checks before it launches anything"""
    c = RC.get(name)
    p, spp, tiles = c["p"], RN.spp_of(c), c["tiles"].astype(np.int64)
    s1, s2, scr, fis = c["tabs"]
    assert 4 <= spp <= 16384 and spp % 4 == 0 and 2 <= p.volume_marches <= 4 and p.max_bounces <= 120
    assert s1.size == spp * (1 + (p.max_bounces + 1) * (3 + p.volume_marches)) and s2.size == spp * 2 * (2 + (p.max_bounces + 1) * (12 + 8 * p.volume_marches))
    assert scr.size == p.width * p.height and scr.size * 4 < 100 * 1024 and fis.size == 512
    owned = np.zeros(c["n_pool"] // 64, int)
    for x0, y0, ew, eh, base, n, _fb, _fp in tiles.tolist():
        assert 1 <= ew * eh <= 1024 and x0 + ew <= p.width and y0 + eh <= p.height and n == ew * eh * spp and base % 64 == 0
        owned[base // 64:base // 64 + (n + 63) // 64] += 1
    assert c["n_pool"] % 64 == 0 and (owned == 1).all()
    assert c["kills"] and set(c["kills"]) <= set(RN.MUTANTS)
    if name in RC.VALUES:
        assert len({(t[2], t[3]) for t in tiles.tolist()}) >= 3 and tiles[:, 5].sum() >= 2048


def test_cases_are_what_their_names_say():
    m = {n: RC.measure(RC.get(n)) for n in RC.NAMES}
    for n in RC.NAMES:
        print(n, m[n])
    g = lambda n: RC.get(n)
    assert m["one_pixel"]["paths"] == 4 and g("one_pixel")["n_pool"] == 64 and m["one_pixel"]["padding_share"] == 60 / 64
    assert [tuple(t[:4]) for t in g("edge_50x37")["tiles"].tolist()] == [(x, y, 16, 16) for x in (0, 16, 32) for y in (0, 16)]
    for n, spp in (("edge_21x13_spp4", 4), ("edge_21x13_spp12", 12)):
        t = g(n)["tiles"].astype(np.int64)
        assert {(5, 8), (8, 5), (5, 5), (8, 8)} == {(a, b) for a, b in t[:, 2:4].tolist()} and RN.spp_of(g(n)) == spp
        assert (t[:, 5] % 64 != 0).sum() >= 3 and m[n]["padding_share"] > 0
    assert tuple(g("wide_32x4")["tiles"][0][2:4]) == (32, 4) and tuple(g("tall_4x32")["tiles"][0][2:4]) == (4, 32)
    t = g("permuted")["tiles"].astype(np.int64)
    assert len(t) >= 7 and len({(a, b) for a, b in t[:, 2:4].tolist()}) == len(t)
    by_base = np.argsort(t[:, 4])
    assert (np.diff(by_base) < 0).sum() >= 2 and (np.diff(by_base) > 0).sum() >= 2  # the pool order is neither the list order nor its reverse
    assert m["many_tiles"]["tiles"] == 1280 and RN.spp_of(g("many_tiles")) == 4 and set(map(tuple, g("many_tiles")["tiles"][:, 2:4].tolist())) == {(2, 2)}
    for n, groups in (("groups_256", 256), ("groups_320", 320), ("groups_1024", 1024)):
        assert m[n]["groups_per_tile"][1] == groups and tuple(g(n)["tiles"][0][2:4]) == (32, 32)
    assert m["groups_1024"]["paths"] == 65536 + 2 * 64 and max(v["paths"] for v in m.values()) == m["groups_1024"]["paths"]
    assert RN.spp_of(g("spp_16384")) == 16384 and m["spp_16384"]["tiles"] == 2 and m["spp_16384"]["paths"] == 2 * 16384
    c = g("far_corner")
    assert (c["p"].width, c["p"].height) == (8192, 3) and (c["tiles"][:, 0] + c["tiles"][:, 2]).max() == 8192
    c = g("far_bottom")
    assert (c["p"].width, c["p"].height) == (3, 8192) and (c["tiles"][:, 1] + c["tiles"][:, 3]).max() == 8192
    c = g("packed")
    assert c["tiles"][:, 7].all() and len(set(c["tiles"][:, 6].tolist())) == 3
    assert not any(g(n)["tiles"][:, 7].any() for n in RC.NAMES if n != "packed")
    # the sampler's edges: every class of sum is there, at hundreds of (path, set) positions
    f = m["fract_edges"]
    for k in ("nan_sums", "inf_sums", "sum_one", "sum_below_one", "sum_above_one", "sum_negative", "sum_neg_zero", "sum_subnormal", "sum_big"):
        assert f[k] >= 25, (k, f[k])
    scr = g("fract_edges")["tabs"][2]
    for v in (0.0, -0.0, 1.0 - 2.0 ** -24, 1.0):
        assert (scr.view(np.uint32) == f32(v).view(np.uint32)).sum() >= 3, v
    assert sum(m[n]["nan_sums"] + m[n]["inf_sums"] + m[n]["sum_negative"] for n in RC.NAMES if n != "fract_edges") == 0
    # the filter's edges
    f = m["fis_edges"]
    assert f["u_half"] >= 50 and f["index_510"] >= 100 and f["index_0"] >= 100 and f["t_zero"] >= 500, f
    assert len(RC.exact_index_us()) >= 100
    fis = g("fis_edges")["tabs"][3]
    assert fis[0] != 0 and np.unique(fis).size == 512 and (np.diff(fis) < 0).sum() > 100 and np.array_equal(fis, g("fis_tables_custom")["tabs"][3])
    tabs = [g(n)["tabs"][3] for n in RC.FILTERS]
    assert all(not np.array_equal(a, b) for i, a in enumerate(tabs) for b in tabs[:i]) and len(tabs) == 4
    # time and camera
    assert g("time_static")["wd"].camera.animated == 0
    assert g("time_zero_range")["p"].time_start == g("time_zero_range")["p"].time_end and g("time_zero_range")["wd"].camera.animated
    assert g("time_negative_range")["p"].time_end < g("time_negative_range")["p"].time_start and g("time_offset")["p"].time_start == 3.25
    seen = {(g(n)["wd"].camera.kind, g(n)["wd"].camera.animated) for n in RC.NAMES if n.startswith("anim_")}
    assert seen == {(0, b) for b in (1, 2, 4, 7)} | {(2, b) for b in (1, 2, 4, 7)} | {(1, b) for b in (1, 2, 4, 8, 15)}
    c = g("thin_lens_sets")
    spp, s2 = RN.spp_of(c), c["tabs"][1]
    assert c["wd"].camera.kind == 1 and c["wd"].camera.aperture > 0 and (s2[:2 * spp] != s2[2 * spp:4 * spp]).all()
    lens_centre = 0
    for t in range(len(c["tiles"])):
        xs, ys, s = RN.slot_paths(c, t)
        sc = c["tabs"][2][xs + ys * int(c["p"].width)]
        lens_centre += int(((RN.RS.fract(s2[2 * s + 2 * spp] + sc) == 0.5) & (RN.RS.fract(s2[1 + 2 * s + 2 * spp] + sc) == 0.5)).sum())
    print("thin_lens_sets: paths at a == 0 && b == 0", lens_centre)
    assert lens_centre >= 50
    assert {(g(n)["p"].volume_marches, g(n)["p"].max_bounces) for n in RC.NAMES if n.startswith("records_")} == {(v, b) for v in (2, 3, 4) for b in (0, 1, 8, 120)}
    c = g("records_vm4_b120")
    assert np.array_equal(c["tabs"][0], np.arange(c["tabs"][0].size)) and np.array_equal(c["tabs"][1], np.arange(c["tabs"][1].size)) and c["tabs"][1].size < 2 ** 24


@pytest.mark.parametrize("name", RC.NAMES)
def test_case_kills_the_wrong_statements_it_names(name):
    c = RC.get(name)
    right = RN.reference(c)
    for mut in c["kills"]:
        wrong = RN.reference(c, mutant=mut)
        d = RN.differing(wrong, right)
        share = RN.changed_paths(right, wrong)
        print(name, mut, "paths changed %.3f" % share, {k: v for k, v in d.items() if v})
        seen = {k: v for k, v in d.items() if c["only"] is None or k in c["only"]}
        assert sum(seen.values()) > 0, (name, mut)
        if mut in RC.SHARE_MUTANTS:
            assert share >= 0.10, (name, mut, share)


def test_every_mutant_is_named():
    named = {m for n in RC.NAMES for m in RC.get(n)["kills"]}
    assert named == set(RN.MUTANTS), set(RN.MUTANTS) ^ named
    for n in RC.NAMES:  # the cases the issue names for a mutant do name it
        k = RC.get(n)["kills"]
        if n.startswith("anim_") or n in ("time_negative_range", "time_offset"):
            assert "own_lane_time" in k
        if n.startswith("records_") and RC.get(n)["p"].max_bounces:
            assert "records_depth_off" in k
    assert "lens_set0" in RC.get("thin_lens_sets")["kills"] and {"clamp_one", "mult_le0"} <= set(RC.get("fis_edges")["kills"])
    assert "ew_for_eh" in RC.get("wide_32x4")["kills"] and "ew_for_eh" in RC.get("tall_4x32")["kills"] and "ew_for_eh" in RC.get("edge_21x13_spp4")["kills"]
    assert "pix_transposed" in RC.get("far_corner")["kills"] and "no_half" in RC.get("one_pixel")["kills"]


@pytest.mark.parametrize("vm", [0, 1, 2, 3, 4])
def test_records_statement_equals_the_plain_fetch(vm):
    """src/film.rs:568-587 as a loop, at every volume_marches the reference can be built with (the ABI takes 2..4) and a depth-120 frame"""
    spp, B = 4, 120 if vm in (0, 4) else 3
    n1, n2 = 3 + vm, 12 + 8 * vm
    s1, s2 = np.arange(spp * (1 + (B + 1) * n1), dtype=f32), np.arange(spp * 2 * (2 + (B + 1) * n2), dtype=f32)

    class Pp:
        samples, volume_marches, max_bounces = 1, vm, B
    rec = RN.records({"p": Pp, "tabs": (s1, s2)})
    assert rec.shape == ((B + 1) * spp, 8 + n2)
    for depth in (0, 1, B):
        for s in range(spp):
            want = [s1[s + spp * (1 + k + depth * n1)] for k in range(n1)] + [0.0] * (8 - n1)
            for i in range(n2):
                dim, set_ = i % 2, i // 2
                want.append(s2[dim + s * 2 + spp * 2 * (2 + set_ + depth * n2 // 2)])
            assert rec[depth * spp + s].tolist() == want
    assert rec.max() == spp * 2 * (2 + (B + 1) * n2 // 2) - 1  # the last record ends at set 2 + (B + 1) * n2 / 2: the reference requests twice the 2-D sets it reads
