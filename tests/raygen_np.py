"""A numpy statement of the ray-generation stage on the inputs of rayn_hip_probe_raygen: what k_batch_setup, k_raygen and k_pack_tables have to leave behind.
Written from the definition - the tile closure's ray-gen loop (src/film.rs:456-529), Samples::sample_* (src/sampler.rs), FilterImportanceSampler::sample
(src/filter.rs:222-235), the per-bounce sample fetch (src/film.rs:568-587) - and from the pool layout DESIGN.md states, not from the kernels:
  - the rays themselves are restatement_np.raygen, the function restatement_np.render builds its films from;
  - a tile's paths lie in its pool segment in the loop's order (x outer, y inner, sample innermost), the segment is padded to whole 64-slot groups;
  - a path slot starts as WRay::new left it (radiance 0, throughput 1, no hit, no emitted sample); a padding slot is only marked empty;
  - the packed record of (depth, sample) holds that depth's 1-D sets 1 + k + depth * n1 and 2-D sets 2 + c / 2 + depth * n2 / 2.
MUTANTS names the wrong readings the cases of tests/raygen_cases.py have to tell from the statement.  TEST INFRASTRUCTURE."""
import numpy as np

import restatement_np as RS

f32 = np.float32
INVALID, OBJ_NONE, TERM_NONE = 0xFFFFFFFF, 0xFF, 0xFF
SENTINEL, SURPLUS = 0xC0FFEE5A, 128
PLANES = ("geo0", "geo1", "col0", "col1", "aov")
WORDS = ("term_key", "term_info", "q", "pgrp_tile", "tgb", "tgc")
CTL = ("q_groups", "q_valid", "b_groups", "b_valid", "head_extend", "job_count", "head_shadow", "overflow")
MUTANTS = ("ew_for_eh",          # lx = lpix / ew, ly = lpix % ew
           "own_lane_time",      # an animated camera evaluated at the lane's own time
           "time_word_lane0",    # the ray's time word = lane 0's time
           "lens_set0",          # the thin lens reads 2-D set 0
           "no_half",            # pixel centre without + 0.5
           "pix_transposed",     # pix = y + x * height
           "clamp_one",          # |u| clamped at 1.0, not 0.99999
           "mult_le0",           # the sign from u <= 0
           "lerp_swapped",       # the inverse CDF's two entries exchanged in the lerp
           "records_depth_off")  # the packed record of depth d holds the sets of depth d + 1


def spp_of(case):
    return 4 * int(case["p"].samples)


def slot_paths(case, t, mutant=None):
    """pixel and sample of every path slot of tile t, in slot order -> (xs, ys, s)"""
    x0, y0, ew, eh, _base, n_paths = [int(v) for v in case["tiles"][t][:6]]
    spp, W, H = spp_of(case), int(case["p"].width), int(case["p"].height)
    p = np.arange(n_paths, dtype=np.int64)
    s, lpix = p % spp, p // spp
    div = ew if mutant == "ew_for_eh" else eh
    xs, ys = x0 + lpix // div, y0 + lpix % div
    if mutant == "ew_for_eh":
        xs, ys = xs % W, ys % H  # the wrong reading leaves the tile (and may leave the film)
    return xs, ys, s


def loop_paths(case, t):
    """the ray-gen loop's own order: for x { for y { for samp { 4 lanes } } }"""
    x0, y0, ew, eh = [int(v) for v in case["tiles"][t][:4]]
    xs, ys, sn = np.meshgrid(np.arange(x0, x0 + ew), np.arange(y0, y0 + eh), np.arange(spp_of(case)), indexing="ij")
    return xs.reshape(-1), ys.reshape(-1), sn.reshape(-1)


def tile_rays(case, t, fma=False, mutant=None):
    """the statement's rays of tile t in slot order: origin, dir [n, 3], time [n] float32, pixel, sample [n] uint32"""
    p, cam = case["p"], case["wd"].camera
    xs, ys, s = slot_paths(case, t, mutant)
    with RS.fused_policy(fma):
        r = RS.raygen(cam, int(p.width), int(p.height), spp_of(case), p.time_start, p.time_end, case["tabs"], xs, ys, s, mutant)
    time = r["time"]
    if mutant == "time_word_lane0":
        with RS.fused_policy(fma):
            time = RS.raygen(cam, int(p.width), int(p.height), spp_of(case), p.time_start, p.time_end, case["tabs"], xs, ys, (s // 4) * 4)["time"]
    return {"origin": np.stack(r["o"], 1).astype(f32), "dir": np.stack(r["d"], 1).astype(f32), "time": time.astype(f32),
            "pixel": r["pix"].astype(np.uint32), "sample": s.astype(np.uint32)}


def groups_of(case):
    """-> (first group, group count) of every tile's 64-padded segment"""
    tiles = case["tiles"].astype(np.int64)
    return tiles[:, 4] // 64, (tiles[:, 5] + 63) // 64


def padding_share(case):
    return 1.0 - float(case["tiles"][:, 5].astype(np.int64).sum()) / case["n_pool"]


def records(case, mutant=None):
    """[(max_bounces + 1) * spp, 8 + n2]: the per-bounce fetch of src/film.rs:568-587 as the tables hold it (the scramble is added by the reader)"""
    s1d, s2d = [np.asarray(t, f32) for t in case["tabs"][:2]]
    spp, VM, depths = spp_of(case), int(case["p"].volume_marches), int(case["p"].max_bounces) + 1
    n1, n2 = 3 + VM, 12 + 8 * VM
    out = np.zeros((depths, spp, 8 + n2), f32)
    s = np.arange(spp)
    for depth in range(depths):
        d = (depth + 1) % depths if mutant == "records_depth_off" else depth
        for k in range(n1):
            out[depth, :, k] = s1d[s + spp * (1 + k + d * n1)]
        for c in range(n2):
            out[depth, :, 8 + c] = s2d[c % 2 + s * 2 + spp * 2 * (2 + c // 2 + d * n2 // 2)]
    return out.reshape(depths * spp, 8 + n2)


def reference(case, rays=None, fma=False, mutant=None, sentinel=SENTINEL, surplus=SURPLUS):
    """Everything rayn_hip_probe_raygen returns, as the stage has to leave it.  rays = per tile the dict of tile_rays (default: the statement's own; the
    tests pass the oracle's export, which is in the same order)."""
    n_pool, tiles = case["n_pool"], case["tiles"]
    NP, nt = n_pool + surplus, len(tiles)
    out = {k: np.full((NP, 4), sentinel, np.uint32) for k in PLANES}
    out["term_key"], out["q"] = np.full(NP, sentinel, np.uint32), np.full(NP, sentinel, np.uint32)
    out["term_info"] = np.full(NP, sentinel & 0xFF, np.uint8)
    out["pgrp_tile"], out["tgb"], out["tgc"] = np.full(NP // 64, sentinel, np.uint32), np.full(nt + 2, sentinel, np.uint32), np.full(nt + 2, sentinel, np.uint32)
    out["padding"], out["path"] = np.zeros(NP, bool), np.zeros(NP, bool)
    g0, gc = groups_of(case)
    bits = lambda a: np.ascontiguousarray(a, f32).view(np.uint32)
    for t in range(nt):
        r = rays[t] if rays is not None else tile_rays(case, t, fma, mutant)
        base, n = int(tiles[t][4]), int(tiles[t][5])
        seg = slice(base, base + int(gc[t]) * 64)
        out["pgrp_tile"][g0[t]:g0[t] + gc[t]] = t
        out["tgb"][t], out["tgc"][t] = g0[t], gc[t]
        out["term_info"][seg] = TERM_NONE
        out["aov"][seg] = (0, 0, 0, OBJ_NONE)
        out["q"][seg] = INVALID
        out["padding"][base + n:seg.stop] = True
        P = slice(base, base + n)
        out["path"][P] = True
        out["q"][P] = np.arange(base, base + n, dtype=np.uint32)
        out["geo0"][P, 0:3], out["geo0"][P, 3] = bits(r["origin"]), bits(r["dir"][:, 0])
        out["geo1"][P, 0:2], out["geo1"][P, 2], out["geo1"][P, 3] = bits(r["dir"][:, 1:3]), 0, OBJ_NONE | (r["sample"].astype(np.uint32) << 8)
        out["col0"][P] = bits(np.array([0, 0, 0, 1], f32))
        out["col1"][P, 0:2], out["col1"][P, 2], out["col1"][P, 3] = bits(np.array([1, 1], f32)), r["pixel"], bits(r["time"])
    out["ctl"] = dict.fromkeys(CTL, sentinel)
    out["ctl"].update(q_groups=n_pool // 64, q_valid=n_pool, head_extend=0)  # q_valid: the pool size, padding included (kernels.h)
    out["records"] = records(case, mutant)
    return out


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def differing(got, want):
    """per output the number of differing words; in the float planes and the records two NaNs are equal whatever their bits (common.bits_equal)"""
    d = {}
    for k in PLANES + ("records",):
        x, y = words(got[k]).reshape(-1), words(want[k]).reshape(-1)
        if x.shape != y.shape:
            d[k] = max(x.size, y.size)
            continue
        nan = np.isnan(x.view(f32)) & np.isnan(y.view(f32))
        d[k] = int(((x != y) & ~nan).sum())
    for k in WORDS:
        d[k] = int((np.asarray(got[k]) != np.asarray(want[k])).sum()) if np.asarray(got[k]).shape == np.asarray(want[k]).shape else -1
    d["ctl"] = sum(got["ctl"][k] != want["ctl"][k] for k in CTL)
    return d


def changed_paths(a, b):
    """the share of path slots in which the two pool states differ in any plane word"""
    diff = np.zeros(a["path"].size, bool)
    for k in PLANES:
        x, y = a[k], b[k]
        nan = np.isnan(x.view(f32)) & np.isnan(y.view(f32))
        diff |= ((x != y) & ~nan).any(axis=1)
    return float(diff[a["path"]].mean())
