"""The film resolve (Tile::add_sample + tile_finished; k_resolve_reg / k_resolve_blk / k_resolve_huge of rayn_amd/csrc/kernels.hip) stated in numpy,
on the inputs of rayn_hip_probe_resolve.  Written from the definition, not from the kernels - no sort network, no packed key, no shortcut:

  per pixel of every tile, film index = film_base + lpix when the tile is packed, else (x0 + lpix // eh) + (y0 + lpix % eh) * width;
  Color / Background: the contributing samples (term_info != 0xFF) in ascending (depth, slot) order; Color = the strictly sequential binary32 sum, from
      +0.0, of those without the Background flag, divided by float32(spp); Background likewise over the flagged ones;
  Alpha: the number of samples whose object word is not OBJ_NONE, divided by spp;
  WorldNormal: the sequential sum of those samples' xyz in (object, sample index) order, divided by spp.

The sums are np.add.accumulate(dtype=float32) along the sample axis (sequential; np.sum adds pairwise).  A term that does not belong to a sum is replaced
by +0.0: a chain that starts at +0.0 never holds -0.0 (x + -x and +0.0 + -0.0 are +0.0 under round-to-nearest), so adding +0.0 changes nothing.
tests/test_resolve.py checks this file against a plain loop over np.float32 scalars that skips those terms instead.

reference(case, mutant=...) also states the WRONG resolves the cases must tell from the right one (MUTANTS).
Shared by tests/test_resolve.py (CPU) and tests/test_resolve_device.py (the kernels)."""
import numpy as np

OBJ_NONE = 0xFF
TERM_NONE = 0xFF
KEY_SHIFT = 25  # k_resolve_blk's 32-bit key: depth:7 | offset:25
PLANES = (("color", 3), ("alpha", 1), ("background", 3), ("normal", 3))
MUTANTS = ("sample_order", "slot_major", "signed_key32", "ignore_bg", "normal_sample_order", "swap_lx_ly", "flush_subnormals")
ORDER_MUTANTS = ("sample_order", "slot_major", "signed_key32", "normal_sample_order")


def family(spp):
    """the kernel launch_resolve picks for spp"""
    if spp <= 512:
        return "reg<%d>" % (1 if spp <= 64 else 2 if spp <= 128 else 4 if spp <= 256 else 8)
    if spp <= 4096:
        return "blk<%d,8>" % (128 if spp <= 1024 else 256 if spp <= 2048 else 512)
    return "huge"


def tile_pixels(case):
    """(tile index, lpix, first pool slot, film index) of every tile pixel, tile after tile"""
    spp, width = case["spp"], case["width"]
    out = []
    for t, (x0, y0, ew, eh, pool_base, _n, film_base, packed) in enumerate(case["tiles"].tolist()):
        for lpix in range(ew * eh):
            fi = film_base + lpix if packed else (x0 + lpix // eh) + (y0 + lpix % eh) * width
            out.append((t, lpix, pool_base + lpix * spp, fi))
    return out


def _flush(a):
    a = a.copy()
    a[np.abs(a) < np.float32(2.0 ** -126)] = 0.0
    return a


def _seq_sum(v):
    """strictly sequential binary32 sum along axis 1 of (pixels, terms, channels), from +0.0"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.add.accumulate(v, axis=1, dtype=np.float32)[:, -1]


def pixel_terms(case, mutant=None):
    """Per tile pixel, the summation inputs: (col [npix, spp, 3] in summation order, is_color, is_bg [npix, spp]; nrm [npix, spp, 3] in its order, has_obj)."""
    spp = case["spp"]
    px = tile_pixels(case)
    idx = np.array([p[2] for p in px], np.int64)[:, None] + np.arange(spp, dtype=np.int64)[None, :]
    tile = np.array([p[0] for p in px], np.int64)[:, None]
    info = case["term_info"][idx].astype(np.uint64)
    live = info != TERM_NONE
    depth, bg = info & np.uint64(0x7F), (info >> np.uint64(7)) == 1
    slot = case["term_key"][idx].astype(np.uint64)
    last = np.uint64(0xFFFFFFFFFFFFFFFF)
    if mutant == "sample_order":
        key = np.broadcast_to(np.arange(spp, dtype=np.uint64), idx.shape).copy()
    elif mutant == "slot_major":
        key = (slot << np.uint64(7)) | depth
    elif mutant == "signed_key32":  # the 32-bit key of k_resolve_blk compared as int32: depths >= 64 sort first
        base = case["base_hist"][depth.astype(np.int64) * live, tile].astype(np.uint64) if case["base_hist"] is not None else np.uint64(0)
        k32 = ((depth << np.uint64(KEY_SHIFT)) | ((slot - base) & np.uint64((1 << KEY_SHIFT) - 1))).astype(np.uint32)
        key = (k32.view(np.int32).astype(np.int64) + (1 << 31)).astype(np.uint64)
    else:
        key = (depth << np.uint64(32)) | slot
    key = np.where(live, key, last)
    order = np.argsort(key, axis=1, kind="stable")
    take = lambda a: np.take_along_axis(a, order, axis=1)
    col = case["col0"][idx][np.arange(idx.shape[0])[:, None], order]
    live_s, bg_s = take(live), take(bg)
    if mutant == "ignore_bg":
        bg_s = np.zeros_like(bg_s)
    obj = case["obj"][idx]
    has = obj != OBJ_NONE
    okey = np.where(has, obj.astype(np.uint64), last)
    if mutant == "normal_sample_order":
        okey = np.where(has, np.uint64(0), last)
    oorder = np.argsort(okey, axis=1, kind="stable")  # stable: sample order inside an object
    nrm = case["aov"][idx][np.arange(idx.shape[0])[:, None], oorder]
    has_s = np.take_along_axis(has, oorder, axis=1)
    if mutant == "flush_subnormals":
        col, nrm = _flush(col), _flush(nrm)
    return px, col, live_s & ~bg_s, live_s & bg_s, nrm, has_s


def reference(case, sentinel=0, mutant=None):
    """The four planes as float32 arrays of out_pixels pixels ("color" [N, 3], "alpha" [N], "background" [N, 3], "normal" [N, 3]) + "owned" [N] bool;
    a pixel no tile owns holds the word `sentinel`.  With the swap_lx_ly mutant the planes grow as far as its film indices reach."""
    spp = case["spp"]
    px, col, is_c, is_b, nrm, has = pixel_terms(case, mutant)
    n = np.float32(spp)
    zero = np.float32(0.0)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        color = _seq_sum(np.where(is_c[:, :, None], col, zero)) / n
        background = _seq_sum(np.where(is_b[:, :, None], col, zero)) / n
        normal = _seq_sum(np.where(has[:, :, None], nrm, zero)) / n
        alpha = has.sum(axis=1).astype(np.float32) / n
    if mutant == "flush_subnormals":
        color, background, normal = _flush(color), _flush(background), _flush(normal)
    fi = np.array([p[3] for p in px], np.int64)
    if mutant == "swap_lx_ly":
        tiles = case["tiles"].tolist()
        fi = np.array([f if tiles[t][7] else (tiles[t][0] + lpix % tiles[t][3]) + (tiles[t][1] + lpix // tiles[t][3]) * case["width"] for t, lpix, _p, f in px], np.int64)
    N = max(case["out_pixels"], int(fi.max()) + 1)
    out = {}
    for name, ch in PLANES:
        out[name] = np.full((N, ch) if ch > 1 else (N,), sentinel, np.uint32).view(np.float32)
    out["color"][fi], out["alpha"][fi], out["background"][fi], out["normal"][fi] = color, alpha, background, normal
    out["owned"] = np.zeros(N, bool)
    out["owned"][fi] = True
    return out
