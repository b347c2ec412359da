"""numpy restatement of the guided upscaling (rayn_hip_upscale_device; the definition is in include/rayn_hip.h), operation by operation in
float32 and tap by tap in the definition's order, so that the tests can compare the kernel with it bit for bit; only the pixels are
vectorised.  expf is the pinned dm_expf of include/rayn_detmath.h, evaluated by the oracle (denoise_np.oracle_expf).  dtype=np.float64
reads the same formulas in float64 with numpy's exp: a cross-check of the definition, not bit-exact.  It shares no code with
rayn_amd/csrc/upscale.hip.  TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this.

MUTANTS names the wrong readings of one decision each that tests/reproject_cases.py tells from the statement (upscale(..., mutant=);
mutant=None is the statement)."""
import numpy as np

from denoise_np import oracle_expf

MISS = np.uint32(0xFFFFFFFF)
MUTANTS = ("weight_ge",          # a tap of bilinear weight b == 0 is used (b >= 0)
           "nan_weight_counts",  # a NaN guided weight is added instead of skipped
           "tier1_any_match",    # tier 1 is taken as soon as a tap matched, even with Wg == 0 (every expf(-e) underflowed)
           "tier2_skipped")      # a failed tier 1 falls straight to tier 3
PLANES = (("color", 3), ("alpha", 1), ("background", 3), ("normal", 3))


def upscale(film, low_g, high_g, width, height, factor, sigma_plane, sigma_position, dtype=np.float32, bilinear=False, mutant=None):
    """film: {"color": (n, 3), "alpha": (n,), "background": (n, 3), "normal": (n, 3)} of the width x height low film, pixel x + y * width;
    alpha / background / normal may be absent (normal only with sigma_plane == 0).  low_g / high_g: (records (., 4), objects (.,)) of the
    G-buffers at the low and at the high resolution.  bilinear: take tier 2 (the unguided weights) for every pixel, whatever the guides
    say - the plain bilinear reading of the film.  Returns (planes dict of the high film, weight (N,), tier (N,) uint8 in 1..3, the
    largest exponent e of a tap that counted)."""
    assert mutant is None or mutant in MUTANTS, mutant
    f = np.dtype(dtype).type
    expf = oracle_expf if f is np.float32 else np.exp
    w, h, s = int(width), int(height), int(factor)
    W, H = w * s, h * s
    n, N = w * h, W * H
    src = {k: np.asarray(film[k], np.float32).reshape(n, c) for k, c in PLANES if film.get(k) is not None}
    val = {k: v.astype(f) for k, v in src.items()}
    lrec, lobj = np.asarray(low_g[0], np.float32).reshape(n, 4).astype(f), np.asarray(low_g[1]).reshape(n).astype(np.uint32)
    hrec, hobj = np.asarray(high_g[0], np.float32).reshape(N, 4).astype(f), np.asarray(high_g[1]).reshape(N).astype(np.uint32)
    sp, ss = f(np.float32(sigma_plane)), f(np.float32(sigma_position))  # the C entry takes the sigmas as f32
    use_p, use_s = sigma_plane != 0, sigma_position != 0
    Xi, Yi = np.meshgrid(np.arange(W), np.arange(H), indexing="xy")
    Xi, Yi = Xi.reshape(-1), Yi.reshape(-1)
    fin_low = np.isfinite(src["color"]).all(axis=1)

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    with np.errstate(all="ignore"):
        fx = (Xi.astype(f) + f(0.5)) / f(s) - f(0.5)
        fy = (Yi.astype(f) + f(0.5)) / f(s) - f(0.5)
        x0f, y0f = np.floor(fx), np.floor(fy)
        wx1, wy1 = fx - x0f, fy - y0f
        wx0, wy0 = f(1.0) - wx1, f(1.0) - wy1
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        hit = hobj != MISS
        inv_t = f(1.0) / (hrec[:, 3] + f(1e-8))
        kp = f(1.0) / (sp * sp) if use_p else None
        ks = f(1.0) / (ss * ss) if use_s else None

        def sums():
            return np.full(N, -0.0, f), {k: np.full((N, v.shape[1]), -0.0, f) for k, v in val.items()}  # -0.0f: the identity of + for both zeros

        def taps():
            for k in range(4):
                qx, qy = x0 + (k & 1), y0 + (k >> 1)
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                q = np.where(inside, qx + qy * w, 0)
                b = (wx1 if k & 1 else wx0) * (wy1 if k >> 1 else wy0)
                yield q, b, inside & (b >= 0 if mutant == "weight_ge" else b > 0) & fin_low[q]

        def add(use, g, q, Wt, St):
            Wt = np.where(use, Wt + g, Wt)
            for key in St:
                St[key] = np.where(use[:, None], St[key] + g[:, None] * val[key][q], St[key])
            return Wt

        emax = 0.0
        matched = np.zeros(N, bool)
        Wg, Sg = sums()
        if not bilinear:
            for q, b, usable in taps():
                match = usable & (lobj[q] == hobj)
                d = [hrec[:, c] - lrec[q, c] for c in range(3)]
                e = np.zeros(N, f)
                if use_p:
                    nq = val["normal"][q]
                    dpl = np.abs(dot([nq[:, 0], nq[:, 1], nq[:, 2]], d)) * inv_t
                    e = (dpl * dpl) * kp
                if use_s:
                    dps = dot(d, d) * (inv_t * inv_t)
                    e = e + dps * ks if use_p else dps * ks
                g = np.where(hit, b * expf(-e).astype(f), b)
                use = match if mutant == "nan_weight_counts" else match & ~np.isnan(g)
                matched |= use
                if (use & hit).any():
                    emax = max(emax, float(np.max(e[use & hit])))
                Wg = add(use, g, q, Wg, Sg)
        Wb, Sb = sums()
        for q, b, usable in taps():
            Wb = add(usable, b, q, Wb, Sb)
        t1 = matched if mutant == "tier1_any_match" else Wg > 0
        t2 = ~t1 & (Wb > 0) & (mutant != "tier2_skipped")
        qc = np.minimum(Xi // s, w - 1) + np.minimum(Yi // s, h - 1) * w
        out = {}
        for key in val:
            a = np.where(t1[:, None], Sg[key] / Wg[:, None], Sb[key] / Wb[:, None]).astype(np.float32)
            a[~(t1 | t2)] = src[key][qc][~(t1 | t2)]  # verbatim: the float32 bits of the low film
            out[key] = a if a.shape[1] == 3 else a[:, 0]
        weight = np.where(t1, Wg, f(0.0)).astype(np.float32)
    tier = np.where(t1, 1, np.where(t2, 2, 3)).astype(np.uint8)
    return out, weight, tier, emax
