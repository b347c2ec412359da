"""numpy restatement of the variance-guided a-trous denoiser of a progressive render's Color channel (rayn_hip_denoise_variance_device,
include/rayn_hip.h; the spatial half of SVGF, Schied et al., HPG 2017), operation by operation in float32, so that the tests can compare
the kernels with it bit for bit.  expf is the pinned dm_expf of include/rayn_detmath.h, evaluated by the oracle (denoise_np.oracle_expf).
dtype=np.float64 reads the same formula in float64 with numpy's exp (a cross-check of the float32 reading, not bit-exact); the initial
variance is an input of the filter and stays the float32 value in both readings."""
import numpy as np

from denoise_np import H_TAPS, oracle_expf
from progressive_np import tile_rects

LUMA = (0.2126, 0.7152, 0.0722)
# Wrong readings, for tests/post_edge_cases.py (mutant=None: the definition's bits).  Of the initial variance - v_gt0: guided needs
# v > 0; fnn_u32: n (n - 1) in 32 bits before the conversion.  Of the passes - border_le: a tap one step beyond the last row or column
# still counts (it reads the edge pixel), in the 5x5 stencil and in the 3x3 pre-filter; nan_weight_counts: a tap whose weight is NaN is
# added like any other.
# zero_weight_skipped: a tap of weight 0 is left out, where the definition adds its +0 (a sum of -0.0 becomes +0).
# prefilter_counts_unguided: the 3x3 pre-filter of the variance adds a neighbour that is not guided (its v is NaN) like any other.
MUTANTS = ("v_gt0", "fnn_u32", "border_le", "nan_weight_counts", "zero_weight_skipped", "prefilter_counts_unguided")
# n_ge1 (a tile with ONE epoch may be guided): n = 1 divides m2 by (float)0 = +0, which gives an infinity or a NaN for every m2, and a v
# that is not finite is not guided: the reading changes no bit.  (In the accumulate kernel the same reading computes
# e = sqrtf(m2 / 0) / ...: after one epoch m2 is +0 or NaN - d (y - mean) with mean = y - so e is NaN, in neither count: equivalent too.)
EQUIVALENT = ("n_ge1",)
K3 = ((1.0 / 16.0, 1.0 / 8.0, 1.0 / 16.0), (1.0 / 8.0, 1.0 / 4.0, 1.0 / 8.0), (1.0 / 16.0, 1.0 / 8.0, 1.0 / 16.0))  # [dy + 1][dx + 1]


def initial_variance(color, m2, epochs, width, height, tile_size, mutant=None):
    """v_p = m2 / (float)((uint64)n (n - 1)) in f32 for the guided pixels, NaN for the others: pixels in no tile of the reference's
    (x-major, possibly under-covering) grid, tiles with n < 2, a v that is not finite or negative, a colour with a non-finite component.
    color (n, 3), m2 (n) in film pixel order, epochs per tile in the reference's tile order."""
    w, h = int(width), int(height)
    c = np.asarray(color, np.float32).reshape(h * w, 3)
    m2 = np.asarray(m2, np.float32).reshape(h, w)
    v = np.full((h, w), np.nan, np.float32)
    rects = tile_rects(w, h, int(tile_size[0]), int(tile_size[1]))
    epochs = np.asarray(epochs).reshape(-1)
    assert len(epochs) == len(rects)
    with np.errstate(all="ignore"):
        for n, (x0, y0, x1, y1) in zip(epochs, rects):
            n = int(n)
            if n < (1 if mutant == "n_ge1" else 2):
                continue
            fnn = np.array(n * (n - 1) & (0xFFFFFFFF if mutant == "fnn_u32" else ~0), np.uint64).astype(np.float32)  # the C cast: one rounding
            v[y0:y1, x0:x1] = m2[y0:y1, x0:x1] / fnn
        v = v.reshape(-1)
        guided = np.isfinite(v) & ((v > 0) if mutant == "v_gt0" else (v >= 0)) & np.isfinite(c).all(-1)
    return np.where(guided, v, np.float32(np.nan)).astype(np.float32)


def _shift(ys, xs, dy, dx, h, w, mutant=None):
    qy, qx = ys + dy, xs + dx
    inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
    if mutant == "border_le":
        inside = (qy >= 0) & (qy <= h) & (qx >= 0) & (qx <= w)
    return inside, np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)


def atrous(color, alpha, normal, v0, width, height, iterations, sigma_luminance, sigma_normal, sigma_alpha, dtype=np.float32, mutant=None):
    """The passes on the initial variance v0 (n floats, NaN = not guided; initial_variance).  color / normal: width * height * 3 floats,
    alpha: width * height floats; a guide whose sigma is 0 is not read and may be None.  Returns (colour (n, 3), variance (n)); the
    variance of a pixel that is not guided is NaN."""
    f = np.dtype(dtype).type
    expf = oracle_expf if f is np.float32 else np.exp
    w, h = int(width), int(height)
    c = np.asarray(color, np.float32).reshape(h, w, 3).astype(f)
    v = np.asarray(v0, np.float32).reshape(h, w).astype(f)
    use_l, use_n, use_a = sigma_luminance != 0, sigma_normal != 0, sigma_alpha != 0
    n = np.asarray(normal, np.float32).reshape(h, w, 3).astype(f) if use_n else None
    a = np.asarray(alpha, np.float32).reshape(h, w).astype(f) if use_a else None
    # the C entry takes the sigmas as f32; 1 / sigma^2 is evaluated in the working precision
    sl, sn, sa = (f(np.float32(s)) for s in (sigma_luminance, sigma_normal, sigma_alpha))
    kn = f(1.0) / (sn * sn) if use_n else None
    ka = f(1.0) / (sa * sa) if use_a else None
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    # the constants are the float32 ones in both readings, as the film and the state are
    luma = [f(np.float32(k)) for k in LUMA]
    with np.errstate(all="ignore"):
        for i in range(int(iterations)):
            step = 1 << i
            guided = ~np.isnan(v)
            lum = (luma[0] * c[..., 0] + luma[1] * c[..., 1]) + luma[2] * c[..., 2]
            if use_l:
                num, den = f(0.25) * v, np.full((h, w), f(0.25), f)
                for dy in range(-1, 2):
                    for dx in range(-1, 2):
                        if dx == 0 and dy == 0:
                            continue
                        inside, qy, qx = _shift(ys, xs, dy, dx, h, w, mutant)
                        ok = inside if mutant == "prefilter_counts_unguided" else inside & guided[qy, qx]
                        k = f(K3[dy + 1][dx + 1])
                        num = np.where(ok, num + k * v[qy, qx], num)
                        den = np.where(ok, den + k, den)
                inv = f(1.0) / (sl * np.sqrt(num / den) + f(np.float32(1e-8)))
            W0 = f(9.0 / 64.0)
            W = np.full((h, w), W0, f)
            S = W0 * c
            V = (W0 * W0) * v
            for ky in range(-2, 3):
                for kx in range(-2, 3):
                    if kx == 0 and ky == 0:
                        continue
                    inside, qy, qx = _shift(ys, xs, ky * step, kx * step, h, w, mutant)
                    ok = inside & guided[qy, qx]
                    cq, vq = c[qy, qx], v[qy, qx]
                    e = np.zeros((h, w), f)
                    if use_l:
                        e = e + np.abs(lum - lum[qy, qx]) * inv
                    if use_n:
                        d = n - n[qy, qx]
                        e = e + ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * kn
                    if use_a:
                        d = a - a[qy, qx]
                        e = e + (d * d) * ka
                    wt = f(H_TAPS[ky + 2] * H_TAPS[kx + 2]) * expf(-e).astype(f)
                    if mutant != "nan_weight_counts":
                        ok &= ~np.isnan(wt)
                    if mutant == "zero_weight_skipped":
                        ok &= wt != 0
                    W = np.where(ok, W + wt, W)
                    S = np.where(ok[..., None], S + wt[..., None] * cq, S)
                    V = np.where(ok, V + (wt * wt) * vq, V)
            c_new = S / W[..., None]
            v_new = V / (W * W)
            v_new = np.where(np.isfinite(c_new).all(-1) & np.isfinite(v_new), v_new, f(np.nan))  # an overflow: not guided from here on
            c = np.where(guided[..., None], c_new, c)  # a pixel that is not guided passes through unchanged
            v = np.where(guided, v_new, v)
    return c.reshape(h * w, 3), v.reshape(h * w)


def denoise(color, alpha, normal, m2, epochs, width, height, tile_size, iterations, sigma_luminance, sigma_normal, sigma_alpha, dtype=np.float32,
            mutant=None):
    """The whole entry: the initial variance from the progressive state's m2 and per-tile epoch counts, then the passes."""
    v0 = initial_variance(color, m2, epochs, width, height, tile_size, mutant)
    return atrous(color, alpha, normal, v0, width, height, iterations, sigma_luminance, sigma_normal, sigma_alpha, dtype, mutant)
