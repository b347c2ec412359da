"""numpy restatement of the edge-avoiding a-trous denoiser of the Color channel (rayn_hip_denoise_device, include/rayn_hip.h;
Dammertz et al., HPG 2010), operation by operation in float32, so that the tests can compare the kernel with it bit for bit.  expf is the
pinned dm_expf of include/rayn_detmath.h, evaluated by the oracle (oracle_detmath op 0).  dtype=np.float64 reads the same formula in
float64 with numpy's exp (a cross-check of the float32 reading, not bit-exact)."""
import numpy as np

H_TAPS = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
# Wrong readings, for tests/post_edge_cases.py (mutant=None: the definition's bits).  border_le: a tap one step beyond the last row or
# column still counts (it reads the edge pixel); nan_weight_counts: a tap whose weight is NaN is added like any other.
# zero_weight_skipped: a tap of weight 0 is left out, where the definition adds its +0 (a sum of -0.0 becomes +0).
MUTANTS = ("border_le", "nan_weight_counts", "zero_weight_skipped")


def oracle_expf(x):
    from oracle import oracle_py
    return oracle_py.detmath(0, np.ascontiguousarray(x, np.float32).reshape(-1)).reshape(np.shape(x))


def atrous(color, alpha, normal, width, height, iterations, sigma_color, sigma_normal, sigma_alpha, dtype=np.float32, mutant=None):
    """color / normal: width * height * 3 floats, alpha: width * height floats (pixel x + y * width); a guide whose sigma is 0 is not
    read and may be None.  Returns the filtered colour, shape (width * height, 3)."""
    f = np.dtype(dtype).type
    expf = oracle_expf if f is np.float32 else np.exp
    w, h = int(width), int(height)
    c = np.asarray(color, np.float32).reshape(h, w, 3).astype(f)
    use_c, use_n, use_a = sigma_color != 0, sigma_normal != 0, sigma_alpha != 0
    n = np.asarray(normal, np.float32).reshape(h, w, 3).astype(f) if use_n else None
    a = np.asarray(alpha, np.float32).reshape(h, w).astype(f) if use_a else None
    # the C entry takes the sigmas as f32; 1 / sigma^2 is evaluated in the working precision
    sc, sn, sa = (f(np.float32(s)) for s in (sigma_color, sigma_normal, sigma_alpha))
    kn = f(1.0) / (sn * sn) if use_n else None
    ka = f(1.0) / (sa * sa) if use_a else None
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    with np.errstate(all="ignore"):
        for i in range(int(iterations)):
            step = 1 << i
            kc = (f(1.0) / (sc * sc)) * f(1 << (2 * i)) if use_c else None
            W = np.full((h, w), f(9.0 / 64.0), f)
            S = f(9.0 / 64.0) * c
            for ky in range(-2, 3):
                for kx in range(-2, 3):
                    if kx == 0 and ky == 0:
                        continue
                    qy, qx = ys + ky * step, xs + kx * step
                    inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                    if mutant == "border_le":
                        inside = (qy >= 0) & (qy <= h) & (qx >= 0) & (qx <= w)
                    qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                    cq = c[qy, qx]
                    ok = inside & np.isfinite(cq).all(-1)
                    e = np.zeros((h, w), f)
                    if use_c:
                        d = c - cq
                        e = e + ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * kc
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
            out = S / W[..., None]
            c = np.where(np.isfinite(c).all(-1)[..., None], out, c)  # a non-finite centre passes through unchanged
    return c.reshape(h * w, 3)
