"""numpy restatement of the luminance moments of the temporal accumulate (rayn_hip_temporal_accumulate_moments_device) and of the variance
estimate in front of the a-trous passes (rayn_hip_denoise_temporal_variance_device), written from the definitions in include/rayn_hip.h,
binary32 operation by operation.  The colour and the history come from temporal_np.accumulate, the passes from denoise_variance_np.atrous;
nothing here shares code with rayn_amd/csrc.  tests/test_temporal_variance_device.py compares the kernels with it bit for bit.  TEST
INFRASTRUCTURE: nothing under rayn_amd/ imports this."""
import numpy as np

import denoise_variance_np as V
import temporal_np as T

f32 = np.float32
MISS = T.MISS
TEMPORAL_MIN_HISTORY = f32(4.0)  # SVGF's threshold between the spatial and the temporal estimate
WINDOW = 3                       # the spatial estimate's window is (2 * 3 + 1)^2 at unit spacing
# Wrong readings of the variance estimate, for tests/post_edge_cases.py (mutant=None: the definition's bits).  nprime_gt4: the temporal
# estimate needs n' > 4; nprime_gt1: a pixel (and a tap of the window) needs n' > 1; d_ge0: d >= 0 ? d : 0, which lets d = -0.0 through.
MUTANTS = ("nprime_gt4", "nprime_gt1", "d_ge0")


def luminance(c):
    """(0.2126f r + 0.7152f g) + 0.0722f b of (n, 3) colours"""
    c = np.asarray(c, f32)
    with np.errstate(all="ignore"):
        return (((f32(0.2126) * c[..., 0]).astype(f32) + (f32(0.7152) * c[..., 1]).astype(f32)).astype(f32) + (f32(0.0722) * c[..., 2]).astype(f32)).astype(f32)


def moments_bytes(width, height):
    """8 bytes per pixel; 0 where the history size is 0 (a zero-sized film, or 2^31 pixels and more)"""
    n = int(width) * int(height)
    return 8 * n if width > 0 and height > 0 and n < 1 << 31 else 0


def accumulate(width, height, color, normal, rec, obj, prev, prev_moments, prev_cam, prev_time, cur_time, hitables, max_history, depth_tolerance,
               normal_min):
    """One temporal accumulate with moments.  Arguments as temporal_np.accumulate, plus prev_moments (n, 2) or None (with prev None).
    Returns (out colour, (A', B', N', O'), moments (n, 2))."""
    assert (prev is None) == (prev_moments is None)
    n = width * height
    out, hist = T.accumulate(width, height, color, normal, rec, obj, prev, prev_cam, prev_time, cur_time, hitables, max_history, depth_tolerance, normal_min)
    color = np.asarray(color, f32).reshape(n, 3)
    normal = np.asarray(normal, f32).reshape(n, 3)
    rec, obj = np.asarray(rec, f32).reshape(n, 4), np.asarray(obj, np.uint32).reshape(n)
    with np.errstate(all="ignore"):
        y = luminance(color)
        y2 = (y * y).astype(f32)
    cfin = np.isfinite(color).all(axis=1)
    # a pixel that resets: (y, y2), and (0, 0) for a colour that is not finite
    mom = np.where(cfin[:, None], np.stack([y, y2], axis=1), f32(0.0)).astype(f32)
    if prev is None:
        return out, hist, mom
    pA, pB, pN, pO = [np.asarray(a) for a in prev]
    pA, pB, pN, pO = pA.reshape(n, 4), pB.reshape(n, 4), pN.reshape(n, 4), pO.reshape(n)
    pM = np.asarray(prev_moments, f32).reshape(n, 2)
    with np.errstate(all="ignore"):
        # steps 2 - 4 of the colour's definition give the taps, their weights and their order
        dt = f32(f32(cur_time) - f32(prev_time))
        Pp = [rec[:, c].copy() for c in range(3)]
        for k, (animated, vel) in enumerate(hitables):
            if animated:
                for c in range(3):
                    Pp[c] = np.where(obj == k, (rec[:, c] - (f32(vel[c]) * dt).astype(f32)).astype(f32), Pp[c]).astype(f32)
        ok, fx, fy, te = T.project(prev_cam, prev_time, Pp, width, height)
        ok = ok & cfin & (obj != MISS)
        x0f, y0f = np.floor(fx).astype(f32), np.floor(fy).astype(f32)
        wx = [None, (fx - x0f).astype(f32)]
        wy = [None, (fy - y0f).astype(f32)]
        wx[0], wy[0] = (f32(1.0) - wx[1]).astype(f32), (f32(1.0) - wy[1]).astype(f32)
        x0 = np.where(np.isfinite(x0f), np.clip(x0f, -2.0, 2.0 ** 31), -2.0).astype(np.int64)
        y0 = np.where(np.isfinite(y0f), np.clip(y0f, -2.0, 2.0 ** 31), -2.0).astype(np.int64)
        tol = (f32(depth_tolerance) * te).astype(f32)
        W, S1, S2, N = (np.zeros(n, f32) for _ in range(4))
        S = np.zeros((n, 3), f32)
        for j in range(4):
            qx, qy = x0 + (j & 1), y0 + (j >> 1)
            counts = ok & (qx >= 0) & (qx < width) & (qy >= 0) & (qy < height)
            q = np.where(counts, qx + qy * width, 0)
            counts &= pA[q, 3] >= f32(1.0)
            counts &= pO[q] == obj
            counts &= np.abs((pB[q, 3] - te).astype(f32)) <= tol
            if f32(normal_min) > f32(-1.0):
                counts &= T.dot([normal[:, 0], normal[:, 1], normal[:, 2]], [pN[q, 0], pN[q, 1], pN[q, 2]]) >= f32(normal_min)
            w = (wx[j & 1] * wy[j >> 1]).astype(f32)
            W = np.where(counts, (W + w).astype(f32), W)
            for c in range(3):
                S[:, c] = np.where(counts, (S[:, c] + (w * pA[q, c]).astype(f32)).astype(f32), S[:, c])
            N = np.where(counts, (N + (w * pA[q, 3]).astype(f32)).astype(f32), N)
            S1 = np.where(counts, (S1 + (w * pM[q, 0]).astype(f32)).astype(f32), S1)
            S2 = np.where(counts, (S2 + (w * pM[q, 1]).astype(f32)).astype(f32), S2)
        h = (S / W[:, None]).astype(f32)
        n1 = np.fmin(((N / W).astype(f32) + f32(1.0)).astype(f32), f32(max_history)).astype(f32)
        a = (f32(1.0) / n1).astype(f32)
        blend = (h + (a[:, None] * (color - h).astype(f32)).astype(f32)).astype(f32)
        blended = ok & (W > 0) & np.isfinite(blend).all(axis=1)  # else the pixel reset
        h1, h2 = (S1 / W).astype(f32), (S2 / W).astype(f32)
        m1 = (h1 + (a * (y - h1).astype(f32)).astype(f32)).astype(f32)
        m2 = (h2 + (a * (y2 - h2).astype(f32)).astype(f32)).astype(f32)
        take = blended & np.isfinite(m1) & np.isfinite(m2)
    mom[take] = np.stack([m1, m2], axis=1)[take]
    # the colour derived here for the predicate is the one temporal_np wrote
    assert np.array_equal(np.where(blended[:, None], blend, color).view(np.uint32), np.asarray(out, f32).view(np.uint32))
    return out, hist, mom


def initial_variance(width, height, color, obj, n_hist, moments, mutant=None):
    """The variance the pack kernel hands to the passes: NaN = not guided.  color (n, 3): the accumulated colour; obj (n,): the G-buffer
    objects; n_hist (n,): n' of the new history; moments (n, 2)."""
    w, h = int(width), int(height)
    n = w * h
    c = np.asarray(color, f32).reshape(n, 3)
    obj = np.asarray(obj, np.uint32).reshape(n)
    nh = np.asarray(n_hist, f32).reshape(n)
    m = np.asarray(moments, f32).reshape(n, 2)
    cfin = np.isfinite(c).all(axis=1)
    with np.errstate(all="ignore"):
        has = (nh > f32(1.0)) if mutant == "nprime_gt1" else (nh >= f32(1.0))
        pos = (lambda d: d >= 0) if mutant == "d_ge0" else (lambda d: d > 0)
        candidate = (obj != MISS) & cfin & has
        temporal = candidate & ((nh > TEMPORAL_MIN_HISTORY) if mutant == "nprime_gt4" else (nh >= TEMPORAL_MIN_HISTORY))
        spatial = candidate & ~temporal
        d = (m[:, 1] - (m[:, 0] * m[:, 0]).astype(f32)).astype(f32)
        vt = (np.where(pos(d), d, f32(0.0)).astype(f32) / nh).astype(f32)
        # the spatial estimate: 7x7 at unit spacing, raster order, centre included
        lum = luminance(c).reshape(h, w)
        tap_ok = (has & cfin).reshape(h, w)
        o2 = obj.reshape(h, w)
        ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
        k, s1, s2 = (np.zeros((h, w), f32) for _ in range(3))
        for dy in range(-WINDOW, WINDOW + 1):
            for dx in range(-WINDOW, WINDOW + 1):
                qy, qx = ys + dy, xs + dx
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                counts = inside & tap_ok[qy, qx] & (o2[qy, qx] == o2)
                lq = lum[qy, qx]
                k = np.where(counts, (k + f32(1.0)).astype(f32), k)
                s1 = np.where(counts, (s1 + lq).astype(f32), s1)
                s2 = np.where(counts, (s2 + (lq * lq).astype(f32)).astype(f32), s2)
        mu = (s1 / k).astype(f32)
        ds = ((s2 / k).astype(f32) - (mu * mu).astype(f32)).astype(f32)
        vs = np.where(pos(ds), ds, f32(0.0)).astype(f32).reshape(n)
        v = np.where(temporal, vt, np.where(spatial, vs, f32(np.nan))).astype(f32)
        v = np.where(np.isfinite(v), v, f32(np.nan)).astype(f32)
    return v, k.reshape(n)


def denoise(width, height, color, alpha, normal, obj, n_hist, moments, iterations, sigma_luminance, sigma_normal, sigma_alpha, mutant=None):
    """The whole entry: the initial variance, then denoise_variance_np's passes.  Returns (colour (n, 3), variance (n))."""
    v0, _ = initial_variance(width, height, color, obj, n_hist, moments, mutant)
    return V.atrous(color, alpha, normal, v0, width, height, iterations, sigma_luminance, sigma_normal, sigma_alpha)
