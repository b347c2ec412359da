"""numpy restatement of the write-back of rayn_hip_denoise_temporal_variance_feedback_device (include/rayn_hip.h): the first a-trous pass
of the variance-guided filter of a temporally accumulated colour, blended into plane A of the history that the next frame reprojects
(SVGF's feedback edge).  It sits on top of temporal_variance_np (the variance estimate) and denoise_variance_np (the passes), binary32
operation by operation; nothing here shares code with rayn_amd/csrc.  tests/test_temporal_feedback_device.py compares the kernels with it
bit for bit.  TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this."""
import numpy as np

import denoise_variance_np as V
import temporal_variance_np as TV

f32 = np.float32


def check_feedback(beta):
    """The entry's rule for the strength: finite and in [0, 1]"""
    b = float(beta)
    return np.isfinite(b) and 0.0 <= b <= 1.0


def first_pass(width, height, color, alpha, normal, obj, n_hist, moments, sigma_luminance, sigma_normal, sigma_alpha):
    """(c', v') of pass 0 (step 1, on the packed records) for every pixel: V.atrous does not expose its passes, so it runs with one."""
    v0, _ = TV.initial_variance(width, height, color, obj, n_hist, moments)
    return V.atrous(color, alpha, normal, v0, width, height, 1, sigma_luminance, sigma_normal, sigma_alpha)


def write_back(A, color, c1, v1, beta):
    """Plane A (n, 4) of the history after the write-back.  color (n, 3): the accumulated colour, pass 0's input; (c1, v1): what pass 0
    computed.  beta == 0 returns A's bits; else a pixel whose v1 is not NaN and whose fb = c + beta * (c1 - c) has three finite
    components gets fb as its colour, its fourth component n' keeps its bits, and every other pixel is untouched."""
    assert check_feedback(beta)
    A = np.array(A, f32, copy=True)
    n = A.shape[0]
    if float(beta) == 0.0:
        return A
    c = np.asarray(color, f32).reshape(n, 3)
    c1 = np.asarray(c1, f32).reshape(n, 3)
    v1 = np.asarray(v1, f32).reshape(n)
    with np.errstate(all="ignore"):
        d = (c1 - c).astype(f32)
        m = (f32(beta) * d).astype(f32)
        fb = (c + m).astype(f32)
    take = ~np.isnan(v1) & np.isfinite(fb).all(axis=1)
    A[take, :3] = fb[take]
    return A


def feedback(width, height, color, alpha, normal, obj, hist, moments, sigma_luminance, sigma_normal, sigma_alpha, beta):
    """The history (A, B, N, O) after the entry's call: only A's colour changes.  hist: the NEW history of the accumulate that wrote
    `color`; its n' drives the variance estimate."""
    A, B, N, O = hist
    A = np.asarray(A, f32)
    if float(beta) == 0.0:
        assert check_feedback(beta)
        return (A.copy(), B, N, O)
    c1, v1 = first_pass(width, height, color, alpha, normal, obj, A[:, 3], moments, sigma_luminance, sigma_normal, sigma_alpha)
    return (write_back(A, color, c1, v1, beta), B, N, O)


def denoise(width, height, color, alpha, normal, obj, hist, moments, iterations, sigma_luminance, sigma_normal, sigma_alpha, beta):
    """The whole entry: (colour (n, 3), variance (n)) - temporal_variance_np.denoise's, whatever beta - and the history afterwards."""
    c, v = TV.denoise(width, height, color, alpha, normal, obj, np.asarray(hist[0], f32)[:, 3], moments, iterations, sigma_luminance, sigma_normal, sigma_alpha)
    return c, v, feedback(width, height, color, alpha, normal, obj, hist, moments, sigma_luminance, sigma_normal, sigma_alpha, beta)
