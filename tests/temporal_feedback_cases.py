"""The adversarial history and film shared by tests/test_temporal_feedback.py (CPU) and tests/test_temporal_feedback_device.py (GPU), and
the restatement's result for them.  TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this."""
import itertools

import numpy as np

import temporal_feedback_np as TF
import temporal_np as T
from temporal_cases import SPECIAL, pack_inputs

f32 = np.float32
W0, H0 = 37, 29  # no multiple of 16
SIGMAS = list(itertools.product((0.0, 4.0), (0.0, 0.4), (0.0, 0.3)))  # every on/off combination of luminance / normal / alpha


def adversarial_inputs(w, h, seed):
    """temporal_cases.pack_inputs' of the denoise entry (objects with misses, history lengths 0 .. 8, NaN, inf, -1 and 0.5,
    special values over colour, guides and moments) with a history whose colour is adversarial too: the special values that are finite
    anywhere, the others where n' >= 1 does not hold - a history pixel with n' >= 1 has a finite colour, the accumulate sees to that.
    Two hand-made patches of one surface (one object, normal and alpha, n' = 4): single pixels of 3e38 among -3e38, where c' - c
    overflows unless the luminance term keeps the neighbours out, and a patch of the largest float, whose luminance is not finite."""
    assert w >= 32 and h >= 28
    inp = pack_inputs(w, h, seed)
    rng = np.random.default_rng(seed + 900)
    n = w * h
    big = rng.choice(n, n // 8, replace=False)
    inp["color"][big] = rng.choice(np.array([3.0e38, -3.0e38, 1.7e38, -1.7e38], f32), (big.size, 3))
    A, B, N, O = (a.copy() for a in T.split_history(inp["hist"], n))
    fmax = np.finfo(f32).max
    for (y0, y1, x0, x1), colour in (((2, 11, 3, 15), lambda x, y: 3.0e38 if x % 3 == 0 and y % 3 == 0 else -3.0e38), ((18, 26, 20, 30), lambda x, y: fmax)):
        for y, x in itertools.product(range(y0, y1), range(x0, x1)):
            p = x + y * w
            inp["color"][p], inp["normal"][p], inp["alpha"][p], inp["obj"][p], inp["n1"][p], inp["mom"][p] = colour(x, y), (0.0, 0.0, 1.0), 1.0, 1, 4.0, (0.5, 0.3)
            A[p], O[p] = (0.5, 0.25, 0.125, 4.0), 1
    rgb = A[:, :3].reshape(-1)  # a copy: the slice is not contiguous
    idx = rng.choice(rgb.size, rgb.size // 6, replace=False)
    rgb[idx] = np.resize(SPECIAL, idx.size)
    A[:, :3] = rgb.reshape(n, 3)
    with np.errstate(invalid="ignore"):
        has_history = A[:, 3] >= f32(1.0)
    bad = has_history & ~np.isfinite(A[:, :3]).all(axis=1)
    A[bad, :3] = np.array([3.0e38, -0.0, 1e-45], f32)
    inp["hist"] = T.join_history(A, B, N, O)
    return inp


def restate(w, h, inp, L, sigmas, beta):
    """(colour, variance, (A, B, N, O)) of the restatement for the inputs above"""
    n = w * h
    return TF.denoise(w, h, inp["color"], inp["alpha"], inp["normal"], inp["obj"], T.split_history(inp["hist"], n), inp["mom"], L, *sigmas, beta)
