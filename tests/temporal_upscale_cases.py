"""Sizes, factors, sigma pairs and the synthetic frame sequence shared by tests/test_temporal_upscale.py (CPU) and
tests/test_temporal_upscale_device.py (GPU).  TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this."""
import numpy as np

import temporal_np as T
import upscale_np as U

f32 = np.float32
SIZES = [(24, 16), (20, 12), (25, 19)]
FACTORS = [1, 2, 3, 4]
SIGMAS = [(0.02, 0.05), (0.0, 0.05), (0.02, 0.0), (0.0, 0.0)]


def synthetic(w, h, s, seed, adversarial, shift=0.0):
    """A low film and the two G-buffers around the plane z = 0 as an orthographic camera at x = shift sees it (the generator of
    tests/test_upscale_device.py with a moving camera): random objects with misses, depth noise, normals near +z; `adversarial` scatters
    NaN / inf / denormal / huge values over every plane and guide and gives regions of the high G-buffer objects no low pixel shows."""
    rng = np.random.default_rng(seed)
    n, N = w * h, w * h * s * s
    lrec, _, nrm = T.ortho_plane_gbuffer(w, h, origin_x=shift, pixel=4.0 / h)
    hrec, _, _ = T.ortho_plane_gbuffer(w * s, h * s, origin_x=shift, pixel=4.0 / (h * s))
    lrec[:, 2], hrec[:, 2] = rng.normal(0.0, 0.05, n), rng.normal(0.0, 0.05, N)
    lrec[:, 3], hrec[:, 3] = f32(4.0) - lrec[:, 2], f32(4.0) - hrec[:, 2]
    pick = np.array([0, 1, 1, 1, 2, 0xFFFFFFFF], np.uint32)
    # objects in world-space stripes, so that a moving camera sees the same object at the same place; a few pixels at random
    lobj = pick[((lrec[:, 0] + 40.0) * 1.7).astype(np.int64) % pick.size].copy()
    hobj = pick[((hrec[:, 0] + 40.0) * 1.7).astype(np.int64) % pick.size].copy()
    flip = rng.random(N) < 0.1
    hobj[flip] = rng.choice(pick, int(flip.sum()))
    lrec[lobj == U.MISS] = (0.0, 0.0, 0.0, np.inf)
    hrec[hobj == U.MISS] = (0.0, 0.0, 0.0, np.inf)
    film = {"color": rng.gamma(0.6, 0.5, (n, 3)).astype(f32), "alpha": rng.random(n).astype(f32), "background": rng.random((n, 3)).astype(f32),
            "normal": (nrm + rng.normal(0.0, 0.3, (n, 3))).astype(f32)}
    if adversarial:
        Yi = np.repeat(np.arange(h * s), w * s)
        special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 3.0e38, -3.0e38, 1e-45, -1e-40, 1e30, -1e30], f32)
        for plane in (film["color"], film["alpha"], film["background"], film["normal"], lrec, hrec):
            flat = plane.reshape(-1)
            idx = rng.choice(flat.size, min(flat.size // 4, 6 * special.size), replace=False)
            flat[idx] = np.resize(special, idx.size)
        hrec[rng.choice(N, 6, replace=False), 3] = (0.0, -1e-8, 1e30, 3.0e38, 1e-45, -0.0)
        hobj[Yi < 2 * s] = 5  # two low rows' worth of pixels whose object no tap shows: tier 2
        film["color"][(np.arange(n) % w) >= w - 3] = np.nan  # three dead columns: tier 3 along the right border
    return film, (lrec, lobj), (hrec, hobj)


def sequence(w, h, s, seed, adversarial, frames=3):
    """`frames` synthetic frames under an orthographic camera that moves 0.3 high pixels per frame: [(film, low_g, high_g, camera at the
    HIGH size, time_start)]"""
    out = []
    for k in range(frames):
        shift = 0.3 * k * 4.0 / (h * s)
        film, low_g, high_g = synthetic(w, h, s, seed + 1000 * k, adversarial, shift)
        out.append((film, low_g, high_g, T.ortho_camera(w * s, h * s, origin_x=shift, pixel=4.0 / (h * s)), 0.25 * k))
    return out
