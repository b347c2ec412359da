"""The adaptive scene, the hand-made films and the oracle-driven epoch renderer shared by tests/test_progressive.py (CPU) and
tests/test_progressive_device.py (GPU).  TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this."""
import numpy as np

import progressive_np as PN
from common import case

F32 = np.float32

# The adaptive scene of the loop tests (CPU here, GPU in test_progressive_device.py): MandelBox, part sky, part fractal.
ADAPTIVE = dict(target_error=0.2, noise_floor=0.05, min_epochs=3, max_epochs=40, outlier_permille=100)
W, H, TILE, SAMPLES, BOUNCES = 48, 32, (16, 16), 1, 3


def oracle_epochs(oracle, name, frame=1, fma=False, w=W, h=H, samples=SAMPLES, bounces=BOUNCES):
    """render_epoch(seed, tile_subset) of scene `name` through the CPU oracle, and the frame parameters"""
    wd, p = case(name, w, h, samples, bounces, frame=frame)
    film_tables = oracle.build_tables(4 * samples, bounces, p.volume_marches, frame, w, h, fma=fma)[2:]

    def render_epoch(seed, subset):
        rd = oracle.build_tables(4 * samples, bounces, p.volume_marches, seed, w, h, fma=fma)[:2]
        return oracle.render(wd, p, tuple(rd) + tuple(film_tables), tile_subset=subset, fma=fma)[0]
    return render_epoch, p


def film(w, h, seed, special=False):
    rng = np.random.default_rng(seed)
    n = w * h
    f = {"color": rng.gamma(0.6, 0.5, (n, 3)).astype(F32), "alpha": rng.choice(np.array([0.0, 0.25, 1.0], F32), n),
         "background": rng.uniform(0, 1, (n, 3)).astype(F32), "normal": rng.normal(size=(n, 3)).astype(F32)}
    if special:
        vals = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 3.0e38, -3.0e38, 1e-45, -1e-45, 1e-39], F32)
        for key in PN.FILM_KEYS:
            flat = f[key].reshape(-1)
            idx = rng.choice(flat.size, min(flat.size, 2 * vals.size), replace=False)
            flat[idx] = np.resize(vals, idx.size)
    return f


def restated_arrays(st):
    return {"sum_color": st.sum["color"], "sum_alpha": st.sum["alpha"], "sum_background": st.sum["background"], "sum_normal": st.sum["normal"],
            "mean_y": st.mean_y, "m2": st.m2, "epochs": st.epochs, "retired": st.retired, "outliers": st.outliers, "max_e": st.max_e}
