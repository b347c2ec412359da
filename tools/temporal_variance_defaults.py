#!/usr/bin/env python3
"""What the variance-guided denoiser buys a temporally accumulated sequence, on the CPU: the sequence of
tools/temporal_defaults.py (the oracle's renders and closest hits of temporal_np.DefaultsCase: shipped scene, 160x96, moving camera, 8
frames at samples=2) accumulated with Temporal()'s defaults and the luminance moments by the numpy restatement
(tests/temporal_variance_np.py), then the last frame filtered with every point of the grid.  Score: the MSE of the saturated Color +
Background of the last frame against a samples=256 render of it, as a ratio to the raw last frame's.

    python tools/temporal_variance_defaults.py                 # baselines and the grid
    python tools/temporal_variance_defaults.py --recommended   # baselines and the recommended point (the figure the GPU test cites)
    python tools/temporal_variance_defaults.py --size 320x192  # the same at another size
"""
import argparse
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import denoise_np  # noqa: E402
import temporal_np as T  # noqa: E402
import temporal_variance_np as TV  # noqa: E402

RECOMMENDED = (1, 4.0, 0.4, 0.3)  # iterations, sigma_luminance, sigma_normal, sigma_alpha: the best point of the grid at 160x96
GRID = list(itertools.product((1, 2, 3), (1.0, 2.0, 4.0, 8.0), (0.0, 0.4, 0.7), (0.3,)))


def accumulate_sequence(wd, frames, W, H, temporal):
    """The accumulated colour, the new history's n' and the moments of the last frame"""
    prev, mom, prev_time = None, None, 0.0
    for p, film, (rec, obj) in frames:
        out, prev, mom = TV.accumulate(W, H, film["color"], film["normal"], rec, obj, prev, mom, wd.camera, prev_time, p.time_start, T.world_hitables(wd),
                                       temporal.max_history, temporal.depth_tolerance, temporal.normal_min)
        prev_time = p.time_start
    return out, prev[0][:, 3], mom


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recommended", action="store_true")
    ap.add_argument("--size", default=None, help="WxH instead of DefaultsCase's 160x96")
    args = ap.parse_args()
    import rayn_amd as R
    import temporal_defaults as TD
    from oracle import oracle_py
    oracle_py.build()
    D = T.DefaultsCase
    if args.size:
        D.W, D.H = (int(v) for v in args.size.split("x"))
        TD.W, TD.H = D.W, D.H
    W, H = D.W, D.H
    wd, frames, want = TD.cpu_sequence(oracle_py)
    tp = R.Temporal()
    acc, n_hist, mom = accumulate_sequence(wd, frames, W, H, tp)
    last, (_, obj) = frames[-1][1], frames[-1][2]
    bg = last["background"]
    raw = D.mse(last["color"], bg, want)
    print(f"{W}x{H}: raw last frame MSE {raw:.4e}; history n' >= 4 on {float((n_hist >= 4).mean()):.3f} of the pixels, 1 <= n' < 4 on "
          f"{float(((n_hist >= 1) & (n_hist < 4)).mean()):.3f}")
    print(f"Temporal() alone: {D.mse(acc, bg, want) / raw:.4f}x")
    d = R.Denoise()
    fixed = denoise_np.atrous(acc, last["alpha"], last["normal"], W, H, d.iterations, d.sigma_color, d.sigma_normal, d.sigma_alpha)
    print(f"Temporal() + Denoise(): {D.mse(fixed, bg, want) / raw:.4f}x")
    for it, sl, sn, sa in ([RECOMMENDED] if args.recommended else GRID):
        c, _ = TV.denoise(W, H, acc, last["alpha"], last["normal"], obj, n_hist, mom, it, sl, sn, sa)
        print(f"Temporal() + VarianceDenoise({it}, {sl}, {sn}, {sa}): {D.mse(c, bg, want) / raw:.4f}x", flush=True)


if __name__ == "__main__":
    main()
