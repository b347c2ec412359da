#!/usr/bin/env python3
"""What feeding the filtered colour back into the temporal history buys a sequence, on the CPU: the sequence of
tools/temporal_variance_defaults.py (the oracle's renders and closest hits of temporal_np.DefaultsCase: shipped scene, 160x96, moving
camera, 8 frames at samples=2) accumulated with Temporal()'s defaults and the luminance moments by the numpy restatement, every frame's
first a-trous pass blended into the history the next frame reprojects with strength beta (tests/temporal_feedback_np.py), then the last
frame filtered.  Score: the MSE of the saturated Color + Background of the last frame against a samples=256 render of it, as a ratio to
the raw last frame's.  beta = 0 is tools/temporal_variance_defaults.py's table: 0.4571x at (1, 4.0) is this tool's self-check.

    python tools/temporal_feedback_defaults.py                          # the grid, then max_history 8 at the best three points with beta > 0
    python tools/temporal_feedback_defaults.py --point 0.5 1 4.0        # one point: beta, iterations, sigma_luminance (the figure the GPU test cites)
    python tools/temporal_feedback_defaults.py --point 0.5 1 4.0 --max-history 8
"""
import argparse
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import temporal_feedback_np as TF  # noqa: E402
import temporal_np as T  # noqa: E402
import temporal_variance_np as TV  # noqa: E402

SIGMA_NORMAL, SIGMA_ALPHA = 0.4, 0.3
BETAS, ITERATIONS, SIGMAS_LUMINANCE = (0.0, 0.25, 0.5, 0.75, 1.0), (1, 2), (1.0, 2.0, 4.0)
SELF_CHECK = ((0.0, 1, 4.0), 0.4571)  # DESIGN.md section 8, the table of tools/temporal_variance_defaults.py


def feedback_sequence(wd, frames, W, H, temporal, beta, sigma_luminance):
    """The accumulated colour, the history and the moments of the last frame, every frame's history having taken the write-back.  The
    write-back is pass 0's, so it does not depend on the number of passes."""
    prev, mom, prev_time = None, None, 0.0
    hit = T.world_hitables(wd)
    for p, film, (rec, obj) in frames:
        out, prev, mom = TV.accumulate(W, H, film["color"], film["normal"], rec, obj, prev, mom, wd.camera, prev_time, p.time_start, hit,
                                       temporal.max_history, temporal.depth_tolerance, temporal.normal_min)
        fed = TF.feedback(W, H, out, film["alpha"], film["normal"], obj, prev, mom, sigma_luminance, SIGMA_NORMAL, SIGMA_ALPHA, beta)
        hist, prev = prev, fed  # the last frame's filter reads the history as the accumulate left it: only n' is read, which never changes
        prev_time = p.time_start
    return out, hist, mom


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", nargs=3, type=float, metavar=("BETA", "ITERATIONS", "SIGMA_LUMINANCE"), default=None)
    ap.add_argument("--max-history", type=int, default=None, help="instead of Temporal()'s (with --point)")
    args = ap.parse_args()
    import dataclasses
    import rayn_amd as R
    import temporal_defaults as TD
    from oracle import oracle_py
    oracle_py.build()
    D = T.DefaultsCase
    W, H = D.W, D.H
    wd, frames, want = TD.cpu_sequence(oracle_py)
    last, (_, obj) = frames[-1][1], frames[-1][2]
    bg = last["background"]
    raw = D.mse(last["color"], bg, want)
    print(f"{W}x{H}: raw last frame MSE {raw:.4e}")

    def ratios(tp, beta, sl):
        """{iterations: ratio} for one sequence"""
        acc, hist, mom = feedback_sequence(wd, frames, W, H, tp, beta, sl)
        out = {}
        for it in ITERATIONS:
            c, _ = TV.denoise(W, H, acc, last["alpha"], last["normal"], obj, hist[0][:, 3], mom, it, sl, SIGMA_NORMAL, SIGMA_ALPHA)
            out[it] = D.mse(c, bg, want) / raw
        return out

    def show(tp, beta, it, sl, r):
        print(f"Temporal(max_history={tp.max_history}, feedback={beta}) + VarianceDenoise({it}, {sl}, {SIGMA_NORMAL}, {SIGMA_ALPHA}): {r:.4f}x", flush=True)

    tp = R.Temporal()
    if args.point is not None:
        beta, it, sl = args.point[0], int(args.point[1]), args.point[2]
        if args.max_history is not None:
            tp = dataclasses.replace(tp, max_history=args.max_history)
        assert it in ITERATIONS
        show(tp, beta, it, sl, ratios(tp, beta, sl)[it])
        return
    grid = {}
    for beta, sl in itertools.product(BETAS, SIGMAS_LUMINANCE):
        for it, r in ratios(tp, beta, sl).items():
            grid[(beta, it, sl)] = r
            show(tp, beta, it, sl, r)
    point, figure = SELF_CHECK
    assert f"{grid[point]:.4f}" == f"{figure:.4f}", f"beta = 0 must reproduce tools/temporal_variance_defaults.py: {grid[point]:.4f} != {figure}"
    best = sorted((k for k in grid if k[0] > 0), key=grid.get)[:3]
    print("best three with beta > 0: " + ", ".join(f"{k} {grid[k]:.4f}x" for k in best))
    long = dataclasses.replace(tp, max_history=8)
    for beta, it, sl in [point] + best:
        show(long, beta, it, sl, ratios(long, beta, sl)[it])


if __name__ == "__main__":
    main()
