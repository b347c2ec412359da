#!/usr/bin/env python3
"""Whether a Catmull-Rom resample of the temporal history lets a longer history pay, on the CPU: the sequence of
tools/temporal_defaults.py (the oracle's renders and closest hits of temporal_np.DefaultsCase: shipped scene, 160x96, moving camera, 8
frames at samples=2) accumulated by the numpy restatement (tests/temporal_resample_np.py) for resample {bilinear, catmull_rom} x max_history
{2, 4, 8, 16, 32}, alone and with VarianceDenoise(1, 4.0, 0.4, 0.3) on the last frame.  Score: the MSE of the saturated Color + Background
of the last frame against a samples=256 render of it, as a ratio to the raw last frame's.  The bilinear points at max_history 4 must
reproduce 0.4940x and 0.4571x (tools/temporal_defaults.py, tools/temporal_variance_defaults.py): the tool asserts both.

    python tools/temporal_resample_defaults.py

A history cannot be longer than the sequence, so 8 frames cannot tell max_history 8, 16 and 32 apart.  When the 8-frame grid does not
separate 16 from 32 the tool goes on to a 16-frame sequence (the same 8 frames and 8 more, scored on frame 16) and prints that grid too.
There max_history 16 and 32 still coincide - separating them would take more than 16 frames, which is not run: both grids already rise
from max_history 4 on.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import temporal_np as T  # noqa: E402
import temporal_resample_np as TR  # noqa: E402
import temporal_variance_np as TV  # noqa: E402

RECOMMENDED = (1, 4.0, 0.4, 0.3)  # tools/temporal_variance_defaults.py
RESAMPLES, HISTORIES = ("bilinear", "catmull_rom"), (2, 4, 8, 16, 32)
SELF_CHECK = {False: 0.4940, True: 0.4571}  # bilinear, max_history 4: alone, with RECOMMENDED


def resample_sequence(wd, frames, W, H, temporal):
    """The accumulated colour, the new history's n', the moments and the arm codes of the last frame"""
    from rayn_amd import _abi
    prev, mom, prev_time = None, None, 0.0
    hit = T.world_hitables(wd)
    mode = _abi.TEMPORAL_RESAMPLE[temporal.resample]
    for p, film, (rec, obj) in frames:
        if prev is None:
            out, prev, mom, arm = TR.accumulate_first(W, H, film["color"], film["normal"], rec, obj, True)
        else:
            out, prev, mom, arm = TR.accumulate(W, H, film["color"], film["normal"], rec, obj, prev, mom, wd.camera, prev_time, p.time_start, hit,
                                                temporal.max_history, temporal.depth_tolerance, temporal.normal_min, mode)
        prev_time = p.time_start
    return out, prev[0][:, 3], mom, arm


def grid_of(oracle, wd, frames, pref):
    """Print and return {(resample, max_history, denoised): ratio} for one sequence of (frame params, film, G-buffer), scored on its last
    frame against a render of it under the reference parameters pref."""
    import rayn_amd as R
    D = T.DefaultsCase
    W, H = D.W, D.H
    ref, _ = oracle.render(wd, pref, oracle.build_tables(4 * D.REF_SAMPLES, D.BOUNCES, pref.volume_marches, pref.frame, W, H))
    want = np.clip(ref["color"].astype(np.float64) + ref["background"], 0.0, 1.0)
    last, (_, obj) = frames[-1][1], frames[-1][2]
    bg = last["background"]
    raw = D.mse(last["color"], bg, want)
    print(f"{W}x{H}, {len(frames)} frames: raw last frame MSE {raw:.4e}", flush=True)
    grid = {}
    for resample in RESAMPLES:
        for mh in HISTORIES:
            tp = R.Temporal(max_history=mh, resample=resample)
            acc, n_hist, mom, arm = resample_sequence(wd, frames, W, H, tp)
            c, _ = TV.denoise(W, H, acc, last["alpha"], last["normal"], obj, n_hist, mom, *RECOMMENDED)
            grid[(resample, mh, False)], grid[(resample, mh, True)] = D.mse(acc, bg, want) / raw, D.mse(c, bg, want) / raw
            share = float((arm == TR.ARM_CUBIC).sum()) / max(1, int((arm != TR.ARM_RESET).sum()))
            print(f"Temporal(max_history={mh:2d}, resample={resample!r:13s}): {grid[(resample, mh, False)]:.4f}x alone, "
                  f"{grid[(resample, mh, True)]:.4f}x + VarianceDenoise{RECOMMENDED}; cubic arm on {share:.3f} of the last frame's non-reset pixels, "
                  f"reset on {float((arm == TR.ARM_RESET).mean()):.3f} of all", flush=True)
    for dn in (False, True):
        best = min((k for k in grid if k[0] == "catmull_rom" and k[2] == dn), key=grid.get)
        base = min((k for k in grid if k[0] == "bilinear" and k[2] == dn), key=grid.get)
        print(f"{'with VarianceDenoise' if dn else 'alone'}: best catmull_rom max_history {best[1]} {grid[best]:.4f}x; best bilinear max_history {base[1]} {grid[base]:.4f}x")
    return grid


def main():
    import rayn_amd as R
    from oracle import oracle_py
    oracle_py.build()
    D = T.DefaultsCase
    W, H = D.W, D.H
    wd, ps, pref = D.scene()  # the 8 frames of the sequence and the reference parameters of the last one
    more = [R.frame_params(W, H, D.SAMPLES, D.BOUNCES, frame=f) for f in range(ps[-1].frame + 1, 2 * ps[-1].frame + 1)]

    def rendered(p):
        film, _ = oracle_py.render(wd, p, oracle_py.build_tables(4 * D.SAMPLES, D.BOUNCES, p.volume_marches, p.frame, W, H))
        return p, film, T.gbuffer_oracle(oracle_py, wd, p)

    frames = [rendered(p) for p in ps]
    grid = grid_of(oracle_py, wd, frames, pref)
    for dn, figure in SELF_CHECK.items():
        got = grid[("bilinear", 4, dn)]
        assert f"{got:.4f}" == f"{figure:.4f}", f"bilinear at max_history 4 must reproduce DESIGN.md section 8: {got:.4f} != {figure}"
    if all(grid[(r, 16, dn)] == grid[(r, 32, dn)] for r in RESAMPLES for dn in (False, True)):
        print(f"{len(frames)} frames do not separate max_history 16 from 32: the same sequence continued to {len(frames) + len(more)} frames", flush=True)
        frames += [rendered(p) for p in more]
        grid_of(oracle_py, wd, frames, R.frame_params(W, H, D.REF_SAMPLES, D.BOUNCES, frame=more[-1].frame))


if __name__ == "__main__":
    main()
