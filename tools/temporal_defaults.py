#!/usr/bin/env python3
"""How the defaults of rayn_amd.Temporal were chosen, on the CPU: the oracle renders the shipped scene at 160x96
under a camera whose origin moves (setup_s3's drift), 8 frames at samples=2 (8 spp), the oracle's closest hit gives every frame's G-buffer,
and the numpy restatement of the accumulate (tests/temporal_np.py) runs the sequence for every point of the grid.  Score: the MSE of the
saturated Color + Background of the last frame against a samples=256 render of that frame, as a ratio to the raw last frame's.

    python tools/temporal_defaults.py            # the grid
    python tools/temporal_defaults.py --defaults # the shipped defaults only (the figure tests/test_temporal_device.py cites)
"""
import argparse
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import temporal_np as T  # noqa: E402

D = T.DefaultsCase
W, H, SAMPLES, REF_SAMPLES, BOUNCES, scene, mse = D.W, D.H, D.SAMPLES, D.REF_SAMPLES, D.BOUNCES, D.scene, D.mse


def cpu_sequence(oracle):
    """Every frame's film and G-buffer, and the saturated reference image of the last frame, all from the CPU oracle."""
    wd, ps, pref = scene()
    frames = []
    for p in ps:
        film, _ = oracle.render(wd, p, oracle.build_tables(4 * SAMPLES, BOUNCES, p.volume_marches, p.frame, W, H))
        frames.append((p, film, T.gbuffer_oracle(oracle, wd, p)))
    ref, _ = oracle.render(wd, pref, oracle.build_tables(4 * REF_SAMPLES, BOUNCES, pref.volume_marches, pref.frame, W, H))
    want = np.clip(ref["color"].astype(np.float64) + ref["background"], 0.0, 1.0)
    return wd, frames, want


def ratio(wd, frames, want, max_history, depth_tolerance, normal_min):
    """MSE of the temporally accumulated last frame / MSE of the raw last frame"""
    prev, prev_time = None, 0.0
    for p, film, (rec, obj) in frames:
        out, prev = T.accumulate(W, H, film["color"], film["normal"], rec, obj, prev, wd.camera, prev_time, p.time_start, T.world_hitables(wd),
                                 max_history, depth_tolerance, normal_min)
        prev_time = p.time_start
    last = frames[-1][1]
    return mse(out, last["background"], want) / mse(last["color"], last["background"], want)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--defaults", action="store_true")
    args = ap.parse_args()
    import rayn_amd as R
    from oracle import oracle_py
    oracle_py.build()
    wd, frames, want = cpu_sequence(oracle_py)
    d = R.Temporal()
    print(f"Temporal() = ({d.max_history}, {d.depth_tolerance}, {d.normal_min}): {ratio(wd, frames, want, d.max_history, d.depth_tolerance, d.normal_min):.4f}x")
    if args.defaults:
        return
    for mh, dt, nm in itertools.product((2, 4, 8, 16, 32), (0.0025, 0.01, 0.05, 0.25), (-1.0, 0.5, 0.9)):
        print(f"max_history {mh:3d} depth_tolerance {dt:6.4f} normal_min {nm:4.1f}: {ratio(wd, frames, want, mh, dt, nm):.4f}x", flush=True)


if __name__ == "__main__":
    main()
