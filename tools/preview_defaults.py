#!/usr/bin/env python3
"""How the default radius of rayn_amd.Preview was chosen and, on a GPU, what a preview costs.

    python tools/preview_defaults.py             # CPU: the shipped scene (rayn_amd.setup) at 160x96, 16 AO rays per pixel, through the
                                                 # numpy restatement (tests/preview_np.py) for the radii 0.025 * 2^k: the mean and the
                                                 # variance of the ao over the fractal's pixels; the default is the smallest radius within 2 % of the largest variance
    python tools/preview_defaults.py --profile   # GPU, no scoring: 20 previews at 1280x720 with K = 4 and K = 8 for a kernel trace,
                                                 # and their wall time per call around a device synchronise
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import rayn_amd as R  # noqa: E402
from rayn_amd import film as F  # noqa: E402
from rayn_amd import setup as S  # noqa: E402


def radius_table(w=160, h=96, samples=16):
    import preview_np as PN
    from oracle import oracle_py as O
    O.build()
    cam, world = S.setup((w, h))
    wd = world.to_desc(cam)
    p = R.frame_params(w, h, 1, 0)
    tab, scr = F.preview_tables(samples, 1, w, h)
    fractal = next(i for i in range(wd.n_hitables) if wd.hitables[i].kind == 1)
    rows = []
    for k in range(7):
        radius = 0.025 * 2 ** k
        ref = PN.preview(O, wd, p, tab, scr, radius, 1.0)
        ao = ref["ao"][ref["object"] == fractal].astype(np.float64)
        rows.append((radius, ao.mean(), ao.var()))
        print(f"radius {radius:6.3f}: mean ao {ao.mean():.3f}, variance {ao.var():.4f} over {ao.size} pixels", flush=True)
    best = max(r[2] for r in rows)
    print(f"largest variance {best:.4f} at radius {max(rows, key=lambda r: r[2])[0]}; the smallest radius within 2 % of it (the default): "
          f"{min(r[0] for r in rows if r[2] >= 0.98 * best)}")


def profile(w=1280, h=720, calls=20):
    import torch
    cam, world = S.setup((w, h))
    ctx = R.Context(0)
    ctx.upload_world(world.to_desc(cam))
    p = R.frame_params(w, h, 1, 0)
    for samples in (4, 8):
        pv = R.Preview(samples=samples)
        tab, scr = F.preview_tables(samples, 1, w, h)
        d_tab, d_scr = torch.from_numpy(tab).cuda(), torch.from_numpy(scr).cuda()
        out, g = F.alloc_device_film(w, h, "cuda"), F.alloc_gbuffer(w, h, "cuda")
        scratch = torch.empty(F.preview_scratch_bytes(w, h, samples), dtype=torch.uint8, device="cuda")
        for _ in range(3):
            ctx.preview(p, pv, d_tab, out, d_scr, None, g, scratch)
        torch.cuda.synchronize()
        times = []
        for _ in range(calls):
            t0 = time.perf_counter()
            ctx.preview(p, pv, d_tab, out, d_scr, None, g, scratch)
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        times.sort()
        print(f"preview {w}x{h} K = {samples}: median {times[len(times) // 2]:.3f} ms, min {times[0]:.3f}, max {times[-1]:.3f} per call over {calls} calls", flush=True)
    ctx.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    profile() if args.profile else radius_table()
