#!/usr/bin/env python3
"""What the frame generation (rayn_amd.Interpolate, rayn_hip_interpolate_device) is worth, and how its depth tolerance was confirmed
(DESIGN.md section 8), on the CPU: the oracle renders the frames 1..5 of tests/interpolate_np.InterpCase - the shipped scene at 160x96 under
a camera drift fast enough that the image moves several pixels between keys - at samples=2 (8 spp) and at samples=256, the oracle's closest
hit gives every frame's G-buffer, and the numpy restatement of the kernel (tests/interpolate_np.py) generates the in-between frames for
every = 2 and 4.  Score: the MSE of the saturated Color + Background of a generated frame against the samples=256 render of that frame, as
a ratio to the truly rendered 8-spp frame's; beside it the plain cross-fade of the two keys and the nearer key held.

    python tools/interpolate_defaults.py            # the tables
    python tools/interpolate_defaults.py --defaults # the rows of Interpolate()'s tolerance only (what tests/test_interpolate_device.py cites)
    python tools/interpolate_defaults.py --profile  # GPU, no scoring: 20 generated frames at 1280x720 and at 1920x1080 for a kernel trace,
                                                    # and their wall time per call around a device synchronise
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import interpolate_np as I  # noqa: E402
import temporal_np as T  # noqa: E402

D, IC = T.DefaultsCase, I.InterpCase
W, H = D.W, D.H


def cpu_frames(oracle, samples):
    """(world description, {frame: (params, film, G-buffer)}) from the CPU oracle"""
    wd, ps = IC.scene(samples)
    out = {}
    for f, p in ps.items():
        film, _ = oracle.render(wd, p, oracle.build_tables(4 * samples, D.BOUNCES, p.volume_marches, p.frame, W, H))
        out[f] = (p, film, T.gbuffer_oracle(oracle, wd, p))
    return wd, out


def generate(wd, frames, f, fa, fb, tol):
    (pa, film_a, ga), (pb, film_b, gb), (pt, _, gt) = frames[fa], frames[fb], frames[f]
    ka = I.Key({k: film_a[k] for k in ("color", "background")}, ga[0], ga[1], wd.camera, pa.time_start)
    kb = I.Key({k: film_b[k] for k in ("color", "background")}, gb[0], gb[1], wd.camera, pb.time_start)
    return I.interpolate(W, H, ka, kb, gt[0], gt[1], pt.time_start, T.world_hitables(wd), tol)


def motion(wd, frames, f, fk):
    """mean |fx - X| over the hit pixels of frame f projected into key fk"""
    rec, obj = frames[f][2]
    ok, fx, _, _ = T.project(wd.camera, frames[fk][0].time_start, [rec[:, 0], rec[:, 1], rec[:, 2]], W, H)
    xs = np.meshgrid(np.arange(W), np.arange(H), indexing="xy")[0].reshape(-1)
    m = ok & (obj != T.MISS)
    return float(np.abs(fx[m] - xs[m]).mean())


def rows(wd, keys, noisy, want, every, tol):
    """[(frame, guided, cross-fade, nearer key, source shares, motion)] as ratios to the rendered 8-spp frame"""
    out = []
    for f, fa, fb in IC.keys_of(every):
        raw = noisy[f][1]
        base = D.mse(raw["color"], raw["background"], want[f])
        g, src = generate(wd, keys, f, fa, fb, tol)
        ta, tb, ts = keys[fa][0].time_start, keys[fb][0].time_start, keys[f][0].time_start
        x = IC.cross_fade(keys[fa][1], keys[fb][1], ta, tb, ts)
        near = keys[fa][1] if ts - ta <= tb - ts else keys[fb][1]
        out.append((f, D.mse(g["color"], g["background"], want[f]) / base, D.mse(x["color"], x["background"], want[f]) / base,
                    D.mse(near["color"], near["background"], want[f]) / base, np.bincount(src, minlength=5) / src.size, motion(wd, keys, f, fa)))
    return out


def show(title, table):
    print(title)
    for f, g, x, near, share, mot in table:
        mark = "" if g < x else "  **no gain over the cross-fade**"
        print(f"  frame {f}: guided {g:.4f}x  cross-fade {x:.4f}x  nearer key {near:.4f}x  sources " + " ".join(f"{s:.3f}" for s in share)
              + f"  mean |fx - X| {mot:.2f} px{mark}", flush=True)


def counted_bytes(n):
    """The algorithmic traffic of one call over n pixels with all four planes, every byte counted once: the pixel's guide (16 + 4), both
    keys' objects, depths and planes (2 x (4 + 4 + 40)) and the planes written (40)."""
    return n * (20 + 2 * 48 + 40)


def profile(calls=20):
    import torch
    import rayn_amd as R
    from rayn_amd import film as F
    from rayn_amd import setup as S
    from rayn_amd.scene import Linear
    for w, h in ((1280, 720), (1920, 1080)):
        cam, world = S.setup((w, h))
        c = world.cameras.get(cam)
        c.origin = Linear(c.origin, R.vec3(*IC.DRIFT))
        desc = world.to_desc(cam)
        ctx = R.Context(0)
        ctx.upload_world(desc)
        ps = [R.frame_params(w, h, 1, 1, frame=f) for f in (1, 2, 3)]
        keys = []
        for p in (ps[0], ps[2]):
            film, g = F.alloc_device_film(w, h, "cuda"), F.alloc_gbuffer(w, h, "cuda")
            ctx.render_device(p, [torch.from_numpy(t).cuda() for t in R.build_tables(4, 1, p.volume_marches, p.frame, w, h)], film)
            ctx.gbuffer(p, g)
            keys.append((film, g, desc.camera, p.time_start))
        g_t, out = F.alloc_gbuffer(w, h, "cuda"), F.alloc_device_film(w, h, "cuda")
        src = torch.empty(w * h, dtype=torch.int32, device="cuda")
        ctx.gbuffer(ps[1], g_t)
        itp = R.Interpolate()
        ctx.interpolate(ps[1], itp, keys[0], keys[1], g_t, out, src)  # warm
        torch.cuda.synchronize()
        share = np.bincount(src.cpu().numpy(), minlength=5) / (w * h)
        times = []
        for _ in range(calls):
            t0 = time.perf_counter()
            ctx.interpolate(ps[1], itp, keys[0], keys[1], g_t, out)
            torch.cuda.synchronize()
            times.append(1e6 * (time.perf_counter() - t0))
        print(f"{w}x{h}: {calls} calls, wall per call median {np.median(times):.1f} us (min {min(times):.1f}, max {max(times):.1f}); counted bytes "
              f"{counted_bytes(w * h) / 1e6:.1f} MB; sources " + " ".join(f"{s:.3f}" for s in share), flush=True)
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--defaults", action="store_true")
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    if args.profile:
        return profile()
    import rayn_amd as R
    from oracle import oracle_py
    oracle_py.build()
    wd, noisy = cpu_frames(oracle_py, D.SAMPLES)
    _, clean = cpu_frames(oracle_py, D.REF_SAMPLES)
    want = {f: np.clip(clean[f][1]["color"].astype(np.float64) + clean[f][1]["background"], 0.0, 1.0) for f in clean}
    tol = R.Interpolate().depth_tolerance
    print(f"drift {IC.DRIFT} per second, {IC.RATE} frames a second, {W}x{H}, keys at {4 * D.SAMPLES} spp, reference {4 * D.REF_SAMPLES} spp")
    for every in (2, 4):
        show(f"every = {every}, depth_tolerance {tol}, {4 * D.SAMPLES}-spp keys", rows(wd, noisy, noisy, want, every, tol))
        show(f"every = {every}, depth_tolerance {tol}, {4 * D.REF_SAMPLES}-spp keys (geometry error without noise)", rows(wd, clean, noisy, want, every, tol))
    if args.defaults:
        return
    print("depth_tolerance grid: mean guided ratio over the generated frames (8-spp keys | 1024-spp keys)")
    for t in (0.0025, 0.01, 0.05, 0.25, 1.0):
        cells = []
        for every in (2, 4):
            for keys in (noisy, clean):
                cells.append(float(np.mean([r[1] for r in rows(wd, keys, noisy, want, every, t)])))
        print(f"  depth_tolerance {t:6.4f}: every 2: {cells[0]:.4f}x | {cells[1]:.4f}x   every 4: {cells[2]:.4f}x | {cells[3]:.4f}x", flush=True)


if __name__ == "__main__":
    main()
