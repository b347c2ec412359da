#!/usr/bin/env python3
"""How the defaults of rayn_amd.Supersample were chosen and what temporal supersampling buys, on the GPU.  Per scene
- the shipped one (rayn_amd.setup) and the sphere scene s0, whose noise is low and whose error is lost resolution - and per camera - the
moving one of the temporal sections (the origin drifts by (0.9, -0.3, 0.15) per unit of time) and a static one - 8 frames are rendered at
160x96 with 32 spp (the paths of a native 320x192 frame at 8 spp), rebuilt at 320x192, and the LAST frame is scored against a native 320x192
render of it at 1024 spp: the MSE of the saturated Color + Background of
  (a) Upscale(2) alone, the last frame on its own,
  (b) the composition: Supersample(jitter=False, confidence=False) - Upscale(2), then Temporal() at the high size,
  (c) jitter alone: Supersample(jitter=True, confidence=False),
  (d) jitter + confidence: Supersample(jitter=True, confidence=True),
  (e) native Temporal(): 8 frames rendered at 320x192 with 8 spp and accumulated at that size,
each as a ratio to (n), the last native 320x192 frame at 8 spp on its own.

    python tools/supersample_defaults.py             # the table
    python tools/supersample_defaults.py --profile   # no scoring: at 640x360 -> 1280x720 and 960x540 -> 1920x1080, 20 times each, k_upscale
                                                     # + k_temporal_accumulate at the high size and k_temporal_upscale with and without a
                                                     # low camera, all with a previous history, for a kernel trace
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import rayn_amd as R  # noqa: E402
from rayn_amd import film as F  # noqa: E402
from rayn_amd import setup as S  # noqa: E402
from rayn_amd.scene import Linear  # noqa: E402

BOUNCES = 3
LOW, FACTOR, FRAMES = (160, 96), 2, list(range(1, 9))
LOW_SAMPLES, NATIVE_SAMPLES, REF_SAMPLES = 8, 2, 256  # x 4 spp


def scene(name, res, moving):
    cam, world = S.SCENES[name](res)
    if moving:
        c = world.cameras.get(cam)
        c.origin = Linear(c.origin, R.vec3(0.9, -0.3, 0.15))
    return world.to_desc(cam)


def render(ctx, desc, res, samples, frame):
    """One frame through the camera of `desc` (uploaded here): (device film, frame params)."""
    import torch
    p = R.frame_params(res[0], res[1], samples, BOUNCES, frame=frame)
    ctx.upload_world(desc)
    out = F.alloc_device_film(res[0], res[1], "cuda")
    ctx.render_device(p, [torch.from_numpy(t).cuda() for t in R.build_tables(4 * samples, BOUNCES, p.volume_marches, frame, res[0], res[1])], out)
    return out, p


def saturated(color, background, res):
    w, h = res
    return np.clip(color.cpu().numpy().reshape(h, w, 3).astype(np.float64) + background.cpu().numpy().reshape(h, w, 3), 0.0, 1.0)


def supersampled(ctx, name, moving, sup, up, tp):
    """The last frame of the sequence through Context.temporal_upscale: the saturated image."""
    import torch
    (w, h), s = LOW, up.factor
    W, H = w * s, h * s
    desc = scene(name, LOW, moving)
    hist = [torch.empty(F.temporal_history_bytes(W, H), dtype=torch.uint8, device="cuda") for _ in range(2)]
    g_low, g_high, out = F.alloc_gbuffer(w, h, "cuda"), F.alloc_gbuffer(W, H, "cuda"), F.alloc_device_film(W, H, "cuda")
    prev_start = None
    for i, frame in enumerate(FRAMES):
        low = type(desc).from_buffer_copy(desc)
        p0 = R.frame_params(w, h, LOW_SAMPLES, BOUNCES, frame=frame)
        if sup.jitter:
            low.camera = F.jittered_camera(desc.camera, *sup.offset(s, i), p0.time_start)
        film, p = render(ctx, low, LOW, LOW_SAMPLES, frame)
        ctx.gbuffer(p, g_low)
        ctx.upload_world(desc)
        ctx.gbuffer(F._scaled_params(p, s), g_high)
        ctx.temporal_upscale(p, up, tp, sup, film, g_low, g_high, None if i == 0 else hist[(i + 1) % 2], None if i == 0 else desc.camera,
                             0.0 if i == 0 else prev_start, hist[i % 2], out, low.camera if sup.jitter else None)
        prev_start = p.time_start
    return saturated(out["color"], out["background"], (W, H))


def table(name, moving):
    import torch
    ctx = R.Context(0)
    try:
        (w, h), s = LOW, FACTOR
        res = (w * s, h * s)
        up, tp = R.Upscale(s), R.Temporal()
        ref, _ = render(ctx, scene(name, res, moving), res, REF_SAMPLES, FRAMES[-1])
        want = saturated(ref["color"], ref["background"], res)
        mse = lambda img: float(np.mean((img - want) ** 2))
        # (n) and (e): native frames at 8 spp, the last one alone and all of them accumulated
        desc = scene(name, res, moving)
        hist = [torch.empty(F.temporal_history_bytes(*res), dtype=torch.uint8, device="cuda") for _ in range(2)]
        g, acc, prev_start = F.alloc_gbuffer(*res, "cuda"), torch.empty(res[0] * res[1], 3, dtype=torch.float32, device="cuda"), None
        for i, frame in enumerate(FRAMES):
            film, p = render(ctx, desc, res, NATIVE_SAMPLES, frame)
            ctx.gbuffer(p, g)
            ctx.temporal_accumulate(p, tp, film, g, None if i == 0 else hist[(i + 1) % 2], None if i == 0 else desc.camera, 0.0 if i == 0 else prev_start,
                                    hist[i % 2], acc)
            prev_start = p.time_start
        n, e = mse(saturated(film["color"], film["background"], res)), mse(saturated(acc, film["background"], res))
        # (a): the last low frame through Upscale alone
        low_desc = scene(name, LOW, moving)
        film, p = render(ctx, low_desc, LOW, LOW_SAMPLES, FRAMES[-1])
        g_low, g_high, out = F.alloc_gbuffer(w, h, "cuda"), F.alloc_gbuffer(*res, "cuda"), F.alloc_device_film(*res, "cuda")
        ctx.gbuffer(p, g_low)
        ctx.gbuffer(F._scaled_params(p, s), g_high)
        ctx.upscale(p, up, film, g_low, g_high, out)
        a = mse(saturated(out["color"], out["background"], res))
        rows = [("(a) Upscale alone", a)]
        for label, sup in (("(b) composition", R.Supersample(jitter=False, confidence=False)), ("(c) jitter", R.Supersample(jitter=True, confidence=False)),
                           ("(d) jitter + confidence", R.Supersample(jitter=True, confidence=True))):
            rows.append((label, mse(supersampled(ctx, name, moving, sup, up, tp))))
        rows.append(("(e) native Temporal()", e))
        print(f"{name}, {'moving' if moving else 'static'} camera: {w}x{h} at {4 * LOW_SAMPLES} spp -> x{s}, {len(FRAMES)} frames, last frame against {4 * REF_SAMPLES} spp; "
              f"(n) native {4 * NATIVE_SAMPLES} spp MSE {n:.6e}")
        for label, v in rows:
            print(f"  {label:26s} MSE {v:.6e}  ratio to (n) {v / n:.4f}", flush=True)
    finally:
        ctx.close()


def profile():
    import torch
    ctx = R.Context(0)
    try:
        for low_res in ((640, 360), (960, 540)):
            s = 2
            w, h = low_res
            W, H = w * s, h * s
            desc = scene("ship", low_res, True)
            up, tp = R.Upscale(s), R.Temporal()
            film, p = render(ctx, desc, low_res, 1, 1)
            ph = F._scaled_params(p, s)
            g_low, g_high = F.alloc_gbuffer(w, h, "cuda"), F.alloc_gbuffer(W, H, "cuda")
            scratch = torch.empty(F.gbuffer_scratch_bytes(W, H), dtype=torch.uint8, device="cuda")
            ctx.gbuffer(p, g_low, scratch)
            ctx.gbuffer(ph, g_high, scratch)
            hist = [torch.empty(F.temporal_history_bytes(W, H), dtype=torch.uint8, device="cuda") for _ in range(2)]
            out, acc = F.alloc_device_film(W, H, "cuda"), torch.empty(W * H, 3, dtype=torch.float32, device="cuda")
            ctx.upscale(p, up, film, g_low, g_high, out)
            ctx.temporal_accumulate(ph, tp, out, g_high, None, None, 0.0, hist[0], acc)  # a history to reproject
            low_cam = F.jittered_camera(desc.camera, 0.25, -0.25, p.time_start)
            for _ in range(20):
                ctx.upscale(p, up, film, g_low, g_high, out)
                ctx.temporal_accumulate(ph, tp, out, g_high, hist[0], desc.camera, p.time_start, hist[1], acc)
                ctx.temporal_upscale(p, up, tp, R.Supersample(jitter=False, confidence=False), film, g_low, g_high, hist[0], desc.camera, p.time_start, hist[1], out)
                ctx.temporal_upscale(p, up, tp, R.Supersample(), film, g_low, g_high, hist[0], desc.camera, p.time_start, hist[1], out, low_cam)
            torch.cuda.synchronize()
            print(f"profiled {low_res} -> {(W, H)}")
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    if args.profile:
        return profile()
    for name in ("ship", "s0"):
        for moving in (True, False):
            table(name, moving)


if __name__ == "__main__":
    main()
