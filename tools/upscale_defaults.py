#!/usr/bin/env python3
"""How the defaults of rayn_amd.Upscale were chosen and what guided upscaling buys, on the GPU.  Per scene - the
shipped one (rayn_amd.setup) and the sphere scene s0, whose image is dominated by silhouettes - a low film of 160x96 at 32 spp is upscaled
by 2 and scored against a native 320x192 render at 1024 spp: the MSE of the saturated Color + Background of
  (a) the low film through Upscale(2, sigma_plane, sigma_position),
  (b) the low film through plain bilinear: the same entry with every high pixel given an object no tap shows, tier 2 everywhere,
  (c) a native 320x192 render at 8 spp - the paths of (a),
  (d) (c) through Denoise().

    python tools/upscale_defaults.py            # the four images for both scenes at the shipped defaults, then the sigma grid over (a)
    python tools/upscale_defaults.py --defaults # the four images for both scenes, no grid
    python tools/upscale_defaults.py --small    # (a) / (b) on s0 at 80x48 -> 160x96 against 256 spp: the size a test could afford
    python tools/upscale_defaults.py --profile  # no scoring: the G-buffer passes and the kernel at 640x360 -> 1280x720 and
                                                # 960x540 -> 1920x1080, 20 times each, for a kernel trace
"""
import argparse
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import rayn_amd as R  # noqa: E402
from rayn_amd import film as F  # noqa: E402
from rayn_amd import setup as S  # noqa: E402

BOUNCES = 3
K = R.ChannelKind
KINDS = [K.Color, K.Alpha, K.Background, K.WorldNormal]


def render(scene, res, samples, frame=1):
    cam, world = S.SCENES[scene](res)
    film = R.Film(KINDS, res)
    film.render_frame_into(world, cam, R.PathTracingIntegrator(max_bounces=BOUNCES, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE),
                           R.BlackmanHarrisFilter(S.FILTER_RADIUS), S.TILE_SIZE, frame, None, samples)
    return film


def saturated(color, background, res):
    w, h = res
    return np.clip(np.asarray(color, np.float64).reshape(h, w, 3) + np.asarray(background, np.float64).reshape(h, w, 3), 0.0, 1.0)


def film_image(film):
    return saturated(film.channel(K.Color), film.channel(K.Background), film.res)


class Case:
    """One low film with both G-buffers on the device, and the reference image."""

    def __init__(self, scene, low_res, s, low_samples, ref_samples):
        import torch
        self.s, self.low_res, self.res = s, low_res, (low_res[0] * s, low_res[1] * s)
        self.want = film_image(render(scene, self.res, ref_samples))
        self.low = render(scene, low_res, low_samples)
        p = self.low._last_params
        self.p = p
        w, h = low_res
        W, H = self.res
        self.g_low, self.g_high = F.alloc_gbuffer(w, h, self.low.device), F.alloc_gbuffer(W, H, self.low.device)
        self.low.ctx.gbuffer(p, self.g_low)
        self.low.ctx.gbuffer(F._scaled_params(p, s), self.g_high)
        self.g_none = dict(self.g_high, object=torch.full_like(self.g_high["object"], -2))  # 0xFFFFFFFE: an object no tap shows
        self.out = F.alloc_device_film(W, H, self.low.device)

    def mse(self, img):
        return float(np.mean((img - self.want) ** 2))

    def upscaled(self, up, bilinear=False):
        self.low.ctx.upscale(self.p, up, self.low.channels, self.g_low, self.g_none if bilinear else self.g_high, self.out)
        return self.mse(saturated(self.out["color"].cpu().numpy(), self.out["background"].cpu().numpy(), self.res))


def four_images(scene, low_res=(160, 96), s=2, low_samples=8, native_samples=2, ref_samples=256):
    c = Case(scene, low_res, s, low_samples, ref_samples)
    d = R.Upscale(s)
    a, b = c.upscaled(d), c.upscaled(d, bilinear=True)
    native = render(scene, c.res, native_samples)
    cc = c.mse(film_image(native))
    dd = c.mse(saturated(native.denoised_color(R.Denoise()).cpu().numpy(), native.channel(K.Background), c.res))
    print(f"{scene}: {low_res[0]}x{low_res[1]} at {4 * low_samples} spp -> x{s}, against {4 * ref_samples} spp; Upscale() = ({d.sigma_plane}, {d.sigma_position})")
    print(f"  MSE (a) guided {a:.6e}  (b) bilinear {b:.6e}  (c) native {4 * native_samples} spp {cc:.6e}  (d) native denoised {dd:.6e}")
    print(f"  ratios (a)/(c) {a / cc:.4f}  (b)/(c) {b / cc:.4f}  (d)/(c) {dd / cc:.4f}  (a)/(b) {a / b:.4f}", flush=True)
    return c, cc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--defaults", action="store_true")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    if args.profile:
        import torch
        for low_res in ((640, 360), (960, 540)):
            low = render("ship", low_res, 1)
            p, s = low._last_params, 2
            W, H = low_res[0] * s, low_res[1] * s
            g_low, g_high = F.alloc_gbuffer(*low_res, low.device), F.alloc_gbuffer(W, H, low.device)
            scratch = torch.empty(F.gbuffer_scratch_bytes(W, H), dtype=torch.uint8, device=low.device)
            out = F.alloc_device_film(W, H, low.device)
            for _ in range(20):
                low.ctx.gbuffer(p, g_low, scratch)
                low.ctx.gbuffer(F._scaled_params(p, s), g_high, scratch)
                low.ctx.upscale(p, R.Upscale(s), low.channels, g_low, g_high, out)
            torch.cuda.synchronize()
            print(f"profiled {low_res} -> {(W, H)}")
        return
    if args.small:
        for scene in ("s0", "ship"):
            c = Case(scene, (80, 48), 2, 8, 64)
            for d in (R.Upscale(2), R.Upscale(2, 0.02, 0.0)):
                a, b = c.upscaled(d), c.upscaled(d, bilinear=True)
                print(f"{scene} 80x48 at 32 spp -> x2 against 256 spp, ({d.sigma_plane}, {d.sigma_position}): (a) {a:.6e} (b) {b:.6e} (a)/(b) {a / b:.4f}", flush=True)
        return
    for scene in ("ship", "s0"):
        c, cc = four_images(scene)
        if args.defaults:
            continue
        for sp, ss in itertools.product((0.0, 0.005, 0.01, 0.02, 0.05, 0.1, 0.3), (0.0, 0.01, 0.02, 0.05, 0.1, 0.3)):
            print(f"  sigma_plane {sp:5.3f} sigma_position {ss:5.3f}: (a)/(c) {c.upscaled(R.Upscale(2, sp, ss)) / cc:.4f}", flush=True)


if __name__ == "__main__":
    main()
