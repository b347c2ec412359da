"""Progressive rendering of rayn's shipped scene (rayn_amd.setup, 1280x720, SAMPLES = 2 (8 spp) per epoch, 3 bounces, the BlackmanHarris
filter, 16x16 tiles) with Film.render_progressive: epochs are accumulated on the GPU, tiles whose error estimate has met the target retire
and later epochs render only the tiles still active.  Prints one line per epoch and writes the final PNGs and the sample-count image.

    python examples/render_progressive.py [--out renders_progressive] [--max-epochs 64] [--target-error 0.05] [--non-adaptive]
                                          [--checkpoint FILE] [--resume FILE] [--denoise {atrous,variance}]

--checkpoint writes the state after the last epoch; --resume continues the render such a file was made from (same arguments otherwise).
--denoise also writes the Color image after a denoiser: `atrous` (also a bare --denoise) is the fixed-sigma a-trous filter
(rayn_amd.Denoise() defaults), `variance` the one guided by the per-pixel variance this render measured (rayn_amd.VarianceDenoise()
defaults; it needs at least two epochs)."""
import argparse
import dataclasses
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import rayn_amd as R  # noqa: E402
from rayn_amd import image  # noqa: E402
from rayn_amd import setup as S  # noqa: E402

SAMPLES, MAX_INDIRECT_BOUNCES = 2, 3  # src/setup.rs:16-25
K = R.ChannelKind
CHANNELS = [K.Color, K.Alpha, K.Background, K.WorldNormal]
WRITE = [K.Alpha, K.WorldNormal, K.Color]  # src/main.rs:87-91


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="renders_progressive", help="output folder")
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--frame", type=int, default=1)
    ap.add_argument("--samples", type=int, default=SAMPLES, help="samples per epoch (spp = 4 * samples)")
    ap.add_argument("--max-epochs", type=int, default=None)
    ap.add_argument("--min-epochs", type=int, default=None)
    ap.add_argument("--target-error", type=float, default=None)
    ap.add_argument("--noise-floor", type=float, default=None)
    ap.add_argument("--outlier-permille", type=int, default=None)
    ap.add_argument("--non-adaptive", action="store_true", help="no tile retires: every epoch renders the whole frame")
    ap.add_argument("--checkpoint", default=None, help="write the state to this file after the last epoch")
    ap.add_argument("--resume", default=None, help="continue the render this checkpoint was made from")
    ap.add_argument("--denoise", nargs="?", const="atrous", default=None, choices=("atrous", "variance"),
                    help="also write the denoised Color: atrous = rayn_amd.Denoise(), variance = rayn_amd.VarianceDenoise()")
    args = ap.parse_args()
    given = {k: getattr(args, k) for k in ("max_epochs", "min_epochs", "target_error", "noise_floor", "outlier_permille") if getattr(args, k) is not None}
    prog = dataclasses.replace(R.Progressive(), adaptive=not args.non_adaptive, **given)
    cam, world = S.setup((args.width, args.height))
    integ = R.PathTracingIntegrator(max_bounces=MAX_INDIRECT_BOUNCES, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE)
    filt = R.BlackmanHarrisFilter(S.FILTER_RADIUS)
    film = R.Film(CHANNELS, (args.width, args.height))
    t0 = [time.perf_counter()]

    def on_epoch(r):
        now = time.perf_counter()
        st = r["stats"][-1]
        rendered = st["tiles"]
        print(f"epoch {r['epochs']:4d}: {rendered:6d} tiles rendered in {st['ms_total']:8.2f} ms ({1e3 * (now - t0[0]):8.2f} ms wall), "
              f"{len(r['active_tiles']):6d} still active, {r['totals']['outlier_pixels']:8d} outlier pixels, max e {r['totals']['max_e']:.4f}")
        t0[0] = now

    print(prog)
    start = time.perf_counter()
    rep = film.render_progressive(world, cam, integ, filt, S.TILE_SIZE, args.frame, None, args.samples, prog, on_epoch=on_epoch, resume=args.resume)
    wall = time.perf_counter() - start
    te = rep["tile_epochs"]
    print(f"{rep['epochs']} epochs, {len(rep['stats'])} in this run, in {wall:.3f} s; per-tile epochs min {te.min()} mean {te.mean():.2f} max {te.max()}; "
          f"{rep['paths']} paths traced, {rep['paths_non_adaptive']} for the same epochs over the whole frame "
          f"({rep['paths'] / max(rep['paths_non_adaptive'], 1):.3f}x)")
    base = f"{4 * args.samples}_spp_x{rep['epochs']}"
    film.save_to(WRITE, args.out, base)
    if args.denoise:
        film.save_to([K.Color], args.out, base, denoise=R.VarianceDenoise() if args.denoise == "variance" else R.Denoise())
    image.save(os.path.join(args.out, f"{base}_sample_count.png"), film.sample_count_image()[:, :, None])
    if args.checkpoint:
        film.save_checkpoint(args.checkpoint)
        print(f"checkpoint written to {args.checkpoint}")


if __name__ == "__main__":
    main()
