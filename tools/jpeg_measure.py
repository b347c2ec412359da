#!/usr/bin/env python3
"""The measurements of the JPEG encoder in DESIGN.md section 8 (needs a GPU; nothing here is a test).

  rocprofv3 --kernel-trace --output-format csv -d DIR -o jpeg -- python tools/jpeg_measure.py kernels
      Enqueues, for 1280x720 and 1920x1080, for the shipped scene's rendered Color image and its preview Color image, at quality 90, for
      both subsamplings and the restart intervals 8, 16, 32, 64 and one MCU row: one warm encode and REPEAT timed ones, in a fixed order;
      behind each image's JPEG encodes the device PNG encoder (Context.png_encode) on the same image, the same way.
  python tools/jpeg_measure.py parse DIR/.../jpeg_kernel_trace.csv
      Groups that trace's launches back into the configurations - the order is the one `kernels` enqueues - and prints per configuration
      the mean time of every kernel and the transform kernel's bytes/s on its algorithmic bytes (3 B read per pixel + 2 B per coefficient).
  python tools/jpeg_measure.py sizes [--width 1280 --height 720]
      File bytes of the same two images: the JPEG at quality 90 for both subsamplings and every restart interval above, Pillow's at the
      same quality (libjpeg, optimised tables off, no restart markers), the PNG of png="device" and "device-lz77", and the PSNR of both
      JPEGs' decodes (Pillow) against the 8-bit source.
"""
import argparse
import csv
import io
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SAMPLES, MAX_INDIRECT_BOUNCES, FRAME = 2, 3, 2   # examples/render_sequence.py
REPEAT = 3
QUALITY = 90
SIZES = ((1280, 720), (1920, 1080))
INTERVALS = (8, 16, 32, 64, "row")
JPEG_KERNELS = ("k_jpeg_transform", "k_jpeg_segment", "k_jpeg_layout", "k_jpeg_compact")
PNG_KERNELS = ("k_png_filter", "k_png_block", "k_png_layout", "k_png_compact")


def interval(ri, w, sub):
    return -(-w // (16 if sub else 8)) if ri == "row" else ri


def configurations():
    """(width, height, content, subsampling, restart interval or "png") in the order `kernels` enqueues them"""
    out = []
    for w, h in SIZES:
        for content in ("rendered", "preview"):
            out += [(w, h, content, sub, ri) for sub in (0, 1) for ri in INTERVALS] + [(w, h, content, None, "png")]
    return out


def images(w, h):
    """{"rendered", "preview"}: the 8-bit Color image of the shipped scene's frame on the device, (tensor, bytes per pixel)"""
    import torch
    import rayn_amd as R
    from rayn_amd import setup as S
    K = R.ChannelKind
    cam, world = S.setup((w, h))
    film = R.Film([K.Color, K.Alpha, K.Background, K.WorldNormal], (w, h))
    film.render_frame_into(world, cam, R.PathTracingIntegrator(max_bounces=MAX_INDIRECT_BOUNCES, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE),
                           R.BlackmanHarrisFilter(S.FILTER_RADIUS), S.TILE_SIZE, FRAME, None, SAMPLES)
    preview = film.render_preview(R.Preview())
    with torch.cuda.device(film.device):
        return film, {"rendered": film._pixels_device(K.Color, False, None, None), "preview": preview._pixels_device(K.Color, False, None, None)}


def cmd_kernels(args):
    import torch
    from rayn_amd import film as F
    made = {}
    for w, h, content, sub, ri in configurations():
        if (w, h) not in made:
            made[w, h] = images(w, h)
        film, imgs = made[w, h]
        d_img, bpp = imgs[content]
        if ri == "png":
            d_out = torch.empty(F.png_stream_bound(w, h, bpp), dtype=torch.uint8, device=film.device)
            d_scr = torch.empty(F.png_scratch_bytes(w, h, bpp), dtype=torch.uint8, device=film.device)
            for _ in range(1 + REPEAT):
                film.ctx.png_encode(w, h, bpp, d_img, d_out, d_scr)
        else:
            r = interval(ri, w, sub)
            d_out = torch.empty(F.jpeg_scan_bound(w, h, bpp, sub, r), dtype=torch.uint8, device=film.device)
            d_scr = torch.empty(F.jpeg_scratch_bytes(w, h, bpp, sub, r), dtype=torch.uint8, device=film.device)
            for _ in range(1 + REPEAT):
                film.ctx.jpeg_encode(w, h, bpp, d_img, d_out, QUALITY, sub, r, d_scr)
        torch.cuda.synchronize()
        words = d_out[:16].cpu().numpy().view("<u4")
        print(f"{w}x{h} {content} sub={sub} ri={ri}: {words[0]} bytes, header {[int(v) for v in words[1:]]}", flush=True)


def cmd_parse(args):
    rows = []
    with open(args.trace) as f:
        for r in csv.DictReader(f):
            kind = next((k for k in JPEG_KERNELS + PNG_KERNELS if k in r["Kernel_Name"]), None)
            if kind is not None:
                rows.append((int(r["Start_Timestamp"]), kind, int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    confs = configurations()
    per = 4 * (1 + REPEAT)
    if len(rows) != per * len(confs):
        sys.exit(f"{len(rows)} encoder launches in the trace, {per * len(confs)} expected")
    for c, (w, h, content, sub, ri) in enumerate(confs):
        mine = rows[c * per + 4:(c + 1) * per]  # without the warm encode
        kernels = PNG_KERNELS if ri == "png" else JPEG_KERNELS
        assert [k for _, k, _ in mine] == list(kernels) * REPEAT, (c, [k for _, k, _ in mine])
        mean = {k: sum(d for _, kk, d in mine if kk == k) / REPEAT / 1e3 for k in kernels}
        totals = [sum(d for _, _, d in mine[4 * i:4 * i + 4]) / 1e3 for i in range(REPEAT)]
        parts = ", ".join(f"{k} {mean[k]:.1f}" for k in kernels)
        line = f"{w}x{h} {content:8s} {'png device' if ri == 'png' else f'sub={sub} ri={ri}':14s}: {sum(mean.values()):8.1f} us per image ({parts}); spread {max(totals) - min(totals):.1f} us"
        if ri != "png":
            side = 16 if sub else 8
            mcus = -(-w // side) * -(-h // side)
            algorithmic = 3 * w * h + 128 * mcus * (6 if sub else 3)
            line += f"; k_jpeg_transform {algorithmic / (mean['k_jpeg_transform'] * 1e-6) / 1e12:.3f} TB/s on {algorithmic / 1e6:.1f} MB"
        print(line)


def _psnr(a, b):
    import numpy as np
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def cmd_sizes(args):
    import numpy as np
    import torch
    from PIL import Image
    import rayn_amd as R
    from rayn_amd import film as F
    from rayn_amd import image
    w, h = args.width, args.height
    film, imgs = images(w, h)
    for content, (d_img, bpp) in imgs.items():
        src = d_img.cpu().numpy().reshape(h, w, bpp)
        print(f"{content} {w}x{h}, {src.size} raw bytes:")
        for lz in (False, True):
            d_out = torch.empty(F.png_stream_bound(w, h, bpp), dtype=torch.uint8, device=film.device)
            film.ctx.png_encode(w, h, bpp, d_img, d_out, lz77=lz)
            n = len(image.png_from_stream(w, h, bpp, image.png_stream_of(d_out.cpu().numpy())))
            print(f"  png {'device-lz77' if lz else 'device':12s} {n:9d} bytes")
        for sub in (0, 1):
            b = io.BytesIO()
            Image.fromarray(src).save(b, "JPEG", quality=QUALITY, subsampling=2 if sub else 0)
            pil = np.asarray(Image.open(io.BytesIO(b.getvalue())).convert("RGB"))
            print(f"  Pillow q{QUALITY} {'4:2:0' if sub else '4:4:4'} {len(b.getvalue()):9d} bytes, PSNR {_psnr(pil, src):.2f} dB")
            for ri in INTERVALS:
                options = R.Jpeg(QUALITY, "420" if sub else "444", interval(ri, w, sub))
                d_out = torch.empty(F.jpeg_scan_bound(w, h, bpp, sub, options.restart), dtype=torch.uint8, device=film.device)
                film.ctx.jpeg_encode(w, h, bpp, d_img, d_out, QUALITY, sub, options.restart)
                data = image.jpeg_from_scan(w, h, bpp, options, d_out.cpu().numpy())
                dec = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
                print(f"  jpeg q{QUALITY} {'4:2:0' if sub else '4:4:4'} ri={str(ri):3s} {len(data):9d} bytes = {len(data) / len(b.getvalue()):.3f} x Pillow, PSNR {_psnr(dec, src):.2f} dB")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("sizes")
    s.add_argument("--width", type=int, default=1280)
    s.add_argument("--height", type=int, default=720)
    sub.add_parser("kernels")
    p = sub.add_parser("parse")
    p.add_argument("trace")
    args = ap.parse_args()
    {"sizes": cmd_sizes, "kernels": cmd_kernels, "parse": cmd_parse}[args.cmd](args)


if __name__ == "__main__":
    main()
