#!/usr/bin/env python3
"""The measurements of the EXR encoder in DESIGN.md section 8 (needs a GPU; nothing here is a test).

  python tools/exr_measure.py sizes [--width 1280 --height 720]
      The shipped scene's frame (examples/render_sequence.py's settings) and a preview frame through Film.save_exr in every mode, all
      film channels HALF: file bytes, their ratios to "host" (zlib level 6, the same chunks), raw chunks, and the encoder's time between
      device events (warm, the mean of 5).
  rocprofv3 --kernel-trace --stats -d DIR -o exr -- python tools/exr_measure.py kernels
      Enqueues, for 1280x720 and 1920x1080, for RGBA and for all ten film channels, HALF, for both block formats: one warm encode and
      REPEAT timed ones of the shipped scene's frame, in a fixed order.
  python tools/exr_measure.py parse DIR/exr_kernel_trace.csv
      Groups that trace's launches back into the configurations - the order is the one `kernels` enqueues - and prints per configuration
      the mean time of every kernel and the pack kernel's bytes/s on its algorithmic bytes (plane words read + RAW and P written).
"""
import argparse
import csv
import os
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SAMPLES, MAX_INDIRECT_BOUNCES, FRAME = 2, 3, 2   # examples/render_sequence.py
REPEAT = 3
SIZES = ((1280, 720), (1920, 1080))
ENCODER_KERNELS = ("k_exr_pack", "k_png_block", "k_png_lz_block", "k_exr_layout", "k_exr_compact")


def configurations():
    """(width, height, name, lz77) in the order `kernels` enqueues them"""
    return [(w, h, name, lz) for w, h in SIZES for name in ("rgba", "ten") for lz in (False, True)]


def rendered_film(w, h):
    import rayn_amd as R
    from rayn_amd import setup as S
    K = R.ChannelKind
    cam, world = S.setup((w, h))
    film = R.Film([K.Color, K.Alpha, K.Background, K.WorldNormal], (w, h))
    film.render_frame_into(world, cam, R.PathTracingIntegrator(max_bounces=MAX_INDIRECT_BOUNCES, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE),
                           R.BlackmanHarrisFilter(S.FILTER_RADIUS), S.TILE_SIZE, FRAME, None, SAMPLES)
    return R, film, world, cam


def channels_of(R, film, name):
    from rayn_amd import film as F
    K = R.ChannelKind
    return F.exr_channels([K.Color, K.Alpha] if name == "rgba" else list(film.channel_kinds), film.channels, True)


def cmd_kernels(args):
    import torch
    from rayn_amd import film as F
    films = {}
    for w, h, name, lz in configurations():
        if (w, h) not in films:
            films[w, h] = rendered_film(w, h)
        R, film, _, _ = films[w, h]
        chans = channels_of(R, film, name)
        layout = F.exr_layout(chans)
        d_out = torch.empty(F.exr_stream_bound(w, h, layout), dtype=torch.uint8, device=film.device)
        d_scr = torch.empty(F.exr_scratch_bytes(w, h, layout, lz), dtype=torch.uint8, device=film.device)
        for _ in range(1 + REPEAT):
            film.ctx.exr_encode(w, h, chans, d_out, d_scr, lz77=lz)
        torch.cuda.synchronize()
        words = d_out[:16].cpu().numpy().view("<u4")
        print(f"{w}x{h} {name} lz77={int(lz)}: body {words[0]} bytes, {words[1]} chunks, {words[2]} raw, {words[3]} blocks", flush=True)


def cmd_parse(args):
    rows = []
    with open(args.trace) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            kind = next((k for k in ("k_exr_pack", "k_png_lz_block", "k_png_block", "k_exr_layout", "k_exr_compact") if k in name), None)
            segmented = kind is not None and (kind.startswith("k_exr") or "<true>" in name or "ILb1E" in name)  # not the PNG entries' own
            if segmented:
                rows.append((int(r["Start_Timestamp"]), kind, int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    per = 4 * (1 + REPEAT)
    confs = configurations()
    if len(rows) != per * len(confs):
        sys.exit(f"{len(rows)} encoder launches in the trace, {per * len(confs)} expected")
    for c, (w, h, name, lz) in enumerate(confs):
        mine = rows[c * per + 4:(c + 1) * per]  # without the warm encode
        ns = {}
        for _, kind, d in mine:
            ns.setdefault(kind, []).append(d)
        n_ch, size = (4, 8) if name == "rgba" else (10, 20)
        algorithmic = w * h * (4 * n_ch + 2 * size)  # plane words read, RAW and P written
        mean = {k: sum(v) / len(v) / 1e3 for k, v in ns.items()}
        total = sum(mean.values())
        parts = ", ".join(f"{k} {mean[k]:.1f}" for k in ENCODER_KERNELS if k in mean)
        print(f"{w}x{h} {name:4s} lz77={int(lz)}: {total:8.1f} us per image ({parts}); k_exr_pack {algorithmic / (mean['k_exr_pack'] * 1e-6) / 1e12:.2f} TB/s "
              f"on {algorithmic / 1e6:.1f} MB; spread of the total over {REPEAT} images "
              f"{(max(sum(x) for x in zip(*ns.values())) - min(sum(x) for x in zip(*ns.values()))) / 1e3:.1f} us")


def cmd_sizes(args):
    import torch
    from rayn_amd import film as F
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import exr_read
    w, h = args.width, args.height
    R, film, world, cam = rendered_film(w, h)
    preview = film.render_preview(R.Preview())
    with tempfile.TemporaryDirectory() as d:
        for label, f in (("rendered", film), ("preview", preview)):
            sizes = {}
            for mode in F.EXR_ENCODERS:
                path = os.path.join(d, f"{label}_{mode}.exr")
                f.save_exr(path, exr=mode)
                info = {}
                exr_read.read(open(path, "rb").read(), info)
                sizes[mode] = (os.path.getsize(path), sum(1 for c in info["chunks"] if c[3]), len(info["chunks"]))
            chans = F.exr_channels(list(f.channel_kinds), f.channels, True)
            layout = F.exr_layout(chans)
            times = {}
            for lz in (False, True):
                d_out = torch.empty(F.exr_stream_bound(w, h, layout), dtype=torch.uint8, device=f.device)
                d_scr = torch.empty(F.exr_scratch_bytes(w, h, layout, lz), dtype=torch.uint8, device=f.device)
                f.ctx.exr_encode(w, h, chans, d_out, d_scr, lz77=lz)
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(5):
                    f.ctx.exr_encode(w, h, chans, d_out, d_scr, lz77=lz)
                b.record()
                torch.cuda.synchronize()
                times["device-lz77" if lz else "device"] = a.elapsed_time(b) / 5
            raw = w * h * sum(2 for _ in chans)
            print(f"{label} {w}x{h}, {len(chans)} HALF channels, {raw} raw bytes:")
            for mode in F.EXR_ENCODERS:
                n, raws, chunks = sizes[mode]
                t = f", encode {times[mode]:.3f} ms (device events, warm)" if mode in times else ""
                print(f"  {mode:12s} {n:9d} bytes = {n / sizes['host'][0]:.3f} x host, {n / raw:.3f} x raw, {raws} of {chunks} chunks raw{t}")


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
