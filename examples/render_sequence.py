"""rayn's main loop (src/main.rs:47-96) over a frame range on the GPU with Film.render_sequence: rayn's shipped scene
(rayn_amd.setup, 1280x720, SAMPLES = 2 (8 spp), 3 bounces, the BlackmanHarris filter, 16x16 tiles) rendered frame by frame and
written as PNGs (Alpha, WorldNormal, Color, as rayn's main writes them).  Prints per-frame render times and frames/s.

    python examples/render_sequence.py --frames 1:49 [--out renders_seq] [--compare-loop | --denoise [atrous|variance]] [--temporal] [--feedback B]
                                      [--resample {bilinear,catmull_rom}] [--display [--exposure auto|EV] [--tone T] [--bloom LEVELS] [--adaptation S]]
                                      [--upscale S [--temporal --supersample [--no-jitter] [--confidence | --no-confidence]]]
                                      [--preview [K] [--ao-radius R]] [--interpolate K [--interp-tolerance D]] [--png {host,device,device-lz77}]
                                      [--exr {host,device,device-lz77} [--exr-float]]

--compare-loop also times the plain loop on the same frames: Film.render_frame_into, then the host post-process (the film copied to
the host channel by channel and rayn_amd.image's numpy arms, as Film.save_to did before it ran on the device), and checks that
both loops wrote the same bytes.  --denoise runs the a-trous denoiser (rayn_amd.Denoise() defaults, an extension) on every frame's
Color before its post-process and writes _color_denoised.png instead of _color.png.  --temporal accumulates every frame's Color over the
frames before it (rayn_amd.Temporal() defaults, an extension: a primary-hit G-buffer pass and a reprojection per frame) under a camera whose
origin drifts, and writes _color_temporal.png (_color_temporal_denoised.png with --denoise).  --temporal --denoise variance filters the
accumulated colour with the variance-guided denoiser instead, its variance estimated from luminance moments the accumulate carries along
(rayn_amd.VarianceDenoise(1, 4.0, 0.4, 0.3), the setting recommended for sequences); it needs --temporal.  --feedback B (in [0, 1],
default 0 = off) also blends the output of every frame's first a-trous pass into the history the next frame reprojects, with strength B
(rayn_amd.Temporal(feedback=B)); it needs --temporal --denoise variance.  --resample catmull_rom resamples the history with the 4x4
Catmull-Rom filter instead of the bilinear one wherever the whole footprint is valid (rayn_amd.Temporal(resample=...)); it needs --temporal.
--display sends every frame's Color through the HDR display transform (rayn_amd.Display, an extension) after whatever else is on and writes
_display after the Color file's suffix: --exposure auto (the default) or an EV, --tone aces|reinhard|linear, --bloom LEVELS (0 = off, the
default; rayn_amd.Bloom() defaults otherwise) and --adaptation SECONDS (auto exposure follows the frames with this time constant).
--upscale S (1..8) renders every frame at --width x --height and rebuilds it on the device at S times that size, guided by the primary-hit
G-buffer traced at both resolutions (rayn_amd.Upscale(S) defaults, an extension); every written image is the high one and gets _xS after
its suffix; --denoise atrous and --display then work on the upscaled film.  It does not combine with --compare-loop, and with --temporal
only through --supersample: the temporal history then lives at the upscaled size and every low frame is rendered through a camera offset
by a fraction of a low pixel, so that over S * S frames every high pixel has had a sample at its own centre (rayn_amd.Supersample()
defaults, an extension: jitter on, confidence off); --no-jitter switches the jitter off, --confidence weighs every frame by its nearest low
sample and --no-confidence says the default aloud.  The Color file is _color_temporal_xS.png.
--preview [K] runs the preview integrator in place of the render (rayn_amd.Preview, an extension): every frame is the geometry alone -
primary hit, viewer-facing normal and the ambient occlusion of K rays per pixel (default rayn_amd.Preview().samples) of length --ao-radius R
(default rayn_amd.Preview().radius) - and the Color file gets _preview right after _color.  --temporal, --denoise atrous and --display work
on it; --upscale, --denoise variance and --compare-loop do not combine with it.
--interpolate K (2..16) renders only every K-th frame of the range, and the last, and generates the frames between two rendered keys from
them (rayn_amd.Interpolate(K), an extension): each generated frame traces its own primary-hit G-buffer, projects every pixel's hit into
both keys and blends the taps that show the same surface by time; --interp-tolerance D is the relative depth tolerance of a tap (default
rayn_amd.Interpolate().depth_tolerance).  The camera's origin drifts as for --temporal, every Color file gets _interp right after _color,
and --denoise atrous and --display work on the generated frames too; --temporal, --upscale, --preview, --denoise variance and
--compare-loop do not combine with it.
--png device encodes every file's stream on the device (Film.render_sequence(png="device"), an extension: adaptive row filters, run-length
and Huffman coding; the writer threads only frame it) instead of calling zlib on the host; the files keep their names and pixels, not
their bytes, so it does not combine with --compare-loop.  --png device-lz77 is the same with the encoder that also finds LZ77 matches
(png="device-lz77"): about twice the encoder time, smaller Color files - much smaller with --preview - and larger masks and normals.  The
total size of the written files is printed for every encoder.
--exr also writes one multi-channel OpenEXR file per frame (Film.render_sequence(exr=...), an extension: the written channels as HALF
layers, FLOAT with --exr-float, ZIP-compressed scanlines): device encodes the chunks on the render stream (Context.exr_encode),
device-lz77 the same with LZ77 matches, host calls zlib in the writer threads.  The PNGs do not change; the EXR files' total size is
printed on its own.
--jpeg [Q] also writes a baseline JPEG next to every PNG, same name, .jpg (Film.render_sequence(jpeg=rayn_amd.Jpeg(Q)), an extension: the scan
is encoded on the render stream, quality Q, default 90, 4:2:0; --jpeg-444 keeps the chroma at full size).  --video PATH also writes one
Motion-JPEG AVI of the frames' Color image with the same parameters (video=rayn_amd.Video(PATH)); with --no-images the video is all the
call writes.  The .jpg files' total size and the video's are printed on their own.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import rayn_amd as R  # noqa: E402
from rayn_amd import image  # noqa: E402
from rayn_amd import setup as S  # noqa: E402
from rayn_amd.scene import Linear  # noqa: E402

SAMPLES, MAX_INDIRECT_BOUNCES = 2, 3  # src/setup.rs:16-25
FRAME_RATE, SHUTTER_SPEED = 24, 1.0 / 24.0  # src/main.rs:47-49
K = R.ChannelKind
CHANNELS = [K.Color, K.Alpha, K.Background, K.WorldNormal]
WRITE = [K.Alpha, K.WorldNormal, K.Color]  # src/main.rs:87-91


def host_save_to(film, write_channels, output_folder, base_name):
    """The host post-process of the plain loop (not transparent): every channel copied to the host, image.py's arms, PNG."""
    os.makedirs(output_folder, exist_ok=True)
    for kind in write_channels:
        if kind == K.Color:
            img = image.color_image(film.channel(K.Color), background=film.channel(K.Background))
        elif kind == K.Alpha:
            img = image.alpha_image(film.channel(K.Alpha))
        elif kind == K.Background:
            img = image.background_image(film.channel(K.Background))
        else:
            img = image.normal_image(film.channel(K.WorldNormal))
        suffix = {K.Color: "color", K.Alpha: "alpha", K.Background: "background", K.WorldNormal: "normal"}[kind]
        image.save(os.path.join(output_folder, f"{base_name}_{suffix}.png"), img)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", default="1:25", help="frame range first:end (end exclusive, like rayn's frame_range)")
    ap.add_argument("--out", default="renders_seq", help="output folder")
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--writers", type=int, default=None, help="PNG writer threads (at most 8; default 2 per written channel)")
    ap.add_argument("--compare-loop", action="store_true", help="also time the plain render_frame_into + host post-process loop")
    ap.add_argument("--denoise", nargs="?", const="atrous", default=None, choices=["atrous", "variance"],
                    help="denoise every frame's Color: atrous (rayn_amd.Denoise() defaults; what a bare --denoise means) or variance "
                         "(rayn_amd.VarianceDenoise(1, 4.0, 0.4, 0.3) on the temporally accumulated colour; needs --temporal)")
    ap.add_argument("--temporal", action="store_true", help="accumulate every frame's Color over the frames before it (rayn_amd.Temporal() defaults); the camera's origin drifts")
    ap.add_argument("--feedback", type=float, default=0.0, metavar="B",
                    help="strength in [0, 1] with which every frame's first a-trous pass is fed back into the temporal history (0 = off); "
                         "needs --temporal --denoise variance")
    ap.add_argument("--resample", choices=("bilinear", "catmull_rom"), default="bilinear",
                    help="the filter that resamples the temporal history at the reprojected position (default bilinear); needs --temporal")
    ap.add_argument("--display", action="store_true", help="send every frame's Color through the HDR display transform (rayn_amd.Display)")
    ap.add_argument("--exposure", default="auto", help="auto (metered, the default) or an EV: the exposure scale is 2^EV; needs --display")
    ap.add_argument("--tone", choices=("aces", "reinhard", "linear"), default="aces", help="the tone operator (default aces); needs --display")
    ap.add_argument("--bloom", type=int, default=0, metavar="LEVELS", help="bloom over this many pyramid levels, 1..8 (0 = off, the default); needs --display")
    ap.add_argument("--adaptation", type=float, default=None, metavar="S", help="time constant in seconds of the auto exposure's adaptation over the frames; needs --display")
    ap.add_argument("--upscale", type=int, default=None, metavar="S",
                    help="render at --width x --height and rebuild every frame at S times that size (1..8) with rayn_amd.Upscale(S)")
    ap.add_argument("--supersample", action="store_true",
                    help="keep the temporal history at the upscaled size and jitter the low frames' camera (rayn_amd.Supersample()); needs --upscale and --temporal")
    ap.add_argument("--no-jitter", action="store_true", help="every low frame samples the same lattice (Supersample(jitter=False)); needs --supersample")
    ap.add_argument("--confidence", action="store_true", help="weigh every frame by its nearest low sample (Supersample(confidence=True)); needs --supersample")
    ap.add_argument("--no-confidence", action="store_true", help="every frame counts fully in the history (Supersample(confidence=False), the default); needs --supersample")
    ap.add_argument("--preview", nargs="?", type=int, const=R.Preview().samples, default=None, metavar="K",
                    help="run the preview integrator in place of the render: primary hit, normal and the ambient occlusion of K rays per pixel (1..64)")
    ap.add_argument("--ao-radius", type=float, default=None, metavar="R", help="length of the preview's ambient-occlusion rays in world units; needs --preview")
    ap.add_argument("--interpolate", type=int, default=None, metavar="K",
                    help="render every K-th frame (2..16) and the last, and generate the frames between two rendered keys (rayn_amd.Interpolate(K))")
    ap.add_argument("--interp-tolerance", type=float, default=None, metavar="D",
                    help="relative depth tolerance of a key's tap (default rayn_amd.Interpolate().depth_tolerance); needs --interpolate")
    ap.add_argument("--png", choices=("host", "device", "device-lz77"), default="host",
                    help="where the PNG streams are encoded: host (zlib in the writer threads, the default), device (filter, run-length and Huffman kernels on the "
                         "render stream) or device-lz77 (the same with LZ77 matches)")
    ap.add_argument("--exr", choices=("host", "device", "device-lz77"), default=None,
                    help="also write one multi-channel OpenEXR file per frame: host (zlib in the writer threads), device (the chunks encoded on the render "
                         "stream) or device-lz77 (the same with LZ77 matches)")
    ap.add_argument("--exr-float", action="store_true", help="write the EXR layers as FLOAT, the film's own bits (default HALF); needs --exr")
    ap.add_argument("--jpeg", nargs="?", type=int, const=R.Jpeg().quality, default=None, metavar="Q",
                    help="also write a baseline JPEG next to every PNG, encoded on the render stream, at quality Q (1..100, default 90); with --video alone, the video's quality")
    ap.add_argument("--jpeg-444", action="store_true", help="keep the chroma at full size (default 4:2:0); needs --jpeg or --video")
    ap.add_argument("--video", default=None, metavar="PATH", help="also write one Motion-JPEG AVI of the frames' Color image to PATH")
    ap.add_argument("--no-images", action="store_true", help="write the video alone: no PNG, .jpg or EXR; needs --video")
    args = ap.parse_args()
    if args.jpeg is not None and not 1 <= args.jpeg <= 100:
        ap.error("--jpeg must be in 1..100")
    if args.jpeg_444 and args.jpeg is None and args.video is None:
        ap.error("--jpeg-444 sets up the JPEG encoder: add --jpeg or --video")
    if args.no_images and args.video is None:
        ap.error("--no-images leaves the video alone: add --video")
    if args.no_images and args.compare_loop:
        ap.error("--compare-loop compares the image files: it does not combine with --no-images")
    if args.exr_float and args.exr is None:
        ap.error("--exr-float chooses the EXR pixel type: add --exr")
    if args.png != "host" and args.compare_loop:
        ap.error("--compare-loop compares the files byte for byte with the host encoder's: use one or the other")
    if args.interp_tolerance is not None and args.interpolate is None:
        ap.error("--interp-tolerance sets up the frame generation: add --interpolate")
    if args.interpolate is not None and not 2 <= args.interpolate <= 16:
        ap.error("--interpolate must be in 2..16")
    if args.interpolate is not None and (args.temporal or args.upscale is not None or args.preview is not None or args.denoise == "variance" or args.compare_loop):
        ap.error("--interpolate does not combine with --temporal, --upscale, --preview, --denoise variance or --compare-loop")
    if args.ao_radius is not None and args.preview is None:
        ap.error("--ao-radius sets up the preview integrator: add --preview")
    if args.preview is not None and (args.upscale is not None or args.denoise == "variance" or args.compare_loop):
        ap.error("--preview does not combine with --upscale, --denoise variance or --compare-loop")
    if args.upscale is not None and not 1 <= args.upscale <= 8:
        ap.error("--upscale must be in 1..8")
    if args.supersample and not (args.upscale is not None and args.temporal):
        ap.error("--supersample joins --upscale and --temporal: add both")
    if (args.no_jitter or args.no_confidence or args.confidence) and not args.supersample:
        ap.error("--no-jitter, --confidence and --no-confidence set up --supersample: add --supersample")
    if args.confidence and args.no_confidence:
        ap.error("--confidence and --no-confidence contradict each other")
    if args.supersample and (args.denoise == "variance" or args.feedback != 0.0 or args.resample != "bilinear"):
        ap.error("--supersample does not combine with --denoise variance, --feedback or --resample catmull_rom")
    if args.upscale is not None and args.temporal and not args.supersample:
        ap.error("--upscale with --temporal is not built: the temporal histories live at one resolution (add --supersample)")
    if args.upscale is not None and args.compare_loop:
        ap.error("--compare-loop compares with the host post-process, which has no upscaling: use one or the other")
    if not args.display and (args.exposure != "auto" or args.tone != "aces" or args.bloom or args.adaptation is not None):
        ap.error("--exposure, --tone, --bloom and --adaptation set up the display transform: add --display")
    if args.display and args.compare_loop:
        ap.error("--compare-loop compares with the host post-process, which has no display transform: use one or the other")
    if args.resample != "bilinear" and not args.temporal:
        ap.error("--resample chooses the resampling filter of the temporal accumulation: add --temporal")
    if (args.denoise or args.temporal) and args.compare_loop:
        ap.error("--compare-loop compares with the host post-process, which has neither a denoiser nor a temporal accumulation: use one or the other")
    if args.denoise == "variance" and not args.temporal:
        ap.error("--denoise variance estimates its variance from the temporal accumulation: add --temporal")
    if args.feedback != 0.0 and not (args.temporal and args.denoise == "variance"):
        ap.error("--feedback feeds the variance-guided filter's first pass back into the temporal history: add --temporal --denoise variance")
    if not 0.0 <= args.feedback <= 1.0:
        ap.error("--feedback must be in [0, 1]")
    denoise = {None: None, "atrous": R.Denoise(), "variance": R.VarianceDenoise(1, 4.0, 0.4, 0.3)}[args.denoise]
    temporal = R.Temporal(feedback=args.feedback, resample=args.resample) if args.temporal else None
    display = None
    if args.display:
        display = R.Display(exposure="auto" if args.exposure == "auto" else float(args.exposure), tone=args.tone,
                            bloom=R.Bloom(levels=args.bloom) if args.bloom else None, adaptation=args.adaptation)
    upscale = R.Upscale(args.upscale) if args.upscale is not None else None
    supersample = None
    if args.supersample:
        supersample = R.Supersample(jitter=not args.no_jitter, confidence=True if args.confidence else False if args.no_confidence else R.Supersample().confidence)
    preview = None
    if args.preview is not None:
        preview = R.Preview(samples=args.preview, radius=R.Preview().radius if args.ao_radius is None else args.ao_radius)
    interpolate = None
    if args.interpolate is not None:
        interpolate = R.Interpolate(args.interpolate, R.Interpolate().depth_tolerance if args.interp_tolerance is None else args.interp_tolerance)
    jpeg_options = R.Jpeg(R.Jpeg().quality if args.jpeg is None else args.jpeg, "444" if args.jpeg_444 else "420")
    jpeg = jpeg_options if args.jpeg is not None else None

    def video_at(path):
        return None if args.video is None else R.Video(path, jpeg_options, not args.no_images)
    first, end = (int(x) for x in args.frames.split(":"))
    frames = list(range(first, end))
    base = f"{SAMPLES * 4}_spp"
    cam, world = S.setup((args.width, args.height))
    if temporal is not None or interpolate is not None:  # something to reproject: the camera of BASELINE config 5 (rayn_amd.setup.setup_s3)
        c = world.cameras.get(cam)
        c.origin = Linear(c.origin, R.vec3(0.9, -0.3, 0.15))
    integ = R.PathTracingIntegrator(max_bounces=MAX_INDIRECT_BOUNCES, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE)
    filt = R.BlackmanHarrisFilter(S.FILTER_RADIUS)

    film = R.Film(CHANNELS, (args.width, args.height))
    # warm-up: code objects, the context's first-frame arena and the writer path (not timed)
    film.render_sequence(world, cam, integ, filt, S.TILE_SIZE, frames[:1], FRAME_RATE, SHUTTER_SPEED, SAMPLES, WRITE,
                         os.path.join(args.out, "warmup"), base, writers=args.writers, denoise=denoise, temporal=temporal, display=display, upscale=upscale, supersample=supersample, preview=preview,
                         interpolate=interpolate, png=args.png, exr=args.exr, exr_half=not args.exr_float, jpeg=jpeg,
                         video=video_at(os.path.join(args.out, "warmup", os.path.basename(args.video or ""))))
    t0 = time.perf_counter()
    stats = film.render_sequence(world, cam, integ, filt, S.TILE_SIZE, frames, FRAME_RATE, SHUTTER_SPEED, SAMPLES, WRITE,
                                 os.path.join(args.out, "sequence"), base, writers=args.writers, denoise=denoise, temporal=temporal, display=display, upscale=upscale, supersample=supersample, preview=preview,
                         interpolate=interpolate, png=args.png, exr=args.exr, exr_half=not args.exr_float, jpeg=jpeg, video=video_at(args.video))
    seq_s = time.perf_counter() - t0
    seq_dir = os.path.join(args.out, "sequence")
    pngs, exrs = ([n for n in os.listdir(seq_dir) if n.endswith(ext)] for ext in (".png", ".exr"))
    print(f"--png {args.png}: {sum(os.path.getsize(os.path.join(seq_dir, n)) for n in pngs)} bytes in {len(pngs)} files")
    if args.exr is not None:
        print(f"--exr {args.exr}{' --exr-float' if args.exr_float else ''}: {sum(os.path.getsize(os.path.join(seq_dir, n)) for n in exrs)} bytes in {len(exrs)} files")
    if jpeg is not None:
        jpgs = [n for n in os.listdir(seq_dir) if n.endswith(".jpg")]
        print(f"--jpeg {jpeg}: {sum(os.path.getsize(os.path.join(seq_dir, n)) for n in jpgs)} bytes in {len(jpgs)} files")
    if args.video is not None:
        print(f"--video {args.video}{' --no-images' if args.no_images else ''}: {os.path.getsize(args.video)} bytes, {len(frames)} frames of {jpeg_options}")
    if preview is not None:  # the preview is enqueued, not waited for: there is no per-frame render time to report
        print(f"render_sequence --preview {preview}{' --temporal ' + str(temporal) if temporal else ''}{' --denoise ' + str(denoise) if denoise else ''}"
              f"{' --display ' + str(display) if display else ''}: {len(frames)} frames in {seq_s:.3f} s = {len(frames) / seq_s:.2f} frames/s")
        return
    for st in stats:
        print(f"frame {st['frame']:4d}: generated" if st.get("generated") else f"frame {st['frame']:4d}: render {st['ms_total']:8.2f} ms")
    if interpolate is not None:
        keys = [st for st in stats if not st.get("generated")]
        print(f"render_sequence --interpolate {interpolate}{' --denoise ' + str(denoise) if denoise else ''}{' --display ' + str(display) if display else ''}: "
              f"{len(frames)} frames ({len(keys)} rendered, {len(frames) - len(keys)} generated) in {seq_s:.3f} s = {len(frames) / seq_s:.2f} frames/s "
              f"(render alone: {sum(st['ms_total'] for st in keys) / len(keys):.2f} ms per rendered frame)")
        return
    print(f"render_sequence{' --denoise ' + str(denoise) if denoise else ''}{' --temporal ' + str(temporal) if temporal else ''}{' --display ' + str(display) if display else ''}{' --upscale ' + str(upscale) if upscale else ''}{' --supersample ' + str(supersample) if supersample else ''}: {len(frames)} frames in {seq_s:.3f} s = {len(frames) / seq_s:.2f} frames/s "
          f"(render alone: {sum(st['ms_total'] for st in stats) / len(frames):.2f} ms/frame)")

    if args.compare_loop:
        plain = R.Film(CHANNELS, (args.width, args.height))
        loop_dir = os.path.join(args.out, "loop")
        f32 = np.float32
        plain.render_frame_into(world, cam, integ, filt, S.TILE_SIZE, frames[0], None, SAMPLES)  # warm-up of the plain film's context (not timed)
        t0 = time.perf_counter()
        for frame in frames:
            start = f32(frame) * (f32(1.0) / f32(FRAME_RATE))
            t1 = time.perf_counter()
            plain.render_frame_into(world, cam, integ, filt, S.TILE_SIZE, frame, (float(start), float(f32(start + f32(SHUTTER_SPEED)))), SAMPLES)
            t2 = time.perf_counter()
            host_save_to(plain, WRITE, loop_dir, f"{base}_{frame:04d}")
            t3 = time.perf_counter()
            print(f"plain loop frame {frame:4d}: render_frame_into {1e3 * (t2 - t1):8.2f} ms, host save_to {1e3 * (t3 - t2):8.2f} ms")
        loop_s = time.perf_counter() - t0
        print(f"plain loop: {len(frames)} frames in {loop_s:.3f} s = {len(frames) / loop_s:.2f} frames/s")
        print(f"speed-up of render_sequence over the plain loop: {loop_s / seq_s:.2f}x")
        same = all(open(os.path.join(loop_dir, n), "rb").read() == open(os.path.join(args.out, "sequence", n), "rb").read()
                   for n in sorted(os.listdir(loop_dir)))
        print(f"identical PNGs: {same} ({len(os.listdir(loop_dir))} files)")
        if not same:
            sys.exit(1)


if __name__ == "__main__":
    main()
