"""Host-side mirror of rayn's `Film` (src/film.rs:175-378) on top of the C ABI.

    film = Film([ChannelKind.Color, ChannelKind.Alpha, ChannelKind.Background, ChannelKind.WorldNormal], (w, h))
    film.render_frame_into(world, camera, integrator, filter, tile_size, frame, time_range, samples)
    film.save_to([ChannelKind.Color], "renders", "64_spp", False)

`render_frame_into` has the reference's signature (src/film.rs:382-395).  Device memory, the stream
and (for N>1 ranks) the process group come from PyTorch; the arithmetic is all in librayn_hip.so.

The option dataclasses live in rayn_amd.options, Context and the device-argument checks in rayn_amd.context; every name of both is
re-exported here.
"""
import dataclasses
import os

import numpy as np

from . import _abi, image  # noqa: F401
from . import progressive as _prog
from .context import *  # noqa: F401,F403
from .options import *  # noqa: F401,F403
from .params import frame_params
from .progressive import Progressive, progressive_seed  # noqa: F401


def _scaled_params(p, factor):
    """A copy of the frame parameters p with the resolution multiplied by factor: the frame of an upscaled film."""
    ph = type(p).from_buffer_copy(p)
    ph.width, ph.height = int(p.width) * int(factor), int(p.height) * int(factor)
    return ph


_CHANNEL_KEY = {ChannelKind.Color: "color", ChannelKind.Alpha: "alpha", ChannelKind.Background: "background", ChannelKind.WorldNormal: "normal"}
_SAVE_TO_ERR = {ChannelKind.Color: "Attempted to write Color channel with insufficient channels",  # src/film.rs:283-287
                ChannelKind.Alpha: "Attempted to write Alpha channel but it didn't exist",  # :341-345
                ChannelKind.Background: "Attempted to write Background channel but it didn't exist",  # :292-296
                ChannelKind.WorldNormal: "Attempted to write WorldNormal channel but it didn't exist"}  # :316-320


# What a film's channel kinds allow: plain functions of the kinds, shared by Film's methods and plan_sequence.

def _have_mask(channel_kinds):
    return sum(1 << k.value for k in channel_kinds)


def _save_jobs(channel_kinds, write_channels, transparent_background):
    jobs = []
    for kind in write_channels:
        bpp = save_to_bpp(kind, _have_mask(channel_kinds), transparent_background)
        if bpp < 0:
            raise ValueError(_SAVE_TO_ERR[kind])
        jobs.append((kind, bpp, _CHANNEL_KEY[kind]))
    return jobs


def _upscale_plan(channel_kinds, upscale):
    if not isinstance(upscale, Upscale):
        raise ValueError(f"upscale must be an Upscale, got {upscale!r}")
    if ChannelKind.Color not in channel_kinds:
        raise ValueError("Attempted to upscale a film without a Color channel")
    return upscale.without(_have_mask(channel_kinds)), [_CHANNEL_KEY[k] for k in ChannelKind if k in channel_kinds]


def _denoise_params(channel_kinds, denoise):
    """`denoise` with the terms of the guides the film lacks switched off; a film without Color raises ValueError."""
    if ChannelKind.Color not in channel_kinds:
        raise ValueError("Attempted to denoise the Color channel but it didn't exist")
    return denoise.without(_have_mask(channel_kinds))


PNG_ENCODERS = ("host", "device", "device-lz77")


def _check_png(png):
    """`png` of save_to and render_sequence: "host" (zlib on the host, the files the reference's loop writes), "device" (the stream of
    Context.png_encode, framed on the host: smaller files of the same pixels) or "device-lz77" (Context.png_encode_lz77: the same with
    LZ77 matches, smaller again on smooth and flat images)"""
    if png not in PNG_ENCODERS:
        raise ValueError(f"png must be one of {PNG_ENCODERS}, got {png!r}")
    return png


def _check_jpeg(jpeg):
    if not isinstance(jpeg, Jpeg):
        raise ValueError(f"jpeg must be a Jpeg, got {jpeg!r}")


def _jpeg_jobs(jobs):
    """`jobs` ((kind, bytes per pixel, suffix)) if every image has a JPEG form; ValueError for one with 4 bytes per pixel"""
    for kind, bpp, _ in jobs:
        if bpp == 4:
            raise ValueError(f"Attempted to write the {kind.name} image with alpha as a JPEG: JPEG has no alpha (transparent_background)")
    return jobs


def _check_sequence_jpeg(plan, write_channels, jpeg, video):
    """render_sequence's jpeg= and video= against its plan, before anything renders: (index of the job the video shows or None, whether
    the call writes its image files)"""
    if jpeg is not None:
        _check_jpeg(jpeg)
        _jpeg_jobs(plan.jobs)
    if video is None:
        return None, True
    if not isinstance(video, Video):
        raise ValueError(f"video must be a Video, got {video!r}")
    shown = [j for j, (kind, _, _) in enumerate(plan.jobs) if kind == ChannelKind.Color]
    if not shown:
        raise ValueError("video= shows the sequence's Color image: name ChannelKind.Color in write_channels")
    _jpeg_jobs([plan.jobs[shown[0]]])
    return shown[0], video.images


EXR_ENCODERS = ("host", "device", "device-lz77")
# the layers of an EXR file: kind -> (the device film's key, the channel names of the plane's words in order)
_EXR_LAYERS = {ChannelKind.Color: ("color", ("R", "G", "B")), ChannelKind.Alpha: ("alpha", ("A",)),
               ChannelKind.Background: ("background", ("background.R", "background.G", "background.B")),
               ChannelKind.WorldNormal: ("normal", ("N.X", "N.Y", "N.Z"))}


def _check_exr(exr, allow_none=False):
    """`exr` of save_exr and render_sequence: "host" (zlib per chunk on the host), "device" (Context.exr_encode, framed on the host) or
    "device-lz77" (the same with LZ77 matches); render_sequence also takes None, no EXR files."""
    if not (exr in EXR_ENCODERS or (allow_none and exr is None)):
        raise ValueError(f"exr must be one of {EXR_ENCODERS}, got {exr!r}")
    return exr


def _exr_kinds(channel_kinds, channels):
    """The kinds an EXR file holds, `channels` or every kind of the film, in the film's order; ValueError for one the film lacks, for a
    kind named twice and for none at all"""
    kinds = list(channel_kinds if channels is None else channels)
    for k in kinds:
        if k not in channel_kinds:
            raise ValueError(f"Attempted to write {k.name} channel but it didn't exist")
    if len(set(kinds)) != len(kinds) or not kinds:
        raise ValueError("an EXR file holds every kind once and at least one")
    return kinds


def exr_channels(kinds, d_film, half=True, d_gbuffer=None):
    """The channel list of Context.exr_encode - (name, tensor, stride, offset, type), sorted by name - of the planes of `kinds` in the
    device film `d_film`: HALF, or FLOAT for half=False.  d_gbuffer (alloc_gbuffer's planes) adds P.X, P.Y, P.Z and Z, always FLOAT, and
    the UINT id."""
    t = image.EXR_HALF if half else image.EXR_FLOAT
    out = []
    for kind in kinds:
        key, names = _EXR_LAYERS[kind]
        out += [(n, d_film[key], len(names), k, t) for k, n in enumerate(names)]
    if d_gbuffer is not None:
        out += [(n, d_gbuffer["records"], 4, k, image.EXR_FLOAT) for k, n in enumerate(("P.X", "P.Y", "P.Z", "Z"))]
        out.append(("id", d_gbuffer["object"], 1, 0, image.EXR_UINT))
    return sorted(out, key=lambda c: c[0].encode())


def exr_layout(channels):
    return [(s, o, t) for _, _, s, o, t in channels]


def _exr_bound(w, h, channels):
    """exr_stream_bound of a channel list; ValueError for a film too large for one file"""
    bound = exr_stream_bound(w, h, exr_layout(channels))
    if not bound:
        raise ValueError(f"a {w}x{h} EXR file of these {len(channels)} channels reaches 2^31 bytes: write fewer channels or HALF")
    return bound


def _check_display(display):
    if not isinstance(display, Display):
        raise ValueError(f"display must be a Display, got {display!r}")


@dataclasses.dataclass(frozen=True)
class SequencePlan:
    """What one render_sequence call does, as plan_sequence resolved it.  denoise, display, upscale, supersample, temporal: the
    options as the loop uses them - a denoiser without the terms of the guides the film lacks, the upscale without its plane term on
    a film without WorldNormal, and None for whatever switched itself off.  variance: `denoise` was given as a VarianceDenoise.
    up_keys: the keys of the planes the upscale rebuilds (None without one).  jobs: [(kind, bytes per pixel, file suffix)] of
    every written image, the suffixes final.  preview: the Preview that takes the render's place, or None.  interpolate: the Interpolate
    that generates the frames between the rendered keys, or None; interp_keys: the keys of the planes it generates.  png: "host",
    "device" or "device-lz77", where and how the files' streams are encoded."""
    denoise: object
    display: object
    upscale: object
    supersample: object
    temporal: object
    variance: bool
    up_keys: object
    jobs: list
    transparent_background: bool = False
    preview: object = None
    interpolate: object = None
    interp_keys: object = None
    png: str = "host"
    exr: object = None       # None, or one of EXR_ENCODERS: every frame also writes one EXR file
    exr_kinds: object = None  # the kinds that file holds: write_channels', in the film's order

    def out_res(self, res):
        """The size of the written images of a film of resolution `res`."""
        s = 1 if self.upscale is None else self.upscale.factor
        return res[0] * s, res[1] * s


def plan_sequence(channel_kinds, write_channels, transparent_background=False, denoise=None, display=None, upscale=None, supersample=None,
                  temporal=None, preview=None, interpolate=None, png="host", exr=None):
    """The SequencePlan of render_sequence's arguments for a film of `channel_kinds`: every rule of its docstring that decides what
    runs and what the files are called, and every ValueError it raises before anything renders, in the order it raises them.  Host
    only: no context, no torch, no directory.  `interpolate` must be an Interpolate.  It raises ValueError together with `temporal`,
    with `upscale`, with `supersample` and with `preview`: none of these compositions is built.  It raises ValueError with a
    VarianceDenoise, as every sequence without `temporal` does.  It needs the film's Color channel.  It puts _interp right after
    _color in the name of every Color image of the call, where _temporal would stand.  `png` must be one of PNG_ENCODERS - checked first -
    and changes no file name.  `exr` must be None or one of EXR_ENCODERS - checked right behind it - and changes no PNG."""
    _check_png(png)
    _check_exr(exr, allow_none=True)
    color = ChannelKind.Color
    variance = isinstance(denoise, VarianceDenoise)
    interp_keys = None
    if interpolate is not None:
        if not isinstance(interpolate, Interpolate):
            raise ValueError(f"interpolate must be an Interpolate, got {interpolate!r}")
        for name, other in (("temporal", temporal), ("upscale", upscale), ("supersample", supersample), ("preview", preview)):
            if other is not None:
                raise ValueError(f"interpolate= with {name}= is not built: the generated frames are made from plain rendered keys at one resolution")
        if color not in channel_kinds:
            raise ValueError("Attempted to interpolate a film without a Color channel")
        interp_keys = [_CHANNEL_KEY[k] for k in ChannelKind if k in channel_kinds]
    if preview is not None:
        if not isinstance(preview, Preview):
            raise ValueError(f"preview must be a Preview, got {preview!r}")
        if upscale is not None or supersample is not None:
            raise ValueError("preview= with upscale= or supersample= is not built: a preview is cheap at the full resolution")
        if variance:
            raise ValueError("preview= with a VarianceDenoise is not built: the preview's ambient occlusion carries no variance estimate")
        if color not in channel_kinds:
            raise ValueError("Attempted to preview into a film without a Color channel")
    if supersample is not None:
        if not isinstance(supersample, Supersample):
            raise ValueError(f"supersample must be a Supersample, got {supersample!r}")
        if upscale is None or temporal is None:
            raise ValueError("supersample= joins upscale= and temporal=: pass both")
        if not isinstance(temporal, Temporal):
            raise ValueError(f"temporal must be a Temporal, got {temporal!r}")
        if variance:
            raise ValueError("supersample= with a VarianceDenoise is not built: the luminance moments live at one resolution")
        if temporal.resample != "bilinear":
            raise ValueError("supersample= with Temporal.resample != 'bilinear' is not built")
        if float(temporal.feedback) > 0.0:
            raise ValueError("supersample= with Temporal.feedback > 0 is not built")
    if variance and temporal is None:
        raise ValueError("render_sequence renders plain frames: VarianceDenoise needs the state of a progressive render")
    if isinstance(temporal, Temporal) and float(temporal.feedback) > 0.0 and not variance:
        raise ValueError("Temporal.feedback > 0 feeds a VarianceDenoise's first pass back into the history: pass one as `denoise`")
    up_keys = None
    if upscale is not None:
        if temporal is not None and supersample is None:
            raise ValueError("temporal= together with upscale= is not built: the temporal histories live at one resolution")
        upscale, up_keys = _upscale_plan(channel_kinds, upscale)
    jobs = _save_jobs(channel_kinds, write_channels, transparent_background)
    shown = color in write_channels  # without a Color image nothing shows what denoise, temporal and display make: they switch off
    if denoise is not None:
        if variance:  # its guides are required, not switched off: checked with the temporal arguments below
            _denoise_params(channel_kinds, denoise)
            denoise = denoise if shown else None
        else:
            denoise = _denoise_params(channel_kinds, denoise) if shown else None
    if temporal is not None:
        if not isinstance(temporal, Temporal):
            raise ValueError(f"temporal must be a Temporal, got {temporal!r}")
        if color not in channel_kinds or ChannelKind.WorldNormal not in channel_kinds:
            raise ValueError("temporal accumulation needs the film's Color and WorldNormal channels")
        if variance and denoise is not None and float(denoise.sigma_alpha) != 0.0 and ChannelKind.Alpha not in channel_kinds:
            raise ValueError("variance-guided denoising of a temporal sequence needs the film's Alpha channel when sigma_alpha != 0")
        if not shown:
            temporal = supersample = None  # the plain path (upscale= alone with supersample=)
    if display is not None:
        _check_display(display)
        display = display if shown else None
    shown_suffix = ("color" + ("_preview" if preview is not None else "") + ("_temporal" if temporal is not None else "")
                    + ("_interp" if interpolate is not None else "") + ("_denoised" if denoise is not None else "")
                    + ("_display" if display is not None else ""))
    scale = "" if upscale is None else f"_x{upscale.factor}"
    jobs = [(kind, bpp, (shown_suffix if kind == color else suffix) + scale) for kind, bpp, suffix in jobs]
    return SequencePlan(denoise, display, upscale, supersample, temporal, variance, up_keys, jobs, bool(transparent_background), preview,
                        interpolate, interp_keys, png, exr, None if exr is None else [k for k in ChannelKind if k in write_channels])


class _SequencePost:
    """What render_sequence enqueues between a frame's render and the copies of its images: the buffers of every optional stage,
    allocated once, and the stages of one frame in their order.  The film's channels (d_film) stay what the integrator wrote."""

    def __init__(self, film, plan, desc, d_film):
        import torch
        self.ctx, self.plan, self.desc, self.d_film, self.mask = film.ctx, plan, desc, d_film, film.have_mask()
        (w, h), (ow, oh), dev = film.res, plan.out_res(film.res), film.device
        self.res, self.out_res = (w, h), (ow, oh)
        nbytes = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)
        if plan.denoise is not None:
            self.d_denoised = torch.empty(ow * oh, 3, dtype=torch.float32, device=dev)
            self.d_scratch = nbytes((denoise_variance_scratch_bytes if plan.variance else denoise_scratch_bytes)(ow, oh))
        if plan.upscale is not None:
            self.d_glow, self.d_ghigh = alloc_gbuffer(w, h, dev), alloc_gbuffer(ow, oh, dev)
            self.d_uscratch = nbytes(gbuffer_scratch_bytes(ow, oh))  # serves both passes
            d_up_full = alloc_device_film(ow, oh, dev)
            self.d_up = {k: d_up_full[k] for k in plan.up_keys}
            self.d_low = {k: d_film[k] for k in plan.up_keys}
        self.d_mom = [None, None]
        if plan.temporal is not None and plan.variance and plan.denoise is not None:
            self.d_mom = [nbytes(temporal_moments_bytes(w, h)) for _ in range(2)]
        if plan.supersample is not None:  # the histories live at the high size; the G-buffers are the upscale's
            self.d_hist = [nbytes(temporal_history_bytes(ow, oh)) for _ in range(2)]
            self.desc_low = type(desc).from_buffer_copy(desc)  # the world as the low frame is rendered: the camera is set per frame
        elif plan.temporal is not None:
            self.d_gbuf = alloc_gbuffer(w, h, dev)
            self.d_gscratch = nbytes(gbuffer_scratch_bytes(w, h)) if plan.preview is None else None
            self.d_hist = [nbytes(temporal_history_bytes(w, h)) for _ in range(2)]
            self.d_accum = torch.empty(w * h, 3, dtype=torch.float32, device=dev)
        self.prev_start = None  # time_start of the frame the newest history belongs to
        self.low_cam = None  # the jittered camera the current low frame was rendered with
        if plan.display is not None:
            d = plan.display
            self.d_dstate = self.ctx.display_state() if d.auto else None
            self.d_dscratch = nbytes(display_scratch_bytes(ow, oh, d.levels)) if d.auto or d.levels else None
        self.shown_start = None  # the start of the frame the display state last metered
        if plan.interpolate is not None:  # two keys used in turn, one generated frame
            self.d_keys = [d_film, alloc_device_film(w, h, dev)]
            self.d_kgbuf = [alloc_gbuffer(w, h, dev) for _ in range(2)]
            self.d_ggbuf = alloc_gbuffer(w, h, dev)
            self.d_igscratch = nbytes(gbuffer_scratch_bytes(w, h))
            d_gen_full = alloc_device_film(w, h, dev)
            self.d_gen = {k: d_gen_full[k] for k in plan.interp_keys}
        if plan.preview is not None:
            k = int(plan.preview.samples)
            self.d_psamples = torch.empty(k, 2, dtype=torch.float32, device=dev)
            self.d_pscramble = torch.from_numpy(preview_tables(k, 0, w, h)[1]).to(dev)
            self.d_pscratch = nbytes(preview_scratch_bytes(w, h, k))

    def preview(self, p, stream):
        """In place of frame p's render: upload the frame's AO sample table and enqueue the preview into the film, and into the temporal
        stage's G-buffer when there is one."""
        import torch
        plan = self.plan
        self.d_psamples.copy_(torch.from_numpy(preview_tables(plan.preview.samples, p.frame, 1, 1)[0]))
        self.ctx.preview(p, plan.preview, self.d_psamples, self.d_film, self.d_pscramble, None, getattr(self, "d_gbuf", None), self.d_pscratch, stream)

    def jitter(self, i, p):
        """Before frame i's render: with a jittering Supersample, upload the world under the frame's offset camera."""
        sup, self.low_cam = self.plan.supersample, None
        if sup is not None and sup.jitter:
            self.low_cam = jittered_camera(self.desc.camera, *sup.offset(self.plan.upscale.factor, i), p.time_start)
            self.desc_low.camera = self.low_cam
            self.ctx.upload_world(self.desc_low)

    def key_gbuffer(self, slot, p, stream):
        """After the render of the key in `slot` (frame parameters p): trace its G-buffer."""
        self.ctx.gbuffer(p, self.d_kgbuf[slot], self.d_igscratch, stream)

    def generate(self, p, slot_a, p_a, slot_b, p_b, stream):
        """The frame p between the keys in slot_a (frame parameters p_a) and slot_b (p_b): its own G-buffer and the interpolation, into
        the generated film, which is returned."""
        ctx, plan = self.ctx, self.plan
        ctx.gbuffer(p, self.d_ggbuf, self.d_igscratch, stream)
        keys = [({k: self.d_keys[s][k] for k in plan.interp_keys}, self.d_kgbuf[s], self.desc.camera, q.time_start) for s, q in ((slot_a, p_a), (slot_b, p_b))]
        ctx.interpolate(p, plan.interpolate, keys[0], keys[1], self.d_ggbuf, self.d_gen, None, stream)
        return self.d_gen

    def enqueue(self, i, p, stream, d_film=None):
        """After frame i's render (frame parameters p): enqueue its upscale, temporal and denoise stages on the raw `stream`.  d_film: the
        film the frame is in, when it is not the sequence's own (a key's slot or the generated film of an interpolated sequence).
        -> (d_shown, d_base): the film dicts the Color image and the other images are made from."""
        ctx, plan = self.ctx, self.plan
        (w, h), (ow, oh) = self.res, self.out_res
        first = self.prev_start is None  # no history yet
        prev_hist, prev_mom = (None, None) if first else (self.d_hist[(i + 1) % 2], self.d_mom[(i + 1) % 2])
        prev_cam, prev_start = (None, 0.0) if first else (self.desc.camera, self.prev_start)
        d_base = self.d_film if d_film is None else d_film
        if plan.upscale is not None:
            ctx.gbuffer(p, self.d_glow, self.d_uscratch, stream)
            if self.low_cam is not None:
                ctx.upload_world(self.desc)  # the high G-buffer and the history belong to the frame's own camera
            ctx.gbuffer(_scaled_params(p, plan.upscale.factor), self.d_ghigh, self.d_uscratch, stream)
            if plan.supersample is not None:
                ctx.temporal_upscale(p, plan.upscale, plan.temporal, plan.supersample, self.d_low, self.d_glow, self.d_ghigh, prev_hist, prev_cam,
                                     prev_start, self.d_hist[i % 2], self.d_up, self.low_cam, None, stream)
                self.prev_start = p.time_start
            else:
                ctx.upscale(p, plan.upscale, self.d_low, self.d_glow, self.d_ghigh, self.d_up, None, stream)
            d_base = self.d_up
        d_shown = d_base
        if plan.temporal is not None and plan.supersample is None:
            if plan.preview is None:  # a preview has written its own primary hits into d_gbuf
                ctx.gbuffer(p, self.d_gbuf, self.d_gscratch, stream)
            ctx.temporal_accumulate(p, plan.temporal, self.d_film, self.d_gbuf, prev_hist, prev_cam, prev_start, self.d_hist[i % 2], self.d_accum,
                                    stream, prev_mom, self.d_mom[i % 2])
            self.prev_start = p.time_start
            d_shown = dict(self.d_film, color=self.d_accum)
        if plan.denoise is not None:
            if plan.variance:
                ctx.denoise_temporal_variance(w, h, d_shown, self.d_gbuf, self.d_hist[i % 2], self.d_mom[i % 2], self.d_denoised, plan.denoise, None,
                                              self.d_scratch, stream, float(plan.temporal.feedback))
            else:
                ctx.denoise(ow, oh, d_shown, self.d_denoised, plan.denoise, self.d_scratch, stream)
            d_shown = dict(d_base, color=self.d_denoised)
        return d_shown, d_base

    def pixels(self, kind, start, d_src, d_out, stream):
        """Enqueue the 8-bit image of channel `kind` of the frame starting at `start` (f32) from the film dict d_src into d_out: the
        display transform for Color under a Display - its state blends with the frame it last metered - and save_to's arm otherwise."""
        plan, (ow, oh) = self.plan, self.out_res
        if plan.display is not None and kind == ChannelKind.Color:
            adapt = 1.0 if self.shown_start is None else plan.display.adapt(float(start) - float(self.shown_start))
            self.ctx.display(plan.display, self.mask, plan.transparent_background, ow, oh, d_src, d_out, self.d_dstate, self.d_dscratch, adapt,
                             stream=stream)
            self.shown_start = start
        else:
            self.ctx.save_to_pixels(kind, self.mask, plan.transparent_background, ow, oh, d_src, d_out, stream)


class Film:
    """Film::<U4>::new(channels, res) (src/film.rs:184-203)."""

    def __init__(self, channels, res, device=0):
        kinds = list(channels)
        if len(set(kinds)) != len(kinds):
            dup = next(k for k in kinds if kinds.count(k) > 1)
            raise ValueError(f"Attempted to create multiple {dup.name} channels")  # src/film.rs:188
        self._init_state(kinds, res, Context(device), f"cuda:{device}")

    def _init_state(self, kinds, res, ctx, device):
        """Every attribute of a film: __init__ with a context of its own, Film.upscaled with the source film's."""
        self.channel_kinds = kinds
        self.res = (int(res[0]), int(res[1]))
        self.ctx = ctx
        self.device = device
        self.channels = None  # torch tensors after a render
        self.progressive_epoch = 0
        self._progressive = None  # after render_progressive: its device state, geometry, checkpoint key and epoch count
        self._last_params = None  # the frame parameters of the last render (gbuffer)
        self._gbuffer = None  # (frame parameters, device G-buffer) of a render that traced its own primary hits (render_preview)
        self.ao = None  # render_preview: the ambient-occlusion plane, a float32 device tensor of one float per pixel
        self._last_camera = None  # the rayn_camera of the world the last render uploaded (interpolated)

    def render_frame_into(self, world, camera, integrator, filter, tile_size, frame, time_range, samples, tile_first=0, tile_step=1):
        """Film::render_frame_into (src/film.rs:382-628); the film is overwritten, not accumulated (:91)."""
        import torch
        w, h = self.res
        p = frame_params(w, h, samples, integrator.max_bounces, integrator.volume_marches, frame, time_range, tile_size, tile_first, tile_step)
        desc = world.to_desc(camera)
        self.ctx.upload_world(desc)
        self._last_camera = desc.camera
        tables = build_tables(4 * samples, integrator.max_bounces, integrator.volume_marches, frame, w, h, filter)
        with torch.cuda.device(self.device):
            d_tables = [torch.from_numpy(t).to(self.device) for t in tables]
            out = alloc_device_film(w, h, self.device)
            self.ctx.render_device(p, d_tables, out)
            torch.cuda.synchronize()
        self.channels = out
        self._last_params = p
        self.progressive_epoch += 1
        return self.ctx.stats()

    def channel(self, kind):
        if kind not in self.channel_kinds:
            raise KeyError(f"Attempted to read {kind.name} channel but it didn't exist")
        w, h = self.res
        t = self.channels[_CHANNEL_KEY[kind]].cpu().numpy()
        return t.reshape(h, w, 3) if t.ndim == 2 else t.reshape(h, w)

    def _gbuffer_device(self):
        """gbuffer's device planes (alloc_gbuffer's), enqueued on the current stream.  Under torch.cuda.device."""
        if self._last_params is None:
            raise ValueError("the film holds no rendered frame (render_frame_into, render_sequence or render_progressive has not run)")
        if self._gbuffer is not None and self._gbuffer[0] is self._last_params:
            return self._gbuffer[1]
        g = alloc_gbuffer(self.res[0], self.res[1], self.device)
        self.ctx.gbuffer(self._last_params, g)
        return g

    def gbuffer(self):
        """The primary-hit G-buffer of the last rendered frame (rayn_hip_gbuffer_device, an extension): one centre ray per pixel at the
        frame's time_start through the product closest-hit kernel.  Returns {"position": float32 (h, w, 3), "t": float32 (h, w; +inf for
        a miss), "object": uint32 (h, w; 0xFFFFFFFF for a miss)}, rows bottom-up like the film."""
        import torch
        w, h = self.res
        with torch.cuda.device(self.device):
            g = self._gbuffer_device()
            rec = g["records"].cpu().numpy().reshape(h, w, 4)
            obj = g["object"].cpu().numpy().view(np.uint32).reshape(h, w)
        return {"position": rec[..., :3].copy(), "t": rec[..., 3].copy(), "object": obj}

    def _upscale_plan(self, upscale):
        """(`upscale` with the plane term off for a film without WorldNormal, the keys of the planes this film holds); ValueError for
        anything that is no Upscale and for a film without Color."""
        return _upscale_plan(self.channel_kinds, upscale)

    def upscaled(self, upscale, want_weight=False):
        """A NEW Film of upscale.factor times this film's resolution, rebuilt from the last rendered frame by the guided upscaling (Upscale
        `upscale`, rayn_hip_upscale_device, an extension): the G-buffer of the frame is traced at both resolutions and every channel the
        film holds is upsampled with the same guided weights; a film without WorldNormal loses the plane term.  The new film has the same
        channel kinds and shares this film's Context and device; its channels are the upscaled planes, so channel, pixels, save_to,
        save_hdr, denoised_color(Denoise(...)), display_color and display= work on it unchanged, and its gbuffer() is the high G-buffer.
        It holds no progressive state (a VarianceDenoise raises its ValueError).  This film is not changed.  With want_weight, returns
        (film, weight): the summed guided weight of every high pixel as float32 (H, W), rows bottom-up, 0 where a fallback was taken.
        ValueError when this film holds no rendered frame."""
        import torch
        up, keys = self._upscale_plan(upscale)
        if self._last_params is None or self.channels is None:
            raise ValueError("the film holds no rendered frame (render_frame_into, render_sequence or render_progressive has not run)")
        w, h = self.res
        p = self._last_params
        ph = _scaled_params(p, up.factor)
        W, H = int(ph.width), int(ph.height)
        with torch.cuda.device(self.device):
            g_low, g_high = alloc_gbuffer(w, h, self.device), alloc_gbuffer(W, H, self.device)
            d_scratch = torch.empty(max(gbuffer_scratch_bytes(W, H), 1), dtype=torch.uint8, device=self.device)
            self.ctx.gbuffer(p, g_low, d_scratch)
            self.ctx.gbuffer(ph, g_high, d_scratch)
            full = alloc_device_film(W, H, self.device)
            d_out = {k: full[k] for k in keys}
            d_weight = torch.empty(W * H, dtype=torch.float32, device=self.device) if want_weight else None
            self.ctx.upscale(p, up, {k: self.channels[k] for k in keys}, g_low, g_high, d_out, d_weight)
            out = Film.__new__(Film)
            out._init_state(list(self.channel_kinds), (W, H), self.ctx, self.device)
            out.channels = d_out
            out.progressive_epoch = self.progressive_epoch
            out._last_params = ph
            if want_weight:
                return out, d_weight.cpu().numpy().reshape(H, W)
            return out

    def interpolated(self, other, time_start, interpolate=None):
        """A NEW Film of this film's size that holds a frame GENERATED for the start time `time_start` between two rendered frames: this
        film (key A) and `other` (key B), two films of the same size on the same device whose last renders were of the same world through
        the same camera at two different start times, this film's first (Interpolate `interpolate`, rayn_hip_interpolate_device, an
        extension).  The G-buffers of both keys and of the generated frame are traced under the world this film's render uploaded; every
        channel the films hold is generated with the same weights.  The new film has the same channel kinds and shares this film's
        Context and device, so channel, pixels, save_to, save_hdr, denoise=Denoise(...) and display= work on it unchanged, and its
        gbuffer() is the generated frame's own.  It holds no progressive state.  Neither key is changed.  The counterpart of upscaled.
        ValueError when either film holds no rendered frame, the films differ in size, channels or device, or the times are out of
        order."""
        import torch
        interpolate = Interpolate() if interpolate is None else interpolate
        if not isinstance(interpolate, Interpolate):
            raise ValueError(f"interpolate must be an Interpolate, got {interpolate!r}")
        if not isinstance(other, Film):
            raise ValueError(f"other must be a Film, got {other!r}")
        if ChannelKind.Color not in self.channel_kinds:
            raise ValueError("Attempted to interpolate a film without a Color channel")
        if other.res != self.res or set(other.channel_kinds) != set(self.channel_kinds) or other.device != self.device:
            raise ValueError("the two key films must have the same size, channels and device")
        for f in (self, other):
            if f._last_params is None or f.channels is None or f._last_camera is None:
                raise ValueError("a key film holds no rendered frame (render_frame_into, render_sequence or render_progressive has not run)")
        pa, pb = self._last_params, other._last_params
        ts = float(np.float32(time_start))
        if not (pa.time_start < pb.time_start and pa.time_start <= ts <= pb.time_start):  # a NaN fails
            raise ValueError(f"time_start must lie between the keys' start times {pa.time_start!r} < {pb.time_start!r}, got {time_start!r}")
        w, h = self.res
        pt = type(pa).from_buffer_copy(pa)
        pt.time_start, pt.time_end = ts, float(np.float32(np.float32(ts) + (np.float32(pa.time_end) - np.float32(pa.time_start))))
        keys = [_CHANNEL_KEY[k] for k in ChannelKind if k in self.channel_kinds]
        with torch.cuda.device(self.device):
            g_a, g_b, g_t = (alloc_gbuffer(w, h, self.device) for _ in range(3))
            d_scratch = torch.empty(max(gbuffer_scratch_bytes(w, h), 1), dtype=torch.uint8, device=self.device)
            for p, g in ((pa, g_a), (pb, g_b), (pt, g_t)):
                self.ctx.gbuffer(p, g, d_scratch)
            full = alloc_device_film(w, h, self.device)
            d_out = {k: full[k] for k in keys}
            self.ctx.interpolate(pt, interpolate, ({k: self.channels[k] for k in keys}, g_a, self._last_camera, pa.time_start),
                                 ({k: other.channels[k] for k in keys}, g_b, other._last_camera, pb.time_start), g_t, d_out)
            out = Film.__new__(Film)
            out._init_state(list(self.channel_kinds), (w, h), self.ctx, self.device)
            out.channels = d_out
            out.progressive_epoch = self.progressive_epoch
            out._last_params = pt
            out._gbuffer = (pt, g_t)
            out._last_camera = self._last_camera
            return out

    def render_preview(self, preview=None, frame=None, world=None, camera=None, time_range=None):
        """A NEW Film of this film's size that holds the preview integrator's image (Preview `preview`, rayn_hip_preview_device, an
        extension): the primary hit of every pixel's centre ray, its viewer-facing normal and its ambient occlusion - the geometry alone, in
        milliseconds.  Without `world`, the preview is of the last rendered frame: its uploaded world and frame parameters (ValueError
        when the film holds none), with `frame` (default: that frame's number) choosing the AO directions.  With `world` and `camera`, that
        world is uploaded first and the frame is `frame` (default 1) over `time_range` (default: the frame's own, as render_frame_into
        takes it); nothing needs to have been rendered.  The sample table is 2-D set 0 of build_rd_tables(samples, 0, 2, frame), the scramble
        build_film_tables' (preview_tables), so successive frames get different directions.

        The new film has the channels Color, Alpha and WorldNormal (the preview has no Background), shares this film's Context and device,
        and channel, pixels, save_to, save_hdr, denoise=Denoise(...) and display= work on it unchanged; its gbuffer() returns the preview's
        own primary hits without tracing again, and its `ao` attribute is the ambient-occlusion plane (a float32 device tensor of one float
        per pixel, film order).  This film is not changed."""
        import torch
        preview = Preview() if preview is None else preview
        if not isinstance(preview, Preview):
            raise ValueError(f"preview must be a Preview, got {preview!r}")
        w, h = self.res
        if world is not None:
            frame = 1 if frame is None else int(frame)
            p = frame_params(w, h, 1, 0, 2, frame, time_range)
            self.ctx.upload_world(world.to_desc(camera))
        else:
            if self._last_params is None:
                raise ValueError("the film holds no rendered frame (render_frame_into, render_sequence or render_progressive has not run): pass world= and camera=")
            p = type(self._last_params).from_buffer_copy(self._last_params)
            if frame is not None:
                p.frame = int(frame)
        samples, scramble = preview_tables(preview.samples, int(p.frame), w, h)
        with torch.cuda.device(self.device):
            full = alloc_device_film(w, h, self.device)
            d_out = {k: full[k] for k in ("color", "alpha", "normal")}
            g = alloc_gbuffer(w, h, self.device)
            d_ao = torch.empty(w * h, dtype=torch.float32, device=self.device)
            self.ctx.preview(p, preview, torch.from_numpy(samples).to(self.device), d_out, torch.from_numpy(scramble).to(self.device), d_ao, g)
            out = Film.__new__(Film)
            out._init_state([ChannelKind.Color, ChannelKind.Alpha, ChannelKind.WorldNormal], (w, h), self.ctx, self.device)
            out.channels = d_out
            out.progressive_epoch = self.progressive_epoch
            out._last_params = p
            out._gbuffer = (p, g)
            out.ao = d_ao
            return out

    def have_mask(self):
        """bit k = ChannelKind k is among the film's channels (the have_mask of rayn_save_to_bpp)"""
        return _have_mask(self.channel_kinds)

    def _save_jobs(self, write_channels, transparent_background):
        """[(kind, bytes per pixel, file suffix)] of a save_to call; raises the reference's Err text as ValueError before anything runs."""
        return _save_jobs(self.channel_kinds, write_channels, transparent_background)

    def _variance_state(self):
        """The progressive render behind the film's channels, for a VarianceDenoise; ValueError when there is none or it is too short."""
        pr = self._progressive
        if pr is None or self.channels is not pr["film"]:
            raise ValueError("VarianceDenoise needs the state of a progressive render, and the film holds none (render_progressive has not "
                             "run, or another render has replaced its film)")
        if pr["epochs"] < 2:
            raise ValueError(f"VarianceDenoise needs a progressive render of at least two epochs (the variance of one sample is unknown), "
                             f"this one has run {pr['epochs']}")
        return pr

    def _color_plane(self):
        """An uninitialised float32 device tensor of shape (n, 3): room for one Color plane of this film."""
        import torch
        return torch.empty(self.res[0] * self.res[1], 3, dtype=torch.float32, device=self.device)

    def _shown_film(self, denoise):
        """The film dict a Color image is made from: the channels, with denoised_color(denoise) as their colour under a denoiser."""
        return self.channels if denoise is None else dict(self.channels, color=self.denoised_color(denoise))

    def _denoise_variance(self, params, want_variance):
        import torch
        params = _denoise_params(self.channel_kinds, params)
        pr = self._variance_state()
        w, h = self.res
        with torch.cuda.device(self.device):
            out = self._color_plane()
            var = torch.empty(w * h, dtype=torch.float32, device=self.device) if want_variance else None
            self.ctx.denoise_variance(pr["params"], self.channels, pr["state"], out, params, var)
            return out, var

    def denoised_color(self, params):
        """The film's Color after a denoiser as a float32 device tensor of shape (n, 3), pixels in the film's order: the a-trous filter
        (Denoise `params`, rayn_hip_denoise_device) or the variance-guided one (VarianceDenoise `params`,
        rayn_hip_denoise_variance_device), which uses the state of the progressive render the film holds and raises ValueError when it
        holds none or that render has run fewer than two epochs.  A guide the film lacks is switched off; the film itself is not
        changed."""
        import torch
        if isinstance(params, VarianceDenoise):
            return self._denoise_variance(params, False)[0]
        params = _denoise_params(self.channel_kinds, params)
        w, h = self.res
        with torch.cuda.device(self.device):
            out = self._color_plane()
            self.ctx.denoise(w, h, self.channels, out, params)
            return out

    def denoised_variance(self, params):
        """The variance of the mean luminance after the variance-guided denoiser (VarianceDenoise `params`) - what is left of the
        progressive render's estimate once the filter has averaged it with squared weights - as float32 (h, w), rows bottom-up like
        error_map; NaN where the filter had no estimate to go by (the pixel passed through).  ValueError as denoised_color."""
        w, h = self.res
        return self._denoise_variance(params, True)[1].cpu().numpy().reshape(h, w)

    def display_color(self, display, denoise=None, transparent_background=False, display_state=None, adapt=1.0):
        """The film's Color after the HDR display transform (Display `display`, rayn_hip_display_color_device) as a float32 device tensor
        of shape (n, 3), pixels in the film's order: exposed, bloomed and tone-mapped, before gamma and quantisation.  The input is Color
        + Background when the film has a Background and transparent_background is false, as in save_to; with `denoise`, the denoised
        Color.  display_state (Context.display_state()) and adapt: as Context.display; None = this image's own metering."""
        import torch
        _check_display(display)
        self._save_jobs([ChannelKind.Color], transparent_background)
        w, h = self.res
        with torch.cuda.device(self.device):
            out = self._color_plane()
            self.ctx.display(display, self.have_mask(), transparent_background, w, h, self._shown_film(denoise), out, display_state, None, adapt)
            return out

    def pixels(self, kind, transparent_background=False, denoise=None, display=None, display_state=None, adapt=1.0):
        """The 8-bit image Film::save_to writes for channel `kind` (rows top-down; (h, w, 4 / 3 / 1) uint8), computed on the device
        (rayn_hip_save_to_pixels_device); only the 8-bit image is copied back.  Channels the film lacks are not read.  With `denoise`
        (a Denoise or a VarianceDenoise), the Color image is made from denoised_color(denoise); the other channels are unchanged.
        With `display` (a Display, an extension), the Color image goes through the HDR display transform (after the denoiser, if any;
        rayn_hip_display_pixels_device) with display_state and adapt as Context.display takes them; the other channels ignore it."""
        import torch
        w, h = self.res
        with torch.cuda.device(self.device):
            out, bpp = self._pixels_device(kind, transparent_background, denoise, display, display_state, adapt)
            return out.cpu().numpy().reshape(h, w, bpp)  # .cpu() waits for the current stream, where the kernels were enqueued

    def _pixels_device(self, kind, transparent_background, denoise, display, display_state=None, adapt=1.0):
        """pixels' image as it is enqueued on the current stream: (the uint8 device tensor, bytes per pixel).  Under torch.cuda.device."""
        import torch
        ((kind, bpp, _),) = self._save_jobs([kind], transparent_background)
        if display is not None:
            _check_display(display)
        w, h = self.res
        film = self._shown_film(denoise) if kind == ChannelKind.Color else self.channels
        out = torch.empty(h * w * bpp, dtype=torch.uint8, device=self.device)
        if display is not None and kind == ChannelKind.Color:
            self.ctx.display(display, self.have_mask(), transparent_background, w, h, film, out, display_state, None, adapt)
        else:
            self.ctx.save_to_pixels(kind, self.have_mask(), transparent_background, w, h, film, out)
        return out, bpp

    def save_to(self, write_channels, output_folder, base_name, transparent_background=False, denoise=None, display=None, png="host"):
        """Film::save_to (src/film.rs:205-378) - the post-process after the hot path, arm by arm (on the device: pixels); the
        reference's Err(String) cases raise ValueError with the same text.  The PNGs are those of rayn_amd.image (host reference).
        With `denoise` (a Denoise or a VarianceDenoise, extensions), the Color image is made from the denoised Color and written as
        {base_name}_color_denoised.png instead of {base_name}_color.png; the other channels are unchanged.  With `display` (a Display, an
        extension) the Color image goes through the HDR display transform and its file name gets _display appended:
        {base_name}_color_display.png, {base_name}_color_denoised_display.png.  With png="device" (an extension) the stream inside
        every file is encoded on the device (Context.png_encode: adaptive row filters, run-length and Huffman coding) and framed by
        image.png_from_stream: the same names and the same pixels in files of other, on rendered images smaller, bytes.  png="device-lz77"
        is the same with the encoder that also finds LZ77 matches (Context.png_encode_lz77).  Any other value raises ValueError before
        anything is written."""
        _check_png(png)
        os.makedirs(output_folder, exist_ok=True)
        for kind in write_channels:
            ((kind, _, suffix),) = self._save_jobs([kind], transparent_background)  # the reference fails at the first bad channel, after writing the ones before
            if denoise is not None and kind == ChannelKind.Color:
                suffix = "color_denoised"
            if display is not None and kind == ChannelKind.Color:
                suffix += "_display"
            path = os.path.join(output_folder, f"{base_name}_{suffix}.png")
            if png == "host":
                image.save(path, self.pixels(kind, transparent_background, denoise, display))
                continue
            import torch
            w, h = self.res
            with torch.cuda.device(self.device):
                d_img, bpp = self._pixels_device(kind, transparent_background, denoise, display)
                d_enc = torch.empty(png_stream_bound(w, h, bpp), dtype=torch.uint8, device=self.device)
                self.ctx.png_encode(w, h, bpp, d_img, d_enc, lz77=png == "device-lz77")
                encoded = d_enc.cpu().numpy()  # waits for the current stream
            with open(path, "wb") as f:
                f.write(image.png_from_stream(w, h, bpp, image.png_stream_of(encoded)))

    def save_jpeg(self, write_channels, output_folder, base_name, jpeg=Jpeg(), denoise=None, display=None, transparent_background=False):
        """save_to's images as baseline JPEG files (an extension): {base_name}_{suffix}.jpg with save_to's suffixes, the scan encoded on
        the device (Context.jpeg_encode with the Jpeg `jpeg`) and framed by image.jpeg_from_scan.  A grey image (Alpha) has one form and
        ignores the subsampling.  JPEG has no alpha: a kind whose image has 4 bytes per pixel - Color under transparent_background -
        raises ValueError, like a `jpeg` that is no Jpeg and a channel save_to rejects, before anything is written."""
        import torch
        _check_jpeg(jpeg)
        jobs = _jpeg_jobs(self._save_jobs(list(write_channels), transparent_background))
        os.makedirs(output_folder, exist_ok=True)
        w, h = self.res
        for kind, bpp, suffix in jobs:
            if denoise is not None and kind == ChannelKind.Color:
                suffix = "color_denoised"
            if display is not None and kind == ChannelKind.Color:
                suffix += "_display"
            sub = jpeg.mode(bpp)
            with torch.cuda.device(self.device):
                d_img, bpp = self._pixels_device(kind, transparent_background, denoise, display)
                d_enc = torch.empty(jpeg_scan_bound(w, h, bpp, sub, jpeg.restart), dtype=torch.uint8, device=self.device)
                self.ctx.jpeg_encode(w, h, bpp, d_img, d_enc, jpeg.quality, sub, jpeg.restart)
                encoded = d_enc.cpu().numpy()  # waits for the current stream
            with open(os.path.join(output_folder, f"{base_name}_{suffix}.jpg"), "wb") as f:
                f.write(image.jpeg_from_scan(w, h, bpp, jpeg, encoded))

    def save_exr(self, path, channels=None, half=True, gbuffer=False, transparent_background=False, denoise=None, exr="device"):
        """Write the float film to `path` as ONE multi-channel OpenEXR file (an extension; scanlines, ZIP compression; include/rayn_hip.h
        defines the chunks): the kinds `channels`, by default every kind the film holds - without Background under
        transparent_background, the foreground alone - as the layers R G B (Color; with `denoise`, denoised_color's, as in save_to), A
        (Alpha), background.R .G .B (kept as its own layer, not added in) and N.X .Y .Z (WorldNormal), HALF or, with half=False, FLOAT,
        the film's own bits.  gbuffer=True adds gbuffer()'s P.X P.Y P.Z and Z, always FLOAT, and the UINT id (a miss stays 0xFFFFFFFF).
        exr: "device" encodes the chunks on the GPU (Context.exr_encode) and frames them on the host (image.exr_from_chunks),
        "device-lz77" the same with LZ77 matches, "host" makes the same file layout with zlib (image.save_exr_host); anything else
        raises ValueError before anything is written.  A film whose file would reach 2^31 bytes raises ValueError too."""
        import torch
        _check_exr(exr)
        if channels is None and transparent_background:
            channels = [k for k in self.channel_kinds if k != ChannelKind.Background]
        kinds = _exr_kinds(self.channel_kinds, channels)
        if self.channels is None:
            raise ValueError("the film holds no rendered frame (render_frame_into, render_sequence or render_progressive has not run)")
        w, h = self.res
        with torch.cuda.device(self.device):
            film = self._shown_film(denoise) if ChannelKind.Color in kinds else self.channels
            chans = exr_channels(kinds, film, half, self._gbuffer_device() if gbuffer else None)
            bound = _exr_bound(w, h, chans)
            if exr == "host":
                image.save_exr_host(path, w, h, [(n, ty, t.reshape(-1).cpu().numpy().view(np.uint32)[o::s][:w * h]) for n, t, s, o, ty in chans])
                return
            d_enc = torch.empty(bound, dtype=torch.uint8, device=self.device)
            self.ctx.exr_encode(w, h, chans, d_enc, lz77=exr == "device-lz77")
            encoded = d_enc.cpu().numpy()  # waits for the current stream
        data = image.exr_from_chunks(w, h, [(n, ty) for n, _, _, _, ty in chans], encoded)
        with open(path, "wb") as f:
            f.write(data)

    def save_hdr(self, path, transparent_background=False):
        """Write the float Color channel to `path` as a little-endian PFM (image.save_pfm; rows bottom-up, like the film): Color +
        Background when the film has a Background and transparent_background is false, as save_to composes them, else Color.  Host only."""
        rgb = self.channel(ChannelKind.Color)
        if ChannelKind.Background in self.channel_kinds and not transparent_background:
            with np.errstate(invalid="ignore", over="ignore"):
                rgb = (rgb + self.channel(ChannelKind.Background)).astype(np.float32)
        image.save_pfm(path, rgb)

    def render_progressive(self, world, camera, integrator, filter, tile_size, frame, time_range, samples, progressive=None, on_epoch=None,
                           resume=None):
        """Render frame `frame` progressively (an extension; include/rayn_hip.h has the definition): a series of epochs, each an ordinary
        render of the frame (render_frame_into's arguments) under the sample tables of progressive_seed(frame, epoch), accumulated on the
        device.  After every epoch film.channels holds the mean film of all epochs so far, so pixels / save_to / denoise= work on it
        unchanged; denoise=VarianceDenoise() also uses what the render measured (the per-pixel variance in its state).  With progressive.adaptive, tiles whose error estimate has met the target retire and later epochs render only the
        tiles still active (Context.set_tile_subset); the render ends when none is left or after progressive.max_epochs.

        The world is uploaded once; scramble and filter tables are built once; epoch e + 1's R_d tables are built on a host thread while
        epoch e renders; per epoch only the active list (16 bytes + 4 per tile) comes back to the host.  on_epoch(report), called after
        every epoch with the report so far (report["epoch_film"]: the device film the epoch rendered; only the tiles
        report["rendered_tiles"], None = all, are current), may return False to stop.  resume=path continues the render a checkpoint
        (save_checkpoint) was made from; ValueError if it belongs to another render.  The tile subset is cleared on every exit path.

        Returns the report (a dict): epochs (run in total, those before a resume included), seed and rendered_tiles of the last epoch,
        active_tiles, totals, tile_epochs (per-tile epoch counts), paths traced by this call, paths_non_adaptive (what its epochs would
        have traced over the whole frame), and stats (Context.stats() of every epoch of this call plus "epoch" and "seed")."""
        import concurrent.futures as cf
        import torch
        progressive = Progressive() if progressive is None else progressive
        w, h = self.res
        spp, mb, vm = 4 * samples, integrator.max_bounces, integrator.volume_marches
        p0 = frame_params(w, h, samples, mb, vm, frame, time_range, tile_size)
        progressive_seed(frame, progressive.max_epochs - 1, mb, vm)  # every seed of the run is valid, or nothing renders
        desc = world.to_desc(camera)
        key = _prog.checkpoint_key((w, h), tile_size, samples, mb, vm, frame, (p0.time_start, p0.time_end), filter, desc, progressive,
                                   self.ctx.fma_policy)
        rects = _prog.tile_rects(w, h, tile_size)
        covered = sum((x1 - x0) * (y1 - y0) for x0, y0, x1, y1 in rects)
        first, restored = 0, None
        if resume is not None:
            saved, restored, first = _prog.read_checkpoint(resume)
            _prog.check_key(saved, key)
        report = {"epochs": first, "seed": None, "rendered_tiles": None, "active_tiles": None, "totals": None, "tile_epochs": None, "paths": 0,
                  "paths_non_adaptive": 0, "stats": [], "epoch_film": None}
        table_pool = cf.ThreadPoolExecutor(max_workers=1, thread_name_prefix="rayn-rd-tables")
        try:
            with torch.cuda.device(self.device):
                stream = torch.cuda.current_stream()
                self.ctx.upload_world(desc)
                self._last_camera = desc.camera
                d_state = torch.empty(_prog.state_bytes(w, h, tile_size), dtype=torch.uint8, device=self.device)
                d_mean = alloc_device_film(w, h, self.device)
                if restored is None:
                    self.ctx.progressive_reset(p0, d_state, stream.cuda_stream)
                else:
                    d_state.copy_(torch.from_numpy(_prog.join_state(restored, w, h, tile_size)))
                    for k, v in _prog.mean_film(restored, w, h, tile_size).items():
                        d_mean[k].copy_(torch.from_numpy(v).reshape(d_mean[k].shape))
                self.channels = d_mean
                self._progressive = {"state": d_state, "params": p0, "key": key, "epochs": first, "noise_floor": progressive.noise_floor,
                                     "film": d_mean}
                self._last_params = p0
                active, totals = self.ctx.progressive_fetch_active(p0, d_state, stream.cuda_stream)
                report.update(active_tiles=active, totals=totals)
                if first < progressive.max_epochs and len(active):
                    seeds = (progressive_seed(frame, e, mb, vm) for e in range(first, progressive.max_epochs))
                    tables = RdTablePrefetch(table_pool, seeds, spp, mb, vm, w, h, filter, self.device)
                    d_epoch = alloc_device_film(w, h, self.device)
                    report["epoch_film"] = d_epoch
                epoch = first
                while epoch < progressive.max_epochs and len(active):
                    seed = progressive_seed(frame, epoch, mb, vm)
                    d_tables = tables.next()
                    subset = None if len(active) == len(rects) else active
                    self.ctx.set_tile_subset(subset)
                    # the epoch's render carries the seed as its frame: the table broadcast of a multi-device context keys on it
                    p = frame_params(w, h, samples, mb, vm, seed, (p0.time_start, p0.time_end), tile_size)
                    self.ctx.render_device(p, d_tables, d_epoch, stream.cuda_stream)  # blocking: returns when the epoch's film is complete
                    st = self.ctx.stats()
                    st.update(epoch=epoch, seed=seed)
                    self.ctx.progressive_accumulate(p0, progressive, subset, d_epoch, d_state, d_mean, stream.cuda_stream)
                    active, totals = self.ctx.progressive_fetch_active(p0, d_state, stream.cuda_stream)
                    epoch += 1
                    self.progressive_epoch += 1
                    self._progressive["epochs"] = epoch
                    report["stats"].append(st)
                    report.update(epochs=epoch, seed=seed, rendered_tiles=subset, active_tiles=active, totals=totals,
                                  paths=report["paths"] + st["paths"], paths_non_adaptive=report["paths_non_adaptive"] + covered * spp)
                    if on_epoch is not None and on_epoch(report) is False:
                        break
                report["tile_epochs"] = self.ctx.progressive_tile_report(p0, d_state, stream.cuda_stream)["epochs"]
            return report
        finally:
            self.ctx.set_tile_subset(None)
            table_pool.shutdown(wait=True, cancel_futures=True)

    def _progressive_arrays(self):
        if self._progressive is None:
            raise ValueError("the film holds no progressive render (render_progressive has not run)")
        pr = self._progressive
        w, h = self.res
        return _prog.split_state(pr["state"].cpu().numpy(), w, h, (pr["params"].tile_w, pr["params"].tile_h)), pr

    def save_checkpoint(self, path):
        """Write the progressive render this film holds to `path` (one .npz: the state, the tile records and the key of the render);
        render_progressive(..., resume=path) with the same arguments continues it, bit for bit as if it had not stopped."""
        arrays, pr = self._progressive_arrays()
        _prog.write_checkpoint(path, pr["key"], arrays, pr["epochs"])

    def sample_count_image(self):
        """u8 heat map ((h, w), rows top-down) of the per-tile epoch counts of the progressive render: 255 = the largest count."""
        arrays, pr = self._progressive_arrays()
        w, h = self.res
        return _prog.sample_count_image(arrays["epochs"], w, h, (pr["params"].tile_w, pr["params"].tile_h))

    def error_map(self):
        """The error estimate e_p of every pixel of the progressive render, float32 (h, w), rows bottom-up like the film."""
        arrays, pr = self._progressive_arrays()
        w, h = self.res
        return _prog.error_map(arrays, w, h, (pr["params"].tile_w, pr["params"].tile_h), pr["noise_floor"])

    def render_sequence(self, world, camera, integrator, filter, tile_size, frames, frame_rate, shutter_speed, samples, write_channels,
                        output_folder, base_name, transparent_background=False, writers=None, denoise=None, display=None, upscale=None, supersample=None, preview=None,
                        interpolate=None, png="host", exr=None, exr_half=True, jpeg=None, video=None, temporal=None):
        """rayn's main loop (src/main.rs:58-96) on the GPU: for each frame of `frames`, render_frame_into at
        frame_start = frame as f32 * (1.0 / frame_rate as f32), frame_end = frame_start + shutter_speed (f32, src/main.rs:61-62), then
        save_to(write_channels, output_folder, f"{base_name}_{frame:04d}", transparent_background).  rayn writes every frame under
        one base name (each frame overwrites the last); the per-frame names are an extension.  The images are byte-identical to
        those of that plain loop.  Returns the render stats of every frame (Context.stats() plus "frame").

        The world is uploaded once; the scramble and filter tables are built once; the device film, the device tables and the
        8-bit images are allocated once.  The R_d tables (Samples::new_rd, the only frame-dependent ones) are built on a host
        thread one frame ahead.  After frame k's render returns, its post-process kernels and the copies of its 8-bit images into
        pinned host buffers (two sets, used in turn) are enqueued on the same stream, and a pool of at most 8 writer threads
        encodes the PNGs of frame k while frame k + 1 renders.  A channel combination the reference rejects raises ValueError
        before anything renders; a render or writer error stops the sequence and is raised after every thread has been joined.
        Afterwards film.channels holds the last frame, as the plain loop leaves it.

        With `denoise` (a Denoise), every frame's Color image is made from the denoised Color and written as _color_denoised.png, as
        save_to(..., denoise=denoise) does: the denoiser's kernels go on the render stream ahead of that frame's post-process kernels,
        and its scratch and denoised plane are allocated once.  A VarianceDenoise without `temporal` raises ValueError: a sequence's
        frames are plain renders and carry no variance.

        With `temporal` (a Temporal, an extension), every frame's Color is accumulated over the frames before it: after the render, the
        frame's G-buffer pass and the temporal accumulate go on the render stream, the Color image is made from the accumulated colour and
        written as _color_temporal.png; with `denoise` as well the a-trous filter runs on the accumulated colour and the file is
        _color_temporal_denoised.png.  The two histories, the G-buffer and the scratch are allocated once.  The first frame of a call has
        no history; frames that are not consecutive still reproject, over whatever time lies between their starts.  The film's channels
        stay what the integrator wrote.  temporal=None is the path described above, unchanged.

        With `temporal` and a VarianceDenoise as `denoise`, the accumulate also carries the luminance moments (two more buffers, allocated
        once), and the variance-guided filter runs on the accumulated colour with a variance estimated from them
        (Context.denoise_temporal_variance); the file is _color_temporal_denoised.png.  The film needs its Alpha channel when sigma_alpha
        != 0 (WorldNormal it needs anyway).  Recommended for sequences: VarianceDenoise(1, 4.0, 0.4, 0.3), 0.46x the
        raw frame where Temporal() alone gives 0.49x.

        With temporal.feedback == 0 (the default) the filtered colour is not fed back into the history: every frame's filter is a function
        of that frame's buffers.  With temporal.feedback > 0 the filter of frame i also blends the output of its first pass into frame
        i's history with that strength (rayn_hip_denoise_temporal_variance_feedback_device), so frame i + 1 reprojects what frame i's filter
        left; the file names do not change.  It needs a VarianceDenoise as `denoise` - there is nothing to feed back otherwise - and raises
        ValueError before anything renders without one.  Measured on the sequence of DESIGN.md section 8, no strength above 0 lowered the
        error (0.4675x at best, against 0.4571x): the option is there to be measured on other scenes and sizes, not recommended.

        With `display` (a Display, an extension), every frame's Color image goes through the HDR display transform, after the temporal and
        denoise kernels and in place of the plain Color post-process kernel, on the render stream; the file name gets _display appended to
        whatever suffix it would have had (_color_display.png, _color_temporal_denoised_display.png, ...).  One auto-exposure state serves
        the call: the first frame takes its own metered value, every later one blends with adapt = 1 - exp(-dt / display.adaptation), dt
        the difference of the f32 frame starts (1 without adaptation).  The exposure stays on the device, so nothing synchronises; the
        state and the scratch are allocated once.  display=None is the path described above, unchanged.

        With `upscale` (an Upscale, an extension), every frame is rendered at the film's resolution and rebuilt on the device at
        upscale.factor times that size, as Film.upscaled does: after the render, the frame's G-buffer passes at both resolutions and the
        upscale kernel go on the render stream, every written image is made from the upscaled film and its file name gets _x{factor}
        appended to whatever suffix it would have had (_color_x2.png, _alpha_x2.png, _color_denoised_display_x2.png, ...).  `denoise` (a
        Denoise) and `display` then work on the upscaled film.  The G-buffers, the upscaled film and the scratch are allocated once and
        nothing synchronises.  The film's channels stay the rendered, low frame.  `temporal` together with `upscale` raises ValueError
        unless `supersample` says how the two meet.  upscale=None is the path described above, unchanged.

        With `supersample` (a Supersample, an extension; it needs `upscale` and `temporal` both), the temporal history lives at the
        upscaled resolution: per frame the world is uploaded with the frame's camera offset by supersample.offset(factor, i) low pixels
        (jittered_camera), the frame is rendered and its low G-buffer traced through that camera, the world is uploaded with the frame's
        own camera again, the high G-buffer is traced, and ONE kernel (Context.temporal_upscale) upscales the frame and blends it into
        the full-size history in place of Context.upscale.  The Color image is made from the accumulated colour, every other image from
        the kernel's upscaled planes; the names are those of upscale= with temporal= (_color_temporal_x2.png, ...).  `denoise` (a
        Denoise) and `display` work on the high film as for upscale=.  A VarianceDenoise, temporal.resample != "bilinear" and
        temporal.feedback > 0 raise ValueError before anything renders: moments, Catmull-Rom and feedback are not built at two
        resolutions.  Uploading a world is a host-side copy and every pass stages its own device scene on the stream when it is
        called, so the two uploads per frame need no synchronisation; without jitter there are none.  The histories, G-buffers and
        scratch are allocated once.  Afterwards the uploaded world is the frame's own.  supersample=None is the path described above,
        unchanged.

        With `preview` (a Preview, an extension), every frame is the preview integrator's image in place of the render - primary hit,
        viewer-facing normal, ambient occlusion; Context.preview with the frame's preview_tables - and everything after it is the path
        described above: the film's Color, Alpha and WorldNormal planes are the preview's (a Background plane stays zero), the Color file
        name gets _preview right after _color (_color_preview.png, _color_preview_temporal_denoised_display.png, ...), the other images
        keep their names.  `display`, `denoise` (a Denoise) and `temporal` compose with it; `temporal` reprojects through the preview's own
        primary hits instead of tracing a G-buffer.  `integrator` and `filter` are not looked at (None will do), `samples` neither, and the
        returned stats hold only "frame".  `upscale`, `supersample` and a VarianceDenoise raise ValueError before anything renders.  The
        preview's tables and scratch are allocated once; the preview does not wait for the GPU, so the host runs ahead until a pinned
        image slot is needed again.  preview=None is the path described above, unchanged.

        With `interpolate` (an Interpolate, an extension), only every interpolate.every-th entry of `frames` - and the last - is rendered,
        exactly as above: a KEY.  Every other entry is GENERATED from the nearest key on each side (Context.interpolate): its own G-buffer
        is traced at its own start time, f32(frame) * (1 / frame_rate) like any frame's, every pixel's primary hit is projected into both
        keys, and the taps that show the same surface are blended by time.  `frames` must ascend.  The loop renders key B, then writes
        the frames between A and B in ascending order, then B, so the display's auto-exposure state and the writers see the frames in
        time order.  Two key films and two key G-buffers are used in turn; one G-buffer, one generated film, the scratch and the image
        slots are allocated once, and nothing new synchronises.  `denoise` (a Denoise) and `display` run on a generated film as on a
        rendered one.  Every Color image of the call - keys and generated frames alike, so that the files form one numbered sequence -
        gets _interp right after _color (_color_interp.png, _color_interp_denoised_display.png); the keys' images are byte for byte
        those of the plain loop.  The returned stats of a generated frame are {"frame": f, "generated": True}.  Together with
        `temporal`, `upscale`, `supersample` or `preview` it raises ValueError before anything renders: not built.  View-dependent
        shading and the shadows of moving objects are blended, not reprojected, and a generated frame averages two keys' noise
        (DESIGN.md section 8).  interpolate=None is the path described above, unchanged.

        With png="device" (an extension) the PNG streams are encoded on the device: after each image's post-process kernel the encoder
        (Context.png_encode) goes on the render stream, the encoded buffer - png_stream_bound bytes, whose first word says how many
        count - is copied into the pinned slot in place of the raw image, and the writer thread frames the stream (image.png_from_stream:
        chunk headers and the CRC-32) and writes the file.  The encoded buffers and the encoder's scratch are allocated once and nothing
        new synchronises.  File names do not change and the files decode to the same pixels; their bytes differ from the host
        encoder's.  png="device-lz77" puts the encoder with LZ77 matches (Context.png_encode_lz77) in the same place, with
        the same buffers and a larger scratch.  Any other value raises ValueError before anything renders.  png="host" is the path
        described above, unchanged.

        With `exr` ("host", "device" or "device-lz77"; an extension) every frame ALSO writes {base_name}_{frame:04d}.exr, one multi-channel
        OpenEXR file of the kinds in write_channels as Film.save_exr lays them out (HALF, or FLOAT with exr_half=False): Color from the
        film the Color PNG is made from - accumulated, denoised, upscaled, generated - before any display transform, the other layers
        from the film the other images are made from.  With "device" the chunks are encoded on the render stream behind the frame's PNG
        work (Context.exr_encode), the encoded buffer goes into a pinned slot of its own and a writer thread frames it
        (image.exr_from_chunks); with "host" the float planes go into pinned slots and the writer thread runs image.save_exr_host.
        Buffers and scratch are allocated once and nothing new synchronises.  Any other value raises ValueError before anything renders;
        exr=None leaves every file byte for byte as it is.

        With `jpeg` (a Jpeg, an extension) every PNG of the call also gets a baseline JPEG next to it, same name, .jpg: after the image's
        post-process kernel the encoder (Context.jpeg_encode) goes on the render stream, the encoded buffer - jpeg_scan_bound bytes -
        goes into a pinned slot of its own and a writer thread frames the scan (image.jpeg_from_scan).  With `video` (a Video) the call
        also writes ONE Motion-JPEG AVI (image.AviWriter, at frame_rate) of the frame's shown Color image - the image whose PNG carries
        _color... in its name, after denoise, display, upscale, preview and interpolate - so write_channels must name Color.  Its frames
        are byte for byte what jpeg=video.jpeg writes for that image; they reach the file in frame order through one writer thread of
        their own, and the file is closed - and plays as far as it got - also when the call raises.  Where jpeg= and video.jpeg are equal the image is encoded once for both.  Video(images=False) is the one
        switch that removes files: no PNG, .jpg or EXR is written, only the video.  JPEG has no alpha: under transparent_background a
        Color image raises ValueError, like every wrong value, before anything renders.  With jpeg=None and video=None every file is
        byte for byte as it is."""
        import concurrent.futures as cf
        import torch
        # the rules about the options alone come first and need nothing of the film, not even its channels (a bare Film.__new__ gets them)
        kinds = getattr(self, "channel_kinds", ())
        plan = plan_sequence(kinds, write_channels, transparent_background, denoise, display, upscale, supersample, temporal, preview, interpolate, png, exr)
        video_job, images = _check_sequence_jpeg(plan, write_channels, jpeg, video)
        frames = [int(f) for f in frames]
        os.makedirs(output_folder, exist_ok=True)
        w, h = self.res
        ow, oh = plan.out_res(self.res)
        # the JPEG encodes of a frame: [job, its Jpeg, whether a .jpg is written, whether it is the video's frame]; where jpeg= and
        # video= agree on the options the Color image is encoded once and goes to both
        jpeg_work = [[j, jpeg, True, False] for j in range(len(plan.jobs))] if (jpeg is not None and images) else []
        if video is not None:
            if jpeg_work and video.jpeg == jpeg:
                jpeg_work[video_job][3] = True
            else:
                jpeg_work.append([video_job, video.jpeg, False, True])
        avi = None
        f32 = np.float32
        inv_rate, shutter = f32(1.0) / f32(frame_rate), f32(shutter_speed)
        if plan.preview is not None and integrator is None:
            spp, mb, vm = 4 * samples, 0, 2
        else:
            spp, mb, vm = 4 * samples, integrator.max_bounces, integrator.volume_marches
        n_writers = max(1, min(8, 2 * len(plan.jobs) if writers is None else int(writers)))
        stats, pending = [], [[], []]  # pending[slot]: writer futures still reading that slot's pinned images
        table_pool = cf.ThreadPoolExecutor(max_workers=1, thread_name_prefix="rayn-rd-tables")
        write_pool = cf.ThreadPoolExecutor(max_workers=n_writers, thread_name_prefix="rayn-png")
        video_pool = cf.ThreadPoolExecutor(max_workers=1, thread_name_prefix="rayn-avi")  # one thread: the frames keep their order

        def write(event, img, path):
            event.synchronize()
            image.save(path, img)

        def write_encoded(event, encoded, bpp, path):
            event.synchronize()
            data = image.png_from_stream(ow, oh, bpp, image.png_stream_of(encoded))
            with open(path, "wb") as f:
                f.write(data)

        def write_exr(event, held, named, path):
            event.synchronize()
            if plan.exr == "host":
                planes = {k: t.numpy().reshape(-1).view(np.uint32) for k, t in held.items()}
                image.save_exr_host(path, ow, oh, [(n, ty, a[o::s][:ow * oh]) for n, a, s, o, ty in exr_channels(plan.exr_kinds, planes, exr_half)])
                return
            data = image.exr_from_chunks(ow, oh, named, held.numpy())
            with open(path, "wb") as f:
                f.write(data)

        def write_jpeg(event, encoded, bpp, options, path):
            """The framed file of an encoded scan to `path`, or into the video for None"""
            event.synchronize()
            data = image.jpeg_from_scan(ow, oh, bpp, options, encoded)
            if path is None:
                avi.add(data)
                return
            with open(path, "wb") as f:
                f.write(data)

        def wait_slot(slot):
            for fut in pending[slot]:
                fut.result()  # re-raises a writer's exception
            pending[slot] = []

        try:
            if not frames:
                return stats
            if video is not None:
                avi = image.AviWriter(video.path, ow, oh, frame_rate)
            with torch.cuda.device(self.device):
                stream = torch.cuda.current_stream()
                desc = world.to_desc(camera)
                self.ctx.upload_world(desc)
                self._last_camera = desc.camera
                itp = plan.interpolate
                rendered = frames if itp is None else [f for i, f in enumerate(frames) if itp.is_key(i, len(frames))]
                tables = None if plan.preview is not None else RdTablePrefetch(table_pool, rendered, spp, mb, vm, w, h, filter, self.device)
                d_film = alloc_device_film(w, h, self.device)
                # the video alone: only the image it shows is made, and nothing of the PNG path is allocated
                d_img = [torch.empty(oh * ow * bpp if (images or j == video_job) else 0, dtype=torch.uint8, device=self.device)
                         for j, (_, bpp, _) in enumerate(plan.jobs)]
                post = _SequencePost(self, plan, desc, d_film)
                on_device, lz77 = images and plan.png != "host", plan.png == "device-lz77"
                # what goes to the host per image: the raw image, or the encoder's output (its scratch serves every image in turn)
                h_bytes = [0 if not images else png_stream_bound(ow, oh, bpp) if on_device else oh * ow * bpp for _, bpp, _ in plan.jobs]
                h_img = [[torch.empty(n, dtype=torch.uint8, pin_memory=n > 0) for n in h_bytes] for _ in range(2)]
                if on_device:
                    d_enc = [torch.empty(n, dtype=torch.uint8, device=self.device) for n in h_bytes]
                    d_png_scratch = torch.empty(max((png_scratch_bytes_lz77 if lz77 else png_scratch_bytes)(ow, oh, bpp) for _, bpp, _ in plan.jobs), dtype=torch.uint8, device=self.device)

                if jpeg_work:
                    jpeg_geo = [(plan.jobs[j][1], o.mode(plan.jobs[j][1]), o.restart) for j, o, _, _ in jpeg_work]
                    d_jpeg = [torch.empty(jpeg_scan_bound(ow, oh, bpp, sub, ri), dtype=torch.uint8, device=self.device) for bpp, sub, ri in jpeg_geo]
                    h_jpeg = [[torch.empty(d.numel(), dtype=torch.uint8, pin_memory=True) for d in d_jpeg] for _ in range(2)]
                    d_jpeg_scratch = torch.empty(max(jpeg_scratch_bytes(ow, oh, bpp, sub, ri) for bpp, sub, ri in jpeg_geo), dtype=torch.uint8, device=self.device)

                if plan.exr is not None and images:
                    exr_keys = [_EXR_LAYERS[k][0] for k in plan.exr_kinds]
                    exr_probe = exr_channels(plan.exr_kinds, dict.fromkeys(exr_keys), exr_half)
                    exr_named, exr_bound = [(n, ty) for n, _, _, _, ty in exr_probe], _exr_bound(ow, oh, exr_probe)
                    h_exr = [None, None]  # per slot: the pinned planes ("host", made at the slot's first frame) or the pinned encoded buffer
                    if plan.exr != "host":
                        d_exr = torch.empty(exr_bound, dtype=torch.uint8, device=self.device)
                        d_exr_scratch = torch.empty(exr_scratch_bytes(ow, oh, exr_layout(exr_probe), plan.exr == "device-lz77"), dtype=torch.uint8, device=self.device)
                        h_exr = [torch.empty(exr_bound, dtype=torch.uint8, pin_memory=True) for _ in range(2)]

                def params_of(frame):
                    start = f32(frame) * inv_rate
                    return start, frame_params(w, h, samples, mb, vm, frame, (float(start), float(f32(start + shutter))), tile_size)

                def render(i, frame, d_into):
                    """Frame `frame`, entry i of the call, into the device film d_into -> (start, frame parameters, stats)."""
                    d_tables = None if tables is None else tables.next()
                    for fut in pending[0] + pending[1]:
                        if fut.done() and fut.exception() is not None:
                            raise fut.exception()
                    start, p = params_of(frame)
                    post.jitter(i, p)
                    if plan.preview is not None:
                        post.preview(p, stream.cuda_stream)
                        st = {}
                    else:
                        self.ctx.render_device(p, d_tables, d_into, stream.cuda_stream)  # blocking: returns when the frame is complete
                        st = self.ctx.stats()
                    st["frame"] = frame
                    self.channels = d_into
                    self._last_params = p
                    self.progressive_epoch += 1
                    return start, p, st

                def emit(i, frame, start, p, st, d_src=None):
                    """The images of entry i, whose film is d_src (None: the sequence's own d_film)."""
                    stats.append(st)
                    # Frame k's post-process and copies go on the render stream, so frame k + 1's render (enqueued on the same stream
                    # after them) cannot overwrite d_film or d_img before they have been read; only the pinned slot needs a host-side
                    # wait: its images from frame k - 2 must have been encoded.
                    slot = i % 2
                    wait_slot(slot)
                    d_shown, d_base = post.enqueue(i, p, stream.cuda_stream, d_src)
                    for j, ((kind, bpp, _), d, hbuf) in enumerate(zip(plan.jobs, d_img, h_img[slot])):
                        if not images and j != video_job:
                            continue
                        post.pixels(kind, start, d_shown if kind == ChannelKind.Color else d_base, d, stream.cuda_stream)
                        for n, (jj, o, _, _) in enumerate(jpeg_work):  # behind the image's post-process kernel, on the same stream
                            if jj == j:
                                self.ctx.jpeg_encode(ow, oh, bpp, d, d_jpeg[n], o.quality, o.mode(bpp), o.restart, d_jpeg_scratch, stream.cuda_stream)
                                h_jpeg[slot][n].copy_(d_jpeg[n], non_blocking=True)
                        if not images:
                            continue
                        if on_device:
                            self.ctx.png_encode(ow, oh, bpp, d, d_enc[j], d_png_scratch, stream.cuda_stream, lz77)
                            d = d_enc[j]
                        hbuf.copy_(d, non_blocking=True)
                    if plan.exr is not None and images:  # behind the frame's PNG work, on the same stream
                        d_src_exr = dict(d_base, color=d_shown["color"]) if "color" in exr_keys else d_base
                        if plan.exr == "host":
                            if h_exr[slot] is None:
                                h_exr[slot] = {k: torch.empty(d_src_exr[k].shape, dtype=d_src_exr[k].dtype, pin_memory=True) for k in exr_keys}
                            for k, hbuf in h_exr[slot].items():
                                hbuf.copy_(d_src_exr[k], non_blocking=True)
                        else:
                            self.ctx.exr_encode(ow, oh, exr_channels(plan.exr_kinds, d_src_exr, exr_half), d_exr, d_exr_scratch, stream.cuda_stream,
                                                plan.exr == "device-lz77")
                            h_exr[slot].copy_(d_exr, non_blocking=True)
                    done = torch.cuda.Event()
                    done.record(stream)
                    for n, (jj, o, to_file, to_video) in enumerate(jpeg_work):
                        _, bpp, suffix = plan.jobs[jj]
                        if to_file:
                            path = os.path.join(output_folder, f"{base_name}_{frame:04d}_{suffix}.jpg")
                            pending[slot].append(write_pool.submit(write_jpeg, done, h_jpeg[slot][n].numpy(), bpp, o, path))
                        if to_video:
                            pending[slot].append(video_pool.submit(write_jpeg, done, h_jpeg[slot][n].numpy(), bpp, o, None))
                    if not images:
                        return
                    if plan.exr is not None:
                        pending[slot].append(write_pool.submit(write_exr, done, h_exr[slot], exr_named, os.path.join(output_folder, f"{base_name}_{frame:04d}.exr")))
                    for (_, bpp, suffix), hbuf in zip(plan.jobs, h_img[slot]):
                        path = os.path.join(output_folder, f"{base_name}_{frame:04d}_{suffix}.png")
                        if on_device:
                            pending[slot].append(write_pool.submit(write_encoded, done, hbuf.numpy(), bpp, path))
                        else:
                            pending[slot].append(write_pool.submit(write, done, hbuf.numpy().reshape(oh, ow, bpp), path))

                if itp is None:
                    for i, frame in enumerate(frames):
                        start, p, st = render(i, frame, d_film)
                        emit(i, frame, start, p, st)
                else:
                    # key B is rendered, then the frames between A and B are generated and written in ascending order, then B: the
                    # display state and every writer see the frames in time order.  Both keys' films and G-buffers are used in turn.
                    keys = [i for i in range(len(frames)) if itp.is_key(i, len(frames))]
                    slot_a, a = 0, None  # a: (entry, frame parameters) of key A
                    for n_key, ib in enumerate(keys):
                        slot_b = n_key % 2
                        start_b, p_b, st_b = render(ib, frames[ib], post.d_keys[slot_b])
                        post.key_gbuffer(slot_b, p_b, stream.cuda_stream)
                        if a is not None:
                            for ig in range(a[0] + 1, ib):
                                start, p = params_of(frames[ig])
                                if not (a[1].time_start <= p.time_start <= p_b.time_start):
                                    raise ValueError(f"interpolate= needs ascending frames: frame {frames[ig]} does not lie between its keys "
                                                     f"{frames[a[0]]} and {frames[ib]}")
                                d_gen = post.generate(p, slot_a, a[1], slot_b, p_b, stream.cuda_stream)
                                emit(ig, frames[ig], start, p, {"frame": frames[ig], "generated": True}, d_gen)
                        emit(ib, frames[ib], start_b, p_b, st_b, post.d_keys[slot_b])
                        slot_a, a = slot_b, (ib, p_b)
                wait_slot(0)
                wait_slot(1)
            return stats
        finally:
            # on success everything has been waited for already; on an error this joins the threads before it propagates
            write_pool.shutdown(wait=True, cancel_futures=True)
            video_pool.shutdown(wait=True, cancel_futures=True)
            table_pool.shutdown(wait=True, cancel_futures=True)
            if avi is not None:
                avi.close()  # also after an error: what was written plays
