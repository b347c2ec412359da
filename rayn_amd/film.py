"""Host-side mirror of rayn's `Film` (src/film.rs:175-378) on top of the C ABI.

    film = Film([ChannelKind.Color, ChannelKind.Alpha, ChannelKind.Background, ChannelKind.WorldNormal], (w, h))
    film.render_frame_into(world, camera, integrator, filter, tile_size, frame, time_range, samples)
    film.save_to([ChannelKind.Color], "renders", "64_spp", False)

`render_frame_into` has the reference's signature (src/film.rs:382-395).  Device memory, the stream
and (for N>1 ranks) the process group come from PyTorch; the arithmetic is all in librayn_hip.so.
"""
import ctypes as C
import dataclasses
import enum
import os

import numpy as np

from . import _abi, image
from . import progressive as _prog
from ._lib import RaynHipError, lib
from .params import frame_params
from .progressive import Progressive, progressive_seed  # noqa: F401


class ChannelKind(enum.Enum):  # src/film.rs:103-120
    Color = 0
    Alpha = 1
    Background = 2
    WorldNormal = 3


@dataclasses.dataclass(frozen=True)
class Denoise:
    """Parameters of the edge-avoiding a-trous denoiser of the Color channel (rayn_hip_denoise_device, an extension: rayn has no
    denoiser).  `iterations` a-trous passes (1..8, steps 1, 2, 4, ...); the sigmas weigh the squared colour (linear radiance), normal
    and alpha distances of a tap.  The colour sigma halves with every pass, the guides' stay fixed.  A sigma of 0 switches its term
    off; any other must be finite and in [2^-30, 2^30].

    The defaults were chosen on the shipped scene (rayn_amd.setup at 160x96, the MSE of the saturated Color + Background at 8 spp
    against 1024 spp, over a grid of the three sigmas): five passes, colour 0.5 (Dammertz's value, in linear radiance), normals 0.4
    and alpha 0.3.  They bring the MSE to 0.75x that of the noisy film; at that size the scene's fractal detail is pixel-sized, and
    a single pass (iterations=1, sigma_color=0, sigma_normal=0.7, sigma_alpha=0.3) does better, 0.50x."""
    iterations: int = 5
    sigma_color: float = 0.5
    sigma_normal: float = 0.4
    sigma_alpha: float = 0.3

    def __post_init__(self):
        if isinstance(self.iterations, bool) or not isinstance(self.iterations, (int, np.integer)) or not 1 <= self.iterations <= 8:
            raise ValueError(f"Denoise.iterations must be an int in 1..8, got {self.iterations!r}")
        for name in ("sigma_color", "sigma_normal", "sigma_alpha"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)):
                raise ValueError(f"Denoise.{name} must be a number, got {v!r}")
            f = float(v)  # the C entry takes it as an f32: check that value too
            if not (f == 0.0 or (2.0 ** -30 <= f <= 2.0 ** 30 and 2.0 ** -30 <= float(np.float32(f)) <= 2.0 ** 30)):
                raise ValueError(f"Denoise.{name} must be 0 (off) or finite in [2^-30, 2^30], got {v!r}")

    def without(self, have_mask):
        """These parameters with the terms of the guides the film lacks (bit k of have_mask = ChannelKind k) switched off."""
        return dataclasses.replace(self, sigma_normal=self.sigma_normal if have_mask & 8 else 0.0,
                                   sigma_alpha=self.sigma_alpha if have_mask & 2 else 0.0)


@dataclasses.dataclass(frozen=True)
class VarianceDenoise:
    """Parameters of the variance-guided a-trous denoiser of a progressive render's Color channel (rayn_hip_denoise_variance_device, an
    extension: rayn has neither a denoiser nor a progressive render; the spatial half of SVGF, Schied et al., HPG 2017).  `iterations`
    a-trous passes (1..8, steps 1, 2, 4, ...).  The luminance edge-stop of a tap is |l_p - l_q| / (sigma_luminance * sd_p), sd_p the
    local standard deviation of the pixel's mean luminance as the progressive state measured it (3x3 pre-filtered), so a pixel the
    render found noisy is smoothed widely and one it found converged is left alone; the variance is filtered along with the colour.
    sigma_normal and sigma_alpha weigh the squared normal and alpha distances as Denoise's do.  A sigma of 0 switches its term off; any
    other must be finite and in [2^-30, 2^30].

    The defaults were chosen on the shipped scene (rayn_amd.setup at 160x96; the MSE of the saturated Color + Background against 1024
    spp of a non-adaptive progressive render of 32 spp and of an adaptive one capped at 16 epochs) over a grid around SVGF's (5 passes,
    sigma 4) and Denoise's (0.4, 0.3): one pass, luminance 2, normals 0.4, alpha 0.3 bring the MSE to 0.75x / 0.86x that of the mean
    film where Denoise() raises it to 1.22x / 3.77x.  As for Denoise, the scene's fractal detail is pixel-sized at that size and every
    further pass blurs it: SVGF's five passes at sigma 4 give 1.49x / 2.27x (DESIGN.md section 8 has the grid)."""
    iterations: int = 1
    sigma_luminance: float = 2.0
    sigma_normal: float = 0.4
    sigma_alpha: float = 0.3

    def __post_init__(self):
        if isinstance(self.iterations, bool) or not isinstance(self.iterations, (int, np.integer)) or not 1 <= self.iterations <= 8:
            raise ValueError(f"VarianceDenoise.iterations must be an int in 1..8, got {self.iterations!r}")
        for name in ("sigma_luminance", "sigma_normal", "sigma_alpha"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)):
                raise ValueError(f"VarianceDenoise.{name} must be a number, got {v!r}")
            f = float(v)  # the C entry takes it as an f32: check that value too
            if not (f == 0.0 or (2.0 ** -30 <= f <= 2.0 ** 30 and 2.0 ** -30 <= float(np.float32(f)) <= 2.0 ** 30)):
                raise ValueError(f"VarianceDenoise.{name} must be 0 (off) or finite in [2^-30, 2^30], got {v!r}")

    def without(self, have_mask):
        """These parameters with the terms of the guides the film lacks (bit k of have_mask = ChannelKind k) switched off."""
        return dataclasses.replace(self, sigma_normal=self.sigma_normal if have_mask & 8 else 0.0,
                                   sigma_alpha=self.sigma_alpha if have_mask & 2 else 0.0)


@dataclasses.dataclass(frozen=True)
class Temporal:
    """Parameters of the temporal accumulation of a sequence's Color channel (rayn_hip_temporal_accumulate_device, an extension: rayn
    renders every frame on its own; the temporal half of SVGF, Schied et al., HPG 2017).  Every frame's accumulated Color is reprojected
    onto the next frame through the world position of each pixel's primary hit (rayn_hip_gbuffer_device) and blended with it, out = h +
    (c - h) / n, n the history length + 1 capped at `max_history` (1..65536; 1 = no accumulation).  A bilinear tap of the history counts
    when it shows the same object, its recorded hit distance is within `depth_tolerance` (relative; finite, >= 0) of the reprojected one
    and its normal has at least the dot product `normal_min` (in [-1, 1]; -1 switches the test off) with the pixel's.

    The defaults were chosen on the shipped scene (rayn_amd.setup at 160x96 under a camera whose origin moves, 8 frames of 8 spp; the MSE
    of the saturated Color + Background of the last frame against 1024 spp) over a grid of the three (tools/temporal_defaults.py; DESIGN.md
    section 8 has it): a history of 4, a depth tolerance of 5 % and the normal test off bring the MSE to 0.49x that of the raw frame.  The
    film's WorldNormal is the mean of a pixel's sample normals, far from unit length on the fractal, and a floor on its dot product throws
    away most of the history (0.81x at 0.5, 0.94x at 0.9); a longer history gains nothing over 8 frames (0.51x) and blurs more.

    `feedback` (finite, in [0, 1]; 0 = off, the default) is the strength of SVGF's feedback edge and needs a VarianceDenoise beside it in
    render_sequence: the output of the filter's first a-trous pass c' is blended into the history the next frame reprojects, c + feedback *
    (c' - c) (rayn_hip_denoise_temporal_variance_feedback_device).  It is not part of rayn_temporal_params: the strength travels as that
    entry's argument.  On the sequence above no strength above 0 lowered the error - 0.4675x at the best point (0.25, with
    VarianceDenoise(1, 2.0, 0.4, 0.3)) against 0.4571x without feedback (DESIGN.md section 8 has the grid) - so nothing is recommended.

    `resample` ("bilinear", the default, or "catmull_rom") is the filter that resamples the history at the reprojected position.
    "catmull_rom" (rayn_hip_temporal_accumulate_resample_device) reads the 4x4 footprint with Catmull-Rom weights wherever all 16 taps
    count, clamps the result to the range of the four inner taps, and is the bilinear filter everywhere else; it blurs less per
    reprojection.  Like feedback it is not part of rayn_temporal_params.  On the sequence above it did not lower the error - 0.4583x against
    0.4571x with VarianceDenoise(1, 4.0, 0.4, 0.3), 0.4994x against 0.4940x alone - and a max_history above 4 stayed worse under both filters
    (DESIGN.md section 8 has the grids), so nothing is recommended."""
    max_history: int = 4
    depth_tolerance: float = 0.05
    normal_min: float = -1.0
    feedback: float = 0.0
    resample: str = "bilinear"

    def __post_init__(self):
        if isinstance(self.max_history, bool) or not isinstance(self.max_history, (int, np.integer)) or not 1 <= self.max_history <= 65536:
            raise ValueError(f"Temporal.max_history must be an int in 1..65536, got {self.max_history!r}")
        for name in ("depth_tolerance", "normal_min", "feedback"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)):
                raise ValueError(f"Temporal.{name} must be a number, got {v!r}")
        with np.errstate(over="ignore"):
            d = float(np.float32(self.depth_tolerance))  # the C entry takes it as an f32: check that value too
        if not (np.isfinite(d) and d >= 0.0 and float(self.depth_tolerance) >= 0.0):
            raise ValueError(f"Temporal.depth_tolerance must be finite and >= 0, got {self.depth_tolerance!r}")
        if not -1.0 <= float(self.normal_min) <= 1.0:
            raise ValueError(f"Temporal.normal_min must be in [-1, 1], got {self.normal_min!r}")
        if not 0.0 <= float(self.feedback) <= 1.0:  # a NaN fails both
            raise ValueError(f"Temporal.feedback must be finite and in [0, 1], got {self.feedback!r}")
        if not isinstance(self.resample, str) or self.resample not in _abi.TEMPORAL_RESAMPLE:
            raise ValueError(f"Temporal.resample must be one of {sorted(_abi.TEMPORAL_RESAMPLE)}, got {self.resample!r}")

    def to_abi(self):
        return _abi.TemporalParams(int(self.max_history), float(self.depth_tolerance), float(self.normal_min))

    def resample_to_abi(self):
        return _abi.TemporalResampleParams(_abi.TEMPORAL_RESAMPLE[self.resample])


def _number(owner, name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)):
        raise ValueError(f"{owner}.{name} must be a number, got {v!r}")
    return float(v)


@dataclasses.dataclass(frozen=True)
class Bloom:
    """The bloom of a Display: the part of the exposed colour above `threshold` (finite, >= 0), blurred over a pyramid of `levels` (1..8)
    halvings and added back with weight `strength` (finite, >= 0) over the levels' mean."""
    threshold: float = 1.0
    strength: float = 0.5
    levels: int = 5

    def __post_init__(self):
        if isinstance(self.levels, bool) or not isinstance(self.levels, (int, np.integer)) or not 1 <= self.levels <= 8:
            raise ValueError(f"Bloom.levels must be an int in 1..8, got {self.levels!r}")
        for name in ("threshold", "strength"):
            f = _number("Bloom", name, getattr(self, name))
            with np.errstate(over="ignore"):
                ok = np.isfinite(f) and f >= 0.0 and np.isfinite(np.float32(f))  # the C entry takes it as an f32: check that value too
            if not ok:
                raise ValueError(f"Bloom.{name} must be finite and >= 0, got {getattr(self, name)!r}")


@dataclasses.dataclass(frozen=True)
class Display:
    """Parameters of the HDR display transform of the Color channel (rayn_hip_display_pixels_device, an extension: rayn's save_to clamps
    the film to [0, 1]; include/rayn_hip.h has the definition): exposure, optional bloom, a tone operator, then save_to's own gamma and
    8-bit quantisation.

    `exposure`: "auto" meters the film - the exposure scale is `key` (finite, > 0) over the geometric mean of the luminance - or a
    number, an EV: the scale is 2^EV (|EV| <= 100).  `tone`: "aces" (Narkowicz's fit), "reinhard" (extended Reinhard on luminance; a
    luminance of `white`, in [2^-30, 2^30], maps to 1) or "linear".  `bloom`: None or a Bloom.  `adaptation`: None, or the time constant in
    seconds (finite, > 0) with which render_sequence lets the metered value follow the frames, m += (m_now - m) * (1 - exp(-dt /
    adaptation)); a single image always takes its own metered value.

    Display(exposure=0.0, tone="linear") is the identity: the image is save_to's, byte for byte."""
    exposure: object = "auto"
    key: float = 0.18
    tone: str = "aces"
    white: float = 4.0
    bloom: object = None
    adaptation: object = None

    def __post_init__(self):
        if isinstance(self.exposure, str):
            if self.exposure != "auto":
                raise ValueError(f"Display.exposure must be 'auto' or an EV number, got {self.exposure!r}")
        elif not abs(_number("Display", "exposure", self.exposure)) <= 100.0:  # a NaN fails
            raise ValueError(f"Display.exposure must be 'auto' or a finite EV with |EV| <= 100, got {self.exposure!r}")
        k = _number("Display", "key", self.key)
        with np.errstate(over="ignore"):
            if not (np.isfinite(k) and k > 0.0 and np.isfinite(np.float32(k)) and np.float32(k) > 0.0):
                raise ValueError(f"Display.key must be finite and > 0, got {self.key!r}")
        if not isinstance(self.tone, str) or self.tone not in _abi.DISPLAY_TONE:
            raise ValueError(f"Display.tone must be one of {sorted(_abi.DISPLAY_TONE)}, got {self.tone!r}")
        if not 2.0 ** -30 <= _number("Display", "white", self.white) <= 2.0 ** 30:
            raise ValueError(f"Display.white must be finite in [2^-30, 2^30], got {self.white!r}")
        if self.bloom is not None and not isinstance(self.bloom, Bloom):
            raise ValueError(f"Display.bloom must be None or a Bloom, got {self.bloom!r}")
        if self.adaptation is not None:
            a = _number("Display", "adaptation", self.adaptation)
            if not (np.isfinite(a) and a > 0.0):
                raise ValueError(f"Display.adaptation must be None or finite and > 0 seconds, got {self.adaptation!r}")

    @property
    def auto(self):
        return isinstance(self.exposure, str)

    @property
    def levels(self):
        return 0 if self.bloom is None else int(self.bloom.levels)

    def adapt(self, dt):
        """The blend weight of a frame `dt` seconds after the one before it: 1 - exp(-|dt| / adaptation) rounded to f32; 1 without
        adaptation."""
        if self.adaptation is None:
            return 1.0
        return float(np.float32(1.0 - np.exp(-abs(float(dt)) / float(self.adaptation))))

    def to_abi(self, adapt=1.0):
        f32 = np.float32
        w = f32(self.white)
        b = self.bloom
        return _abi.DisplayParams(_abi.DISPLAY_TONE[self.tone], int(self.auto), 1.0 if self.auto else float(f32(2.0 ** float(self.exposure))),
                                  float(self.key), float(adapt), float(f32(1.0) / (w * w)), self.levels,
                                  0.0 if b is None else float(b.threshold), 0.0 if b is None else float(b.strength))


@dataclasses.dataclass(frozen=True)
class Upscale:
    """Parameters of the guided upscaling of a film (rayn_hip_upscale_device, an extension: rayn renders at one resolution; joint bilateral
    upsampling, Kopf et al., SIGGRAPH 2007; include/rayn_hip.h has the definition).  A film rendered at w x h is rebuilt at `factor` (1..8)
    times that size: every high pixel takes the four low pixels of its bilinear footprint that show the object its own primary hit shows
    (the G-buffer is traced at both resolutions, rayn_hip_gbuffer_device), weighted by the bilinear weight times exp(-(dpl / sigma_plane)^2
    - (dps / sigma_position)^2), dpl the distance of the pixel's hit point from the tap's tangent plane (the film's WorldNormal) and dps
    the distance between the two hit points, both relative to the pixel's hit distance.  Where no tap shows the object the plain bilinear
    weights are used.  The same weights serve every channel.  A sigma of 0 switches its term off; any other must be finite and in
    [2^-30, 2^30].  factor=1 is the identity.

    The defaults were chosen on the shipped scene (rayn_amd.setup at 160x96 and 32 spp upscaled to 320x192; the MSE of the saturated Color
    + Background against a native 1024 spp render) over a grid of the two sigmas (tools/upscale_defaults.py; DESIGN.md section 8 has it):
    the plane term off and a wide position term, 0.3.  That brings the MSE to 0.68x that of a native 320x192 render of the same number of
    paths (8 spp), where plain bilinear gives 0.74x, the object test alone 0.70x and the native render through Denoise() 0.67x.  On the
    fractal the film's WorldNormal is the mean of a pixel's sample normals and no tangent plane: every finite sigma_plane on the grid made
    the result worse (0.69x at 0.1, 0.86x at 0.005).  On the sphere scene s0, whose noise is low, the lost resolution dominates: the
    upscaled film has 4.4x the error of the native 8 spp render - 0.72x that of plain bilinear, whatever the sigmas."""
    factor: int = 2
    sigma_plane: float = 0.0
    sigma_position: float = 0.3

    def __post_init__(self):
        if isinstance(self.factor, bool) or not isinstance(self.factor, (int, np.integer)) or not 1 <= self.factor <= 8:
            raise ValueError(f"Upscale.factor must be an int in 1..8, got {self.factor!r}")
        for name in ("sigma_plane", "sigma_position"):
            f = _number("Upscale", name, getattr(self, name))  # the C entry takes it as an f32: check that value too
            if not (f == 0.0 or (2.0 ** -30 <= f <= 2.0 ** 30 and 2.0 ** -30 <= float(np.float32(f)) <= 2.0 ** 30)):
                raise ValueError(f"Upscale.{name} must be 0 (off) or finite in [2^-30, 2^30], got {getattr(self, name)!r}")

    def without(self, have_mask):
        """These parameters with the plane term switched off for a film without WorldNormal (bit k of have_mask = ChannelKind k)."""
        return dataclasses.replace(self, sigma_plane=self.sigma_plane if have_mask & 8 else 0.0)

    def to_abi(self):
        return _abi.UpscaleParams(int(self.factor), float(self.sigma_plane), float(self.sigma_position))


@dataclasses.dataclass(frozen=True)
class Supersample:
    """Parameters of the temporal supersampling of a sequence (rayn_hip_temporal_upscale_device, an extension; temporal upsampling as in
    TAAU / FSR2; include/rayn_hip.h has the definition): render_sequence with `upscale` AND `temporal` keeps the temporal history at the
    upscaled resolution and feeds it, frame after frame, with low frames whose cameras are offset by a fraction of a low pixel.

    `jitter`: frame i of a call renders through the frame's camera offset by offsets(factor)[i % factor^2] low pixels, so that over
    factor^2 frames every high pixel has had a low sample at its own centre; the kernel then finds every high pixel's footprint in the
    low film by projecting its primary hit through that offset camera.  False: every low frame samples the same lattice (offset (0, 0),
    no projection): the composition of Upscale and Temporal at the high size, bit for bit.

    `confidence`: a high pixel blends this frame's value into its history with the weight of the nearest low sample that gave it - 1
    when a low sample hit the pixel's centre, 0.25 in the middle of four - instead of 1 (the entry's conf; the history length grows by
    the same amount).  False: every frame counts fully, as in Temporal.

    The defaults are the best row of the measurement in DESIGN.md section 8 (tools/supersample_defaults.py: 8 frames at 160x96 and 32 spp
    rebuilt at 320x192, the last frame against 1024 spp, as ratios to a native 320x192 frame of the same number of paths): jitter on,
    confidence off.  On the shipped scene jitter alone brings Upscale(2)'s 0.68x to 0.60x under the moving camera and 0.66x to 0.58x
    under a static one (the composition without jitter: 0.66x and 0.61x).  Confidence did not lower the error overall - 0.62x and 0.58x
    on the shipped scene, 3.43x and 3.26x against 3.43x and 3.25x on the sphere scene s0 - so it is off by default.  Native Temporal() at
    320x192 with the same number of paths is better than every row (0.48x and 0.46x; on s0 0.72x and 0.77x against 3.25x - 3.43x): what
    supersampling buys is the render time of the low resolution, not a lower error than the full resolution at equal cost."""
    jitter: bool = True
    confidence: bool = False

    def __post_init__(self):
        for name in ("jitter", "confidence"):
            v = getattr(self, name)
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError(f"Supersample.{name} must be a bool, got {v!r}")

    @staticmethod
    def offsets(factor):
        """The factor^2 camera offsets (jx, jy) of one cycle, in LOW pixels: phase i visits the sub-cell (ix, iy) of a low pixel with
        k = i * (factor + 1) mod factor^2, ix = k mod factor, iy = k div factor - a walk along the diagonals that visits every cell once
        - and its offset is ((ix + 0.5) / factor - 0.5, (iy + 0.5) / factor - 0.5), the centre of that cell relative to the centre of
        the low pixel.  For factor >= 3 no two consecutive phases (the wrap from the last to the first included) share a row or a
        column; for factor 2 the walk is (0, 0), (1, 1), (0, 1), (1, 0): two of its steps are diagonal, which is all a 2 x 2 grid allows."""
        if isinstance(factor, bool) or not isinstance(factor, (int, np.integer)) or not 1 <= factor <= 8:
            raise ValueError(f"Supersample.offsets: factor must be an int in 1..8, got {factor!r}")
        s = int(factor)
        out = []
        for i in range(s * s):
            k = i * (s + 1) % (s * s)
            out.append(((k % s + 0.5) / s - 0.5, (k // s + 0.5) / s - 0.5))
        return out

    def offset(self, factor, i):
        """The offset of frame i of a call: offsets(factor)[i mod factor^2], and (0, 0) without jitter."""
        return self.offsets(factor)[int(i) % (int(factor) ** 2)] if self.jitter else (0.0, 0.0)

    def to_abi(self):
        return _abi.TemporalUpscaleParams(int(bool(self.confidence)))


def jittered_camera(camera, jx, jy, time_start):
    """A copy of the rayn_camera `camera` (an _abi.Camera) offset by (jx, jy) pixels of ITS resolution: the centre ray of its pixel
    (x, y) goes through what `camera` sees at the pixel coordinates (x + 0.5 + jx, y + 0.5 + jy).  With the basis u, v, w the camera has
    at time_start (closures evaluated there, the definition of rayn_hip_temporal_accumulate_device's step 3):
      orthographic:        origin and at both move by u * jx * full_w / res_w + v * jy * full_h / res_h - exact for every pixel;
      pinhole, thin lens:  at moves by (u * jx * 2 half_w / res_w + v * jy * 2 half_h / res_h) * |origin - at|, a small rotation about
                           the origin - exact at the image centre, and off by the perspective's second-order term elsewhere.
    The shift is added to the closures' base values, so a moving camera keeps its velocities.  Computed in float64 and rounded into the
    f32 fields: the temporal supersampling does not assume the shift, it projects through the camera it is given."""
    out = type(camera).from_buffer_copy(camera)
    ts = float(np.float32(time_start))

    def at_time(base, vel, bit):
        b = np.array([base.x, base.y, base.z], np.float64)
        return b + np.array([vel.x, vel.y, vel.z], np.float64) * ts if camera.animated & bit else b

    def unit(a):
        return a / np.sqrt(a @ a)

    o, at, up = at_time(camera.origin, camera.origin_vel, 1), at_time(camera.at, camera.at_vel, 2), at_time(camera.up, camera.up_vel, 4)
    aspect = float(camera.res_w) / float(camera.res_h)
    if camera.kind == _abi.CAM_ORTHOGRAPHIC:
        w = unit(at - o)
        u = unit(np.cross(w, up))
        v = np.cross(u, w)
        full_h = float(camera.vfov_or_size)
        shift = u * (jx * full_h * aspect / camera.res_w) + v * (jy * full_h / camera.res_h)
        moved = (out.origin, out.at)
    elif camera.kind in (_abi.CAM_PINHOLE, _abi.CAM_THIN_LENS):
        w = unit(o - at)
        u = unit(np.cross(up, w))
        v = np.cross(w, u)
        half_h = float(np.tan(np.radians(float(camera.vfov_or_size)) / 2.0))
        shift = (u * (jx * 2.0 * half_h * aspect / camera.res_w) + v * (jy * 2.0 * half_h / camera.res_h)) * np.sqrt((o - at) @ (o - at))
        moved = (out.at,)
    else:
        raise ValueError(f"unknown camera kind {camera.kind!r}")
    for vec in moved:
        vec.x, vec.y, vec.z = vec.x + shift[0], vec.y + shift[1], vec.z + shift[2]
    return out


def display_scratch_bytes(width, height, levels):
    """rayn_display_scratch_bytes: bytes of device scratch the display transform needs for a width x height film with `levels` bloom
    levels (0 for a size it rejects or levels > 8).  A manual exposure without bloom needs none."""
    return int(lib().rayn_display_scratch_bytes(int(width), int(height), int(levels)))


def gbuffer_scratch_bytes(width, height):
    """rayn_gbuffer_scratch_bytes: bytes of device scratch the G-buffer pass needs for a width x height film (0 for a size it rejects)."""
    return int(lib().rayn_gbuffer_scratch_bytes(int(width), int(height)))


def temporal_history_bytes(width, height):
    """rayn_temporal_history_bytes: bytes of one history of the temporal accumulation for a width x height film (0 for a size it rejects)."""
    return int(lib().rayn_temporal_history_bytes(int(width), int(height)))


def temporal_moments_bytes(width, height):
    """rayn_temporal_moments_bytes: bytes of the luminance moments beside one history (a float2 per pixel; 0 for a size the entries reject)."""
    return int(lib().rayn_temporal_moments_bytes(int(width), int(height)))


def alloc_gbuffer(width, height, device="cuda"):
    """The two planes of a G-buffer as Context.gbuffer fills them: records (n, 4) float32 (Px, Py, Pz, t) and object (n,) int32 (the u32
    object index; a miss is -1 = 0xFFFFFFFF)."""
    import torch
    n = width * height
    return {"records": torch.zeros(n, 4, dtype=torch.float32, device=device), "object": torch.zeros(n, dtype=torch.int32, device=device)}


def denoise_scratch_bytes(width, height):
    """rayn_denoise_scratch_bytes: bytes of device scratch the denoiser needs for a width x height film (0 for a size it rejects)."""
    return int(lib().rayn_denoise_scratch_bytes(int(width), int(height)))


def denoise_variance_scratch_bytes(width, height):
    """rayn_denoise_variance_scratch_bytes: bytes of device scratch the variance-guided denoiser needs for a width x height film (0 for a
    size it rejects)."""
    return int(lib().rayn_denoise_variance_scratch_bytes(int(width), int(height)))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def build_tables(spp, max_bounces, volume_marches, frame, width, height, filter=None):
    """Samples::new_rd (src/sampler.rs:18-37), per-pixel scramble (src/film.rs:460-461) and
    FilterImportanceSampler::new (src/filter.rs:196-220) through the product's host builders."""
    s1, s2 = build_rd_tables(spp, max_bounces, volume_marches, frame)
    scr, fis = build_film_tables(width, height, filter)
    return s1, s2, scr, fis


def build_rd_tables(spp, max_bounces, volume_marches, frame):
    """Samples::new_rd (src/sampler.rs:18-37): the only tables that depend on the frame."""
    L = lib()
    n1, n2 = L.rayn_sets_1d(max_bounces, volume_marches), L.rayn_sets_2d(max_bounces, volume_marches)
    s1, s2 = np.zeros(spp * n1, np.float32), np.zeros(spp * 2 * n2, np.float32)
    rc = L.rayn_build_rd_tables(spp, n1, n2, frame, _fp(s1), _fp(s2))
    if rc != 0:
        raise RaynHipError(f"table builder failed: {rc}")
    return s1, s2


def build_film_tables(width, height, filter=None):
    """The per-pixel scramble (src/film.rs:460-461) and FilterImportanceSampler::new (src/filter.rs:196-220)."""
    L = lib()
    kind, radius = (0, 1.5) if filter is None else (filter.kind, filter.radius)
    p0, p1 = getattr(filter, "params", (0.0, 0.0))
    scr, fis = np.zeros(width * height, np.float32), np.zeros(_abi.FIS_TABLE_SIZE, np.float32)
    for rc in (L.rayn_build_scramble(width, height, _fp(scr)), L.rayn_build_fis_table_ex(kind, radius, p0, p1, _fp(fis))):
        if rc != 0:
            raise RaynHipError(f"table builder failed: {rc}")
    return scr, fis


def share_pixels(params):
    """rayn_share_pixels: pixels of the tiles the share (params.tile_first, params.tile_step) owns; its packed film is 10 floats each."""
    return int(lib().rayn_share_pixels(C.byref(params)))


class Context:
    """One rayn_ctx (one GPU).  Fails loudly when the HIP library or a GPU is missing."""

    def __init__(self, device=0):
        """device: one GPU index, or a list of indices for a multi-device context (rayn_hip_create_multi; buffers passed
        to render_device then live on the first one)."""
        self._L = lib()
        h = C.c_void_p()
        if isinstance(device, (list, tuple)):
            ids = (C.c_int * len(device))(*device)
            rc = self._L.rayn_hip_create_multi(ids, len(device), C.byref(h))
            first = device[0] if len(device) else 0
        else:
            rc = self._L.rayn_hip_create(device, C.byref(h))
            first = device
        if rc != 0:
            raise RaynHipError(f"rayn_hip_create(device={device}) failed with {rc} (no usable GPU?)")
        self.h = h
        self.device = first
        self.fma_policy = int(self._L.rayn_hip_fma_policy())  # of this ctx: the library's default until set_fma_policy

    def device_count(self):
        return self._L.rayn_hip_device_count(self.h)

    def _chk(self, rc):
        if rc != 0:
            raise RaynHipError(f"rayn_hip error {rc}: {self._L.rayn_hip_last_error(self.h).decode()}")

    def table_broadcasts(self):
        """multi-device context: peer copies of the sample tables made so far (rayn_hip_table_broadcasts)"""
        return int(self._L.rayn_hip_table_broadcasts(self.h))

    def last_error(self):
        return self._L.rayn_hip_last_error(self.h).decode()

    def upload_world(self, desc):
        self._chk(self._L.rayn_hip_upload_world(self.h, C.byref(desc)))

    def set_profiling(self, timing=True, count_evals=False):
        self._chk(self._L.rayn_hip_set_profiling(self.h, int(timing), int(count_evals)))

    def set_fma_policy(self, policy):
        """0 = unfused mul_add (reference default build, the default), 1 = fused (rayn built with +fma)."""
        self._chk(self._L.rayn_hip_set_fma_policy(self.h, int(policy)))
        self.fma_policy = int(policy)

    def set_workers(self, n_workers, min_paths=1 << 22):
        self._chk(self._L.rayn_hip_set_workers(self.h, int(n_workers), int(min_paths)))

    def set_tile_subset(self, tiles=None):
        """Render only these tiles (reference tile order) until cleared with None / []."""
        arr = np.ascontiguousarray([] if tiles is None else tiles, dtype=np.uint32)
        self._chk(self._L.rayn_hip_set_tile_subset(self.h, arr.ctypes.data_as(C.POINTER(C.c_uint32)), len(arr)))

    def set_trace_tile(self, tile_index):
        self._chk(self._L.rayn_hip_set_trace_tile(self.h, int(tile_index)))

    def trace(self):
        """Packet-order dump of the traced tile: dict of uint32 arrays (depth, obj, px, py, sample, valid)."""
        n = self._L.rayn_hip_get_trace(self.h, None, 0)
        buf = np.zeros((max(n, 0), 6), np.uint32)
        if n > 0:
            self._L.rayn_hip_get_trace(self.h, buf.ctypes.data_as(C.POINTER(C.c_uint32)), n)
        return {k: buf[:, i].copy() for i, k in enumerate(("depth", "obj", "px", "py", "sample", "valid"))}

    def set_batch_paths(self, n):
        self._chk(self._L.rayn_hip_set_batch_paths(self.h, int(n)))

    def set_cold_bytes(self, n):
        """arena bytes of ALL workers together for the context's first frame (rayn_hip_set_cold_bytes, rayn_hip.h); 0 = full-size batches from the first frame"""
        self._chk(self._L.rayn_hip_set_cold_bytes(self.h, int(n)))

    def stats(self):
        s = _abi.Stats()
        self._chk(self._L.rayn_hip_get_stats(self.h, C.byref(s)))
        return s.as_dict()

    def entry_stats(self, entry):
        """What device `entry` of a multi-device context did in the last frame (rayn_hip_get_entry_stats)."""
        s = _abi.Stats()
        self._chk(self._L.rayn_hip_get_entry_stats(self.h, int(entry), C.byref(s)))
        return s.as_dict()

    def eval_counts(self):
        out = (C.c_uint64 * 3)()
        self._chk(self._L.rayn_hip_get_eval_counts(self.h, out))
        return {"extend": out[0], "shade_setup": out[1], "shadow": out[2]}

    def sdf_iterations(self):
        """Fold / orbit iterations run by the evaluations of eval_counts() (instrumented kernels, rayn_hip_get_sdf_iterations)."""
        out = (C.c_uint64 * 3)()
        self._chk(self._L.rayn_hip_get_sdf_iterations(self.h, out))
        return {"extend": out[0], "shade_setup": out[1], "shadow": out[2]}

    def elision_counts(self):
        """Instrumented kernels (rayn_hip_get_elision_counts): shaded slots with throughput exactly (0, 0, 0) whose NEE was elided, and the
        shadow segments they would have parked."""
        out = (C.c_uint64 * 3)()
        self._chk(self._L.rayn_hip_get_elision_counts(self.h, out))
        return {"zero_throughput_slots": out[0], "elided_shadow_jobs": out[1], "samples_out_of_bounds": out[2]}

    def stage_slots(self):
        """Instrumented Mandelbulb shadow-march kernel (rayn_hip_get_stage_slots): lane slots offered by the orbit / epilogue stage of k_shadow_bulb."""
        out = (C.c_uint64 * 2)()
        self._chk(self._L.rayn_hip_get_stage_slots(self.h, out))
        return {"shadow_orbit": out[0], "shadow_epilogue": out[1]}

    def render_host(self, params, tables, out=None):
        """rayn_hip_render_frame with host (numpy) buffers.  Returns the film dict."""
        s1, s2, scr, fis = tables
        n = params.width * params.height
        if out is None:
            out = {"color": np.zeros((n, 3), np.float32), "alpha": np.zeros(n, np.float32),
                   "background": np.zeros((n, 3), np.float32), "normal": np.zeros((n, 3), np.float32)}
        self._chk(self._L.rayn_hip_render_frame(self.h, C.byref(params), _fp(s1), _fp(s2), _fp(scr), _fp(fis), _fp(out["color"]),
                                                _fp(out["alpha"]), _fp(out["background"]), _fp(out["normal"])))
        h, w = params.height, params.width
        return {"color": out["color"].reshape(h, w, 3), "alpha": out["alpha"].reshape(h, w),
                "background": out["background"].reshape(h, w, 3), "normal": out["normal"].reshape(h, w, 3)}

    def probe_shade_limits(self):
        """(stream_blocks, list_ids_per_block, setup_threads): rayn_hip_probe_shade_limits."""
        v = [C.c_uint32() for _ in range(3)]
        self._chk(self._L.rayn_hip_probe_shade_limits(self.h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    RAYGEN_CTL = ("q_groups", "q_valid", "b_groups", "b_valid", "head_extend", "job_count", "head_shadow", "overflow")

    def probe_raygen(self, params, tables, tiles, n_pool, surplus=128, sentinel=0xC0FFEE5A, check=True):
        """rayn_hip_probe_raygen (rayn_hip.h): k_pack_tables, k_batch_setup and k_raygen on the caller's tables and the tile list `tiles` [n_tiles, 8] uint32.
        -> (rc, dict): geo0, geo1, col0, col1, aov [n_pool + surplus, 4] float32, term_key, term_info, q [n_pool + surplus], pgrp_tile [(n_pool + surplus) / 64],
        tgb, tgc [n_tiles + 2], ctl (dict of the eight words, RAYGEN_CTL), records [(max_bounces + 1) * spp, rec_stride * 4] float32 and records_surplus [64].
        Every array is handed over zeroed, so a refused call leaves zeros.  check=False returns a non-zero rc instead of raising."""
        s1, s2, scr, fis = [np.ascontiguousarray(t, np.float32) for t in tables]
        tiles = np.ascontiguousarray(tiles, np.uint32).reshape(-1, 8)
        n_tiles, NP = tiles.shape[0], n_pool + surplus
        out = {k: np.zeros((NP, 4), np.float32) for k in ("geo0", "geo1", "col0", "col1", "aov")}
        out["term_key"], out["term_info"], out["q"] = np.zeros(NP, np.uint32), np.zeros(NP, np.uint8), np.zeros(NP, np.uint32)
        out["pgrp_tile"], out["tgb"], out["tgc"] = np.zeros(max(NP // 64, 1), np.uint32), np.zeros(n_tiles + 2, np.uint32), np.zeros(n_tiles + 2, np.uint32)
        ctl = np.zeros(8, np.uint32)
        spp, stride = 4 * params.samples, 8 + 12 + 8 * params.volume_marches
        recs = np.zeros((params.max_bounces + 1) * spp * stride + 64, np.float32)
        up, bp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)))
        rc = self._L.rayn_hip_probe_raygen(self.h, C.byref(params), _fp(s1), s1.size, _fp(s2), s2.size, _fp(scr), scr.size, _fp(fis), n_tiles, up(tiles), n_pool, surplus,
                                           sentinel, *[_fp(out[k]) for k in ("geo0", "geo1", "col0", "col1", "aov")], up(out["term_key"]), bp(out["term_info"]),
                                           up(out["q"]), up(out["pgrp_tile"]), up(out["tgb"]), up(out["tgc"]), up(ctl), _fp(recs))
        if check:
            self._chk(rc)
        out["ctl"] = dict(zip(self.RAYGEN_CTL, ctl.tolist()))
        out["records"], out["records_surplus"] = recs[:-64].reshape(-1, stride), recs[-64:]
        return rc, out

    def probe_shade(self, params, tables, depth, ref, geo0, geo1, col0, col1, max_slots=None, nee_cap=None, sentinel=0xC0FFEE5A, check=True):
        """rayn_hip_probe_shade (rayn_hip.h): the shade stage of one depth on a binned queue `ref` [n_slots] and the pool records geo0 / geo1 / col0 / col1
        [n_pool, 4] float32 in the pool's own encoding.  -> (rc, dict): the pool as the stage left it (geo0, geo1, col0, col1, aov [n_pool, 4], term_key, term_info
        [n_pool]), alive_mask / bgrp_cnt [n_slots / 64], job_count, shadow_jobs, shadow_kernel.  check=False returns a non-zero rc instead of raising."""
        s1, s2, scr, fis = tables
        ref = np.ascontiguousarray(ref, np.uint32)
        recs = [np.ascontiguousarray(a, np.float32).reshape(-1, 4) for a in (geo0, geo1, col0, col1)]
        n_slots, n_pool = ref.size, recs[0].shape[0]
        assert all(a.shape[0] == n_pool for a in recs)
        out = {k: np.zeros((n_pool, 4), np.float32) for k in ("geo0", "geo1", "col0", "col1", "aov")}
        out["term_key"], out["term_info"] = np.zeros(n_pool, np.uint32), np.zeros(n_pool, np.uint8)
        groups = max(n_slots // 64, 1)
        out["alive_mask"], out["bgrp_cnt"] = np.zeros(groups, np.uint64), np.zeros(groups, np.uint8)
        jobs = np.zeros(3, np.uint64)
        up, bp, qp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64)))
        rc = self._L.rayn_hip_probe_shade(self.h, C.byref(params), _fp(s1), _fp(s2), _fp(scr), _fp(fis), depth, n_slots, n_slots if max_slots is None else max_slots,
                                          n_slots if nee_cap is None else nee_cap, up(ref), n_pool, *[_fp(a) for a in recs], sentinel,
                                          *[_fp(out[k]) for k in ("geo0", "geo1", "col0", "col1", "aov")], up(out["term_key"]), bp(out["term_info"]),
                                          qp(out["alive_mask"]), bp(out["bgrp_cnt"]), qp(jobs))
        if check:
            self._chk(rc)
        out["job_count"], out["shadow_jobs"], out["shadow_kernel"] = int(jobs[0]), int(jobs[1]), ("none", "k_shadow", "k_shadow1", "k_shadow_bulb")[int(jobs[2])]
        return rc, out

    def render_device(self, params, d_tables, d_out, stream=None):
        """rayn_hip_render_frame_device: d_tables/d_out are torch CUDA tensors (kept resident in HBM)."""
        import torch
        ptr = lambda t: C.c_void_p(t.data_ptr())
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        self._chk(self._L.rayn_hip_render_frame_device(self.h, C.byref(params), ptr(d_tables[0]), ptr(d_tables[1]), ptr(d_tables[2]),
                                                       ptr(d_tables[3]), ptr(d_out["color"]), ptr(d_out["alpha"]),
                                                       ptr(d_out["background"]), ptr(d_out["normal"]), C.c_void_p(s)))

    def render_packed(self, params, d_tables, d_packed, stream=None):
        """rayn_hip_render_frame_packed_device: the share (params.tile_first / tile_step) straight into its PACKED planar film
        `d_packed` (a float32 CUDA tensor of >= 10 * share_pixels(params) elements) - what a rank hands to the film gather."""
        import torch
        ptr = lambda t: C.c_void_p(t.data_ptr())
        assert d_packed.dtype == torch.float32 and d_packed.is_contiguous() and d_packed.numel() >= 10 * share_pixels(params)
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        self._chk(self._L.rayn_hip_render_frame_packed_device(self.h, C.byref(params), ptr(d_tables[0]), ptr(d_tables[1]), ptr(d_tables[2]),
                                                              ptr(d_tables[3]), ptr(d_packed), C.c_void_p(s)))

    def unpack_share(self, params, d_packed, d_out, stream=None):
        """rayn_hip_unpack_share_device: scatter the packed film of the share (params.tile_first / tile_step) into the full-resolution
        film `d_out` with one kernel launch on the stream (enqueued, not waited for)."""
        import torch
        ptr = lambda t: C.c_void_p(t.data_ptr())
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        self._chk(self._L.rayn_hip_unpack_share_device(self.h, C.byref(params), ptr(d_packed), ptr(d_out["color"]), ptr(d_out["alpha"]),
                                                       ptr(d_out["background"]), ptr(d_out["normal"]), C.c_void_p(s)))

    def save_to_pixels(self, kind, have_mask, transparent_background, width, height, d_film, d_out, stream=None):
        """rayn_hip_save_to_pixels_device: Film::save_to's post-process of channel `kind` (ChannelKind or its value) from the device film
        `d_film` (a dict of torch CUDA tensors as render_device fills them; channels the arm does not read may be absent) into the uint8
        CUDA tensor `d_out` (width * height * bpp bytes, rows top-down).  Enqueued on the stream, not waited for."""
        import torch
        kind = getattr(kind, "value", kind)
        bpp = save_to_bpp(kind, have_mask, transparent_background)
        n = int(width) * int(height)
        if not (d_out.dtype == torch.uint8 and d_out.is_contiguous() and d_out.numel() >= n * max(bpp, 0)):
            raise ValueError(f"d_out must be a contiguous uint8 tensor of at least {n * max(bpp, 0)} bytes")
        ptrs = []
        for key, floats in (("color", 3), ("alpha", 1), ("background", 3), ("normal", 3)):
            t = d_film.get(key)
            if t is None:
                ptrs.append(None)
                continue
            if not (t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= floats * n):
                raise ValueError(f"d_film[{key!r}] must be a contiguous float32 tensor of at least {floats * n} floats")
            ptrs.append(C.c_void_p(t.data_ptr()))
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        self._chk(self._L.rayn_hip_save_to_pixels_device(self.h, int(kind), int(have_mask), int(bool(transparent_background)), int(width), int(height),
                                                         *ptrs, C.c_void_p(d_out.data_ptr()), C.c_void_p(s)))

    def display_state(self):
        """A fresh state of the display transform's auto exposure: two zeroed 32-bit words {m, valid} on the context's GPU."""
        import torch
        return torch.zeros(2, dtype=torch.int32, device=f"cuda:{self.device}")

    def display(self, display, have_mask, transparent_background, width, height, d_film, d_out, d_state=None, d_scratch=None, adapt=1.0,
                d_out_meter=None, d_out_bloom=None, stream=None):
        """rayn_hip_display_pixels_device / rayn_hip_display_color_device: the HDR display transform (Display `display`) of the Color kind
        of the device film `d_film` (as save_to_pixels takes it).  A uint8 `d_out` (width * height * bpp bytes) receives the 8-bit image,
        rows top-down; a float32 one (width * height * 3 floats) the float plane before gamma and quantisation, in film order.  d_state
        (display_state(); auto exposure only) carries the metered value between calls, blended with weight `adapt`; None = a fresh one.
        d_scratch: a CUDA tensor of at least display_scratch_bytes(width, height, display.levels) bytes, allocated here when None and
        needed.  d_out_meter (2 floats: m, e) and d_out_bloom (width * height * 3 floats) are optional float32 outputs.  Enqueued on the
        stream, not waited for; the exposure never comes to the host."""
        import torch
        n = int(width) * int(height)
        bpp = save_to_bpp(0, have_mask, transparent_background)
        if d_out.dtype == torch.uint8:
            fn, need = self._L.rayn_hip_display_pixels_device, n * max(bpp, 0)
        elif d_out.dtype == torch.float32:
            fn, need = self._L.rayn_hip_display_color_device, 3 * n
        else:
            raise ValueError("d_out must be a uint8 tensor (the image) or a float32 tensor (the float plane)")
        if not (d_out.is_contiguous() and d_out.numel() >= need):
            raise ValueError(f"d_out must be contiguous and hold at least {need} elements")
        for name, t, floats in (("d_out_meter", d_out_meter, 2), ("d_out_bloom", d_out_bloom, 3 * n)):
            if t is not None and not (t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= floats):
                raise ValueError(f"{name} must be a contiguous float32 tensor of at least {floats} floats")
        ptrs = []
        for key, floats in (("color", 3), ("alpha", 1), ("background", 3)):
            t = d_film.get(key)
            if t is None:
                ptrs.append(None)
                continue
            if not (t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= floats * n):
                raise ValueError(f"d_film[{key!r}] must be a contiguous float32 tensor of at least {floats * n} floats")
            ptrs.append(C.c_void_p(t.data_ptr()))
        if display.auto and d_state is None:
            d_state = torch.zeros(2, dtype=torch.int32, device=d_out.device)
        if d_state is not None and not (d_state.dtype == torch.int32 and d_state.is_contiguous() and d_state.numel() >= 2):
            raise ValueError("d_state must be a contiguous int32 tensor of 2 elements (Context.display_state())")
        if d_scratch is None and (display.auto or display.levels):
            d_scratch = torch.empty(max(display_scratch_bytes(width, height, display.levels), 1), dtype=torch.uint8, device=d_out.device)
        if d_scratch is not None and not d_scratch.is_contiguous():
            raise ValueError("d_scratch must be contiguous")
        opt = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        dp = display.to_abi(adapt)
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        self._chk(fn(self.h, C.byref(dp), int(have_mask), int(bool(transparent_background)), int(width), int(height), *ptrs, opt(d_state),
                     opt(d_scratch), 0 if d_scratch is None else d_scratch.numel() * d_scratch.element_size(), C.c_void_p(d_out.data_ptr()),
                     opt(d_out_meter), opt(d_out_bloom), C.c_void_p(s)))

    def upscale(self, params, upscale, d_film, d_low_gbuffer, d_high_gbuffer, d_out_film, d_out_weight=None, stream=None):
        """rayn_hip_upscale_device: the guided upscaling (Upscale `upscale`) of the device film `d_film` of the frame `params` (its width
        and height are the LOW film's) into `d_out_film`, a film dict of upscale.factor times that size.  d_low_gbuffer / d_high_gbuffer:
        the G-buffers (alloc_gbuffer's dicts, as Context.gbuffer fills them) of the frame at the low and at the high resolution.  A plane
        (alpha, background, normal) the film lacks is absent from d_film and d_out_film together and is neither read nor written; "color"
        is required.  d_out_weight: a float32 CUDA tensor of one float per high pixel for the summed guided weight (0 where a fallback
        was taken), or None.  Enqueued on the stream, not waited for."""
        import torch
        s_ = int(upscale.factor)
        n = int(params.width) * int(params.height)
        N = n * s_ * s_
        ptrs = []
        for film, count, what in ((d_film, n, "d_film"), (d_out_film, N, "d_out_film")):
            for key, floats in (("color", 3), ("alpha", 1), ("background", 3), ("normal", 3)):
                t = film.get(key)
                if t is None:
                    ptrs.append(None)
                    continue
                if not (t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= floats * count):
                    raise ValueError(f"{what}[{key!r}] must be a contiguous float32 tensor of at least {floats * count} floats")
                ptrs.append(C.c_void_p(t.data_ptr()))
        gp = []
        for g, count, what in ((d_low_gbuffer, n, "d_low_gbuffer"), (d_high_gbuffer, N, "d_high_gbuffer")):
            rec, obj = g.get("records"), g.get("object")
            if rec is None or not (rec.dtype == torch.float32 and rec.is_contiguous() and rec.numel() >= 4 * count):
                raise ValueError(f"{what}['records'] must be a contiguous float32 tensor of at least {4 * count} floats")
            if obj is None or not (obj.dtype == torch.int32 and obj.is_contiguous() and obj.numel() >= count):
                raise ValueError(f"{what}['object'] must be a contiguous int32 tensor of at least {count} elements")
            gp += [C.c_void_p(rec.data_ptr()), C.c_void_p(obj.data_ptr())]
        if d_out_weight is not None and not (d_out_weight.dtype == torch.float32 and d_out_weight.is_contiguous() and d_out_weight.numel() >= N):
            raise ValueError(f"d_out_weight must be a contiguous float32 tensor of at least {N} floats")
        up = upscale.to_abi()
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        self._chk(self._L.rayn_hip_upscale_device(self.h, int(params.width), int(params.height), C.byref(up), *ptrs[:4], *gp, *ptrs[4:],
                                                  None if d_out_weight is None else C.c_void_p(d_out_weight.data_ptr()), C.c_void_p(s)))

    def temporal_upscale(self, params, upscale, temporal, supersample, d_film, d_low_gbuffer, d_high_gbuffer, d_prev_history, prev_camera,
                         prev_time_start, d_new_history, d_out_film, low_camera=None, d_out_weight=None, stream=None):
        """rayn_hip_temporal_upscale_device: the guided upscaling (Upscale `upscale`) of the low device film `d_film` of the frame `params`
        (its width and height are the LOW film's) fused with the temporal accumulation (Temporal `temporal`; its resample and feedback are
        not part of this entry) at upscale.factor times that size, by the Supersample `supersample`.  d_low_gbuffer / d_high_gbuffer: the
        frame's G-buffers at both resolutions, the low one traced through `low_camera` (an _abi.Camera: the camera the low film was
        rendered with, or None for the frame's own - the default footprint), the high one through the frame's own camera.
        d_prev_history / d_new_history: uint8 CUDA tensors of temporal_history_bytes at the HIGH size (d_prev_history None: no history),
        reprojected through prev_camera at prev_time_start.  d_out_film: a film dict of the high size; "color" receives the ACCUMULATED
        colour, "alpha" / "background" (absent together with d_film's) and "normal" this frame's upscaled planes.  "color" and "normal"
        are required on both sides.  d_out_weight: a float32 CUDA tensor of one float per high pixel, or None.  Enqueued on the stream, not
        waited for."""
        import torch
        s_ = int(upscale.factor)
        n = int(params.width) * int(params.height)
        N = n * s_ * s_
        ptrs = []
        for film, count, what in ((d_film, n, "d_film"), (d_out_film, N, "d_out_film")):
            for key, floats in (("color", 3), ("alpha", 1), ("background", 3), ("normal", 3)):
                t = film.get(key)
                if t is None:
                    ptrs.append(None)
                    continue
                if not (t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= floats * count):
                    raise ValueError(f"{what}[{key!r}] must be a contiguous float32 tensor of at least {floats * count} floats")
                ptrs.append(C.c_void_p(t.data_ptr()))
        gp = []
        for g, count, what in ((d_low_gbuffer, n, "d_low_gbuffer"), (d_high_gbuffer, N, "d_high_gbuffer")):
            rec, obj = g.get("records"), g.get("object")
            if rec is None or not (rec.dtype == torch.float32 and rec.is_contiguous() and rec.numel() >= 4 * count):
                raise ValueError(f"{what}['records'] must be a contiguous float32 tensor of at least {4 * count} floats")
            if obj is None or not (obj.dtype == torch.int32 and obj.is_contiguous() and obj.numel() >= count):
                raise ValueError(f"{what}['object'] must be a contiguous int32 tensor of at least {count} elements")
            gp += [C.c_void_p(rec.data_ptr()), C.c_void_p(obj.data_ptr())]
        if d_out_weight is not None and not (d_out_weight.dtype == torch.float32 and d_out_weight.is_contiguous() and d_out_weight.numel() >= N):
            raise ValueError(f"d_out_weight must be a contiguous float32 tensor of at least {N} floats")
        for name, t in (("d_prev_history", d_prev_history), ("d_new_history", d_new_history)):
            if t is not None and not (t.dtype == torch.uint8 and t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous uint8 tensor")
        if d_new_history is None:
            raise ValueError("d_new_history must be a contiguous uint8 tensor")
        nbytes = d_new_history.numel() if d_prev_history is None else min(d_new_history.numel(), d_prev_history.numel())
        up, tp, sp = upscale.to_abi(), temporal.to_abi(), supersample.to_abi()
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        self._chk(self._L.rayn_hip_temporal_upscale_device(
            self.h, C.byref(params), C.byref(up), C.byref(tp), C.byref(sp), None if low_camera is None else C.byref(low_camera),
            None if prev_camera is None else C.byref(prev_camera), float(prev_time_start), *ptrs[:4], *gp,
            None if d_prev_history is None else C.c_void_p(d_prev_history.data_ptr()), C.c_void_p(d_new_history.data_ptr()), nbytes,
            *ptrs[4:], None if d_out_weight is None else C.c_void_p(d_out_weight.data_ptr()), C.c_void_p(s)))

    def denoise(self, width, height, d_film, d_out_color, params, d_scratch=None, stream=None):
        """rayn_hip_denoise_device: the a-trous denoiser (Denoise `params`) of d_film["color"] into the float32 CUDA tensor d_out_color
        (width * height * 3 floats), guided by d_film["normal"] and d_film["alpha"] (a guide whose sigma is 0 may be absent).
        d_scratch: a CUDA tensor of at least denoise_scratch_bytes(width, height) bytes, allocated here when None.  Enqueued on the
        stream, not waited for."""
        import torch
        n = int(width) * int(height)
        if not (d_out_color.dtype == torch.float32 and d_out_color.is_contiguous() and d_out_color.numel() >= 3 * n):
            raise ValueError(f"d_out_color must be a contiguous float32 tensor of at least {3 * n} floats")
        ptrs = []
        for key, floats in (("color", 3), ("alpha", 1), ("normal", 3)):
            t = d_film.get(key)
            if t is None:
                ptrs.append(None)
                continue
            if not (t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= floats * n):
                raise ValueError(f"d_film[{key!r}] must be a contiguous float32 tensor of at least {floats * n} floats")
            ptrs.append(C.c_void_p(t.data_ptr()))
        if d_scratch is None:
            d_scratch = torch.empty(max(denoise_scratch_bytes(width, height), 1), dtype=torch.uint8, device=d_out_color.device)
        if not d_scratch.is_contiguous():
            raise ValueError("d_scratch must be contiguous")
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        self._chk(self._L.rayn_hip_denoise_device(self.h, int(width), int(height), int(params.iterations), float(params.sigma_color),
                                                  float(params.sigma_normal), float(params.sigma_alpha), *ptrs,
                                                  C.c_void_p(d_out_color.data_ptr()), C.c_void_p(d_scratch.data_ptr()),
                                                  d_scratch.numel() * d_scratch.element_size(), C.c_void_p(s)))

    def denoise_variance(self, params, d_film, d_state, d_out_color, denoise, d_out_variance=None, d_scratch=None, stream=None):
        """rayn_hip_denoise_variance_device: the variance-guided a-trous denoiser (VarianceDenoise `denoise`) of the mean film
        d_film["color"] of a progressive render into the float32 CUDA tensor d_out_color (width * height * 3 floats), guided by
        d_film["normal"] and d_film["alpha"] (a guide whose sigma is 0 may be absent) and by the render's state `d_state` with the film
        geometry of `params` (as progressive_accumulate takes them).  d_out_variance: a float32 CUDA tensor of width * height floats for
        the filtered variance, or None.  d_scratch: a CUDA tensor of at least denoise_variance_scratch_bytes(width, height) bytes,
        allocated here when None.  Enqueued on the stream, not waited for."""
        import torch
        width, height = params.width, params.height
        n = int(width) * int(height)
        if not (d_out_color.dtype == torch.float32 and d_out_color.is_contiguous() and d_out_color.numel() >= 3 * n):
            raise ValueError(f"d_out_color must be a contiguous float32 tensor of at least {3 * n} floats")
        if d_out_variance is not None and not (d_out_variance.dtype == torch.float32 and d_out_variance.is_contiguous() and d_out_variance.numel() >= n):
            raise ValueError(f"d_out_variance must be a contiguous float32 tensor of at least {n} floats")
        ptrs = []
        for key, floats in (("color", 3), ("alpha", 1), ("normal", 3)):
            t = d_film.get(key)
            if t is None:
                ptrs.append(None)
                continue
            if not (t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= floats * n):
                raise ValueError(f"d_film[{key!r}] must be a contiguous float32 tensor of at least {floats * n} floats")
            ptrs.append(C.c_void_p(t.data_ptr()))
        state_ptr, state_bytes = self._prog_state(params, d_state)
        if d_scratch is None:
            d_scratch = torch.empty(max(denoise_variance_scratch_bytes(width, height), 1), dtype=torch.uint8, device=d_out_color.device)
        if not d_scratch.is_contiguous():
            raise ValueError("d_scratch must be contiguous")
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        self._chk(self._L.rayn_hip_denoise_variance_device(self.h, C.byref(params), int(denoise.iterations), float(denoise.sigma_luminance),
                                                           float(denoise.sigma_normal), float(denoise.sigma_alpha), *ptrs, state_ptr, state_bytes,
                                                           C.c_void_p(d_out_color.data_ptr()),
                                                           None if d_out_variance is None else C.c_void_p(d_out_variance.data_ptr()),
                                                           C.c_void_p(d_scratch.data_ptr()), d_scratch.numel() * d_scratch.element_size(),
                                                           C.c_void_p(s)))

    def gbuffer(self, params, d_gbuffer, d_scratch=None, stream=None):
        """rayn_hip_gbuffer_device: the primary-hit G-buffer of the uploaded world under `params` (resolution, time_start, march constants)
        into d_gbuffer (alloc_gbuffer's dict: "records" (n, 4) float32 = (Px, Py, Pz, t), "object" (n,) int32).  d_scratch: a CUDA tensor
        of at least gbuffer_scratch_bytes(width, height) bytes, allocated here when None.  Enqueued on the stream, not waited for."""
        import torch
        n = int(params.width) * int(params.height)
        rec, obj = d_gbuffer["records"], d_gbuffer["object"]
        if not (rec.dtype == torch.float32 and rec.is_contiguous() and rec.numel() >= 4 * n):
            raise ValueError(f"d_gbuffer['records'] must be a contiguous float32 tensor of at least {4 * n} floats")
        if not (obj.dtype == torch.int32 and obj.is_contiguous() and obj.numel() >= n):
            raise ValueError(f"d_gbuffer['object'] must be a contiguous int32 tensor of at least {n} elements")
        if d_scratch is None:
            d_scratch = torch.empty(max(gbuffer_scratch_bytes(params.width, params.height), 1), dtype=torch.uint8, device=rec.device)
        if not d_scratch.is_contiguous():
            raise ValueError("d_scratch must be contiguous")
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        self._chk(self._L.rayn_hip_gbuffer_device(self.h, C.byref(params), C.c_void_p(rec.data_ptr()), C.c_void_p(obj.data_ptr()),
                                                  C.c_void_p(d_scratch.data_ptr()), d_scratch.numel() * d_scratch.element_size(), C.c_void_p(s)))

    def temporal_accumulate(self, params, temporal, d_film, d_gbuffer, d_prev_history, prev_camera, prev_time_start, d_new_history, d_out_color,
                            stream=None, d_prev_moments=None, d_new_moments=None):
        """rayn_hip_temporal_accumulate_device: blend d_film["color"] (guides: d_film["normal"], the G-buffer d_gbuffer of the same frame)
        with the previous frame's history d_prev_history (a uint8 CUDA tensor of temporal_history_bytes, or None: no history) reprojected
        through prev_camera (an _abi.Camera) at prev_time_start, by the Temporal `temporal`.  Writes the accumulated colour to the float32
        CUDA tensor d_out_color (width * height * 3 floats) and the new history to d_new_history.  Enqueued on the stream, not waited for.

        With d_new_moments (a uint8 CUDA tensor of temporal_moments_bytes; d_prev_moments beside d_prev_history, None with it) the call
        goes through rayn_hip_temporal_accumulate_moments_device, which also carries the first and second moment of the luminance through
        the same reprojection - what denoise_temporal_variance reads; colour and history are the same bits.  Both None: the plain entry.

        temporal.resample == "bilinear" calls these two entries; "catmull_rom" goes through rayn_hip_temporal_accumulate_resample_device
        instead, with or without moments, under the same rules."""
        import torch
        n = int(params.width) * int(params.height)
        for key, t, floats in (("color", d_film.get("color"), 3), ("normal", d_film.get("normal"), 3), ("records", d_gbuffer.get("records"), 4)):
            if t is None or not (t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= floats * n):
                raise ValueError(f"{key!r} must be a contiguous float32 tensor of at least {floats * n} floats")
        obj = d_gbuffer.get("object")
        if obj is None or not (obj.dtype == torch.int32 and obj.is_contiguous() and obj.numel() >= n):
            raise ValueError(f"d_gbuffer['object'] must be a contiguous int32 tensor of at least {n} elements")
        if not (d_out_color.dtype == torch.float32 and d_out_color.is_contiguous() and d_out_color.numel() >= 3 * n):
            raise ValueError(f"d_out_color must be a contiguous float32 tensor of at least {3 * n} floats")
        for name, t in (("d_prev_history", d_prev_history), ("d_new_history", d_new_history)):
            if t is not None and not (t.dtype == torch.uint8 and t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous uint8 tensor")
        if d_new_history is None:
            raise ValueError("d_new_history must be a contiguous uint8 tensor")
        nbytes = d_new_history.numel() if d_prev_history is None else min(d_new_history.numel(), d_prev_history.numel())
        tp = temporal.to_abi()
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        mbytes = 0
        if d_prev_moments is not None or d_new_moments is not None:
            for name, t in (("d_prev_moments", d_prev_moments), ("d_new_moments", d_new_moments)):
                if t is not None and not (t.dtype == torch.uint8 and t.is_contiguous()):
                    raise ValueError(f"{name} must be a contiguous uint8 tensor")
            if d_new_moments is None:
                raise ValueError("d_new_moments must be a contiguous uint8 tensor")
            mbytes = d_new_moments.numel() if d_prev_moments is None else min(d_new_moments.numel(), d_prev_moments.numel())
        if temporal.resample != "bilinear":
            rp = temporal.resample_to_abi()
            self._chk(self._L.rayn_hip_temporal_accumulate_resample_device(
                self.h, C.byref(params), C.byref(tp), C.byref(rp), None if prev_camera is None else C.byref(prev_camera), float(prev_time_start),
                C.c_void_p(d_film["color"].data_ptr()), C.c_void_p(d_film["normal"].data_ptr()), C.c_void_p(d_gbuffer["records"].data_ptr()),
                C.c_void_p(obj.data_ptr()), None if d_prev_history is None else C.c_void_p(d_prev_history.data_ptr()),
                C.c_void_p(d_new_history.data_ptr()), nbytes, None if d_prev_moments is None else C.c_void_p(d_prev_moments.data_ptr()),
                None if d_new_moments is None else C.c_void_p(d_new_moments.data_ptr()), mbytes, C.c_void_p(d_out_color.data_ptr()), C.c_void_p(s)))
            return
        if d_prev_moments is not None or d_new_moments is not None:
            self._chk(self._L.rayn_hip_temporal_accumulate_moments_device(
                self.h, C.byref(params), C.byref(tp), None if prev_camera is None else C.byref(prev_camera), float(prev_time_start),
                C.c_void_p(d_film["color"].data_ptr()), C.c_void_p(d_film["normal"].data_ptr()), C.c_void_p(d_gbuffer["records"].data_ptr()),
                C.c_void_p(obj.data_ptr()), None if d_prev_history is None else C.c_void_p(d_prev_history.data_ptr()),
                C.c_void_p(d_new_history.data_ptr()), nbytes, None if d_prev_moments is None else C.c_void_p(d_prev_moments.data_ptr()),
                C.c_void_p(d_new_moments.data_ptr()), mbytes, C.c_void_p(d_out_color.data_ptr()), C.c_void_p(s)))
            return
        self._chk(self._L.rayn_hip_temporal_accumulate_device(
            self.h, C.byref(params), C.byref(tp), None if prev_camera is None else C.byref(prev_camera), float(prev_time_start),
            C.c_void_p(d_film["color"].data_ptr()), C.c_void_p(d_film["normal"].data_ptr()), C.c_void_p(d_gbuffer["records"].data_ptr()),
            C.c_void_p(obj.data_ptr()), None if d_prev_history is None else C.c_void_p(d_prev_history.data_ptr()),
            C.c_void_p(d_new_history.data_ptr()), nbytes, C.c_void_p(d_out_color.data_ptr()), C.c_void_p(s)))

    def denoise_temporal_variance(self, width, height, d_film, d_gbuffer, d_history, d_moments, d_out_color, denoise, d_out_variance=None,
                                  d_scratch=None, stream=None, feedback=0.0):
        """rayn_hip_denoise_temporal_variance_device: the variance-guided a-trous denoiser (VarianceDenoise `denoise`) of a temporally
        accumulated colour.  d_film["color"] is the ACCUMULATED colour (what temporal_accumulate wrote to d_out_color), d_film["normal"] /
        d_film["alpha"] the film's guides (a guide whose sigma is 0 may be absent), d_gbuffer the frame's G-buffer (its "object" plane is
        read), d_history / d_moments the NEW history and moments of that accumulate.  A pixel's variance comes from its moments once its
        history is 4 frames long, (m2 - m1^2) / n, and from the 7x7 neighbourhood of the accumulated luminance on the same object before
        that - so with Temporal(max_history < 4) only the spatial estimate is ever used.  Writes the float32 CUDA tensor d_out_color
        (width * height * 3 floats) and, when given, d_out_variance (width * height floats; NaN where there was no estimate).  d_scratch: a
        CUDA tensor of at least denoise_variance_scratch_bytes(width, height) bytes, allocated here when None.  Enqueued on the stream,
        not waited for.  Recommended for sequences: VarianceDenoise(1, 4.0, 0.4, 0.3), 0.46x the raw frame where Temporal() alone gives 0.49x.

        feedback (finite, in [0, 1]): 0 takes the entry above and leaves d_history alone.  Anything else goes through
        rayn_hip_denoise_temporal_variance_feedback_device: d_out_color and d_out_variance are the same bits, and the colour of d_history
        becomes c + feedback * (c' - c), c' the output of the first a-trous pass, wherever that pass had an estimate; the history lengths,
        the other planes of the history and the moments are not written."""
        import torch
        feedback = float(feedback)
        if not 0.0 <= feedback <= 1.0:
            raise ValueError(f"feedback must be finite and in [0, 1], got {feedback!r}")
        n = int(width) * int(height)
        if not (d_out_color.dtype == torch.float32 and d_out_color.is_contiguous() and d_out_color.numel() >= 3 * n):
            raise ValueError(f"d_out_color must be a contiguous float32 tensor of at least {3 * n} floats")
        if d_out_variance is not None and not (d_out_variance.dtype == torch.float32 and d_out_variance.is_contiguous() and d_out_variance.numel() >= n):
            raise ValueError(f"d_out_variance must be a contiguous float32 tensor of at least {n} floats")
        ptrs = []
        for key, floats in (("color", 3), ("alpha", 1), ("normal", 3)):
            t = d_film.get(key)
            if t is None:
                ptrs.append(None)
                continue
            if not (t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= floats * n):
                raise ValueError(f"d_film[{key!r}] must be a contiguous float32 tensor of at least {floats * n} floats")
            ptrs.append(C.c_void_p(t.data_ptr()))
        obj = d_gbuffer.get("object")
        if obj is None or not (obj.dtype == torch.int32 and obj.is_contiguous() and obj.numel() >= n):
            raise ValueError(f"d_gbuffer['object'] must be a contiguous int32 tensor of at least {n} elements")
        for name, t in (("d_history", d_history), ("d_moments", d_moments)):
            if t is None or not (t.dtype == torch.uint8 and t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous uint8 tensor")
        if d_scratch is None:
            d_scratch = torch.empty(max(denoise_variance_scratch_bytes(width, height), 1), dtype=torch.uint8, device=d_out_color.device)
        if not d_scratch.is_contiguous():
            raise ValueError("d_scratch must be contiguous")
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        args = (self.h, int(width), int(height), int(denoise.iterations), float(denoise.sigma_luminance), float(denoise.sigma_normal),
                float(denoise.sigma_alpha), *ptrs, C.c_void_p(obj.data_ptr()), C.c_void_p(d_history.data_ptr()), d_history.numel(),
                C.c_void_p(d_moments.data_ptr()), d_moments.numel(), C.c_void_p(d_out_color.data_ptr()),
                None if d_out_variance is None else C.c_void_p(d_out_variance.data_ptr()), C.c_void_p(d_scratch.data_ptr()),
                d_scratch.numel() * d_scratch.element_size())
        if feedback == 0.0:
            self._chk(self._L.rayn_hip_denoise_temporal_variance_device(*args, C.c_void_p(s)))
        else:
            self._chk(self._L.rayn_hip_denoise_temporal_variance_feedback_device(*args, feedback, C.c_void_p(s)))

    @staticmethod
    def _prog_state(params, d_state):
        import torch
        need = _prog.state_bytes(params.width, params.height, (params.tile_w, params.tile_h))
        if not (d_state.dtype == torch.uint8 and d_state.is_contiguous()):
            raise ValueError("d_state must be a contiguous uint8 tensor")
        if need and d_state.numel() < need:
            raise ValueError(f"d_state must hold at least {need} bytes")
        return C.c_void_p(d_state.data_ptr()), d_state.numel()

    def progressive_reset(self, params, d_state, stream=None):
        """rayn_hip_progressive_reset_device: a fresh progressive state for the film geometry of `params` in the uint8 CUDA tensor
        `d_state` (at least rayn_amd.progressive.state_bytes).  Enqueued on the stream, not waited for."""
        import torch
        ptr, nbytes = self._prog_state(params, d_state)
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        self._chk(self._L.rayn_hip_progressive_reset_device(self.h, C.byref(params), ptr, nbytes, C.c_void_p(s)))

    def progressive_accumulate(self, params, progressive, tiles, d_epoch, d_state, d_mean, stream=None):
        """rayn_hip_progressive_accumulate_device: accumulate the epoch film `d_epoch` (a dict of torch CUDA tensors as render_device
        fills them) into the tiles `tiles` (ascending indices; None = every tile) of `d_state`, write those tiles' mean film to `d_mean`,
        retire tiles by the Progressive `progressive` and compact the active list.  Enqueued on the stream, not waited for."""
        import torch
        n = params.width * params.height
        ptrs = []
        for film in (d_epoch, d_mean):
            for key, floats in (("color", 3), ("alpha", 1), ("background", 3), ("normal", 3)):
                t = film.get(key)
                if t is None or not (t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= floats * n):
                    raise ValueError(f"film[{key!r}] must be a contiguous float32 tensor of at least {floats * n} floats")
                ptrs.append(C.c_void_p(t.data_ptr()))
        ptr, nbytes = self._prog_state(params, d_state)
        arr, n_tiles = None, 0
        if tiles is not None:
            arr = np.ascontiguousarray(tiles, dtype=np.uint32)
            n_tiles = len(arr)
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        pp = progressive.to_abi()
        self._chk(self._L.rayn_hip_progressive_accumulate_device(self.h, C.byref(params), C.byref(pp),
                                                                 None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_uint32)), n_tiles,
                                                                 *ptrs[:4], ptr, nbytes, *ptrs[4:], C.c_void_p(s)))

    def progressive_fetch_active(self, params, d_state, stream=None):
        """rayn_hip_progressive_fetch_active (blocking): (the ascending list of the tiles not retired as a uint32 array, totals dict)."""
        import torch
        ptr, nbytes = self._prog_state(params, d_state)
        cap = int(self._L.rayn_tile_count(params.width, params.height, params.tile_w, params.tile_h))
        out = np.zeros(max(cap, 1), np.uint32)
        tot = _abi.ProgressiveTotals()
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        n = self._L.rayn_hip_progressive_fetch_active(self.h, C.byref(params), ptr, nbytes, out.ctypes.data_as(C.POINTER(C.c_uint32)), cap,
                                                      C.byref(tot), C.c_void_p(s))
        if n < 0:
            self._chk(int(n))
        return out[:n].copy(), {"active_tiles": int(tot.active_tiles), "max_e": float(tot.max_e), "outlier_pixels": int(tot.outlier_pixels)}

    def progressive_tile_report(self, params, d_state, stream=None):
        """rayn_hip_progressive_tile_report (blocking): dict of per-tile arrays epochs, retired, outliers (uint32) and max_e (float32)."""
        import torch
        ptr, nbytes = self._prog_state(params, d_state)
        t = max(int(self._L.rayn_tile_count(params.width, params.height, params.tile_w, params.tile_h)), 1)
        rep = {"epochs": np.zeros(t, np.uint32), "retired": np.zeros(t, np.uint32), "outliers": np.zeros(t, np.uint32), "max_e": np.zeros(t, np.float32)}
        up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        self._chk(self._L.rayn_hip_progressive_tile_report(self.h, C.byref(params), ptr, nbytes, up(rep["epochs"]), up(rep["retired"]),
                                                           up(rep["outliers"]), _fp(rep["max_e"]), C.c_void_p(s)))
        return rep

    def close(self):
        if self.h:
            self._L.rayn_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def save_to_bpp(kind, have_mask, transparent_background=False):
    """rayn_save_to_bpp: bytes per pixel of the image Film::save_to writes for channel `kind` given the film's channels (bit k of
    have_mask = ChannelKind k), or -1 where the reference returns Err.  Host only."""
    return int(lib().rayn_save_to_bpp(int(getattr(kind, "value", kind)), int(have_mask), int(bool(transparent_background))))


def alloc_device_film(width, height, device="cuda"):
    import torch
    n = width * height
    return {"color": torch.zeros(n, 3, dtype=torch.float32, device=device), "alpha": torch.zeros(n, dtype=torch.float32, device=device),
            "background": torch.zeros(n, 3, dtype=torch.float32, device=device), "normal": torch.zeros(n, 3, dtype=torch.float32, device=device)}


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

    def render_frame_into(self, world, camera, integrator, filter, tile_size, frame, time_range, samples, tile_first=0, tile_step=1):
        """Film::render_frame_into (src/film.rs:382-628); the film is overwritten, not accumulated (:91)."""
        import torch
        w, h = self.res
        p = frame_params(w, h, samples, integrator.max_bounces, integrator.volume_marches, frame, time_range, tile_size, tile_first, tile_step)
        self.ctx.upload_world(world.to_desc(camera))
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
        key = {ChannelKind.Color: "color", ChannelKind.Alpha: "alpha", ChannelKind.Background: "background", ChannelKind.WorldNormal: "normal"}[kind]
        w, h = self.res
        t = self.channels[key].cpu().numpy()
        return t.reshape(h, w, 3) if t.ndim == 2 else t.reshape(h, w)

    def gbuffer(self):
        """The primary-hit G-buffer of the last rendered frame (rayn_hip_gbuffer_device, an extension): one centre ray per pixel at the
        frame's time_start through the product closest-hit kernel.  Returns {"position": float32 (h, w, 3), "t": float32 (h, w; +inf for
        a miss), "object": uint32 (h, w; 0xFFFFFFFF for a miss)}, rows bottom-up like the film."""
        import torch
        if self._last_params is None:
            raise ValueError("the film holds no rendered frame (render_frame_into, render_sequence or render_progressive has not run)")
        w, h = self.res
        with torch.cuda.device(self.device):
            g = alloc_gbuffer(w, h, self.device)
            self.ctx.gbuffer(self._last_params, g)
            rec = g["records"].cpu().numpy().reshape(h, w, 4)
            obj = g["object"].cpu().numpy().view(np.uint32).reshape(h, w)
        return {"position": rec[..., :3].copy(), "t": rec[..., 3].copy(), "object": obj}

    def _upscale_plan(self, upscale):
        """(`upscale` with the plane term off for a film without WorldNormal, the keys of the planes this film holds); ValueError for
        anything that is no Upscale and for a film without Color."""
        if not isinstance(upscale, Upscale):
            raise ValueError(f"upscale must be an Upscale, got {upscale!r}")
        if ChannelKind.Color not in self.channel_kinds:
            raise ValueError("Attempted to upscale a film without a Color channel")
        return upscale.without(self.have_mask()), [_CHANNEL_KEY[k] for k in ChannelKind if k in self.channel_kinds]

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

    def have_mask(self):
        """bit k = ChannelKind k is among the film's channels (the have_mask of rayn_save_to_bpp)"""
        return sum(1 << k.value for k in self.channel_kinds)

    def _save_jobs(self, write_channels, transparent_background):
        """[(kind, bytes per pixel, file suffix)] of a save_to call; raises the reference's Err text as ValueError before anything runs."""
        jobs = []
        for kind in write_channels:
            bpp = save_to_bpp(kind, self.have_mask(), transparent_background)
            if bpp < 0:
                raise ValueError(_SAVE_TO_ERR[kind])
            jobs.append((kind, bpp, _SAVE_TO_SUFFIX[kind]))
        return jobs

    def _denoise_params(self, denoise):
        """`denoise` with the terms of the guides this film lacks switched off; a film without Color raises ValueError."""
        if ChannelKind.Color not in self.channel_kinds:
            raise ValueError("Attempted to denoise the Color channel but it didn't exist")
        return denoise.without(self.have_mask())

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

    def _denoise_variance(self, params, want_variance):
        import torch
        params = self._denoise_params(params)
        pr = self._variance_state()
        w, h = self.res
        with torch.cuda.device(self.device):
            out = torch.empty(w * h, 3, dtype=torch.float32, device=self.device)
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
        params = self._denoise_params(params)
        w, h = self.res
        with torch.cuda.device(self.device):
            out = torch.empty(w * h, 3, dtype=torch.float32, device=self.device)
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
        if not isinstance(display, Display):
            raise ValueError(f"display must be a Display, got {display!r}")
        self._save_jobs([ChannelKind.Color], transparent_background)
        w, h = self.res
        with torch.cuda.device(self.device):
            film = self.channels
            if denoise is not None:
                film = dict(film, color=self.denoised_color(denoise))
            out = torch.empty(w * h, 3, dtype=torch.float32, device=self.device)
            self.ctx.display(display, self.have_mask(), transparent_background, w, h, film, out, display_state, None, adapt)
            return out

    def pixels(self, kind, transparent_background=False, denoise=None, display=None, display_state=None, adapt=1.0):
        """The 8-bit image Film::save_to writes for channel `kind` (rows top-down; (h, w, 4 / 3 / 1) uint8), computed on the device
        (rayn_hip_save_to_pixels_device); only the 8-bit image is copied back.  Channels the film lacks are not read.  With `denoise`
        (a Denoise or a VarianceDenoise), the Color image is made from denoised_color(denoise); the other channels are unchanged.
        With `display` (a Display, an extension), the Color image goes through the HDR display transform (after the denoiser, if any;
        rayn_hip_display_pixels_device) with display_state and adapt as Context.display takes them; the other channels ignore it."""
        import torch
        ((kind, bpp, _),) = self._save_jobs([kind], transparent_background)
        if display is not None and not isinstance(display, Display):
            raise ValueError(f"display must be a Display, got {display!r}")
        w, h = self.res
        with torch.cuda.device(self.device):
            film = self.channels
            if denoise is not None and kind == ChannelKind.Color:
                film = dict(film, color=self.denoised_color(denoise))
            out = torch.empty(h * w * bpp, dtype=torch.uint8, device=self.device)
            if display is not None and kind == ChannelKind.Color:
                self.ctx.display(display, self.have_mask(), transparent_background, w, h, film, out, display_state, None, adapt)
            else:
                self.ctx.save_to_pixels(kind, self.have_mask(), transparent_background, w, h, film, out)
            return out.cpu().numpy().reshape(h, w, bpp)  # .cpu() waits for the current stream, where the kernels were enqueued

    def save_to(self, write_channels, output_folder, base_name, transparent_background=False, denoise=None, display=None):
        """Film::save_to (src/film.rs:205-378) - the post-process after the hot path, arm by arm (on the device: pixels); the
        reference's Err(String) cases raise ValueError with the same text.  The PNGs are those of rayn_amd.image (host reference).
        With `denoise` (a Denoise or a VarianceDenoise, extensions), the Color image is made from the denoised Color and written as
        {base_name}_color_denoised.png instead of {base_name}_color.png; the other channels are unchanged.  With `display` (a Display, an
        extension) the Color image goes through the HDR display transform and its file name gets _display appended:
        {base_name}_color_display.png, {base_name}_color_denoised_display.png."""
        os.makedirs(output_folder, exist_ok=True)
        for kind in write_channels:
            ((kind, _, suffix),) = self._save_jobs([kind], transparent_background)  # the reference fails at the first bad channel, after writing the ones before
            if denoise is not None and kind == ChannelKind.Color:
                suffix = "color_denoised"
            if display is not None and kind == ChannelKind.Color:
                suffix += "_display"
            image.save(os.path.join(output_folder, f"{base_name}_{suffix}.png"), self.pixels(kind, transparent_background, denoise, display))

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
                    next_rd = table_pool.submit(build_rd_tables, spp, mb, vm, progressive_seed(frame, first, mb, vm))
                    scr, fis = build_film_tables(w, h, filter)
                    d_tables, d_epoch = None, alloc_device_film(w, h, self.device)
                    report["epoch_film"] = d_epoch
                epoch = first
                while epoch < progressive.max_epochs and len(active):
                    seed = progressive_seed(frame, epoch, mb, vm)
                    s1, s2 = next_rd.result()
                    if d_tables is None:
                        d_tables = [torch.from_numpy(t).to(self.device) for t in (s1, s2, scr, fis)]
                    else:
                        d_tables[0].copy_(torch.from_numpy(s1))  # synchronous copies from pageable memory: the previous render has returned
                        d_tables[1].copy_(torch.from_numpy(s2))
                    if epoch + 1 < progressive.max_epochs:
                        next_rd = table_pool.submit(build_rd_tables, spp, mb, vm, progressive_seed(frame, epoch + 1, mb, vm))
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
                        output_folder, base_name, transparent_background=False, writers=None, denoise=None, display=None, upscale=None, supersample=None, temporal=None):
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
        unchanged."""
        import concurrent.futures as cf
        import torch
        variance = isinstance(denoise, VarianceDenoise)
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
        if upscale is not None:
            if temporal is not None and supersample is None:
                raise ValueError("temporal= together with upscale= is not built: the temporal histories live at one resolution")
            upscale, up_keys = self._upscale_plan(upscale)
        frames = [int(f) for f in frames]
        jobs = self._save_jobs(write_channels, transparent_background)
        if denoise is not None:
            if variance:  # its guides are required, not switched off: checked with the temporal arguments below
                self._denoise_params(denoise)
                denoise = denoise if ChannelKind.Color in write_channels else None
            else:
                denoise = self._denoise_params(denoise) if ChannelKind.Color in write_channels else None
            jobs = [(kind, bpp, "color_denoised" if denoise is not None and kind == ChannelKind.Color else suffix) for kind, bpp, suffix in jobs]
        if temporal is not None:
            if not isinstance(temporal, Temporal):
                raise ValueError(f"temporal must be a Temporal, got {temporal!r}")
            if ChannelKind.Color not in self.channel_kinds or ChannelKind.WorldNormal not in self.channel_kinds:
                raise ValueError("temporal accumulation needs the film's Color and WorldNormal channels")
            if variance and denoise is not None and float(denoise.sigma_alpha) != 0.0 and ChannelKind.Alpha not in self.channel_kinds:
                raise ValueError("variance-guided denoising of a temporal sequence needs the film's Alpha channel when sigma_alpha != 0")
            if ChannelKind.Color not in write_channels:
                temporal = supersample = None  # nothing shows the accumulated colour: the plain path (upscale= alone with supersample=)
            else:
                jobs = [(kind, bpp, ("color_temporal" if denoise is None else "color_temporal_denoised") if kind == ChannelKind.Color else suffix)
                        for kind, bpp, suffix in jobs]
        if display is not None:
            if not isinstance(display, Display):
                raise ValueError(f"display must be a Display, got {display!r}")
            if ChannelKind.Color not in write_channels:
                display = None
            else:
                jobs = [(kind, bpp, suffix + "_display" if kind == ChannelKind.Color else suffix) for kind, bpp, suffix in jobs]
        if upscale is not None:
            jobs = [(kind, bpp, f"{suffix}_x{upscale.factor}") for kind, bpp, suffix in jobs]
        os.makedirs(output_folder, exist_ok=True)
        w, h = self.res
        ow, oh = (w, h) if upscale is None else (w * upscale.factor, h * upscale.factor)  # the size of the written images
        f32 = np.float32
        inv_rate, shutter = f32(1.0) / f32(frame_rate), f32(shutter_speed)
        spp, mb, vm = 4 * samples, integrator.max_bounces, integrator.volume_marches
        n_writers = max(1, min(8, 2 * len(jobs) if writers is None else int(writers)))
        mask = self.have_mask()
        stats, pending = [], [[], []]  # pending[slot]: writer futures still reading that slot's pinned images
        table_pool = cf.ThreadPoolExecutor(max_workers=1, thread_name_prefix="rayn-rd-tables")
        write_pool = cf.ThreadPoolExecutor(max_workers=n_writers, thread_name_prefix="rayn-png")

        def write(event, img, path):
            event.synchronize()
            image.save(path, img)

        def wait_slot(slot):
            for fut in pending[slot]:
                fut.result()  # re-raises a writer's exception
            pending[slot] = []

        try:
            if not frames:
                return stats
            with torch.cuda.device(self.device):
                stream = torch.cuda.current_stream()
                desc = world.to_desc(camera)
                self.ctx.upload_world(desc)
                next_rd = table_pool.submit(build_rd_tables, spp, mb, vm, frames[0])
                scr, fis = build_film_tables(w, h, filter)
                s1, s2 = next_rd.result()
                d_tables = [torch.from_numpy(t).to(self.device) for t in (s1, s2, scr, fis)]
                d_film = alloc_device_film(w, h, self.device)
                d_img = [torch.empty(oh * ow * bpp, dtype=torch.uint8, device=self.device) for _, bpp, _ in jobs]
                if denoise is not None:
                    d_denoised = torch.empty(ow * oh, 3, dtype=torch.float32, device=self.device)
                    d_scratch = torch.empty((denoise_variance_scratch_bytes if variance else denoise_scratch_bytes)(ow, oh), dtype=torch.uint8, device=self.device)
                if upscale is not None:
                    d_glow, d_ghigh = alloc_gbuffer(w, h, self.device), alloc_gbuffer(ow, oh, self.device)
                    d_uscratch = torch.empty(gbuffer_scratch_bytes(ow, oh), dtype=torch.uint8, device=self.device)  # serves both passes
                    d_up_full = alloc_device_film(ow, oh, self.device)
                    d_up = {k: d_up_full[k] for k in up_keys}
                    d_low = {k: d_film[k] for k in up_keys}
                d_mom = [None, None]
                if temporal is not None and variance and denoise is not None:
                    d_mom = [torch.empty(temporal_moments_bytes(w, h), dtype=torch.uint8, device=self.device) for _ in range(2)]
                if supersample is not None:  # the histories live at the high size; the G-buffers are the upscale's
                    d_hist = [torch.empty(temporal_history_bytes(ow, oh), dtype=torch.uint8, device=self.device) for _ in range(2)]
                    prev_start = None
                    desc_low = type(desc).from_buffer_copy(desc)  # the world as the low frame is rendered: the camera is set per frame
                elif temporal is not None:
                    d_gbuf = alloc_gbuffer(w, h, self.device)
                    d_gscratch = torch.empty(gbuffer_scratch_bytes(w, h), dtype=torch.uint8, device=self.device)
                    d_hist = [torch.empty(temporal_history_bytes(w, h), dtype=torch.uint8, device=self.device) for _ in range(2)]
                    d_accum = torch.empty(w * h, 3, dtype=torch.float32, device=self.device)
                    prev_start = None
                if display is not None:
                    d_dstate = self.ctx.display_state() if display.auto else None
                    d_dscratch = (torch.empty(display_scratch_bytes(ow, oh, display.levels), dtype=torch.uint8, device=self.device)
                                  if display.auto or display.levels else None)
                    shown_start = None  # the start of the frame the state last metered
                h_img = [[torch.empty(oh * ow * bpp, dtype=torch.uint8, pin_memory=True) for _, bpp, _ in jobs] for _ in range(2)]
                for i, frame in enumerate(frames):
                    if i:
                        s1, s2 = next_rd.result()
                        d_tables[0].copy_(torch.from_numpy(s1))  # synchronous copies from pageable memory: the previous render has returned
                        d_tables[1].copy_(torch.from_numpy(s2))
                    if i + 1 < len(frames):
                        next_rd = table_pool.submit(build_rd_tables, spp, mb, vm, frames[i + 1])
                    for fut in pending[0] + pending[1]:
                        if fut.done() and fut.exception() is not None:
                            raise fut.exception()
                    start = f32(frame) * inv_rate
                    p = frame_params(w, h, samples, mb, vm, frame, (float(start), float(f32(start + shutter))), tile_size)
                    low_cam = None
                    if supersample is not None and supersample.jitter:
                        low_cam = jittered_camera(desc.camera, *supersample.offset(upscale.factor, i), p.time_start)
                        desc_low.camera = low_cam
                        self.ctx.upload_world(desc_low)
                    self.ctx.render_device(p, d_tables, d_film, stream.cuda_stream)  # blocking: returns when the frame is complete
                    st = self.ctx.stats()
                    st["frame"] = frame
                    stats.append(st)
                    self.channels = d_film
                    self._last_params = p
                    self.progressive_epoch += 1
                    # Frame k's post-process and copies go on the render stream, so frame k + 1's render (enqueued on the same stream
                    # after them) cannot overwrite d_film or d_img before they have been read; only the pinned slot needs a host-side
                    # wait: its images from frame k - 2 must have been encoded.
                    slot = i % 2
                    wait_slot(slot)
                    d_base = d_film  # what the images are made from
                    if upscale is not None:
                        self.ctx.gbuffer(p, d_glow, d_uscratch, stream.cuda_stream)
                        if low_cam is not None:
                            self.ctx.upload_world(desc)  # the high G-buffer and the history belong to the frame's own camera
                        self.ctx.gbuffer(_scaled_params(p, upscale.factor), d_ghigh, d_uscratch, stream.cuda_stream)
                        if supersample is not None:
                            self.ctx.temporal_upscale(p, upscale, temporal, supersample, d_low, d_glow, d_ghigh,
                                                      None if prev_start is None else d_hist[(i + 1) % 2], None if prev_start is None else desc.camera,
                                                      0.0 if prev_start is None else prev_start, d_hist[i % 2], d_up, low_cam, None, stream.cuda_stream)
                            prev_start = p.time_start
                        else:
                            self.ctx.upscale(p, upscale, d_low, d_glow, d_ghigh, d_up, None, stream.cuda_stream)
                        d_base = d_up
                    d_shown = d_base  # what the Color image is made from
                    if temporal is not None and supersample is None:
                        self.ctx.gbuffer(p, d_gbuf, d_gscratch, stream.cuda_stream)
                        self.ctx.temporal_accumulate(p, temporal, d_film, d_gbuf, None if prev_start is None else d_hist[(i + 1) % 2],
                                                     None if prev_start is None else desc.camera, 0.0 if prev_start is None else prev_start,
                                                     d_hist[i % 2], d_accum, stream.cuda_stream,
                                                     None if prev_start is None else d_mom[(i + 1) % 2], d_mom[i % 2])
                        prev_start = p.time_start
                        d_shown = dict(d_film, color=d_accum)
                    if denoise is not None:
                        if variance:
                            self.ctx.denoise_temporal_variance(w, h, d_shown, d_gbuf, d_hist[i % 2], d_mom[i % 2], d_denoised, denoise, None, d_scratch,
                                                               stream.cuda_stream, float(temporal.feedback))
                        else:
                            self.ctx.denoise(ow, oh, d_shown, d_denoised, denoise, d_scratch, stream.cuda_stream)
                        d_shown = dict(d_base, color=d_denoised)
                    for (kind, _, suffix), d, hbuf in zip(jobs, d_img, h_img[slot]):
                        src = d_shown if kind == ChannelKind.Color else d_base
                        if display is not None and kind == ChannelKind.Color:
                            adapt = 1.0 if shown_start is None else display.adapt(float(start) - float(shown_start))
                            self.ctx.display(display, mask, transparent_background, ow, oh, src, d, d_dstate, d_dscratch, adapt, stream=stream.cuda_stream)
                            shown_start = start
                        else:
                            self.ctx.save_to_pixels(kind, mask, transparent_background, ow, oh, src, d, stream.cuda_stream)
                        hbuf.copy_(d, non_blocking=True)
                    done = torch.cuda.Event()
                    done.record(stream)
                    for (kind, bpp, suffix), hbuf in zip(jobs, h_img[slot]):
                        path = os.path.join(output_folder, f"{base_name}_{frame:04d}_{suffix}.png")
                        pending[slot].append(write_pool.submit(write, done, hbuf.numpy().reshape(oh, ow, bpp), path))
                wait_slot(0)
                wait_slot(1)
            return stats
        finally:
            # on success everything has been waited for already; on an error this joins the threads before it propagates
            write_pool.shutdown(wait=True, cancel_futures=True)
            table_pool.shutdown(wait=True, cancel_futures=True)


def _scaled_params(p, factor):
    """A copy of the frame parameters p with the resolution multiplied by factor: the frame of an upscaled film."""
    ph = type(p).from_buffer_copy(p)
    ph.width, ph.height = int(p.width) * int(factor), int(p.height) * int(factor)
    return ph


_CHANNEL_KEY = {ChannelKind.Color: "color", ChannelKind.Alpha: "alpha", ChannelKind.Background: "background", ChannelKind.WorldNormal: "normal"}
_SAVE_TO_SUFFIX = {ChannelKind.Color: "color", ChannelKind.Alpha: "alpha", ChannelKind.Background: "background", ChannelKind.WorldNormal: "normal"}
_SAVE_TO_ERR = {ChannelKind.Color: "Attempted to write Color channel with insufficient channels",  # src/film.rs:283-287
                ChannelKind.Alpha: "Attempted to write Alpha channel but it didn't exist",  # :341-345
                ChannelKind.Background: "Attempted to write Background channel but it didn't exist",  # :292-296
                ChannelKind.WorldNormal: "Attempted to write WorldNormal channel but it didn't exist"}  # :316-320
