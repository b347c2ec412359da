"""The option dataclasses of the extensions (denoisers, temporal accumulation, display transform, upscaling, supersampling, preview), ChannelKind
and the camera jitter: host-side values only, validated where they are made.  rayn_amd.film re-exports every name."""
import dataclasses
import enum

import numpy as np

from . import _abi


class ChannelKind(enum.Enum):  # src/film.rs:103-120
    Color = 0
    Alpha = 1
    Background = 2
    WorldNormal = 3


def _int_in(owner, name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f"{owner}.{name} must be an int in {lo}..{hi}, got {v!r}")


def _number(owner, name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)):
        raise ValueError(f"{owner}.{name} must be a number, got {v!r}")
    return float(v)


def _sigma(owner, name, v):
    f = _number(owner, name, v)  # the C entry takes it as an f32: check that value too
    if not (f == 0.0 or (2.0 ** -30 <= f <= 2.0 ** 30 and 2.0 ** -30 <= float(np.float32(f)) <= 2.0 ** 30)):
        raise ValueError(f"{owner}.{name} must be 0 (off) or finite in [2^-30, 2^30], got {v!r}")


def _without_guides(self, have_mask):
    """These parameters with the terms of the guides the film lacks (bit k of have_mask = ChannelKind k) switched off."""
    return dataclasses.replace(self, sigma_normal=self.sigma_normal if have_mask & 8 else 0.0,
                               sigma_alpha=self.sigma_alpha if have_mask & 2 else 0.0)


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
        _int_in("Denoise", "iterations", self.iterations, 1, 8)
        for name in ("sigma_color", "sigma_normal", "sigma_alpha"):
            _sigma("Denoise", name, getattr(self, name))

    without = _without_guides


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
        _int_in("VarianceDenoise", "iterations", self.iterations, 1, 8)
        for name in ("sigma_luminance", "sigma_normal", "sigma_alpha"):
            _sigma("VarianceDenoise", name, getattr(self, name))

    without = _without_guides


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
        _int_in("Temporal", "max_history", self.max_history, 1, 65536)
        for name in ("depth_tolerance", "normal_min", "feedback"):
            _number("Temporal", name, getattr(self, name))
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


@dataclasses.dataclass(frozen=True)
class Bloom:
    """The bloom of a Display: the part of the exposed colour above `threshold` (finite, >= 0), blurred over a pyramid of `levels` (1..8)
    halvings and added back with weight `strength` (finite, >= 0) over the levels' mean."""
    threshold: float = 1.0
    strength: float = 0.5
    levels: int = 5

    def __post_init__(self):
        _int_in("Bloom", "levels", self.levels, 1, 8)
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
        _int_in("Upscale", "factor", self.factor, 1, 8)
        for name in ("sigma_plane", "sigma_position"):
            _sigma("Upscale", name, getattr(self, name))

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


@dataclasses.dataclass(frozen=True)
class Preview:
    """Parameters of the preview integrator (rayn_hip_preview_device, an extension: rayn has one integrator, the path tracer;
    include/rayn_hip.h has the definition): an image of the geometry alone - the primary hit of every pixel's centre ray, its normal turned
    towards the viewer and the ambient occlusion of `samples` (1..64) cosine-weighted rays of length `radius` (world units; finite, > 0),
    ao = the visible fraction.  The colour is ao * (ambient + (1 - ambient) * max(0, n . wo)) in all three channels - a headlight whose
    view-independent part is `ambient` (in [0, 1]; 1 leaves the AO alone) - alpha is 1 on a surface and 0 on the sky or a miss.  No
    material, light or volume is looked at.

    The default radius was chosen on the shipped scene (rayn_amd.setup at 160x96, 16 rays per pixel, the numpy restatement on the CPU:
    tools/preview_defaults.py) among the radii 0.025 * 2^k: the variance of the ao over the fractal's pixels - the contrast between its
    cavities and its open faces - grows with the radius up to 0.8 and is flat from 0.4 on (0.1113 at 0.2, 0.1161 at 0.4, 0.1173 at 0.8,
    0.1099 at 1.6), and a longer ray costs more march steps, so the default is the smallest radius within 2 % of the largest variance:
    0.4 (DESIGN.md section 8 has the table).  It is a look, not a tolerance."""
    samples: int = 8
    radius: float = 0.4
    ambient: float = 0.3

    def __post_init__(self):
        _int_in("Preview", "samples", self.samples, 1, 64)
        r, a = _number("Preview", "radius", self.radius), _number("Preview", "ambient", self.ambient)
        with np.errstate(over="ignore"):
            r32 = float(np.float32(r))  # the C entry takes it as an f32: check that value too
        if not (np.isfinite(r) and r > 0.0 and np.isfinite(r32) and r32 > 0.0):
            raise ValueError(f"Preview.radius must be finite and > 0, got {self.radius!r}")
        if not 0.0 <= a <= 1.0:  # a NaN fails both
            raise ValueError(f"Preview.ambient must be in [0, 1], got {self.ambient!r}")

    def to_abi(self):
        return _abi.PreviewParams(int(self.samples), float(self.radius), float(self.ambient))


@dataclasses.dataclass(frozen=True)
class Interpolate:
    """Parameters of the frame generation of a sequence (rayn_hip_interpolate_device, an extension: rayn renders every frame;
    include/rayn_hip.h has the definition): render_sequence renders every `every`-th frame (2..16) of its list - and the last - as a key
    and generates the frames between two keys from them.  A generated frame traces its own primary-hit G-buffer, projects every pixel's
    hit into both keys and blends, by time, the taps there that show the same object at the projected depth: a tap's recorded hit distance
    may differ from the projected one by `depth_tolerance` (relative; finite, >= 0).  A point one key alone sees is taken from that key; one
    that neither sees is a cross-fade of the keys' own pixels.

    The tolerance was chosen on the shipped scene (rayn_amd.setup at 160x96 under a camera drift of 2 pixels a frame, keys at 8 spp, every
    generated frame of every = 2 and 4 scored against 1024 spp; tools/interpolate_defaults.py, DESIGN.md section 8 has the grid): the error
    falls as the tolerance grows, from 0.76x / 1.03x the rendered 8-spp frame's at Temporal's 5 % to 0.67x / 0.90x at 25 %, and only to 0.61x
    / 0.88x with the depth test as good as off (100 %) - on the fractal, whose depth changes by more than 5 % from one pixel to the next, a
    tight test throws away taps of the right surface.  25 % keeps the test that guards self-occlusion and scale_vel morphing."""
    every: int = 2
    depth_tolerance: float = 0.25

    def __post_init__(self):
        _int_in("Interpolate", "every", self.every, 2, 16)
        _number("Interpolate", "depth_tolerance", self.depth_tolerance)
        with np.errstate(over="ignore"):
            d = float(np.float32(self.depth_tolerance))  # the C entry takes it as an f32: check that value too
        if not (np.isfinite(d) and d >= 0.0 and float(self.depth_tolerance) >= 0.0):
            raise ValueError(f"Interpolate.depth_tolerance must be finite and >= 0, got {self.depth_tolerance!r}")

    def is_key(self, i, n):
        """Is entry i of a list of n frames a key: i a multiple of `every`, or the last entry."""
        return i % int(self.every) == 0 or i == n - 1

    def to_abi(self):
        return _abi.InterpolateParams(float(self.depth_tolerance))


JPEG_DEFAULT_RESTART = 32


@dataclasses.dataclass(frozen=True)
class Jpeg:
    """Parameters of the baseline JPEG encoder (rayn_hip_jpeg_encode_device, an extension: rayn writes PNG only; include/rayn_hip.h has
    the definition).  quality: IJG's 1..100.  subsampling: "420" (chroma at half size; a grey image has one form and ignores it) or
    "444".  restart: the restart interval in MCUs, 1..65535 - a format parameter: every interval is a segment the GPU encodes on its
    own, and costs the file a 2-byte marker, its padding and a DC predictor reset (DESIGN.md section 8 has the measured table behind the
    default)."""
    quality: int = 90
    subsampling: str = "420"
    restart: int = JPEG_DEFAULT_RESTART

    def __post_init__(self):
        _int_in("Jpeg", "quality", self.quality, 1, 100)
        if self.subsampling not in ("420", "444"):
            raise ValueError(f"Jpeg.subsampling must be '420' or '444', got {self.subsampling!r}")
        _int_in("Jpeg", "restart", self.restart, 1, 65535)

    def mode(self, bpp):
        """The encoder's subsampling argument for an image of bpp bytes per pixel: 1 is 4:2:0, 0 is 4:4:4 and what a grey image gets"""
        return 1 if self.subsampling == "420" and bpp == 3 else 0


@dataclasses.dataclass(frozen=True)
class Video:
    """A Motion-JPEG AVI of a sequence (render_sequence's video=, an extension): `path` of the file, `jpeg` the encoder's parameters for
    its frames, images=False to write the video alone - no PNG, .jpg or EXR."""
    path: str
    jpeg: Jpeg = Jpeg()
    images: bool = True

    def __post_init__(self):
        if not isinstance(self.path, (str, bytes)) and not hasattr(self.path, "__fspath__"):
            raise ValueError(f"Video.path must be a path, got {self.path!r}")
        if not isinstance(self.jpeg, Jpeg):
            raise ValueError(f"Video.jpeg must be a Jpeg, got {self.jpeg!r}")
        if not isinstance(self.images, bool):
            raise ValueError(f"Video.images must be a bool, got {self.images!r}")


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
