/* rayn_hip.h — C ABI of the MI355X-native replacement for rayn's per-sample integrator hot path.
 *
 * The reference (fu5ha/rayn, a single Rust binary crate) has no FFI: the replaceable seam is
 *   Film::render_frame_into(&mut self, world:&World, camera:CameraHandle, integrator:&I, filter:&F,
 *                           tile_size:Extent2u, frame:usize, time_range:Range<f32>, samples:usize)
 *   (src/film.rs:382-395), i.e. everything between building the tile list (src/film.rs:397-427) and
 *   tile_finished (src/film.rs:660-691), together with the trait surface that closure drives:
 *   Hitable (src/hitable.rs:8-18), Material/BSDF (src/material.rs:11-38), Light (src/light.rs:5-17),
 *   Camera (src/camera.rs:5-19), Integrator (src/integrator.rs:13-30), Filter (src/filter.rs:7-10).
 * Trait objects cannot cross to a GPU, so the ABI takes the same surface as a CLOSED SET of POD
 * descriptors (every concrete type the reference ships) in scene order — order is semantic
 * (HitableStore::add_hits folds in order, src/hitable.rs:170-210; HitStore::process_hits emits
 * packets object-major, src/hitable.rs:94-134).
 *
 * Plain pointers and sizes only; no C++ or torch types.  All functions return 0 on success or a
 * negative rayn_status; rayn_hip_last_error() gives the text.  Where the reference panics
 * (src/film.rs:127,160,197,667; src/material.rs:431) this ABI returns an error code instead.
 */
#ifndef RAYN_HIP_H
#define RAYN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RAYN_MAX_HITABLES 16
#define RAYN_MAX_MATERIALS 16
#define RAYN_MAX_LIGHTS 16
#define RAYN_FIS_TABLE_SIZE 512 /* FILTER_TABLE_SIZE, src/filter.rs:187 */
#define RAYN_FILM_FLOATS_PER_PIXEL 10 /* Color 3 + Alpha 1 + Background 3 + WorldNormal 3 (src/film.rs:103-120) */

typedef enum {
    RAYN_OK = 0,
    RAYN_ERR_INVALID_ARG = -1,
    RAYN_ERR_NO_DEVICE = -2,
    RAYN_ERR_HIP = -3,
    RAYN_ERR_NO_WORLD = -4,
    RAYN_ERR_OOM = -5
} rayn_status;

typedef struct { float x, y, z; } rayn_vec3;

/* ---- Hitable (src/hitable.rs:8-18) -------------------------------------------------------- */
typedef enum {
    RAYN_HITABLE_SPHERE = 0,    /* Sphere<TR>, src/sphere.rs:7-87 (TR = constant Vec3) */
    RAYN_HITABLE_TRACED_SDF = 1 /* TracedSDF<S>, src/sdf.rs:12-102 */
} rayn_hitable_kind;

typedef enum {
    RAYN_SDF_SPHERE = 0,   /* sdfu::Sphere: |p| - r (used by BASELINE config 1) */
    RAYN_SDF_MANDELBOX = 1, /* MandelBox, src/sdf.rs:104-188 */
    /* EXTENSION, not in the reference (which has no Mandelbulb): power-8 Mandelbulb distance
     * estimator in the trigonometry-free polynomial form (I. Quilez), 'iterations' orbit steps with bailout
     * |w|^2 > 256, d = 0.25*ln(m)*sqrt(m)/dz.  Exists because BASELINE.json names the workload "Mandelbulb". */
    RAYN_SDF_MANDELBULB = 2
} rayn_sdf_kind;

typedef struct {
    uint32_t kind;     /* rayn_hitable_kind */
    uint32_t material; /* MaterialHandle(usize), src/material.rs:55-56 */
    /* RAYN_HITABLE_SPHERE: Sphere::new(transform_seq, radius, material), src/sphere.rs:14-20 */
    rayn_vec3 center;
    float radius;
    /* RAYN_HITABLE_TRACED_SDF: TracedSDF::new(sdf, material), src/sdf.rs:17-21 */
    uint32_t sdf_kind;   /* rayn_sdf_kind */
    uint32_t iterations; /* MandelBox::new(iterations, ..), src/sdf.rs:114 */
    float box_side;      /* BoxFold::new(side_length), src/sdf.rs:151.  Any value: a negative, -0 or NaN side folds as the reference's min(max(p, -l), l) does (the general arm) */
    float min_radius;    /* SphereFold::new(min_radius, fixed_radius), src/sdf.rs:172 */
    float fixed_radius;
    float scale;         /* MandelBox scale, src/sdf.rs:114 */
    float sdf_radius;    /* RAYN_SDF_SPHERE radius */
    /* RAYN_HITABLE_SPHERE with a closure transform_seq (TR: Fn(f32) -> Vec3, src/sphere.rs:7, src/animation.rs:62-68):
     * animated != 0 selects the linear closure |t| center + center_vel * t, evaluated — like the reference — at the ray
     * time of LANE 0 of the packet that calls hit / occluded / get_shading_info.
     * EXTENSION for RAYN_HITABLE_TRACED_SDF (the reference's TracedSDF has no transform and ignores time,
     * src/sdf.rs:12-25): center / animated / center_vel are honoured the same way - the SDF is evaluated in
     * the frame translated by that origin (hit: ray origin - origin; occluded: both ends - origin;
     * get_shading_info: normal estimated at point - origin, the shading point stays in world space).  This
     * is what gives BASELINE config 5 its "animated fractal with time-sampled motion blur".  A zero,
     * non-animated center (all the reference can express) is an exact no-op. */
    uint32_t animated;
    rayn_vec3 center_vel;
    /* EXTENSION for RAYN_SDF_MANDELBOX (scene S3: "time-varying fold/scale params"; the reference's SDFs
     * ignore time, src/sdf.rs:25): the scale as the closure |t| scale + scale_vel * t, evaluated - like every closure-sequenced
     * parameter (src/animation.rs:62-68) - at the ray time of lane 0 of the packet that calls hit / occluded /
     * get_shading_info.  0 (what a zeroed struct holds; the field used to be padding) is the reference's constant scale. */
    float scale_vel;
} rayn_hitable;

/* ---- Material / BSDF (src/material.rs:11-38) ---------------------------------------------- */
typedef enum {
    RAYN_MAT_LAMBERTIAN = 0, /* src/material.rs:85-142 */
    RAYN_MAT_DIELECTRIC = 1, /* src/material.rs:144-257; 'exponent' is the REMAPPED roughness */
    RAYN_MAT_SKY = 2,        /* src/material.rs:394-449 */
    RAYN_MAT_EMISSIVE = 3    /* src/material.rs:451-520 (inner Lambertian 0.5 is never sampled) */
} rayn_material_kind;

typedef struct {
    uint32_t kind;  /* rayn_material_kind */
    rayn_vec3 a;    /* albedo | albedo | sky top | emission */
    rayn_vec3 b;    /* -      | -      | sky bottom | - */
    float exponent; /* Dielectric: 1 + (1-roughness)^4 * 300, Dielectric::new_remap src/material.rs:167-174 */
} rayn_material;

/* ---- Light (src/light.rs:5-17): SphereLight::new(pos, rad, emission), src/light.rs:26-34 -- */
typedef struct {
    rayn_vec3 pos;
    float rad;
    rayn_vec3 emission;
    uint32_t _pad;
} rayn_light;

/* ---- Camera (src/camera.rs:5-19) ---------------------------------------------------------- */
typedef enum {
    RAYN_CAM_PINHOLE = 0,  /* src/camera.rs:41-119 */
    RAYN_CAM_THIN_LENS = 1, /* src/camera.rs:120-213 */
    RAYN_CAM_ORTHOGRAPHIC = 2 /* src/camera.rs:215-285 */
} rayn_camera_kind;

typedef struct {
    uint32_t kind;      /* rayn_camera_kind */
    float res_w, res_h; /* 'resolution: Vec2' argument of ::new */
    float vfov_or_size; /* vfov in degrees (pinhole, thin lens) | vertical_size (orthographic) */
    rayn_vec3 origin, at, up;
    float aperture;     /* thin lens */
    rayn_vec3 focus;    /* thin lens */
    /* Time-sequenced parameters (src/animation.rs): the reference lets origin/at/up/focus be closures
     * Fn(f32) -> Vec3.  Closures cannot cross the ABI; the closed set offers the linear closure
     * |t| base + vel * t per parameter (bit 0 origin, 1 at, 2 up, 3 focus of 'animated').  As in the
     * reference (src/animation.rs:62-68) a closure is evaluated at the time of LANE 0 of the ray-gen
     * packet (sample 4*floor(s/4) of the pixel) for all four lanes. */
    uint32_t animated;
    rayn_vec3 origin_vel, at_vel, up_vel, focus_vel;
} rayn_camera;

/* ---- World (src/world.rs:7-13) + VolumeParams (src/volume.rs:1-5) ------------------------- */
typedef struct {
    uint32_t n_hitables, n_materials, n_lights;
    rayn_hitable hitables[RAYN_MAX_HITABLES];    /* HitableStore, scene order */
    rayn_material materials[RAYN_MAX_MATERIALS]; /* MaterialStore */
    rayn_light lights[RAYN_MAX_LIGHTS];          /* Vec<Box<dyn Light>> */
    rayn_camera camera;                          /* the CameraHandle passed to render_frame_into */
    uint32_t has_scattering; /* coeff_scattering: Option<f32> */
    float coeff_scattering;
    uint32_t has_extinction; /* coeff_extinction: Option<f32> */
    float coeff_extinction;
} rayn_world_desc;

/* ---- arguments of Film::render_frame_into + the constants it reads ------------------------ */
typedef struct {
    uint32_t width, height;   /* Film.res, src/film.rs:180 */
    uint32_t samples;         /* 'samples' (spp = 4*samples), src/film.rs:391,434,439; closed-set limit: <= 4096 (16384 spp) */
    uint32_t tile_w, tile_h;  /* tile_size, src/main.rs:69 */
    uint32_t max_bounces;     /* PathTracingIntegrator.max_bounces, src/integrator.rs:34; closed-set limit: <= 120 */
    uint32_t volume_marches;  /* VOLUME_MARCHES_PER_SAMPLE (>= 2: samples_1d[3],[4] are indexed), src/setup.rs:25 */
    uint32_t frame;           /* seeds the sample tables, src/film.rs:434 */
    float time_start, time_end; /* time_range, src/main.rs:61-62 */
    uint32_t max_marches;     /* MAX_MARCHES = 256, src/sdf.rs:9 */
    uint32_t max_vis_marches; /* MAX_VIS_MARCHES = 100, src/sdf.rs:10 */
    float sdf_detail_scale;   /* SDF_DETAIL_SCALE, src/setup.rs:37 */
    float world_radius;       /* WORLD_RADIUS, src/setup.rs:33 */
    /* multi-GPU film partition (no reference counterpart; tiles are independent, src/film.rs:439-627):
     * this call renders the tiles k (reference tile order) with (k + k / tile_step) % tile_step == tile_first: every run of
     * tile_step consecutive tiles holds each owner once, and the assignment rotates from run to run so that no owner is
     * locked to a fixed lattice of image rows (measured: the plain k % 8 lattice left one of 8 ranks 7 % slower). */
    uint32_t tile_first, tile_step;
} rayn_frame_params;

/* counters + timings of the last render (device work only) */
typedef struct {
    uint64_t paths;          /* camera paths started */
    uint64_t segments;       /* valid rays extended (one per path per depth reached) */
    uint64_t shaded_slots;   /* packet lanes shaded incl. padding lanes */
    uint64_t tiles;
    uint64_t batches;
    double ms_total;         /* HIP-event time of the whole render on the ctx stream */
    double ms_raygen, ms_extend, ms_bin, ms_shade, ms_compact, ms_resolve; /* ms_shade = k_shade_setup */
    uint64_t launches_extend, launches_shade;
    uint64_t queue_bytes_bin;     /* algorithmic HBM bytes of the bin stage */
    double ms_shadow, ms_finish; /* k_shadow, k_shade_finish */
    uint64_t queue_bytes_compact; /* algorithmic HBM bytes of the repack stage */
    uint64_t shadow_jobs;         /* shadow segments marched by k_shadow (29 algorithmic bytes each: 4 ref + 24 segment in, 1 visibility out) */
} rayn_stats;

typedef struct rayn_ctx rayn_ctx;

/* Film::new (src/film.rs:184-203) + device selection: one ctx = one GPU ... */
int rayn_hip_create(int device, rayn_ctx** out);
/* ... or several ("rayn_hip_create(device_ids[], n)", the call being internally multi-GPU): one
 * context over n_devices GPUs of this process, replacing rayon's tile tasks (src/film.rs:630-691) with one renderer per GPU.
 * Every other entry point takes it like a single-device ctx; ALL device pointers passed to rayn_hip_render_frame_device
 * then live on devices[0].  Per frame the tiles of the call's share are dealt to the devices in rotation (the j-th owned
 * tile goes to device (j + j / n) % n), scene and tables are replicated, every device renders its tiles with its own
 * streams, and each device other than devices[0] sends the pixels of its tiles to devices[0] with ONE peer copy over xGMI
 * (hipMemcpyPeerAsync of 10 floats per pixel) - the only data that crosses devices.  A device id may repeat (the entries
 * then share that GPU and split its memory budget; used by the single-GPU tests).  rayn_hip_set_trace_tile returns
 * RAYN_ERR_INVALID_ARG on a multi-device ctx. */
int rayn_hip_create_multi(const int* devices, int n_devices, rayn_ctx** out);
int rayn_hip_device_count(const rayn_ctx* ctx); /* entries of the context (1 for rayn_hip_create) */
/* Multi-device context: the sample tables / scramble / filter table are copied to every peer when a frame's (four table pointers, width, height, samples,
 * max_bounces, volume_marches, frame) differ from the last broadcast to that peer - not every frame (r6).  A host that REWRITES its tables in place under
 * unchanged parameters calls rayn_hip_upload_world again (it forgets the broadcast) or passes other buffers.  Returns the peer copies of the tables made so
 * far (one per peer and broadcast; diagnostics / tests). */
uint64_t rayn_hip_table_broadcasts(const rayn_ctx* ctx);
void rayn_hip_destroy(rayn_ctx* ctx);
const char* rayn_hip_last_error(const rayn_ctx* ctx);

/* setup::setup() result (src/setup.rs:46-170) flattened; replaces passing &World. */
int rayn_hip_upload_world(rayn_ctx* ctx, const rayn_world_desc* world);

/* Film::render_frame_into (src/film.rs:382-628) incl. tile_finished's normalisation
 * (src/film.rs:82-98,660-691).  HOST pointers.  Tables are the ones Samples::new_rd
 * (src/sampler.rs:18-37), the per-pixel SmallRng scramble (src/film.rs:460-461) and
 * FilterImportanceSampler::new (src/filter.rs:187-220) produce:
 *   samples_1d: spp*sets_1d floats, samples_2d: 2*spp*sets_2d floats, scramble: width*height,
 *   fis_table: 512.  Outputs are full-resolution, bottom-up rows like the reference's film
 *   (the flip happens only in save_to, src/film.rs:236): color/background/normal 3 floats per
 *   pixel interleaved, alpha 1.  Pixels of tiles this call does not own are left untouched. */
int rayn_hip_render_frame(rayn_ctx* ctx, const rayn_frame_params* p,
                          const float* samples_1d, const float* samples_2d,
                          const float* scramble, const float* fis_table,
                          float* out_color, float* out_alpha, float* out_background,
                          float* out_normal);

/* Same, but every pointer is a DEVICE pointer on the ctx's GPU and the work is enqueued on
 * 'hip_stream' (a hipStream_t; NULL = the ctx's own stream), after everything already queued there.
 * The call is BLOCKING: it returns when the frame is complete (it waits once, at the end, to read the
 * frame statistics back; queue sizes stay on the device and the depth loop of a frame with <= 8 bounces never synchronises -
 * deeper ones read the queue size back every 4th depth from depth 8 on, to stop enqueueing depths for a batch whose paths have
 * all terminated).
 * This is the entry the bench and the multi-GPU paths use. */
int rayn_hip_render_frame_device(rayn_ctx* ctx, const rayn_frame_params* p,
                                 const float* d_samples_1d, const float* d_samples_2d,
                                 const float* d_scramble, const float* d_fis_table,
                                 float* d_out_color, float* d_out_alpha, float* d_out_background,
                                 float* d_out_normal, void* hip_stream);

int rayn_hip_get_stats(const rayn_ctx* ctx, rayn_stats* out);
/* entry 0 .. rayn_hip_device_count() - 1 of a multi-device context: what THAT device did in the last frame (its own tiles, segments,
 * batches; ms_total = HIP events around its share on its own stream, table broadcast and film copy excluded) - rayn_hip_get_stats holds
 * the sums and, in ms_total, the whole multi-device frame on devices[0]'s clock.  A single-device ctx has the one entry 0. */
int rayn_hip_get_entry_stats(const rayn_ctx* ctx, int entry, rayn_stats* out);

/* ---- the film gather of a multi-PROCESS launch (one process per GPU; no reference counterpart: tiles are independent,
 * src/film.rs:439-627, and the reference's tile_finished copies each finished tile into the one film, src/film.rs:660-691) ----
 * A rank that owns the share (tile_first, tile_step) renders it straight into a PACKED PLANAR film of its own pixels - no
 * full-resolution film exists on that rank and nothing is packed afterwards: Color 3N | Alpha N | Background 3N | WorldNormal 3N
 * floats for the N = rayn_share_pixels(p) pixels of its tiles, tile after tile in ascending reference tile order, pixel-major (x outer,
 * y inner) inside a tile.  That buffer is what crosses xGMI (ONE ncclGather / peer copy); the receiving rank scatters it into its
 * full-resolution film with rayn_hip_unpack_share_device (p carrying the SENDER's tile_first / tile_step): one kernel launch,
 * enqueued on hip_stream and not waited for; the share's tile list is uploaded the first time a share is seen and cached in the ctx for its
 * lifetime (one list of <= 32 B per tile per distinct (resolution, tile size, tile_first, tile_step): a fixed partition costs N - 1 lists).
 * It is the same packed layout and the same two kernels rayn_hip_create_multi uses between the devices of one process. */
uint64_t rayn_share_pixels(const rayn_frame_params* p);
int rayn_hip_render_frame_packed_device(rayn_ctx* ctx, const rayn_frame_params* p,
                                        const float* d_samples_1d, const float* d_samples_2d,
                                        const float* d_scramble, const float* d_fis_table,
                                        float* d_packed /* 10 * rayn_share_pixels(p) floats */, void* hip_stream);
int rayn_hip_unpack_share_device(rayn_ctx* ctx, const rayn_frame_params* p, const float* d_packed,
                                 float* d_out_color, float* d_out_alpha, float* d_out_background,
                                 float* d_out_normal, void* hip_stream);

/* ---- Film::save_to's per-pixel post-process (src/film.rs:205-378) on the device ----------------------------------------
 * kind: ChannelKind (0 Color, 1 Alpha, 2 Background, 3 WorldNormal, src/film.rs:103-120); bit k of have_mask = ChannelKind k is
 * among the film's channels (bits above 3 are ignored).  The arms: Color + Alpha with transparent_background -> RGBA, the colour
 * saturated and gamma-corrected (2.2), the alpha quantised; Color + Background, not transparent -> RGB of (color + background),
 * saturated and gamma-corrected; Color without Background, not transparent -> RGB, gamma-corrected but NOT saturated; Background
 * -> RGB, saturated and gamma-corrected; WorldNormal -> RGB of n * 0.5 + 0.5; Alpha -> grey.  Quantisation is
 * `(v * 255.0).min(255.0).max(0.0) as u8` with Rust's f32::min / max; powf is the pinned dm_powf (rayn_detmath.h).
 * Bytes per pixel of the image for that combination (4, 3 or 1), or -1 where the reference returns Err.  Host only; needs no GPU. */
int rayn_save_to_bpp(uint32_t kind, uint32_t have_mask, int transparent_background);
/* Enqueue the post-process of one channel on 'hip_stream' (NULL = the ctx's own stream; not waited for).  DEVICE pointers on the
 * ctx's GPU (devices[0] of a multi-device ctx), the film in the layout rayn_hip_render_frame_device writes (bottom-up rows);
 * the channels the arm does not read may be NULL.  d_out receives width * height * bpp bytes, rows top-down.  A combination
 * the reference rejects returns RAYN_ERR_INVALID_ARG with the reference's Err text as the last error; so do a missing buffer
 * the arm reads and a zero-sized image. */
int rayn_hip_save_to_pixels_device(rayn_ctx* ctx, uint32_t kind, uint32_t have_mask, int transparent_background,
                                   uint32_t width, uint32_t height, const float* d_color, const float* d_alpha,
                                   const float* d_background, const float* d_normal, uint8_t* d_out, void* hip_stream);

/* ---- denoiser of the film's Color channel (an EXTENSION: rayn has no denoiser) -------------------------------------------------
 * The edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010), guided by WorldNormal and Alpha, on the film's planar layout
 * (pixel x + y * width).  `iterations` L in 1..8; iteration i = 0 .. L-1 uses step 2^i and reads the previous iteration's colour.
 * kc = 1 / sigma_color^2, kn = 1 / sigma_normal^2, ka = 1 / sigma_alpha^2 (f32).  A pixel whose colour has a non-finite component
 * passes through; otherwise W = 9/64, S = (9/64) c_p, and for the 24 other taps of the 5x5 stencil in raster order (ky = -2..2
 * outer, kx = -2..2 inner), q = p + (kx, ky) 2^i, skipped outside the image or where c_q has a non-finite component:
 *   e = (d_c * kc * 4^i + d_n * kn) + d_a * ka   (squared distances of colour, normal and alpha; a term whose sigma is 0 is left out)
 *   w = (h[ky+2] * h[kx+2]) * expf(-e), h = {1/16, 1/4, 3/8, 1/4, 1/16}, expf = dm_expf (rayn_detmath.h); a NaN w skips the tap
 *   W += w, S += w * c_q;   out_p = S / W.
 * All f32, no contraction, IEEE division.  Only Color is filtered; Alpha, Background and WorldNormal stay as rendered.
 * Bytes of device scratch rayn_hip_denoise_device needs for a width x height film (0 for a size it rejects).  Host only; needs no GPU. */
size_t rayn_denoise_scratch_bytes(uint32_t width, uint32_t height);
/* Enqueue the filter on 'hip_stream' (NULL = the ctx's own stream; not waited for), on the ctx's GPU (devices[0] of a multi-device
 * ctx).  DEVICE pointers: d_color / d_normal 3 floats per pixel, d_alpha 1, d_out_color 3; d_scratch 16-byte aligned, at least
 * rayn_denoise_scratch_bytes.  A sigma of 0 switches its term off (that guide may be NULL); any other sigma must be finite and in
 * [2^-30, 2^30].  RAYN_ERR_INVALID_ARG with a last error text for: a zero-sized image or width * height >= 2^31, iterations outside
 * 1..8, a bad sigma, a NULL colour, output or scratch, a NULL guide whose sigma is not 0, too little or misaligned scratch, and
 * d_out_color == d_color.  The inputs are not modified. */
int rayn_hip_denoise_device(rayn_ctx* ctx, uint32_t width, uint32_t height, uint32_t iterations, float sigma_color, float sigma_normal,
                            float sigma_alpha, const float* d_color, const float* d_alpha, const float* d_normal, float* d_out_color,
                            void* d_scratch, size_t scratch_bytes, void* hip_stream);

/* ---- HDR display transform of the film's Color channel (an EXTENSION: rayn's save_to clamps the film to [0, 1]) ------------------
 * Auto exposure, bloom and a tone operator between the float film and save_to's gamma 2.2 and 8-bit quantisation.  All arithmetic f32,
 * no contraction, IEEE '/'; logf / expf / powf are dm_logf / dm_expf / dm_powf (rayn_detmath.h); rmin / rmax are Rust's f32::min / max
 * (a NaN operand yields the other operand).  Film pixels in film order (bottom-up rows), n = width * height.  Only the Color kind is
 * transformed, through the three arms of save_to that have_mask and transparent_background select.
 *
 * Input colour: c = color + background in the Color + Background arm, c = color in the other two.  A non-finite component of c counts
 * as 0 in metering and in the bloom's bright pass and passes through unchanged in the final step.
 * Luminance: lum(c) = (0.2126 c.r + 0.7152 c.g) + 0.0722 c.b.
 *
 * Metering (auto exposure only).  Pixel i contributes v_i = logf(rmax(lum(c_i), 1e-4f)), k_i = 1 when all three components of c_i are
 * finite and lum(c_i) > 0, else v_i = 0, k_i = 0.  The order of the sum is fixed.  Stage 1: blocks of 256 consecutive film pixels
 * (indices >= n contribute 0); in a block the halving tree a[j] += a[j + s] for s = 128, 64, ..., 1 (j < s); the block's partial is
 * a[0]; the counts likewise in u32.  Stage 2: 256 accumulators, accumulator t adds the partials t, t + 256, t + 512, ... in ascending
 * order starting from 0, then the same tree once more gives the sum S and the count N.
 *   N == 0: the state is left as it is and the exposure scale is e = 1.
 *   otherwise m_now = S / (float)N; m = m_now if the state's valid word is 0 or adapt == 1, else m = m_prev + (m_now - m_prev) * adapt;
 *   the state becomes {m, 1}; e = key / expf(m).
 * The STATE is two 32-bit words in device memory, {m (f32), valid (u32)}; all zeros = fresh.  It carries m from frame to frame.
 * Manual exposure skips all of it: e = exposure_scale (a caller turning an EV into a scale uses 2^EV rounded to f32).
 *
 * Bloom (levels L in 1..8; 0 = off).  Bright pass D_0 = rmax(e * c - threshold, 0) per component, non-finite components of c read as 0.
 * Level k has w_k = (w_k-1 + 1) / 2 by h_k = (h_k-1 + 1) / 2 pixels (a dimension that reaches 1 stays 1).  Downsample, k = 1..L:
 *   D_k(x, y) = ((A + B) + (C + D)) * 0.25f, the taps at (2x, 2y), (2x + 1, 2y), (2x, 2y + 1), (2x + 1, 2y + 1) of level k - 1, each
 *   coordinate clamped to the edge.
 * Upsample: U_L = D_L, U_k = D_k + up(U_k+1) for k = L - 1 .. 0.  up is the bilinear 2x filter: along x, an even x reads the taps x / 2
 * - 1 with weight 0.25 and x / 2 with 0.75, an odd x reads x / 2 with 0.75 and x / 2 + 1 with 0.25 (integer division, each tap clamped to
 * the edge); the same along y; with a, b the taps of the first row and c, d those of the second,
 *   up = wy0 * (wx0 * a + wx1 * b) + wy1 * (wx0 * c + wx1 * d).
 * The bloom is B = U_0 * (strength / (float)(L + 1)), the scalar computed once in f32.
 *
 * Tone.  x = e * c + B (x = e * c without bloom), then per `tone`:
 *   0 linear:   d = x
 *   1 reinhard: extended Reinhard on luminance: lx = lum(x); where lx is finite and > 0, d = x * ((1 + lx * iw2) / (1 + lx)), else d = x;
 *               iw2 = 1 / (white * white) is the caller's
 *   2 aces:     Narkowicz's fit per component: y = rmax(x, 0), d = (y * (2.51f * y + 0.03f)) / (y * (2.43f * y + 0.59f) + 0.14f)
 * Output: the arm's own chain of save_to on d - Color + Alpha: quant8(gamma22(saturate1(d))) with the alpha beside it; Color +
 * Background: quant8(gamma22(saturate1(d))), the background being in c already; Color only: quant8(gamma22(d)) - rows flipped top-down.
 * With manual exposure_scale 1, linear and no bloom, d has the bits of c and the image is that of rayn_hip_save_to_pixels_device. */
typedef struct {
    uint32_t tone;
    uint32_t auto_exposure;
    float exposure_scale;
    float key;
    float adapt;
    float iw2;
    uint32_t levels;
    float threshold;
    float strength;
} rayn_display_params;
/* tone: 0 linear, 1 reinhard, 2 aces.  auto_exposure: 0 manual (exposure_scale, finite and >= 0), 1 auto (key finite and > 0; adapt in
 * [0, 1]: 1 = no adaptation).  iw2: finite and >= 0, read by reinhard.  levels: bloom levels, 0 = off, at most 8; threshold finite,
 * strength finite and >= 0.
 * Bytes of device scratch the two display entries need for a width x height film with `levels` bloom levels: a 256-byte header, the
 * metering partials and levels 1 .. L as 16-byte records (0 for a size they reject or levels > 8).  Host only; needs no GPU. */
size_t rayn_display_scratch_bytes(uint32_t width, uint32_t height, uint32_t levels);
/* Enqueue the transform and the Color arm's post-process on 'hip_stream' (NULL = the ctx's own stream; not waited for), on the ctx's GPU
 * (devices[0] of a multi-device ctx).  have_mask, transparent_background, width, height and the DEVICE film pointers as
 * rayn_hip_save_to_pixels_device takes them for the Color kind (a channel the arm does not read may be NULL).  d_state: the two-word
 * state, needed with auto exposure only.  d_scratch: 16-byte aligned, at least rayn_display_scratch_bytes; needed with auto exposure or
 * bloom only.  d_out receives width * height * bpp bytes, rows top-down.  Optional outputs, NULL to skip: d_out_meter, 2 floats {m, e}
 * (m as the state holds it after the call, 0 with manual exposure); d_out_bloom, the plane B as width * height * 3 floats in film
 * order (written with bloom on only).  The exposure scale never leaves the device and the call does not synchronise.  The inputs are
 * not modified.  RAYN_ERR_INVALID_ARG with a last error text for: a channel combination the reference rejects (its Err text), a
 * zero-sized image or width * height >= 2^31, an unknown tone, levels > 8, parameters outside the ranges above, a NULL state with auto
 * exposure, a NULL buffer, and a NULL, misaligned or too small scratch where one is needed. */
int rayn_hip_display_pixels_device(rayn_ctx* ctx, const rayn_display_params* dp, uint32_t have_mask, int transparent_background,
                                   uint32_t width, uint32_t height, const float* d_color, const float* d_alpha, const float* d_background,
                                   void* d_state, void* d_scratch, size_t scratch_bytes, uint8_t* d_out, float* d_out_meter,
                                   float* d_out_bloom, void* hip_stream);
/* The same with the float plane d as the output: d_out_color receives width * height * 3 floats in film order, before the arm's
 * saturate / gamma / quantise (so that a test is not blinded by the 8-bit quantisation).  It must not be d_color or d_background. */
int rayn_hip_display_color_device(rayn_ctx* ctx, const rayn_display_params* dp, uint32_t have_mask, int transparent_background,
                                  uint32_t width, uint32_t height, const float* d_color, const float* d_alpha, const float* d_background,
                                  void* d_state, void* d_scratch, size_t scratch_bytes, float* d_out_color, float* d_out_meter,
                                  float* d_out_bloom, void* hip_stream);

/* ---- progressive rendering (an EXTENSION: rayn carries only an unused progressive_epoch counter, src/film.rs:178-179) ------------
 * A progressive render is a series of EPOCHS: ordinary renders of the same frame, each under its own sample tables, whose finished
 * films are accumulated.  Everything here happens to finished films; the integrator and the film resolve are not involved.
 *
 * Epoch seed.  Samples::new_rd gives set i the sequence offset (offset + i) << 32 (src/sampler.rs:22-29), so consecutive offsets share
 * all but one set, shifted by one dimension.  Epoch e of frame f therefore uses the tables of offset seed(f, e) = f + e * 65536;
 * epoch 0 is the plain frame.  Valid only while the sets of one epoch (3 + (max_bounces + 1) (15 + 9 volume_marches)) number at most
 * 65536 and seed < 2^32: otherwise RAYN_ERR_INVALID_ARG, never a wrap.  The epoch's render call carries the seed in
 * rayn_frame_params.frame (the kernels do not read it; the table broadcast of a multi-device context keys on it).  Scramble and filter
 * tables do not depend on the epoch.  Host only; needs no GPU. */
int rayn_progressive_seed(uint32_t frame, uint32_t epoch, uint32_t max_bounces, uint32_t volume_marches, uint32_t* out_seed);
/* State, per film, in device memory the caller owns: per pixel the ten film floats as running sums and mean_y, m2 (48 bytes: three
 * float4 planes in film pixel order - (sum Color, sum Alpha), (sum Background, mean_y), (sum WorldNormal, m2)); per tile a record of 4 u32
 * (epochs, retired, outliers, bits of max_e); then 4 u32 of totals (active tiles, bits of max e, outlier pixels lo / hi), the active
 * list and the list of the accumulate in flight (one u32 per tile each), in that order.  Bytes of it for a width x height film cut into
 * tile_w x tile_h tiles (0 for a geometry the entries reject).  Host only; needs no GPU. */
size_t rayn_progressive_state_bytes(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h);
typedef struct {
    float target_error;        /* a pixel with e_p > target_error is an outlier; finite, >= 0 */
    float noise_floor;         /* added to |mean_y| in e_p's denominator; finite, >= 0 */
    uint32_t min_epochs;       /* no tile retires before it has this many epochs; >= 2 */
    uint32_t max_epochs;       /* the loop's limit (the entries only validate it); min_epochs .. 65536 */
    uint32_t outlier_permille; /* a tile retires while at most this many per thousand of its pixels are outliers; <= 1000 */
    uint32_t adaptive;         /* 0: no tile ever retires */
} rayn_progressive_params;
typedef struct {
    uint32_t active_tiles;   /* tiles not retired */
    float max_e;             /* the largest max_e of all tiles */
    uint64_t outlier_pixels; /* the sum of all tiles' outliers */
} rayn_progressive_totals;
/* All rayn_hip_progressive_* entries take p for the film's geometry (width, height, tile_w, tile_h; the tiles are the reference's,
 * x-major, src/film.rs:399-427), DEVICE pointers on the ctx's GPU (devices[0] of a multi-device ctx) and 'hip_stream' (NULL = the ctx's
 * own stream); d_state 16-byte aligned, at least rayn_progressive_state_bytes.  RAYN_ERR_INVALID_ARG with a last error text for every
 * rejected argument.
 * Reset: enqueue a fresh state (sums -0.0f - the identity of IEEE addition, so that one epoch's sums are the epoch film's bits - mean_y =
 * m2 = 0, no epochs, nothing retired, every tile active).  Not waited for. */
int rayn_hip_progressive_reset_device(rayn_ctx* ctx, const rayn_frame_params* p, void* d_state, size_t state_bytes, void* hip_stream);
/* Accumulate the epoch film F (the four planes rayn_hip_render_frame_device writes) into the tiles of the list `tiles` (a HOST array of
 * n_tiles strictly ascending tile indices; NULL = every tile) and write those tiles' mean film to d_out_*.  For every pixel of a listed
 * tile, with n = the tile's epochs after increment, all f32, no contraction, IEEE '/' and sqrt:
 *   sum[k] = sum[k] + F[k]                                   k = 0..9
 *   c      = F.color + F.background                          per channel
 *   y      = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b
 *   d      = y - mean_y;  mean_y = mean_y + d / (float)n;  m2 = m2 + d * (y - mean_y)
 *   mean film[k] = sum[k] / (float)n
 *   n >= 2:  se = sqrtf(m2 / (float)(n * (n - 1)));  e_p = se / (fabsf(mean_y) + noise_floor)
 * Pixels of tiles not in the list are neither read nor written (state and mean film).  The tile's record: outliers = its pixels with
 * e_p > target_error (a NaN e_p compares false: a NaN pixel never holds a tile open), max_e = the largest e_p > 0 (0 for n < 2 or where
 * there is none).  With adaptive != 0 the tile retires when n >= min_epochs and outliers * 1000 <= outlier_permille * tile pixels (64-bit
 * integers); a retired tile stays retired.  Then the active (not retired) tiles are compacted into an ascending list and the totals are
 * taken, all on the device.  Enqueued, not waited for.  Rejected: a zero-sized film or tile, width * height >= 2^31, a NULL plane or
 * state, too little or misaligned state, a tile index beyond the tile count, a list not strictly ascending or empty, min_epochs < 2,
 * max_epochs < min_epochs or > 65536, a non-finite or negative target_error / noise_floor, outlier_permille > 1000, and an output plane
 * that is one of the epoch film's planes.  The epoch film is not modified. */
int rayn_hip_progressive_accumulate_device(rayn_ctx* ctx, const rayn_frame_params* p, const rayn_progressive_params* pp,
                                           const uint32_t* tiles, uint32_t n_tiles, const float* d_color, const float* d_alpha,
                                           const float* d_background, const float* d_normal, void* d_state, size_t state_bytes,
                                           float* d_out_color, float* d_out_alpha, float* d_out_background, float* d_out_normal,
                                           void* hip_stream);
/* The active list and the totals of the state as the work queued on the stream leaves them.  BLOCKING: the one small read-back of a
 * progressive epoch (16 bytes + 4 per tile), which the host needs for rayn_hip_set_tile_subset.  out_tiles: HOST array of `cap` entries
 * (cap >= the film's tile count, or out_tiles NULL to fetch the totals alone); out_totals may be NULL.  Returns the number of active
 * tiles (>= 0) or a negative rayn_status. */
int64_t rayn_hip_progressive_fetch_active(rayn_ctx* ctx, const rayn_frame_params* p, const void* d_state, size_t state_bytes,
                                          uint32_t* out_tiles, uint32_t cap, rayn_progressive_totals* out_totals, void* hip_stream);
/* Diagnostics, BLOCKING: every tile's record into HOST arrays of rayn_tile_count entries (any may be NULL). */
int rayn_hip_progressive_tile_report(rayn_ctx* ctx, const rayn_frame_params* p, const void* d_state, size_t state_bytes,
                                     uint32_t* out_epochs, uint32_t* out_retired, uint32_t* out_outliers, float* out_max_e,
                                     void* hip_stream);

/* ---- variance-guided denoiser of a progressive render's Color channel (an EXTENSION: rayn has neither a denoiser nor a progressive
 * render) -- The spatial half of SVGF (Schied et al., HPG 2017): the a-trous filter above with its colour term replaced by a luminance
 * edge-stop scaled by the local standard deviation the progressive state measured, and the variance filtered along with the colour.
 * Film layout and pixel order as rayn_hip_denoise_device.  Inputs: the MEAN film's Color c, Alpha a, WorldNormal nrm (what
 * rayn_hip_progressive_accumulate_device writes to d_out_*) and the state of that render with its geometry p (width, height, tile_w, tile_h).
 * Initial variance.  Pixel p lies in tile k of the reference's grid (x-major; resolutions the grid under-covers have pixels in no tile).
 * With n = that tile's epochs and m2 the state's value, v_p = m2 / (float)((uint64)n * (n - 1)): the variance of the mean, the expression
 * the accumulate takes the square root of.  p is GUIDED when it lies in a tile, n >= 2, v_p is finite and >= 0, and c_p has three
 * finite components.  A pixel that is not guided passes through all passes unchanged and is skipped as a tap (it contributes to no
 * neighbour).  v is the variance of the luminance of Color + Background (that is what the state holds) while the filter acts on Color
 * alone; the two differ only where depth-0 rays miss, i.e. at silhouettes, where the Alpha term guards.
 * Pass i = 0 .. L-1 (L in 1..8), step s = 2^i, on the previous pass's (c, v); kn = 1 / sigma_normal^2, ka = 1 / sigma_alpha^2; for every
 * guided p:
 *   l_x = (0.2126f * c_x.r + 0.7152f * c_x.g) + 0.0722f * c_x.b
 *   g_p = (sum k_j * v_j) / (sum k_j)   3x3 at UNIT spacing around p (not dilated), k = 1/4 centre, 1/8 edges, 1/16 corners, the centre
 *                                       first, then raster order; taps outside the image or not guided are left out of both sums
 *   inv = 1.0f / (sigma_luminance * sqrtf(g_p) + 1e-8f)
 *   W = 9/64, S = W * c_p, V = (W * W) * v_p
 *   the 24 other taps of the 5x5 stencil in raster order, q = p + (kx, ky) * s, skipped outside the image or when q is not guided:
 *     e = (fabsf(l_p - l_q) * inv + d_n * kn) + d_a * ka   (d_n, d_a: squared distances of normal and alpha as in
 *                                                          rayn_hip_denoise_device; a term whose sigma is 0 is left out)
 *     w = (h[ky+2] * h[kx+2]) * expf(-e), h and expf as in rayn_hip_denoise_device; a NaN w skips the tap
 *     W += w, S += w * c_q, V += (w * w) * v_q
 *   c'_p = S / W, v'_p = V / (W * W)
 *   p stays guided when c'_p has three finite components and v'_p is finite; else (an overflow) it keeps c'_p and is not guided from
 *   the next pass on - the same predicate as at the start, so that "not guided" stays one value of the record (v = NaN).
 * The last pass writes the planar 3-float colour and, when d_out_variance is given, v' (1 float per pixel; a pixel that is not guided
 * gets a quiet NaN there: no estimate).  All f32, no contraction, IEEE division and square root.
 * Bytes of device scratch the entry needs for a width x height film: 48 per pixel (two (colour, variance) record planes and one
 * (normal, alpha) record plane); 0 for a size it rejects.  Host only; needs no GPU. */
size_t rayn_denoise_variance_scratch_bytes(uint32_t width, uint32_t height);
/* Enqueue the filter on 'hip_stream' (NULL = the ctx's own stream; not waited for), on the ctx's GPU (devices[0] of a multi-device
 * ctx).  DEVICE pointers: d_color / d_normal 3 floats per pixel, d_alpha 1, d_out_color 3, d_out_variance 1 (may be NULL); d_state 16-byte
 * aligned, at least rayn_progressive_state_bytes; d_scratch 16-byte aligned, at least rayn_denoise_variance_scratch_bytes.  A sigma of 0
 * switches its term off (a guide whose sigma is 0 may be NULL); any other sigma must be finite and in [2^-30, 2^30].
 * RAYN_ERR_INVALID_ARG with a last error text for: what the progressive entries reject in p and d_state (zero-sized film or tile,
 * width * height >= 2^31, a tile size that leaves no tiles, a NULL, too small or misaligned state), iterations outside 1..8, a bad sigma,
 * a NULL colour, output or scratch, a NULL guide whose sigma is not 0, too little or misaligned scratch, d_out_color == d_color, and a
 * d_out_variance that is d_color, d_alpha, d_normal, d_state or d_out_color.  The inputs and the state are not modified. */
int rayn_hip_denoise_variance_device(rayn_ctx* ctx, const rayn_frame_params* p, uint32_t iterations, float sigma_luminance,
                                     float sigma_normal, float sigma_alpha, const float* d_color, const float* d_alpha,
                                     const float* d_normal, const void* d_state, size_t state_bytes, float* d_out_color,
                                     float* d_out_variance, void* d_scratch, size_t scratch_bytes, void* hip_stream);

/* ---- temporal accumulation for frame sequences (an EXTENSION: rayn renders every frame on its own) -- The temporal half of SVGF (Schied
 * et al., HPG 2017): the previous frame's accumulated Color is reprojected onto the current frame through the world position of every
 * pixel's primary hit and blended with the new frame, so that a sequence at few samples per frame approaches the noise of `samples x history`
 * wherever the surface stays visible.  Two passes, both downstream of the film: the film's four channels stay what the integrator wrote.
 *
 * Primary-hit G-buffer.  For every pixel (x, y) of the film (bottom-up rows, pixel x + y * width) ONE ray: uv = (ndc_x * (x + 0.5f),
 * ndc_y * (y + 0.5f)) - the ray-gen kernel's expression with a filter offset of 0 - lens sample (0.5, 0.5), ray time and camera closure
 * time both p->time_start, through the same Camera::get_rays code as a render, under the ctx's mul_add policy.  (0.5, 0.5) is the point
 * concentric_circle_map moves off its singular centre (src/math.rs:205): a thin lens's G-buffer ray starts 0.0001 * aperture beside the
 * lens centre.  The rays go through the scene's PRODUCT extend kernel at depth 0 (HitableStore::add_hits; the kernel rayn_hip_probe_extend
 * runs) as one identity queue.  Per pixel the pass writes a 16-byte record (Px, Py, Pz, t) - t the kernel's hit distance, P = o + t * d as
 * a separate f32 multiply and add under either policy - and the u32 index of the hit object; a miss writes (0, 0, 0, +inf) and 0xFFFFFFFF.
 * Closure-sequenced hitables are evaluated at p->time_start.
 * Bytes of device scratch the pass needs for a width x height film: 53 per pixel of the film rounded up to a multiple of 64 pixels, + 384
 * (0 for a size it rejects).  Host only; needs no GPU. */
size_t rayn_gbuffer_scratch_bytes(uint32_t width, uint32_t height);
/* Enqueue the pass on 'hip_stream' (NULL = the ctx's own stream; not waited for) for the uploaded world and p (its resolution, time_start,
 * max_marches, sdf_detail_scale, world_radius), on the ctx's GPU (devices[0] of a multi-device ctx).  DEVICE pointers: d_out_records 16
 * bytes per pixel and 16-byte aligned, d_out_object one u32 per pixel, d_scratch 16-byte aligned and at least rayn_gbuffer_scratch_bytes.
 * Like a render it replaces the context's device scene.  RAYN_ERR_INVALID_ARG with a last error text for: NULL p, a zero-sized image or
 * width * height >= 2^31, a NULL or misaligned buffer, too little scratch, buffers that overlap, and no uploaded world. */
int rayn_hip_gbuffer_device(rayn_ctx* ctx, const rayn_frame_params* p, void* d_out_records, uint32_t* d_out_object, void* d_scratch,
                            size_t scratch_bytes, void* hip_stream);

/* Temporal accumulate.  A HISTORY of a width x height film is one block of 52 bytes per pixel: plane A (r, g, b, n) - the accumulated Color
 * and the history length n as a float, n = 0: no history - plane B (Px, Py, Pz, t) - that frame's G-buffer record - the WorldNormal as
 * (nx, ny, nz, 0), 16 bytes each, and the object index (u32), in that order, each in film pixel order.  The caller ping-pongs two of them. */
typedef struct {
    uint32_t max_history;  /* the history length stops growing here (the blend weight never falls below 1 / max_history); 1..65536 */
    float depth_tolerance; /* a tap's recorded hit distance may differ from the reprojected one by this fraction of it; finite, >= 0 */
    float normal_min;      /* a tap's normal must have at least this dot product with the pixel's; in [-1, 1], -1 switches the test off */
} rayn_temporal_params;
/* Bytes of one history (0 for a size the entry rejects).  Host only; needs no GPU. */
size_t rayn_temporal_history_bytes(uint32_t width, uint32_t height);
/* Inputs: the current frame's Color c and WorldNormal nrm (3 floats per pixel), its G-buffer (records (P, t), objects obj), the previous
 * frame's history (NULL: none - the first frame) with that frame's camera and time_start, and p for the resolution and the current
 * time_start.  Outputs: the accumulated Color (3 floats per pixel) and the new history.  Hitable motion comes from the uploaded world.
 * All arithmetic f32, no contraction under either mul_add policy, IEEE '/' and sqrtf.  dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z;
 * cross(a, b) = (a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); nz(a) = a * (1.0f / sqrtf(dot(a, a))); vector +, -
 * and * scalar act per component, and "a - b * s" is a multiply, then a subtraction.  Per pixel:
 *   1. Reset: out = c, n' = 1 - and n' = 0 when c has a non-finite component, so that it never becomes a tap - when obj = 0xFFFFFFFF (a
 *      miss), c has a non-finite component, or there is no previous history.
 *   2. Object motion: Pp = P - center_vel * (time_start_cur - time_start_prev) when hitable obj has animated != 0, else Pp = P.  scale_vel
 *      morphing is not reprojected; the depth test catches it.
 *   3. The previous camera at ts = its time_start: o = origin + origin_vel * ts when bit 0 of animated is set, else origin; at and up
 *      likewise (bits 1, 2).
 *        pinhole, thin lens (a pinhole at o):  w = nz(o - at), u = nz(cross(up, w)), v = cross(w, u);  q = Pp - o;  zc = -dot(q, w),
 *          rejected unless zc > 0;  uvx = (dot(q, u) / (zc * half_w) + 1.0f) * 0.5f, uvy = (dot(q, v) / (zc * half_h) + 1.0f) * 0.5f;
 *          te = sqrtf(dot(q, q))
 *        orthographic:  w = nz(at - o), u = nz(cross(w, up)), v = cross(u, w);  ll = (o - u * half_w) - v * half_h;  q = Pp - ll;
 *          uvx = dot(q, u) / full_w, uvy = dot(q, v) / full_h;  te = dot(q, w), rejected unless te > 0
 *      (half_w .. full_h: the constants the camera's ::new derives, src/camera.rs:53-72,134-157,228-240.)
 *      fx = uvx * (float)width - 0.5f, fy = uvy * (float)height - 0.5f, rejected unless both are finite.
 *   4. x0f = floorf(fx), wx1 = fx - x0f, wx0 = 1.0f - wx1, and y likewise; x0, y0 = x0f, y0f as integers (clamped to [-2, 2^31] first,
 *      which changes no result).  Taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) with w = wx0 * wy0, wx1 * wy0, wx0 * wy1,
 *      wx1 * wy1.  A tap counts when it is inside the image, n_tap >= 1, obj_tap == obj, fabsf(t_tap - te) <= depth_tolerance * te and,
 *      with normal_min > -1, dot(nrm, nrm_tap) >= normal_min (a NaN fails every one):  W += w, S += w * c_tap, N += w * n_tap.
 *   5. W > 0:  h = S / W, nh = N / W, n' = fminf(nh + 1.0f, (float)max_history), a = 1.0f / n', out = h + a * (c - h) as separate
 *      operations.  A rejected projection, W <= 0 and an out with a non-finite component reset the pixel as in 1.
 *   New history: A' = (out, n'), B' = (P, t), (nrm, 0) and obj.
 * Enqueued on 'hip_stream' (NULL = the ctx's own stream; not waited for), on the ctx's GPU (devices[0] of a multi-device ctx); DEVICE
 * pointers, records and histories 16-byte aligned.  RAYN_ERR_INVALID_ARG with a last error text for: NULL p or tp, a zero-sized image or
 * width * height >= 2^31, max_history outside 1..65536, a non-finite or negative depth_tolerance, normal_min outside [-1, 1], a NULL
 * buffer (d_prev_history alone may be NULL; prev_camera may be NULL with it), an unknown camera kind, a history_bytes (the size of EACH
 * history) below rayn_temporal_history_bytes, a misaligned record plane or history, an output that overlaps an input, the new history
 * overlapping the previous one or d_out_color, and no uploaded world.  The inputs and the previous history are not modified. */
int rayn_hip_temporal_accumulate_device(rayn_ctx* ctx, const rayn_frame_params* p, const rayn_temporal_params* tp, const rayn_camera* prev_camera,
                                        float prev_time_start, const float* d_color, const float* d_normal, const void* d_gbuffer_records,
                                        const uint32_t* d_gbuffer_object, const void* d_prev_history, void* d_new_history, size_t history_bytes,
                                        float* d_out_color, void* hip_stream);

/* Temporal accumulate with luminance moments: SVGF's noise estimate for sequences.  The MOMENTS of a width x height film are one float2
 * (m1, m2) per pixel in film pixel order, 8 bytes per pixel, beside a history (whose 52-byte layout does not change); the caller ping-pongs
 * two of them with the histories.  Bytes of one (0 for a size rayn_temporal_history_bytes rejects).  Host only; needs no GPU. */
size_t rayn_temporal_moments_bytes(uint32_t width, uint32_t height);
/* rayn_hip_temporal_accumulate_device with the moments carried through the same reprojection: d_out_color and the new history are, bit
 * for bit, what that entry writes for the same inputs.  On top of its definition, f32, no contraction, IEEE '/':
 *   y = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b, y2 = y * y, for the frame's Color c.
 *   A pixel that resets (steps 1 and 5) writes (m1, m2) = (y, y2), and (0, 0) when c is not finite (n' = 0: it is never a tap).
 *   Otherwise, over the taps that count for the colour, with the same w and in the same order: S1 += w * m1_tap, S2 += w * m2_tap;
 *   h1 = S1 / W, h2 = S2 / W; m1' = h1 + a * (y - h1), m2' = h2 + a * (y2 - h2) with the colour's a = 1.0f / n'.
 *   If m1' or m2' is not finite the pixel writes (y, y2); the colour keeps its blended value (an overflow heals on the next frame).
 * d_prev_moments is required exactly when d_prev_history is given; d_new_moments always; moments_bytes is the size of EACH.
 * RAYN_ERR_INVALID_ARG with a last error text for everything rayn_hip_temporal_accumulate_device rejects, and for: a NULL d_new_moments,
 * previous moments without a previous history or a previous history without previous moments, a moments_bytes below
 * rayn_temporal_moments_bytes, moments that are not 16-byte aligned, the new moments overlapping the previous ones, an input or another
 * output, and the previous moments overlapping an output.  The inputs, the previous history and the previous moments are not modified. */
int rayn_hip_temporal_accumulate_moments_device(rayn_ctx* ctx, const rayn_frame_params* p, const rayn_temporal_params* tp,
                                                const rayn_camera* prev_camera, float prev_time_start, const float* d_color, const float* d_normal,
                                                const void* d_gbuffer_records, const uint32_t* d_gbuffer_object, const void* d_prev_history,
                                                void* d_new_history, size_t history_bytes, const void* d_prev_moments, void* d_new_moments,
                                                size_t moments_bytes, float* d_out_color, void* hip_stream);

/* Temporal accumulate with a choice of the history resampling filter of step 4.  The arguments of the two entries above plus rp. */
typedef struct { uint32_t resample; /* 0 bilinear (the existing step 4), 1 Catmull-Rom */ } rayn_temporal_resample_params;
/* d_prev_moments and d_new_moments both NULL: no moments, the outputs of rayn_hip_temporal_accumulate_device (moments_bytes is ignored).
 * Otherwise the rules of rayn_hip_temporal_accumulate_moments_device apply.  resample == 0: the outputs are bit for bit those of these
 * two entries.  resample == 1: steps 1, 2, 3 and 5 (the moments' blend and both non-finite fallbacks included) do not change; all f32, no
 * contraction under either mul_add policy, "a * b + c" a multiply and then an add.  Step 4 becomes:
 *   x0f = floorf(fx), t = fx - x0f, x0 the integer as before; y likewise.  Per axis the weights of the offsets -1, 0, 1, 2:
 *     k_-1 = ((-0.5f * t + 1.0f) * t - 0.5f) * t        k_0 = ((1.5f * t - 2.5f) * t) * t + 1.0f
 *     k_1  = ((-1.5f * t + 2.0f) * t + 0.5f) * t        k_2 = ((0.5f * t - 0.5f) * t) * t
 *   The 16 taps (x0 + i, y0 + j), i, j in -1..2, in raster order (j outer, i inner); a tap counts by step 4's predicate: inside the image,
 *   n_tap >= 1, obj_tap == obj, the depth test and, with normal_min > -1, the normal test.
 *   FULL SUPPORT - all 16 count:  w = kx_i * ky_j;  W += w, S += w * c_tap, N += w * n_tap, and with moments S1 += w * m1_tap,
 *     S2 += w * m2_tap;  h = S / W, nh = N / W, h1 = S1 / W, h2 = S2 / W.  Anti-ringing: every component of h, and h1 and h2, becomes
 *     fminf(fmaxf(v, lo), hi) with lo / hi the minimum / maximum of that quantity over the four inner taps (i, j in 0..1; fminf and fmaxf
 *     return the other operand for a NaN and order -0 below +0; the colours and moments of taps with n >= 1 are finite in a history these
 *     entries wrote).  nh = fmaxf(nh, 1.0f).  Then step 5 from n' = fminf(nh + 1.0f, (float)max_history) on.
 *   ANYTHING LESS - a tap outside the image or rejected: the bilinear step 4 on the four inner taps, exactly (Catmull-Rom weights
 *     renormalised over a partial footprint ring).  An image narrower or lower than 4 pixels therefore never takes the cubic arm.
 * RAYN_ERR_INVALID_ARG with the same last error texts for everything the two entries above reject, and for a NULL rp and resample > 1. */
int rayn_hip_temporal_accumulate_resample_device(rayn_ctx* ctx, const rayn_frame_params* p, const rayn_temporal_params* tp,
                                                 const rayn_temporal_resample_params* rp, const rayn_camera* prev_camera, float prev_time_start,
                                                 const float* d_color, const float* d_normal, const void* d_gbuffer_records,
                                                 const uint32_t* d_gbuffer_object, const void* d_prev_history, void* d_new_history,
                                                 size_t history_bytes, const void* d_prev_moments, void* d_new_moments, size_t moments_bytes,
                                                 float* d_out_color, void* hip_stream);

/* Variance-guided denoiser of a temporally accumulated Color: the passes of rayn_hip_denoise_variance_device on a variance estimated
 * from the moments above (SVGF, section 4.2).  Inputs: the accumulated colour c (3 floats per pixel, what the accumulate wrote to
 * d_out_color), the film's Alpha and WorldNormal, the frame's G-buffer objects obj, the NEW history (for the history length n' in plane A's
 * fourth component) and the NEW moments (m1, m2).  l_x = (0.2126f * c_x.r + 0.7152f * c_x.g) + 0.0722f * c_x.b.  Initial variance of pixel p:
 *   NOT GUIDED (it passes through all passes unchanged and is never a tap) when obj_p = 0xFFFFFFFF, c_p has a non-finite component, or
 *   n'_p >= 1 does not hold.
 *   Temporal estimate, when n'_p >= 4.0f (SVGF's threshold, fixed):  d = m2 - m1 * m1,  v = (d > 0 ? d : 0.0f) / n'_p - the variance of the
 *   accumulated mean, the meaning v has after a progressive render.  With a max_history below 4 this arm is never taken.
 *   Spatial estimate, when 1 <= n'_p < 4:  the 7x7 window at unit spacing around p in raster order, the centre included; a tap q counts
 *   when it is inside the image, obj_q == obj_p, n'_q >= 1 and c_q has three finite components:  k += 1.0f, s1 += l_q, s2 += l_q * l_q;
 *   mu = s1 / k, d = s2 / k - mu * mu, v = d > 0 ? d : 0.0f.
 *   A v that is not finite makes p not guided.
 * Then the passes, the outputs and the parameter ranges of rayn_hip_denoise_variance_device, unchanged.  This entry does NOT feed the
 * filtered colour back into the history (SVGF feeds its first pass back; rayn_hip_denoise_temporal_variance_feedback_device below does).
 * All f32, no contraction, IEEE division.
 * Enqueued on 'hip_stream' (NULL = the ctx's own stream; not waited for), on the ctx's GPU (devices[0] of a multi-device ctx).  DEVICE
 * pointers: d_color / d_normal 3 floats per pixel, d_alpha 1, d_gbuffer_object one u32, d_out_color 3, d_out_variance 1 (may be NULL);
 * d_history and d_moments 16-byte aligned, at least rayn_temporal_history_bytes / rayn_temporal_moments_bytes; d_scratch 16-byte aligned, at
 * least rayn_denoise_variance_scratch_bytes.  RAYN_ERR_INVALID_ARG with a last error text for: a zero-sized image or width * height >= 2^31,
 * iterations outside 1..8, a bad sigma, a NULL colour, object plane, history, moments, output or scratch, a NULL guide whose sigma is not 0,
 * too small a history, moments or scratch, a misaligned history, moments, object plane or scratch, and an output or the scratch overlapping
 * an input or each other.  The inputs are not modified. */
int rayn_hip_denoise_temporal_variance_device(rayn_ctx* ctx, uint32_t width, uint32_t height, uint32_t iterations, float sigma_luminance,
                                              float sigma_normal, float sigma_alpha, const float* d_color, const float* d_alpha,
                                              const float* d_normal, const uint32_t* d_gbuffer_object, const void* d_history, size_t history_bytes,
                                              const void* d_moments, size_t moments_bytes, float* d_out_color, float* d_out_variance,
                                              void* d_scratch, size_t scratch_bytes, void* hip_stream);

/* rayn_hip_denoise_temporal_variance_device with SVGF's feedback edge: the output of the FIRST a-trous pass is blended into the colour of
 * the history, so that the next frame's accumulate reprojects what this frame's filter cleaned.  The arguments of that entry, except that
 * d_history is in/out and that 'feedback' (beta) is the strength.  The records are packed and the 'iterations' passes run exactly as there:
 * for every beta, d_out_color and d_out_variance are bit for bit what that entry writes from the same inputs; the history write is a side
 * effect only.  All f32, no contraction, under either mul_add policy.
 *   beta == 0 writes nothing to the history: it is that entry (no c + 0 * x is evaluated, which would turn -0.0 into +0.0).
 *   beta > 0: take pass 0 - step 1, the pass that reads the packed records.  For every pixel p of the image, with c = p's colour in pass 0's
 *   input record (the accumulated colour d_color) and (c', v') what pass 0 computes for p:
 *     v' is NaN (p not guided on entry, or dropped by pass 0's overflow rule): the history is untouched.
 *     Otherwise, per component, d = c' - c, m = beta * d, fb = c + m.  If fb has three finite components, plane A of the history gets
 *     (fb.r, fb.g, fb.b) and its fourth component n' keeps its bits; if not, the history is untouched.
 *   Planes B, normal and object of the history are never written, nor are the moments (SVGF keeps raw moments too).  A history pixel with
 *   n' >= 1 keeps a finite colour.  With iterations == 1 pass 0 is also the last pass: it writes the planar outputs and the history.
 * RAYN_ERR_INVALID_ARG with a last error text for everything rayn_hip_denoise_temporal_variance_device rejects, for a beta that is not
 * finite or outside [0, 1], and for a history that overlaps anything else: it is an output here.  Nothing is written then. */
int rayn_hip_denoise_temporal_variance_feedback_device(rayn_ctx* ctx, uint32_t width, uint32_t height, uint32_t iterations, float sigma_luminance,
                                                       float sigma_normal, float sigma_alpha, const float* d_color, const float* d_alpha,
                                                       const float* d_normal, const uint32_t* d_gbuffer_object, void* d_history, size_t history_bytes,
                                                       const void* d_moments, size_t moments_bytes, float* d_out_color, float* d_out_variance,
                                                       void* d_scratch, size_t scratch_bytes, float feedback, void* hip_stream);

/* ---- guided upscaling (an EXTENSION: rayn renders at one resolution) -- Joint bilateral upsampling (Kopf et al., SIGGRAPH 2007) of a film
 * rendered at w x h to W x H = s * w x s * h, s = factor.  The guide is traced, not interpolated: the primary-hit G-buffer of the same
 * camera and time_start at both resolutions, BOTH under the low film's uploaded world (rayn_hip_gbuffer_device with p.width, p.height = w, h
 * and = W, H).  The factor keeps the aspect ratio, so the high pass shoots the pixel-centre rays of a camera built at W x H; its depth-0 hit
 * threshold (half_pixel_size, which the camera's own resolution sets) stays the low frame's, so both G-buffers describe the surface the
 * film's samples were shaded on and P - Pq below measures geometry, not the difference of two thresholds.  Geometry edges come out at the
 * high resolution and every rendered sample goes into shading noise.  Downstream of the film: the low film's planes are read, new planes
 * of the high size are written. */
typedef struct {
    uint32_t factor;      /* s, 1..8 */
    float sigma_plane;    /* the distance of the pixel's hit point from the tap's tangent plane, relative to the hit distance; 0 = off */
    float sigma_position; /* the distance between the two hit points, relative to the hit distance; 0 = off */
} rayn_upscale_params;
/* Inputs: the low film (planar Color 3 floats per pixel, Alpha 1, Background 3, WorldNormal 3, pixel x + y * w, rows bottom-up) with its
 * G-buffer (records (Pq, tq), objects oq), and the high G-buffer (records (P, t), objects o).  All arithmetic f32, no contraction under
 * either mul_add policy, IEEE '/', expf = dm_expf (rayn_detmath.h), dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z.  A sigma of 0 switches
 * its term off; any other must be finite and in [2^-30, 2^30].  Per high pixel (X, Y):
 *   1. Footprint: fx = ((float)X + 0.5f) / (float)s - 0.5f, x0f = floorf(fx), wx1 = fx - x0f, wx0 = 1.0f - wx1, and y likewise.  Taps
 *      k = 0..3 at (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) with b_k = wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1.  A tap is
 *      USABLE when it lies inside the low image, b_k > 0 and its Color has three finite components.
 *   2. Guided weights over the usable taps with oq == o (a miss, 0xFFFFFFFF, matches a miss).  A miss pixel: g_k = b_k.  A hit pixel:
 *      inv_t = 1.0f / (t + 1e-8f), d = P - Pq;  with sigma_plane != 0, dpl = fabsf(dot(nq, d)) * inv_t, nq the tap's WorldNormal as the
 *      film holds it (not normalised);  with sigma_position != 0, dps = dot(d, d) * (inv_t * inv_t);  e = (dpl * dpl) * kp + dps * ks with
 *      kp = 1.0f / (sigma_plane * sigma_plane), ks = 1.0f / (sigma_position * sigma_position), a term that is off left out (both off:
 *      e = 0);  g_k = b_k * dm_expf(-e), and a NaN g_k skips the tap.  Wg += g_k and, per component of every present plane, Sg += g_k * v_k,
 *      taps in the order above.  Every sum STARTS AT -0.0f, the identity of + for both zeros.
 *   3. Wg > 0: every component is Sg / Wg.  Else the same sums with g_k = b_k over ALL usable taps (Wb, Sb), and Wb > 0 gives Sb / Wb.
 *      Else the low pixel (min(X / s, w - 1), min(Y / s, h - 1)) (integer division) is copied verbatim, non-finite values included.
 *      d_out_weight (optional, one float per high pixel) receives Wg, and 0 where a fallback was taken.
 * The same weights serve all planes.  With factor == 1 a pixel with a finite Color comes out with the bits it went in with: fx = X, b_0 = 1,
 * the other taps fail b_k > 0, e = 0 or d = 0, dm_expf(-0) = 1, -0.0f + 1 * v = v and v / 1 = v.
 * 'width' and 'height' are the LOW film's.  A plane pointer (Alpha, Background, WorldNormal) may be NULL in input and output together: the
 * film lacks that channel, and it is neither read nor written.  DEVICE pointers; records 16-byte aligned.  Enqueued on 'hip_stream' (NULL =
 * the ctx's own stream; not waited for), on the ctx's GPU (devices[0] of a multi-device ctx); the inputs are not modified.
 * RAYN_ERR_INVALID_ARG with a last error text for: NULL up, a factor outside 1..8, a zero-sized image, W * H >= 2^31 or W or H above 2^23
 * (the pixel centres X + 0.5 must be exact in f32), a bad sigma, a NULL Color, a NULL G-buffer plane, a plane that is NULL on one side only,
 * a NULL WorldNormal with sigma_plane != 0, misaligned records or objects, and an output that overlaps an input or another output. */
int rayn_hip_upscale_device(rayn_ctx* ctx, uint32_t width, uint32_t height, const rayn_upscale_params* up, const float* d_color,
                            const float* d_alpha, const float* d_background, const float* d_normal, const void* d_low_records,
                            const uint32_t* d_low_object, const void* d_high_records, const uint32_t* d_high_object, float* d_out_color,
                            float* d_out_alpha, float* d_out_background, float* d_out_normal, float* d_out_weight, void* hip_stream);

/* ---- temporal supersampling (an EXTENSION: rayn renders at one resolution and every frame on its own) -- The guided upscaling above and
 * the temporal accumulate in ONE kernel whose history lives at the HIGH resolution W x H = s * w x s * h: temporal upsampling as in TAAU /
 * FSR2.  When every low frame is rendered with a different sub-pixel camera offset, over s * s frames every high pixel has had a low sample
 * at its own centre, and the history - the one place where samples of different frames meet - collects the detail no single-frame filter
 * can recover.  The kernel does not assume any particular offset: it finds each high pixel's footprint in the low film by projecting the
 * pixel's primary hit through the camera the low film was rendered with. */
typedef struct { uint32_t confidence; /* 0 off, 1 on */ } rayn_temporal_upscale_params;
/* Inputs: the low film and its G-buffer as rayn_hip_upscale_device takes them (p->width, p->height = w, h; WorldNormal is REQUIRED), the
 * high G-buffer (records (P, t), objects o) traced through the frame's own, unjittered camera, the previous HIGH history (NULL: none) with
 * that frame's camera and time_start, and low_camera: the camera the low film and the low G-buffer were traced through, or NULL.  All
 * arithmetic f32, no contraction under either mul_add policy, IEEE '/' and sqrtf; dot, cross and nz as for
 * rayn_hip_temporal_accumulate_device.  Per high pixel (X, Y):
 *   A. Footprint in the low film.  Default: step 1 of rayn_hip_upscale_device, fx = ((float)X + 0.5f) / (float)s - 0.5f and y likewise.
 *      With low_camera != NULL and o != 0xFFFFFFFF: P through low_camera at ts = p->time_start by exactly step 3 of
 *      rayn_hip_temporal_accumulate_device with the LOW width and height (no object-motion shift: both G-buffers belong to one instant);
 *      its fx, fy are taken unless the projection is rejected or not finite, which keeps the default.  A miss pixel always keeps the
 *      default, so under a jittered low camera its Background is registered less than one low pixel off.  Then x0f = floorf(fx),
 *      wx1 = fx - x0f, wx0 = 1.0f - wx1, y likewise, and x0, y0 by step 4's clamp to [-2, 2^31].  (Here and in C an implementation may
 *      clamp at any bound from 2^23 up - the kernel takes 2^24, which fits an int: W and H are at most 2^23, so every such origin is
 *      outside the image and no result changes.)
 *   B. This frame's value: steps 2 and 3 of rayn_hip_upscale_device on the taps k = 0..3 of that footprint - the same tier order, sums
 *      that start at -0.0f and tap order; tier 3 is the verbatim low pixel (min(X / s, w - 1), min(Y / s, h - 1)) - for every present
 *      plane.  c = the Color, nrm = the WorldNormal; Alpha, Background and WorldNormal go to their outputs and d_out_weight gets Wg, or 0.
 *      conf = 1.0f when confidence == 0 and in tier 3; otherwise conf = the largest b_k over the taps that were ADDED to the sums of the
 *      tier that produced the value (fmaxf from 0.0f): a high pixel whose centre a low sample hit exactly has conf = 1, one in the middle
 *      of four low samples 0.25.
 *   C. Steps 1 to 5 of rayn_hip_temporal_accumulate_device at W x H with c and nrm from B, the high G-buffer, the previous history,
 *      prev_camera at prev_time_start, p->time_start and the uploaded world's hitable velocities, where step 5 reads
 *      n' = fminf(nh + conf, (float)max_history), a = conf / n', out = h + a * (c - h).  A reset keeps n' = 1 (0 for a non-finite c), so
 *      that "n_tap >= 1" keeps its meaning.  New history: A' = (out, n'), B' = (P, t), (nrm, 0) and o.
 * With low_camera == NULL and confidence == 0 every output and the new history are bit for bit those of rayn_hip_upscale_device followed
 * by rayn_hip_temporal_accumulate_device at the high size.  Moments, Catmull-Rom resampling and feedback are not part of this entry.
 * d_out_color: the ACCUMULATED colour, 3 floats per high pixel; d_out_alpha, d_out_background (NULL together with their inputs) and
 * d_out_normal: this frame's upscaled planes; d_out_weight may be NULL.  history_bytes: the size of EACH history, at least
 * rayn_temporal_history_bytes(W, H).  DEVICE pointers, records and histories 16-byte aligned; enqueued on 'hip_stream' (NULL = the ctx's
 * own stream; not waited for), on the ctx's GPU (devices[0] of a multi-device ctx).  RAYN_ERR_INVALID_ARG with a last error text, and
 * nothing written, for: everything rayn_hip_upscale_device and rayn_hip_temporal_accumulate_device reject for the same arguments (the
 * latter at the high size), a NULL WorldNormal, a NULL sp, confidence > 1, an unknown kind of either camera, a history smaller than
 * rayn_temporal_history_bytes(W, H) or misaligned, and a history that overlaps the other history, an input or an output plane.  The
 * inputs and the previous history are not modified. */
int rayn_hip_temporal_upscale_device(rayn_ctx* ctx, const rayn_frame_params* p, const rayn_upscale_params* up, const rayn_temporal_params* tp,
                                     const rayn_temporal_upscale_params* sp, const rayn_camera* low_camera, const rayn_camera* prev_camera,
                                     float prev_time_start, const float* d_color, const float* d_alpha, const float* d_background,
                                     const float* d_normal, const void* d_low_records, const uint32_t* d_low_object, const void* d_high_records,
                                     const uint32_t* d_high_object, const void* d_prev_history, void* d_new_history, size_t history_bytes,
                                     float* d_out_color, float* d_out_alpha, float* d_out_background, float* d_out_normal, float* d_out_weight,
                                     void* hip_stream);

/* ---- preview integrator (an EXTENSION: rayn has one integrator, the path tracer) -- An image of the geometry alone - primary hit,
 * viewer-facing normal and ambient occlusion, a "clay" render - at a small fraction of the film's cost: for placing a camera inside a
 * fractal, for checking an animation's motion before paying for the render, and as an AO AOV.  It runs beside the film path and shares none
 * of its state: the primary hit is the G-buffer pass above, the occlusion of the TracedSDFs goes through the scene's PRODUCT shadow-march
 * kernel (the kernel rayn_hip_probe_shadow runs).
 *
 * Definition.  All arithmetic f32 under the ctx's mul_add policy where the film's own functions honour it (dot, mag_sq, cross,
 * concentric_circle_map, the MandelBox fold); a product and a sum written out below are a separate multiply and add.  For pixel
 * p = x + y * width, bottom-up rows:
 *   1. Primary hit: exactly the G-buffer pass - same ray (direction d), same product extend kernel at depth 0, same record (P, t) and object
 *      index: the records and objects are bit for bit those of rayn_hip_gbuffer_device for the same p.  Every closure time is p->time_start (ts).
 *   2. Background: a miss, or a hit object whose material kind is Sky: colour (0, 0, 0), alpha 0, normal (0, 0, 0), ao 1.  Every other pixel is
 *      a surface with alpha 1.
 *   3. Surface normal at depth 0 as the shade stage takes it (src/sphere.rs:73-86, src/sdf.rs:85-101), h the hit object: a Sphere has
 *      n = normalized(P - center(h, ts)) and offset = 0; a TracedSDF has hps = max(0.0001f, sdf_detail_scale * half_pixel_size_at(t)) - the
 *      depth-0 threshold closure of src/film.rs:540-551 - n = the tetrahedron normal (sdfu normals_fast) of the SDF at P - center(h, ts) with
 *      epsilon hps, four distance evaluations with the MandelBox scale taken at ts, and offset = hps.
 *   4. Viewer side: wo = -d, nf = n * signum(dot(n, wo)).
 *   5. AO rays, k = 0..K-1 with K = samples: u = fract(s[k].x + r_p), v = fract(s[k].y + r_p), s the caller's table of K float pairs
 *      (d_samples) and r_p the pixel's entry of the caller's scramble table (d_scramble: one float per pixel in the layout of the scramble
 *      builder below; NULL: r_p = 0); l = cosine_weighted_in_hemisphere(u, v) (src/math.rs:99-103); w = c0 * l.x + c1 * l.y + c2 * l.z with
 *      (c0, c1, c2) = get_orthonormal_basis(nf) (src/math.rs:49-59); a = P + nf * offset, b = a + w * radius;
 *      vis_k = HitableStore::test_occluded(a, b) (src/hitable.rs:164-168) at ts: the analytic spheres in index order, the TracedSDFs through
 *      the product shadow-march kernel.  A segment a sphere occludes is not marched; a scene without a TracedSDF launches no march.
 *   6. Resolve: ao = (float)(number of k with vis_k == 1) / (float)K - an integer count, independent of order;
 *      hl = ambient + (1.0f - ambient) * max(0.0f, dot(nf, wo)); colour = ao * hl in all three channels; the normal output is nf.
 * The AO rays are parked, marched and counted in rounds of 8, which bounds the scratch and changes no result. */
typedef struct {
    uint32_t samples; /* K: AO rays per pixel, 1..64 */
    float radius;     /* length of an AO ray in world units; finite, > 0 */
    float ambient;    /* the part of the headlight term that does not depend on the view angle; in [0, 1] */
} rayn_preview_params;
/* Bytes of device scratch the entry needs for a width x height image with `samples` AO rays per pixel: the G-buffer pass's scratch, 32 bytes
 * and 29 * min(samples, 8) bytes per pixel of the image rounded up to a multiple of 64 pixels (0 for a size it rejects and for samples
 * outside 1..64).  Host only; needs no GPU. */
size_t rayn_preview_scratch_bytes(uint32_t width, uint32_t height, uint32_t samples);
/* Enqueue the preview on 'hip_stream' (NULL = the ctx's own stream; not waited for) for the uploaded world and p (its resolution, time_start,
 * max_marches, max_vis_marches, sdf_detail_scale, world_radius), on the ctx's GPU (devices[0] of a multi-device ctx).  DEVICE pointers.
 * Outputs in the film's and the G-buffer's layouts, so that the save_to, display, denoise and temporal entries take them unchanged:
 * d_out_color and d_out_normal 3 floats per pixel, d_out_alpha 1; d_out_ao (1 float per pixel), d_out_records (16 bytes per pixel, 16-byte
 * aligned) and d_out_object (one u32 per pixel) may each be NULL.  d_samples: 2 * samples floats, 8-byte aligned.  d_scratch: 16-byte
 * aligned, at least the byte count above.  Like a render it replaces the context's device scene.  RAYN_ERR_INVALID_ARG with a last error text,
 * and nothing written, for: a NULL p or pp, a zero-sized image or width * height >= 2^31, samples outside 1..64, a radius that is not finite
 * and > 0, an ambient outside [0, 1], a NULL d_samples, colour, alpha, normal or scratch, a misaligned buffer, too little scratch, buffers
 * that overlap, and no uploaded world. */
int rayn_hip_preview_device(rayn_ctx* ctx, const rayn_frame_params* p, const rayn_preview_params* pp, const float* d_samples,
                            const float* d_scramble, float* d_out_color, float* d_out_alpha, float* d_out_normal, float* d_out_ao,
                            void* d_out_records, uint32_t* d_out_object, void* d_scratch, size_t scratch_bytes, void* hip_stream);

/* ---- frame generation (an EXTENSION: rayn renders every frame) -- Motion-compensated interpolation of a frame T of a sequence from two
 * RENDERED key frames A and B around it.  Unlike a 2-D optical-flow interpolator it knows the exact geometry of T - its own primary-hit
 * G-buffer, which costs a fiftieth of the render - and therefore which of the two keys sees each point: a point visible in one key only is
 * taken from that key alone, which a cross-fade cannot do.  Downstream of the film: the keys' planes are read, new planes are written. */
typedef struct {
    float depth_tolerance; /* a tap's recorded hit distance may differ from the projected one by this fraction of it; finite, >= 0 */
} rayn_interpolate_params;
/* One key frame: its film planes (planar, pixel x + y * width, rows bottom-up: Color 3 floats per pixel, Alpha 1, Background 3, WorldNormal
 * 3), its G-buffer (16-byte records (P, t), u32 objects; rayn_hip_gbuffer_device at the key's time_start), the camera it was rendered
 * through and its time_start.  DEVICE pointers, except `camera`. */
typedef struct {
    const float* d_color;
    const float* d_alpha;
    const float* d_background;
    const float* d_normal;
    const void* d_records;
    const uint32_t* d_object;
    const rayn_camera* camera;
    float time_start;
} rayn_interpolate_key;
/* Inputs: the keys A (time_start ta) and B (tb), and T's G-buffer (records (P, t), objects o) traced with p->time_start = ts under the same
 * uploaded world; p gives the resolution and ts.  ta < tb and ta <= ts <= tb, all finite.  All arithmetic f32, no contraction under either
 * mul_add policy, IEEE '/' and sqrtf; dot, cross and nz as for rayn_hip_temporal_accumulate_device; every sum STARTS AT -0.0f as in
 * rayn_hip_upscale_device.  s = (ts - ta) / (tb - ta), wB = s, wA = 1.0f - s.  Per pixel (X, Y) of T and for each key K in (A, B):
 *   1. Position in the key.  A hit pixel (o != 0xFFFFFFFF): Pp = P - center_vel * (ts - tK) when hitable o has animated != 0, else P - step
 *      2 of the accumulate with the sign as written, so that for B the point moves forward - then step 3 of the accumulate through K's
 *      camera at tK gives fx, fy, te; a rejected or non-finite projection gives key K no taps.  A miss pixel: fx = (float)X, fy = (float)Y
 *      and no depth: the key's own pixel is the only tap that can count.  scale_vel morphing is not reprojected; the depth test catches it.
 *   2. Taps.  x0f = floorf(fx), wx1 = fx - x0f, wx0 = 1.0f - wx1, y likewise, x0, y0 by step 4's clamp; the taps (x0, y0), (x0 + 1, y0),
 *      (x0, y0 + 1), (x0 + 1, y0 + 1) with b = wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1.  A tap counts when it lies inside the image,
 *      b > 0, the key's object there equals o (a miss matches a miss), for a hit pixel fabsf(t_tap - te) <= depth_tolerance * te, and the
 *      key's Color there has three finite components - tested in that order, a NaN fails every comparison:  W_K += b and, per component
 *      of every present plane, S_K += b * v_tap.
 *   3. Tier 1.  valid_K = W_K > 0, v_K = S_K / W_K.  Both valid: out = v_A * wA + v_B * wB per component, two multiplies and one add.
 *      Only A valid: out = v_A; only B valid: out = v_B.  This is the arm that knows about occlusion.
 *   4. Tier 2, neither key has a tap (the point is hidden or off screen in both).  A key's own pixel (X, Y) is usable when its Color is
 *      finite.  Both usable: the same blend on the verbatim pixels.  One usable: that pixel verbatim.  Neither: key A's pixel verbatim
 *      when wA >= wB, else key B's; non-finite values are copied as they are.
 *   5. d_out_source (optional, one u32 per pixel): the arm that produced the pixel - 0 both keys in tier 1, 1 A only, 2 B only, 3 the
 *      tier-2 blend, 4 a tier-2 single or verbatim pixel.
 * With ts == ta a pixel that finds its taps in A (a static camera and object: its own pixel with b = 1) and taps in B comes out as
 * v_A * 1 + v_B * 0: A's bits for finite values.
 * Alpha, Background and WorldNormal may each be NULL in A, B and the output together: the film lacks that channel, and it is neither
 * read nor written.  Color is required.  Records 16-byte aligned, objects and d_out_source 4-byte aligned.  Enqueued on 'hip_stream'
 * (NULL = the ctx's own stream; not waited for), on the ctx's GPU (devices[0] of a multi-device ctx); hitable motion comes from the
 * uploaded world at the time of the call; the inputs are not modified.  RAYN_ERR_INVALID_ARG with a last error text, and nothing written,
 * for: a NULL p, ip or key, a NULL camera, Color, record or object plane, a plane that is NULL on one side only, an unknown camera kind, a
 * zero-sized image or width * height >= 2^31, times that break the rule above, a non-finite or negative depth_tolerance, misaligned
 * records or objects, an output that overlaps an input or another output, and no uploaded world. */
int rayn_hip_interpolate_device(rayn_ctx* ctx, const rayn_frame_params* p, const rayn_interpolate_params* ip, const rayn_interpolate_key* key_a,
                                const rayn_interpolate_key* key_b, const void* d_gbuffer_records, const uint32_t* d_gbuffer_object,
                                float* d_out_color, float* d_out_alpha, float* d_out_background, float* d_out_normal, uint32_t* d_out_source,
                                void* hip_stream);

/* ---- PNG encoding on the device (an EXTENSION: rayn encodes on the host) -- The zlib stream of a PNG's IDAT chunk from the 8-bit image
 * rayn_hip_save_to_pixels_device / rayn_hip_display_pixels_device write (rows top-down, bpp in {1, 3, 4} bytes per pixel), so that a
 * sequence copies a compressed stream to the host and not the raw image.  Integer arithmetic only; tests/png_np.py restates it and the
 * kernels agree with it byte for byte.  Any inflate accepts the stream.
 *   Filtering.  Per row the five PNG filters None, Sub, Up, Average, Paeth (types 0..4; the row above the first is zeros, the bytes left
 *     of the first pixel are zeros) are evaluated; the row takes the type with the smallest sum of |int8(filtered byte)|, the lowest type
 *     on a tie.  The filtered stream R is h rows of 1 + w * bpp bytes: the type, then the filtered row.  n = h * (1 + w * bpp).
 *   Blocks.  R is cut into blocks of 32768 bytes (the last may be shorter); every block is encoded on its own.
 *   Tokens.  A maximal run of L equal bytes inside a block (runs never cross a block start): the first byte is a literal; of the r = L - 1
 *     others, matches (distance 1) of length 258 while r >= 258, then one match of length r if r >= 3, else r literals.
 *   Code.  Frequencies over the 286 literal/length symbols, end-of-block counting 1.  Code lengths are the depths of the Huffman tree built
 *     by repeatedly merging the two smallest nodes ordered by (weight, index): a leaf's index is its symbol, internal nodes take 286, 287,
 *     ... in creation order (the two-queue construction over the leaves sorted by (weight, symbol), a leaf before an internal node of
 *     equal weight).  While a length exceeds 15 every non-zero frequency f becomes (f + 1) >> 1 and the tree is rebuilt.  Codes are the
 *     canonical codes of RFC 1951 3.2.2.
 *   A Huffman block.  A header of 1222 bits: BFINAL, BTYPE = 2, HLIT = 29, HDIST = 0, HCLEN = 15; the 19 code-length code lengths in the
 *     RFC's order, 4 for the symbols 0..15 and 0 for 16..18 (a complete code: symbol k has the 4-bit code k); the 286 literal/length code
 *     lengths, each as its 4-bit code; the length of the one distance code, 1 if the block has a match, else 0.  Then the tokens - a match
 *     is its length code, its extra bits and the 1-bit distance code 0 - and end-of-block.
 *   Stored fallback.  If that encoding, rounded up to bytes, is not shorter than len + 5 bytes the block is a stored block instead
 *     (BTYPE = 0: one byte BFINAL, LEN, NLEN, the bytes): no block exceeds len + 5 bytes plus its alignment.
 *   Alignment.  Every Huffman block but the final one is followed by an empty stored block: the bits 000, zero padding to the byte, 00 00
 *     FF FF.  The final block is zero-padded.  So every block starts on a byte.
 *   Stream.  78 01, the blocks, the big-endian Adler-32 of R.
 *   Output.  Four little-endian words - the bytes of the zlib stream, n, the number of blocks, the number of stored blocks - then the
 *     zlib stream from byte 16 on, contiguous; the 4-byte word holding its last byte is zero-padded and nothing behind it is written.
 * rayn_png_stream_bound: the bytes d_out must have: 16 + 2 + n + 10 per block + 4, rounded up to 16 (a block is at most len + 5 bytes, its
 * alignment at most 5).  rayn_png_scratch_bytes: the bytes of d_scratch (R, the blocks before their compaction, their sizes).  Both host
 * only, needing no GPU; 0 for a geometry the encoder rejects. */
size_t rayn_png_stream_bound(uint32_t width, uint32_t height, uint32_t bpp);
size_t rayn_png_scratch_bytes(uint32_t width, uint32_t height, uint32_t bpp);
/* Enqueue the encoder on 'hip_stream' (NULL = the ctx's own stream; not waited for), on the ctx's GPU (devices[0] of a multi-device ctx).
 * DEVICE pointers: d_img width * height * bpp bytes, not modified; d_out and d_scratch 16-byte aligned, of at least the byte counts above.
 * RAYN_ERR_INVALID_ARG with a last error text, and nothing written, for: a zero-sized image, a bpp other than 1, 3, 4, a row of more
 * than 2^24 filtered bytes or n >= 2^31 (32-bit offsets), a NULL buffer, a misaligned or too small d_out or d_scratch, d_out == d_img and
 * buffers that overlap. */
int rayn_hip_png_encode_device(rayn_ctx* ctx, uint32_t width, uint32_t height, uint32_t bpp, const uint8_t* d_img, void* d_out, size_t out_bytes,
                               void* d_scratch, size_t scratch_bytes, void* hip_stream);

/* ---- PNG encoding on the device, with LZ77 matches (an EXTENSION) -- A second encoder behind the same interface, whose tokens are
 * literals and LZ77 matches at any distance inside the block.  Integer arithmetic only; tests/png_lz_np.py restates it and the kernels
 * agree with it byte for byte.  Unchanged from rayn_hip_png_encode_device: the filtering and the filtered stream R, the 32768-byte blocks
 * encoded each on its own, the stored fallback at >= len + 5 bytes, the alignment block behind every Huffman block but the final one,
 * 78 01, the Adler-32, the four header words, and rayn_png_stream_bound, which bounds the output.  New, per block B[0..len), with S the
 * row stride 1 + w * bpp:
 *   Candidates at position i.  A distance d is a candidate only if i - d >= 0: no match reaches before the block start.  d = 1.
 *     d = i - prev(i), where prev(i) is the largest j < i with B[j..j+3) == B[i..i+3), defined only when i + 3 <= len (exact byte
 *     equality; there is no hash).  d = S, the row above, if S != 0.
 *   Match length.  m(i, d) is the largest L <= min(258, len - i) with B[i-d+k] == B[i+k] for all k < L; the two ranges may overlap.
 *   Best match.  M(i) is the maximum of m(i, d) over the candidates, D(i) the smallest d that reaches it.  A match needs M >= 3, and a
 *     match of length 3 at D > 4096 is not taken.
 *   Parse.  Greedy from p = 0: the match (M(p), D(p)) and p += M(p), otherwise the literal B[p] and p += 1.  No lazy evaluation.
 *   Codes.  The literal/length code is the construction above over 286 symbols, end-of-block counting 1.  The distance code is the same
 *     construction over the 30 distance symbols of RFC 1951 3.2.5: leaves indexed by symbol, internal nodes 30, 31, ... in creation order,
 *     frequencies halved - independently of the other tree - while a length exceeds 15.  With fewer than two distance symbols in use
 *     the used one gets length 1 and every other length is 0; with none in use symbol 0 gets length 1 (the one incomplete code RFC 1951
 *     and zlib accept).
 *   A Huffman block.  A header of 1338 bits: BFINAL, BTYPE = 2, HLIT = 29, HDIST = 29, HCLEN = 15; the 19 code-length code lengths as
 *     above; the 286 + 30 code lengths, each as its 4-bit code.  Then the tokens - a match is its length code, its extra bits, its
 *     distance code and its extra bits - and end-of-block.
 * rayn_png_scratch_bytes_lz77: the bytes of d_scratch (rayn_png_scratch_bytes and 65536 per block for the match finder's sort).  Host
 * only; 0 for a geometry the encoder rejects.  The entry takes rayn_hip_png_encode_device's arguments and rejects the same inputs. */
size_t rayn_png_scratch_bytes_lz77(uint32_t width, uint32_t height, uint32_t bpp);
int rayn_hip_png_encode_lz77_device(rayn_ctx* ctx, uint32_t width, uint32_t height, uint32_t bpp, const uint8_t* d_img, void* d_out, size_t out_bytes,
                                    void* d_scratch, size_t scratch_bytes, void* hip_stream);
/* The deflate stage of that encoder alone, on n bytes of the caller's at d_data (a DEVICE pointer of any alignment, not modified), which
 * take R's place; stride takes S's (0: no row candidate; any other value is a distance like S).  d_out receives the same four header
 * words and the zlib stream of d_data: a zlib writer for device buffers.  rayn_deflate_stream_bound(n): the bytes d_out must have,
 * 16 + 2 + n + 10 per 32768-byte block + 4, rounded up to 16; rayn_deflate_scratch_bytes(n): the bytes of d_scratch.  Both host only; 0
 * for n == 0 and n >= 2^31.  Enqueued on 'hip_stream' like the encoder.  RAYN_ERR_INVALID_ARG with a last error text, and nothing
 * written, for: n == 0 or n >= 2^31 (32-bit offsets), a NULL buffer, a misaligned (16 bytes) or too small d_out or d_scratch, d_out ==
 * d_data and buffers that overlap. */
size_t rayn_deflate_stream_bound(size_t n);
size_t rayn_deflate_scratch_bytes(size_t n);
int rayn_hip_deflate_lz77_device(rayn_ctx* ctx, const void* d_data, size_t n, uint32_t stride, void* d_out, size_t out_bytes, void* d_scratch,
                                 size_t scratch_bytes, void* hip_stream);

/* ---- OpenEXR scanline chunks with ZIP compression on the device (an EXTENSION: rayn writes no EXR) -- The chunks of a single-part
 * scanline OpenEXR file (compression ZIP, 16 rows per chunk, lineOrder INCREASING_Y) from planes in the film's layout, so that one file
 * per frame carries the float film.  Written from the published file layout; integer arithmetic only; tests/exr_np.py restates it and
 * the kernels agree with it byte for byte.  Conformance with real OpenEXR readers is unpinned: no OpenEXR library was at hand.
 *   Input.  1..16 channels, in the file's order (names ascending byte-wise: the host checks that).  Channel c of pixel p = x + y * width
 *     (rows bottom-up, as the film stores them) is the 32-bit word plane_c[p * stride_c + offset_c]; layout holds (stride, offset, type)
 *     per channel.  type 2 FLOAT and type 0 UINT: the word as it is, size 4.  type 1 HALF: the f32 converted to binary16, size 2.
 *   f32 to half.  Round to nearest even; half denormals are produced; a magnitude >= 65520 becomes the infinity of its sign; the sign of
 *     zero is kept; a magnitude <= 2^-25, f32 denormals included whatever the build's denormal mode, becomes the zero of its sign.  A
 *     NaN becomes sign | 0x7C00 | (mantissa >> 13), with the lowest bit set when that field is 0: a signalling NaN is not quieted.
 *   Rows.  The file's row y is the film's row height - 1 - y.  A row's bytes: for each channel in order its width values, little-endian.
 *     S = width * (sum of the sizes) bytes, always even.
 *   Chunks.  Chunk k covers the rows 16k .. min(16k + 16, height) - 1; RAW_k is those rows concatenated, n_k = S * rows bytes.
 *   Pre-process.  T: the bytes of RAW_k at even indices, then those at odd indices.  P[0] = T[0], P[i] = (T[i] - T[i-1] + 128) & 255.
 *   Deflate.  Z_k is the zlib stream of P_k in the block format above: matches == 0 the run-length blocks of
 *     rayn_hip_png_encode_device, matches == 1 the LZ77 blocks of rayn_hip_deflate_lz77_device with the row candidate's distance S / 2.
 *     Blocks of 32768 bytes restart at every chunk's start; the stored fallback per block, the alignment block behind every Huffman
 *     block but the chunk's last, 78 01 and the chunk's own Adler-32 are unchanged.
 *   Raw fallback.  If Z_k has n_k bytes or more the chunk's payload is RAW_k itself, not pre-processed; else it is Z_k.  A reader tells
 *     the two apart by size == n_k.
 *   Output.  Four little-endian words - the bytes of the body, the chunks, the raw chunks, the deflate blocks (32768-byte blocks over all
 *     chunks, the raw ones included) - then one word per chunk, where it starts in the body; zeros up to a multiple of 16; then the
 *     body, contiguous: per chunk the i32 y = 16k, the i32 payload size, the payload.  The 4-byte word holding the body's last byte is
 *     zero-padded and nothing behind it is written.  rayn_amd.image.exr_from_chunks makes the file of it.
 * rayn_exr_stream_bound: the bytes d_out must have, align16(16 + 4 * chunks) + align16(sum of 8 + n_k): exact, a payload never exceeds
 * n_k.  rayn_exr_scratch_bytes: the bytes of d_scratch (P, RAW, the blocks before their compaction, their sizes; with matches == 1 65536
 * more per block).  layout: n_channels * 3 words on the host.  Both host only; 0 for what the entry rejects. */
size_t rayn_exr_stream_bound(uint32_t width, uint32_t height, uint32_t n_channels, const uint32_t* layout);
size_t rayn_exr_scratch_bytes(uint32_t width, uint32_t height, uint32_t n_channels, const uint32_t* layout, uint32_t matches);
/* Enqueue the encoder on 'hip_stream' (NULL = the ctx's own stream; not waited for), on the ctx's GPU.  d_planes: n_channels DEVICE
 * pointers in an array on the HOST, read before the call returns, like layout; the planes are not modified.  d_out and d_scratch: DEVICE,
 * 16-byte aligned, of at least the byte counts above.  A fixed number of launches whatever the height.  RAYN_ERR_INVALID_ARG with a last
 * error text, and nothing written, for: a zero-sized image, 0 or more than 16 channels, a type other than 0, 1, 2, a stride of 0 or an
 * offset >= the stride, 16 * S >= 2^31 or a bound >= 2^31 (32-bit offsets), matches > 1, a NULL buffer or plane, a misaligned or too
 * small d_out or d_scratch, and an output or scratch that overlaps a plane or the other. */
int rayn_hip_exr_encode_device(rayn_ctx* ctx, uint32_t width, uint32_t height, uint32_t n_channels, const void* const* d_planes,
                               const uint32_t* layout, uint32_t matches, void* d_out, size_t out_bytes, void* d_scratch, size_t scratch_bytes,
                               void* hip_stream);

/* ---- Baseline JPEG scans on the device (an EXTENSION: rayn writes PNG only) -- The entropy-coded scan of a baseline sequential DCT JPEG
 * (SOF0, 8 bits, JFIF) from the 8-bit image rayn_hip_save_to_pixels_device / rayn_hip_display_pixels_device write (rows top-down, bpp in
 * {1, 3} bytes per pixel), so that a sequence can leave lossy stills and a Motion-JPEG file.  Integer arithmetic only; tests/jpeg_np.py
 * restates it and the kernels agree with it byte for byte; libjpeg decodes the files (tests/test_jpeg.py).
 *   Components.  bpp 1: one component, the byte is Y.  bpp 3: Y, Cb, Cr (ids 1, 2, 3).  subsampling 0 is 4:4:4 (8x8 MCU: Y Cb Cr, or Y
 *     alone); 1 is 4:2:0 (16x16 MCU: Y00 Y01 Y10 Y11 Cb Cr, Y01 the right neighbour), bpp 3 only.  The image is padded to whole MCUs by
 *     replicating its last column and row, before conversion and downsampling.
 *   Colour (int32, >> arithmetic).  Y = (19595 R + 38470 G + 7471 B + 32768) >> 16; Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767)
 *     >> 16; Cr = (32768 R - 27439 G - 5329 B + 8388608 + 32767) >> 16.  4:2:0 chroma: (a + b + c + d + 2) >> 2 of the 2x2 converted values.
 *   Transform.  s = sample - 128.  K = {4096, 4017, 3784, 3406, 2896, 2276, 1567, 799} = round(4096 cos(k pi / 16)); T[0][x] = 2896, and
 *     for u >= 1 T[u][x] = +-K[k] with cos((2x+1) u pi / 16) = +-cos(k pi / 16).  Rows: a[y][u] = (sum_x T[u][x] s[y][x] + 1024) >> 11.
 *     Columns: F[v][u] = sum_y T[v][y] a[y][u], the coefficient times 2^15.
 *   Quantisation.  The base tables of ITU T.81 Annex K.1 (Y) and K.2 (Cb, Cr); scale = 5000 / quality below 50, else 200 - 2 quality;
 *     Q = clamp((base * scale + 50) / 100, 1, 255).  m = (|F| + Q * 16384) / (Q * 32768) with F's sign: ties away from zero.  Zigzag order.
 *   Entropy code.  The Huffman tables of Annex K.3 - K.6.  DC: the category bit_length(|d|) of the difference d to the previous block of
 *     the component, then that many bits of d (d + 2^s - 1 when negative).  AC: the code of (run << 4) | size, then the bits; 0xF0 per 16
 *     zeros in front of a non-zero value; 0x00 iff the block ends in zeros.  Bits most significant first; 00 behind every FF byte.
 *   Restart intervals.  Segment k is the MCUs [k Ri, min((k + 1) Ri, total)) in raster order, not cut at row ends; predictors start at 0;
 *     every segment is padded to a byte with 1 bits (an FF made that way is stuffed too); FF D0+(k mod 8) stands between segments k and
 *     k + 1, nothing behind the last.
 *   Output.  Four little-endian words - the bytes of the scan, the segments, the restart interval, the blocks - then the scan with its
 *     markers from byte 16 on, contiguous; the 4-byte word holding its last byte is zero-padded and nothing behind it is written.
 *     rayn_amd.image.jpeg_from_scan makes the file of it.
 * rayn_jpeg_scan_bound: the bytes d_out must have: 16 + per segment of n MCUs 2 * ceil(n * mcu_bits / 8) + 2 per marker, rounded up to 16,
 * where a luminance block is at most 1658 bits and a chrominance block 1660 (the tables' longest codes: csrc/jpeg.h has the derivation)
 * and the factor 2 is the stuffing.  rayn_jpeg_scratch_bytes: the bytes of d_scratch (coefficients, block sizes, the segments before and
 * after the stuffing).  rayn_jpeg_quant_table: the 64 scaled entries of table `which` (0 Y, 1 chroma) at `quality`, in zigzag order as a
 * DQT segment holds them.  rayn_jpeg_huffman_table: BITS into bits[16] and the first min(n, count) HUFFVAL into vals of table `which`
 * (0 DC Y, 1 AC Y, 2 DC chroma, 3 AC chroma: 2 * id + class); returns the count (12 or 162), -1 for a bad argument.  All host only,
 * needing no GPU; the sizes are 0 for a geometry the encoder rejects. */
size_t rayn_jpeg_scan_bound(uint32_t width, uint32_t height, uint32_t bpp, uint32_t subsampling, uint32_t restart_interval);
size_t rayn_jpeg_scratch_bytes(uint32_t width, uint32_t height, uint32_t bpp, uint32_t subsampling, uint32_t restart_interval);
int rayn_jpeg_quant_table(uint32_t quality, uint32_t which, uint8_t* out);
int rayn_jpeg_huffman_table(uint32_t which, uint8_t* bits, uint8_t* vals, uint32_t n);
/* Enqueue the encoder on 'hip_stream' (NULL = the ctx's own stream; not waited for), on the ctx's GPU.  DEVICE pointers: d_img width *
 * height * bpp bytes, not modified; d_out and d_scratch 16-byte aligned, of at least the byte counts above.  Four launches and no memset,
 * whatever the size.  RAYN_ERR_INVALID_ARG with a last error text, and nothing written, for: a zero-sized image or a side above 65535, a
 * bpp other than 1, 3, a subsampling other than 0, 1 or 1 with bpp 1, a restart_interval outside 1..65535, a bound >= 2^31 (32-bit
 * offsets), a quality outside 1..100, a NULL buffer, a misaligned or too small d_out or d_scratch, d_out == d_img and buffers that overlap. */
int rayn_hip_jpeg_encode_device(rayn_ctx* ctx, uint32_t width, uint32_t height, uint32_t bpp, uint32_t quality, uint32_t subsampling,
                                uint32_t restart_interval, const uint8_t* d_img, void* d_out, size_t out_bytes, void* d_scratch,
                                size_t scratch_bytes, void* hip_stream);

/* ---- host-side table builders (the a1/a3/a4 rows of SURVEY.md section 8) ------------------ */
/* 1 + requested_1d_sample_sets(), 2 + requested_2d_sample_sets() (src/film.rs:431-432,
 * src/integrator.rs:39-45). */
uint32_t rayn_sets_1d(uint32_t max_bounces, uint32_t volume_marches);
uint32_t rayn_sets_2d(uint32_t max_bounces, uint32_t volume_marches);
/* Samples::new_rd(spp, sets_1d, sets_2d, frame), src/sampler.rs:18-37. */
int rayn_build_rd_tables(uint32_t spp, uint32_t sets_1d, uint32_t sets_2d, uint64_t frame,
                         float* samples_1d, float* samples_2d);
/* SmallRng::seed_from_u64(x + y*width).gen::<f32>() for every pixel, src/film.rs:460-461. */
int rayn_build_scramble(uint32_t width, uint32_t height, float* scramble);
/* FilterImportanceSampler::new(&F::new(..)), src/filter.rs:187-220, for the reference's four Filter
 * implementations (src/filter.rs:12-49 BlackmanHarris, :51-108 MitchellNetravali(radius, b, c),
 * :110-140 Box, :142-185 LanczosSinc(radius, tau)).  rayn_build_fis_table takes the two
 * parameter-free kinds; _ex takes all four (param0/param1 = b/c for Mitchell, tau/unused for
 * Lanczos).  The sampler assumes a filter without negative lobes (src/filter.rs:194-195); like
 * the reference the builder does not check that. */
enum { RAYN_FILTER_BLACKMAN_HARRIS = 0, RAYN_FILTER_BOX = 1, RAYN_FILTER_MITCHELL = 2, RAYN_FILTER_LANCZOS = 3 };
int rayn_build_fis_table(uint32_t filter_kind, float radius, float* table512);
int rayn_build_fis_table_ex(uint32_t filter_kind, float radius, float param0, float param1,
                            float* table512);
/* number of tiles render_frame_into builds, incl. its under-coverage quirk (src/film.rs:399-404). */
uint32_t rayn_tile_count(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h);

/* ---- diagnostics (no reference counterpart) ------------------------------------------------ */
/* timing: bracket every kernel launch with HIP events and fill rayn_stats.ms_*; count_evals: run
 * the instrumented kernel variants that count SDF distance evaluations (roofline accounting). */
int rayn_hip_set_profiling(rayn_ctx* ctx, int timing, int count_evals);
/* out[0] k_extend (closest-hit marches), out[1] k_shade_setup (normal estimation), out[2] k_shadow (NEE visibility).
 * What is counted, per ray and independent of what other lanes do (every count below is a deterministic function of the scene and the rays; the tests hold them
 * to the CPU oracle's per-lane accounting with ==, tests/test_counters_device.py):
 *   out[0]  every valid ray of the queue against every TracedSDF of the scene (src/hitable.rs:177-198 with the running closest hit as t_max): one evaluation
 *           at the origin, then one per march trip of TracedSDF::hit (src/sdf.rs:59-83) up to and including the trip in which the ray stops (hit, first
 *           distance NaN, or t > t_max), at most max_marches trips.  Analytic spheres and padding entries of the queue cost nothing.
 *   out[1]  4 evaluations (the tetrahedral normal estimator) per valid slot whose hit object is a TracedSDF; none for padding lanes and slots on spheres.
 *   out[2]  every PARKED shadow segment (rayn_stats.shadow_jobs) against the TracedSDFs in index order, up to and including the first that occludes it: per
 *           TracedSDF one evaluation at the segment start, then one per trip of TracedSDF::occluded (src/sdf.rs:25-57) the segment enters - none when
 *           max_vis_marches == 0, or once t > max_dist or the first distance was NaN.
 * A counting context also counts in rayn_hip_probe_extend / _shadow / _shade (below): the four getters then report that probe call. */
int rayn_hip_get_eval_counts(const rayn_ctx* ctx, uint64_t out[3]);
/* the fold / orbit ITERATIONS those evaluations ran, same three kernels (MandelBox::dist always runs `iterations` folds, src/sdf.rs:125-141;
 * the Mandelbulb extension stops at its bailout; a sphere SDF has none): what an evaluation of the scene's own SDF costs is
 * flop_per_iteration * iterations / evaluations + the epilogue - bench.py prices the roofline with it instead of a fixed figure */
int rayn_hip_get_sdf_iterations(const rayn_ctx* ctx, uint64_t out[3]);
/* r6, same instrumented kernels: out[0] = shaded slots whose throughput was exactly (0, 0, 0) and whose NEE was therefore elided - every Le / surface / volume
 * NEE term of src/integrator.rs:70,91-92,128-129 is multiplied by that zero, so their shadow rays are never marched (k_shade_setup, exact: see the
 * kernel) - out[1] = the shadow segments those slots would have parked for TracedSDF::occluded (src/sdf.rs:25-57), out[2] = NEE samples of such
 * slots that were NOT elided because their contribution is not provably finite (then inf * 0 / NaN must keep its bits: tested and marched as ever).
 * The rule, per NEE sample of a VALID slot (n_lights > 0; a surface sample exists when the slot's material receives light, a volume sample when the volume
 * scatters).  zero_w: the slot's throughput is exactly (0, 0, 0) and |vol_T| and |rho_s| are finite.  ELIDED: zero_w, and every |x_c| <= 2^60 and |pdf| >= 2^-60
 * (surface: x = Le * f * cos * tr; volume: x_c = Le_c * tr, pdf = vpdf * lpdf, and |aux| finite too).  A sample is PARKED as a shadow job
 * (rayn_stats.shadow_jobs) iff it is not elided, every analytic sphere's occlusion factor is 1, the scene holds a TracedSDF and - surface samples only - x is
 * not all-zero.  out[0] counts the zero_w slots, out[1] the elided samples that would otherwise have been parked, out[2] the samples of zero_w slots that are
 * not elided. */
int rayn_hip_get_elision_counts(const rayn_ctx* ctx, uint64_t out[3]);
/* r6, same instrumented kernels, single-Mandelbulb scenes only (rayn_amd/csrc/march_bulb.h; zero otherwise): the shadow-march kernel written for that SDF runs an
 * evaluation in two stages - orbit steps, then distance + one step of TracedSDF::occluded (src/sdf.rs:25-57) - each at its own occupancy.
 * out[0] / out[1] = lane slots (64 x wave executions) the orbit / epilogue stage of k_shadow_bulb offered; the lane slots USED are
 * rayn_hip_get_sdf_iterations()[2] (orbit steps) and rayn_hip_get_eval_counts()[2] (epilogues).  Unlike every other counter these two depend on which
 * wave wins which chunk of the job queue (they count executions of a stage per WAVE), so they differ from run to run: multiples of 64 that bound the used slots
 * from above, and no more can be asserted of them. */
int rayn_hip_get_stage_slots(const rayn_ctx* ctx, uint64_t out[2]);
/* A frame's tiles are dealt to up to two workers (host thread + HIP stream + own device memory each) so that one
 * worker's HBM-bound kernels and readbacks run underneath the other's VALU-bound marches.  n_workers 1..4 (default 2).
 * A further worker is only used while every worker still gets full-size batches and the call owns >= min_paths camera
 * paths (default 2^22); min_paths = 0 forces n_workers (tests). */
int rayn_hip_set_workers(rayn_ctx* ctx, int n_workers, uint64_t min_paths);
/* upper limit of the path-pool capacity per worker and batch of tiles (default 2^28 paths, ~89 GB of HBM per worker for a
 * scene without volume); the effective size is also capped so that all workers together use <= 60 % of the free HBM and that
 * the 32-bit [light sample][slot] references of a batch do not overflow. */
int rayn_hip_set_batch_paths(rayn_ctx* ctx, uint64_t paths);
/* First frame of a context (no reference counterpart; the reference renders ONE frame per process, src/main.rs:47-96).  Device
 * memory that a process released is wiped by the driver before another process can use it; a fresh process that takes a
 * full-size arena (up to 60 % of the HBM) right after another one exited runs its first frame up to 3.5 s longer (measured,
 * profiles/r03_cold_start.txt).  The FIRST frame a context renders therefore sizes its batches for arenas of at most `bytes`
 * in total (default 44 GB: one worker with 2^26-path batches of the volume path, 2^27 without - a quarter of the full size,
 * 2.5 % slower); from its second frame on a context uses full-size batches.  The
 * result is bit-identical (batching never changes a pixel: packets are per tile).  0 = full size from the first frame.
 *
 * Environment.  The library reads NO tuning from the environment unless RAYN_HIP_ENV_TUNING=1 is exported at context creation
 * (the measurement scripts under tools/ do); then RAYN_HIP_WORKERS, RAYN_HIP_WORKER_MIN_PATHS, RAYN_HIP_BATCH_PATHS,
 * RAYN_HIP_COLD_BYTES, RAYN_HIP_PROFILE (per-launch HIP events = rayn_hip_set_profiling), RAYN_HIP_REFILL_EXTEND / _SHADOW,
 * RAYN_HIP_PREFETCH_EXTEND / _SHADOW, RAYN_HIP_FAST_PATH and RAYN_HIP_PERSISTENT_BLOCKS preset the corresponding launch
 * parameters of a new context.  None of them changes a pixel. */
int rayn_hip_set_cold_bytes(rayn_ctx* ctx, uint64_t bytes);
/* mul_add policy (include/rayn_detmath.h): 0 = unfused a*b+c, what rayn's default x86-64 build does (wide
 * 0.4.6 without +fma) — the DEFAULT; 1 = fused, what rayn built with -C target-feature=+fma does.
 * rayn_hip_fma_policy() returns the default policy of a new ctx. */
int rayn_hip_fma_policy(void);
int rayn_hip_set_fma_policy(rayn_ctx* ctx, int policy);
/* sizeof() of the ABI structs as compiled: 0 world_desc, 1 frame_params, 2 stats, 3 hitable,
 * 4 material, 5 light, 6 camera, 7 temporal_resample_params, 8 display_params, 9 upscale_params,
 * 10 temporal_upscale_params, 11 preview_params, 12 interpolate_params, 13 interpolate_key — lets a binding verify its layout. */
size_t rayn_hip_sizeof(int which);
/* "" for the product build of the library; the VARIANT name of a `make variant` build (timing experiments: such a build is
 * only ever loaded through RAYN_HIP_LIB + RAYN_HIP_ALLOW_VARIANT=1, and bench.py prints the name in its result line). */
const char* rayn_hip_build_variant(void);

/* Restrict the following renders to the listed tiles (indices in the reference's tile order, src/film.rs:399-427; duplicates
 * and out-of-range indices are an error); n = 0 clears the restriction.  While a subset is set tile_first/tile_step are
 * ignored.  Tiles are independent (src/film.rs:439-627), so a subset render produces exactly the pixels the full frame
 * would: the parity tests use it to compare whole 16x16 tiles at the full BASELINE configurations with oracle digests. */
int rayn_hip_set_tile_subset(rayn_ctx* ctx, const uint32_t* tiles, uint32_t n);

/* Packet-order dump of ONE tile of the next renders (diagnostics; tile_index in the reference's tile order, -1 = off):
 * after every depth's bin stage the tile's binned queue is read back as records of 6 u32 {depth, object, tile x,
 * tile y, sample, valid} in HitStore::process_hits order (src/hitable.rs:94-134: object-major, insertion order, bins
 * padded to x4 with invalid lanes).  rayn_hip_get_trace returns the record count and copies up to cap_records. */
int rayn_hip_set_trace_tile(rayn_ctx* ctx, int tile_index);
int64_t rayn_hip_get_trace(const rayn_ctx* ctx, uint32_t* out, uint64_t cap_records);

/* ---- test probes on caller data (HOST pointers), so that the parity tests can compare single functions with the CPU oracle lane for lane:
 *   rayn_hip_probe_sdf_dist   SDF::dist (src/sdf.rs:125-140) of one TracedSDF, a per-lane device function;
 *   rayn_hip_probe_sdf_dist_as  the same function in ONE named instantiation and division arm: sdf_dist<false, sdfk> of hitable hitable_index with the scale the march
 *                             kernels hand it for a packet of lane-0 time t0 (sdf_scale: scale + scale_vel * t0 when scale_vel != 0).  sdfk = -1 (the kind is read
 *                             from the object), the object's own RAYN_SDF_* kind, or 100 (the 12-iteration MandelBox with the short division, both known at compile
 *                             time).  fast_div = the division arm (0 IEEE '/' and the reference's clamp, 1 div_nr, 2 div_short); it may only LOWER the value the
 *                             upload gave the object (rayn_hip_probe_scene_dispatch): the lower arms are the more general ones.  RAYN_ERR_INVALID_ARG with a text,
 *                             nothing launched and out untouched, for: an sdfk outside {-1, 0, 1, 2, 100}; an sdfk >= 0 that is not the object's kind; sdfk = 100 on
 *                             an object that is not a 12-iteration MandelBox with fast_div 2, or with a fast_div argument other than 2 (that instantiation has no
 *                             other arm); a fast_div above the object's own; what rayn_hip_probe_sdf_dist rejects.
 *   rayn_hip_probe_scene_dispatch  what the VALUES of the uploaded world and p decide, through the build_scene and scene_march_kernels a render calls (the upload-time
 *                             verdict kernel behind fast_div 2 is the only launch): out[0] = the index of the scene's single TracedSDF or -1 (the single-SDF march
 *                             kernels or the generic ones), out[1] = Tuning::sdf_kind (-1, 0, 1, 2 or 100: the instantiation), out[2] = Tuning::bulb (k_shadow_bulb),
 *                             out[3] = DScene::anim_spheres (the kernels carry the packet's lane-0 time), out[4 + i] = DHitable::fast_div of hitable i for i <
 *                             n_hitables and -1 beyond, RAYN_MAX_HITABLES entries.  out holds 4 + RAYN_MAX_HITABLES words.
 *   rayn_hip_probe_extend     HitableStore::add_hits' closest hit (src/hitable.rs:177-198 over Sphere::hit and TracedSDF::hit, src/sdf.rs:59-83) through the
 *                             PRODUCT extend kernel of the uploaded scene (k_extend1, or the generic k_extend of a multi-SDF scene) on a synthetic ray queue of
 *                             the n rays, ray time 0; out_obj 0xFFFFFFFF = none;
 *   rayn_hip_probe_shadow     the TracedSDF::occluded factors of HitableStore::test_occluded (src/hitable.rs:164-168, src/sdf.rs:25-57; the analytic spheres are
 *                             resolved by the shading kernel) through the PRODUCT shadow-march kernel (k_shadow1, k_shadow_bulb, the generic k_shadow) on a
 *                             synthetic job list of the n segments: 1.0 visible, 0.0 occluded;
 *   COUNTING in rayn_hip_probe_extend / _shadow / _shade: while the context's count_evals is on (rayn_hip_set_profiling) these three launch the INSTRUMENTED
 *                             instantiations of the same kernels instead (k_extend<true> / k_extend1<true, -1>; k_shadow<true> / k_shadow1<true, -1> /
 *                             k_shadow_bulb<true, K, STEPS>; k_shade_setup<true> and the scene's shadow march), return the same outputs bit for bit, and leave
 *                             the counters of THAT call in the context: rayn_hip_get_eval_counts / _sdf_iterations / _elision_counts / _stage_slots report it
 *                             (the classes the call did not run are 0) until the next counted probe or frame.  With count_evals off - the default - the probes
 *                             run the product instantiations and leave the context's counters alone.
 *   rayn_hip_probe_detmath    the pinned elementary functions as the kernels evaluate them (op 0 exp, 1 sin, 2 cos, 3 tan, 4 atan2(a,b), 5 pow(a,b),
 *                             14 ln(a)) for ANY float argument: zero, denormals, infinities, NaN, and for sin / cos / tan every finite magnitude
 *                             (above 2^20 through dm_sincos_large's integer reduction).  tests/test_detmath_device.py compares them with the
 *                             oracle on every exponent field.
 *   Ops 6.. check the kernels' exact replacements of IEEE '/' and sqrt against the hardware IEEE
 *   result: 6 Newton-Raphson a/b, 7 IEEE a/b, 8 sqrt(a), 9/10/11 component x/y/z of v/|v| and
 *   12 |v| (a holds n xyz triples), 13 exhaustive sqrt sweep (out[i] = mismatch count over the
 *   65536 float bit patterns starting at bits(a[i])), 14 ln(a) as the Mandelbulb estimator evaluates it (dmf_logf),
 *   15 exhaustive sweep of 1 / sqrt(a) as the kernels evaluate it (rcp_sqrt_rn) against the IEEE sqrt and division (mismatch count over 65536 patterns), 16 that value,
 *   17/18/19 component x/y/z of v/b through the shared-reciprocal division div3_by (a holds n xyz triples, b the n denominators).
 *   rayn_hip_probe_shading    the shading half of the path: the SAME per-lane device functions k_raygen / k_shade_setup / k_shade_finish call, on n lanes
 *                             of caller records, under the ctx's mul_add policy.  Lane i reads in[i * IN .. +IN) and writes out[i * OUT .. +OUT):
 *     op  function (reference)                                        IN  in record                                   OUT  out record
 *      0  Camera::get_rays of the uploaded camera (src/camera.rs)      5  uvx, uvy, lens0, lens1, t0                   6  origin xyz, dir xyz
 *      1  concentric_circle_map (src/math.rs:201-219)                  2  u0, u1                                       2  x, y
 *      2  cosine_weighted_in_hemisphere (src/math.rs:99-103)           2  u0, u1                                       3  xyz
 *      3  cosine_power_weighted (src/math.rs:106-113)                  3  u0, u1, power                                3  xyz
 *      4  get_orthonormal_basis (src/math.rs:49-59)                    3  n xyz                                        9  columns c0, c1, c2
 *      5  f_schlick (src/math.rs:122-124)                              2  cos, f0                                      1  value
 *      6  BSDF::f of material `index`, as called: f(arg0, arg1, n)     9  arg0 xyz, arg1 xyz, n xyz                    3  rgb
 *      7  BSDF::le of material `index`                                 3  wo xyz                                       3  rgb
 *      8  BSDF::scatter of material `index` at a shading point whose   11 wo xyz, normal xyz, s1, u0, u1, u2, u3       7  wi xyz, f rgb, pdf
 *         basis is get_orthonormal_basis(normal), as k_shade_setup builds it
 *      9  SphereLight::sample of light `index` (src/light.rs:38-72)    5  u0, u1, p xyz                                4  point xyz, pdf
 *     10  SphereLight::sample_volume_scattering of light `index` (:75-102)  8  sample, ro xyz, rd xyz, max_distance       2  dist, pdf
 *     11  light index floor(s * nl) clamped to nl - 1, nl = `index`     1  s                                            1  index as float
 *     12  FilterImportanceSampler::sample (src/filter.rs:222-235)      1  u                                            1  value
 *         with aux = the RAYN_FIS_TABLE_SIZE-float inverse CDF (aux is ignored by the other ops)
 *     13  Sphere::hit of hitable `index` (src/sphere.rs:48-72)         8  o xyz, d xyz, t_max, t0                      1  t (FLT_MAX = miss)
 *     14  Sphere::occluded of hitable `index` (src/sphere.rs:24-46)    7  a xyz, b xyz, t0                             1  0 occluded, 1 not
 *         the device runs the prologue of k_shade_setup's spheres_visible (dir = b - a, dist = |dir|, dir / dist) and then
 *         sphere_occluded_dir, the same functions the shade, extend and preview kernels call
 *   Camera closures (rayn_camera.animated) are evaluated at t0, which the reference takes from LANE 0 of the ray-gen packet (a caller comparing
 *   with a 4-wide packet passes one t0 per group of four lanes).  Op 6 rejects Sky (its f panics in the reference) and op 8 takes only Lambertian and
 *   Dielectric: Sky and Emissive never scatter (receives_light is false), so those paths are never reached and are not probed.  Ops 13 and 14
 *   take t0 per lane - the packet's lane-0 time at which a closure centre (rayn_hitable.animated) is sampled; NaN is the time of a packet whose
 *   lane 0 is empty - and return RAYN_ERR_INVALID_ARG with a text when `index` is out of range or names a TracedSDF.
 *   rayn_hip_probe_queue      the queue stages of ONE depth through the PRODUCT kernels and the two stage launchers the depth loop calls, on a caller-built ray queue
 *                             (no scene, no world needed): stage 0 = bin (k_group_hist, k_scan_tile, k_tile_prefix, k_bin_scatter: object-major, insertion-ordered,
 *                             x4-padded packets per tile), stage 1 = repack (k_scan_tile, k_tile_prefix, k_compact_scatter: the stable repack of the survivors).
 *     in   nclass 1..16; tile_groups[n_tiles] = 64-entry groups each tile owns in the ray queue (tiles back to back, 0 allowed); q[e] / ent_obj[e] for the
 *          64 * sum(tile_groups) entries: the queue reference (< n_refs, or 0xFFFFFFFF for a padding entry) and the object byte (a class < nclass, or 0xFF for
 *          a miss; a padding entry carries 0xFF); survive[n_refs] = what the shading kernel would decide for each reference (the probe builds the per-group
 *          survivor ballots and counts from it on the host, from the binned queue as the device left it: invalid slots are dead); cap_groups_bin /
 *          cap_groups_repack = the queue capacities the two k_tile_prefix launches guard; max_entries / max_slots = the upper bounds the grids are sized by
 *          (the kernels take the actual counts from the control block, so larger is allowed); sentinel = a word that is neither 0xFFFFFFFF nor a reference.
 *     out  out_bq / out_qn [out_slots]: the binned queue and the next ray queue.  out_slots >= the slots the input's binned queue needs; every device
 *          buffer is sized by it and not by the caps, and both queues start filled with the sentinel, so a refused stage writes nothing anywhere and a
 *          stray write is visible.  out_tile[n_tiles][5] = output group begin, count of the bin stage; begin, count of the repack; the tile's base_hist
 *          entry.  out_cls_cnt / out_cls_base [n_tiles][16] as the bin stage left them.
 *     ctl_io[12], in and out: q_groups, q_valid, b_groups, b_valid, overflow, segments, shaded_slots, entries_sum, next_sum, job_count, head_shadow,
 *          head_extend of the device control block.  On entry the start values (q_groups is taken from tile_groups instead); on return the final ones.
 *   rayn_hip_probe_march_limits  the sizes that decide the MODE of the persistent march kernels, as the library was built and the context tuned: the entries a
 *                             wave takes from its queue per atomic (chunk); the remaining-entry count below which a fetched chunk puts its wave into the endgame
 *                             (endgame_entries; k_shadow_bulb multiplies it by its rays per lane); the grid cap (persistent_blocks, blocks of 4 waves) and
 *                             k_shadow_bulb's rays per lane (bulb_rays) of the ctx's launch tuning.  No GPU work.  Tests size their probe inputs from these.
 *   rayn_hip_probe_resolve    the film resolve (k_resolve_reg / k_resolve_blk / k_resolve_huge) through the PRODUCT launcher - so the variant is the one the product picks
 *                             for `spp` - on caller-built tiles and termination records (no scene, no world needed; the device scene is zero but for spp and width).
 *     in   width = film width of the unpacked tiles; spp = samples per pixel as the host produces them (a multiple of 4 in 4..16384); tiles[n_tiles][8] = the
 *          device tile words x0, y0, ew, eh, pool_base, n_paths, film_base, film_packed (n_paths is not read by the resolve); max_tile_pixels = the x size of
 *          the grid (>= every tile's ew * eh; larger is allowed, the surplus blocks exit); per path of the n_paths-slot pool: term_info (depth in bits 0..6 |
 *          Background flag in bit 7, 0xFF = no sample), term_key (the termination slot), col0_rgb[3], aov_xyz[3] and aov_obj (the depth-0 object, < 0xFF, or
 *          0xFF for none); base_hist[n_depths][hist_stride] = the slot at which tile t's binned segment of depth d began, at [d * hist_stride + t] (read by
 *          k_resolve_blk only: 512 < spp <= 4096; may be null otherwise); sentinel = the word every output float starts as.
 *     out  out_color[3 N], out_alpha[N], out_background[3 N], out_normal[3 N], N = out_pixels: film planes, or the packed planes of film_packed tiles.  A
 *          pixel no tile owns keeps the sentinel in all ten words.
 *     Rejected with RAYN_ERR_INVALID_ARG - what the kernels could not index, or what their stated preconditions exclude: spp out of range; a tile of no
 *          pixel, of more than 1024 pixels or of more than max_tile_pixels; pool_base + ew * eh * spp beyond n_paths; a film index at or beyond out_pixels,
 *          or one that two tiles own; a contributing sample deeper than 120; an object word that is neither below 0xFF nor 0xFF; for 512 < spp <= 4096 a
 *          depth at or beyond n_depths, hist_stride < n_tiles, a slot below its base_hist entry or 2^25 or more above it; two contributing samples of one
 *          pixel with equal (depth, slot) - a slot holds one path, and the order of such a pair would be undefined.  Only the paths tiles own are looked at.
 *   rayn_hip_probe_raygen     the ray-generation stage through the PRODUCT launchers under the ctx's mul_add policy, as the frame set-up and the batch loop launch them:
 *                             k_pack_tables (the per-(depth, sample) packed sample records), k_batch_setup (the tile of every 64-slot pool group and every tile's group
 *                             range) and k_raygen (the tile ray-gen loop, src/film.rs:456-529, one thread per pool slot) - with the uploaded world's camera, on
 *                             caller-built tables and a caller-built tile list that need not be the reference grid's.
 *     in   p as rayn_hip_render_frame takes it (tile_w / tile_h / tile_first / tile_step are not read: the tiles are given); samples_1d[n_samples_1d],
 *          samples_2d[n_samples_2d], scramble[n_scramble], fis_table[512] with the counts in floats; tiles[n_tiles][8] = the device tile words x0, y0, ew, eh,
 *          pool_base, n_paths, film_base, film_packed (the last two are not read by this stage); n_pool = pool slots, a multiple of 64; surplus = slots of
 *          sentinel every per-slot output holds after the pool, a multiple of 64, at least 128; sentinel = the word every output starts as (term_info: its
 *          low byte): neither 0xFFFFFFFF nor below n_pool, low byte not 0xFF.
 *     out  per slot of the n_pool + surplus: out_geo0 / out_geo1 / out_col0 / out_col1 / out_aov [.][4] in the pool's own encoding (rayn_hip_probe_shade),
 *          out_term_key, out_term_info, out_q (the ray queue); out_pgrp_tile[(n_pool + surplus) / 64]; out_tgb / out_tgc [n_tiles + 2]; out_ctl[8] = the
 *          32-bit words of the control block: q_groups, q_valid, b_groups, b_valid, head_extend, job_count, head_shadow, overflow (k_raygen writes q_groups,
 *          q_valid and head_extend; the others keep the sentinel); out_records[(max_bounces + 1) * 4 * samples * rec_stride * 4 + 64] floats, rec_stride =
 *          (8 + 12 + 8 * volume_marches) / 4: record depth * spp + s = the 3 + VM 1-D sets 1 + k + depth * (3 + VM) of sample s, zeros up to 8 floats, then the
 *          12 + 8 * VM components c of the 2-D sets 2 + c / 2 + depth * (6 + 4 * VM), as the tables hold them (no scramble).
 *          A path slot has origin / dir, hit t 0, OBJ_NONE | sample << 8, radiance 0, throughput 1, its film pixel and time, aov (0, 0, 0, OBJ_NONE), term_info
 *          0xFF and q = its own index; a padding slot (the tail of a tile's last group) has aov and term_info alike, q = 0xFFFFFFFF and nothing else written;
 *          term_key is not written by this stage.
 *     Rejected with RAYN_ERR_INVALID_ARG before anything is launched or written - what the kernels could not index: what rayn_hip_render_frame rejects in p
 *          (volume_marches outside 2..4, max_bounces above 120, samples outside 1..4096 - so spp is a multiple of 4 in 4..16384); a null buffer;
 *          n_samples_1d != spp * rayn_sets_1d or n_samples_2d != spp * 2 * rayn_sets_2d for p's bounces and volume marches; n_scramble != width * height;
 *          n_tiles outside 1..2^20; n_pool 0, not a multiple of 64 or above 2^27; a bad surplus or sentinel; a tile of no pixel or of more than 1024; a tile
 *          that does not lie inside width x height; n_paths != ew * eh * spp; a pool_base that is not a multiple of 64; tiles whose 64-padded segments
 *          [pool_base, pool_base + ceil64(n_paths)) overlap, end beyond n_pool or leave a gap in [0, n_pool) (k_raygen reads pgrp_tile[P / 64] for every
 *          P < n_pool, so a gap would read an unwritten word).  The segments may come in any order.
 *   rayn_hip_probe_shade_limits  the sizes that decide how many grid-stride trips the streaming kernels of the shade stage make, as the library was built: the block
 *                             cap of their grids (stream_blocks; k_shadow_list, k_shade_finish), the [sample][slot] ids a block of k_shadow_list scans per trip
 *                             (list_ids_per_block) and the block size of k_shade_setup (setup_threads; its grid has no cap).  No GPU work.  Tests size the case that
 *                             reaches the second trip from these.
 *   rayn_hip_probe_shade      the shade stage of ONE depth through the PRODUCT launcher (launch_shade: k_shade_setup, k_shadow_list, the shadow-march kernel the
 *                             product picks for the uploaded scene and the ctx's tuning, k_shade_finish) under the ctx's mul_add policy, on a caller-built binned
 *                             queue and path pool - PathTracingIntegrator::integrate (src/integrator.rs:47-204) for n_slots / 4 packets of four lanes.
 *     in   p and the four tables as rayn_hip_render_frame takes them (the packed sample records are built by the product's own kernel); depth <= max_bounces;
 *          n_slots = binned slots, a multiple of 64; slots 4k..4k+3 are one packet; max_slots >= n_slots = the upper bound the grids are sized by (the surplus
 *          exits); nee_cap >= n_slots = the plane stride of the per-slot NEE records; ref[n_slots] = the binned queue: a pool index below n_pool, or 0xFFFFFFFF
 *          for a padding lane; geo0 / geo1 / col0 / col1 [n_pool][4] = the pool records in the pool's own encoding: origin xyz, dir x | dir yz, hit t, bits
 *          (hit object | sample index << 8) | radiance rgb, throughput r | throughput gb, bits (film pixel index), ray time; sentinel = the word that pre-fills what
 *          the kernels may or may not write.
 *          The probe owns every device buffer (the pool, the NEE records, the survivor ballots, the control block with b_groups = n_slots / 64) and pre-fills:
 *          aov, term_key and every float plane of the NEE records with the sentinel; term_info with 0xFF (no sample); the visibility plane with 2 ("march
 *          pending") over all ns * nee_cap entries - the worst stale value: a (sample, slot) the setup kernel forgets becomes a shadow job and an occluded sample;
 *          the job segments with zeros.
 *     out  the pool as the stage left it: out_geo0 / out_geo1 / out_col0 / out_col1 / out_aov [n_pool][4], out_term_key[n_pool], out_term_info[n_pool];
 *          out_alive_mask / out_bgrp_cnt [n_slots / 64] = the survivor ballot and count of every group; out_jobs[3] = job_count and shadow_jobs of the control
 *          block, and the shadow-march kernel launch_shadow_march picks (0 none: no TracedSDF, 1 k_shadow, 2 k_shadow1, 3 k_shadow_bulb).
 *          A spawned lane has its new origin / dir / throughput and its radiance in the pool and its bit in the ballot; a terminated one has term_info = depth |
 *          Background flag (bit 7), term_key = its SLOT and its radiance in col0; a depth-0 hit of a light-receiving object has its WorldNormal sample and object
 *          in aov.  The layout of the NEE records is NOT part of this contract: the probe only checks, after the run, that no word of theirs at a slot index in
 *          [n_slots, nee_cap) changed and that job_count <= ns * n_slots (RAYN_ERR_HIP with a last error text otherwise).
 *     Rejected with RAYN_ERR_INVALID_ARG - what the kernels could not index, or what their stated preconditions exclude: a null buffer; n_slots 0 or not a
 *          multiple of 64; n_pool 0, or n_pool or max_slots above 2^27 (the probe's own size limit); max_slots or nee_cap below n_slots; ns * nee_cap or ns * max_slots beyond 2^32 - 2^26 (32-bit [sample][slot] ids; ns = 4, + 4 *
 *          volume_marches when the volume scatters); a ref that is neither 0xFFFFFFFF nor below n_pool; a pool slot referenced twice; a packet whose lane 0 is
 *          a padding lane while a later lane is not (lane 0 of a bin packet is always a real hit; a packet of four padding lanes is the tail of a group); a
 *          packet whose valid lanes name different objects; an object at or beyond n_hitables; a sample index at or beyond 4 * samples; a pixel index at or
 *          beyond width * height; a depth above max_bounces.  Only the pool records ref names are looked at. */
/*   rayn_hip_probe_huffman   the Huffman construction the PNG block kernels share (huffman_code<286> of the literal/length code and huffman_code<30> of the
 *                             distance code, "PNG encoding on the device" above) alone: one workgroup of 256 threads per count set, through the same template the
 *                             block kernels instantiate.  n_symbols = 286 or 30; counts[n_sets][n_symbols] = the frequencies, each set summing to less than 2^32
 *                             (the node weights are 32-bit), 1 <= n_sets <= 65536.  out_clen[n_sets][n_symbols] = the code lengths 0..15 (depths of the tree,
 *                             frequencies halved while a depth exceeds 15; with fewer than two symbols in use the used one - symbol 0 when there is none - gets 1);
 *                             out_tab[n_sets][n_symbols] = (the canonical code of RFC 1951 3.2.2, bit-reversed) | length << 16, 0 for an unused symbol.  The encoders
 *                             themselves are untouched.  RAYN_ERR_INVALID_ARG with a text for anything else. */
int rayn_hip_probe_huffman(rayn_ctx* ctx, uint32_t n_symbols, uint32_t n_sets, const uint32_t* counts,
                           uint32_t* out_clen, uint32_t* out_tab);
/*   rayn_hip_probe_jpeg_transform   the first kernel of "Baseline JPEG scans on the device" above alone: img[height][width][bpp] on the HOST -> out_coef[blocks][64],
 *                             the int16 quantised coefficients in zigzag order, the blocks in the order of the scan (blocks = MCUs * 1, 3 or 6).  At most 2^20 blocks.
 *   rayn_hip_probe_jpeg_entropy     the other three kernels - Huffman codes per restart segment, stuffing, layout, compaction - on caller coefficients
 *                             coef[blocks][64] (HOST, the layout above) for an image of that geometry.  The probe owns the output and the scratch and fills both,
 *                             whole, with fill_byte (0..255) before the kernels run: the encoder has no memset, and must write the same whatever they held.
 *                             out[out_bytes >= rayn_jpeg_scan_bound] = the bound's bytes: the four header words, the scan, fill_byte behind its last word.
 *                             Rejected with RAYN_ERR_INVALID_ARG: a DC outside [-1024, 1023] or an |AC| above 1023 - the reach of the 13-bit transform at
 *                             Q = 1, within which a DC difference is at most category 11 and an AC size 10, the last symbols of the Annex K tables - besides
 *                             what the entry rejects, a null buffer and more than 2^20 blocks.  RAYN_ERR_HIP with a text if a byte behind either buffer changed. */
int rayn_hip_probe_jpeg_transform(rayn_ctx* ctx, uint32_t width, uint32_t height, uint32_t bpp, uint32_t quality, uint32_t subsampling,
                                  const uint8_t* img, int16_t* out_coef);
int rayn_hip_probe_jpeg_entropy(rayn_ctx* ctx, uint32_t width, uint32_t height, uint32_t bpp, uint32_t subsampling, uint32_t restart_interval,
                                const int16_t* coef, uint32_t fill_byte, uint8_t* out, size_t out_bytes);
int rayn_hip_probe_shade_limits(const rayn_ctx* ctx, uint32_t* stream_blocks, uint32_t* list_ids_per_block,
                                uint32_t* setup_threads);
int rayn_hip_probe_shade(rayn_ctx* ctx, const rayn_frame_params* p, const float* samples_1d, const float* samples_2d,
                         const float* scramble, const float* fis_table, uint32_t depth, uint32_t n_slots,
                         uint32_t max_slots, uint32_t nee_cap, const uint32_t* ref, uint32_t n_pool,
                         const float* geo0, const float* geo1, const float* col0, const float* col1,
                         uint32_t sentinel, float* out_geo0, float* out_geo1, float* out_col0, float* out_col1,
                         float* out_aov, uint32_t* out_term_key, uint8_t* out_term_info,
                         uint64_t* out_alive_mask, uint8_t* out_bgrp_cnt, uint64_t* out_jobs);
int rayn_hip_probe_raygen(rayn_ctx* ctx, const rayn_frame_params* p, const float* samples_1d, uint64_t n_samples_1d,
                          const float* samples_2d, uint64_t n_samples_2d, const float* scramble, uint64_t n_scramble,
                          const float* fis_table, uint32_t n_tiles, const uint32_t* tiles, uint32_t n_pool,
                          uint32_t surplus, uint32_t sentinel, float* out_geo0, float* out_geo1, float* out_col0,
                          float* out_col1, float* out_aov, uint32_t* out_term_key, uint8_t* out_term_info,
                          uint32_t* out_q, uint32_t* out_pgrp_tile, uint32_t* out_tgb, uint32_t* out_tgc,
                          uint32_t* out_ctl, float* out_records);
int rayn_hip_probe_march_limits(const rayn_ctx* ctx, uint32_t* chunk, uint32_t* endgame_entries,
                                uint32_t* persistent_blocks, uint32_t* bulb_rays);
int rayn_hip_probe_sdf_dist(rayn_ctx* ctx, const rayn_frame_params* p, uint32_t hitable_index,
                            const float* pts_xyz, float* out, uint32_t n);
int rayn_hip_probe_sdf_dist_as(rayn_ctx* ctx, const rayn_frame_params* p, uint32_t hitable_index, int32_t sdfk,
                               uint32_t fast_div, float t0, const float* pts_xyz, float* out, uint32_t n);
int rayn_hip_probe_scene_dispatch(rayn_ctx* ctx, const rayn_frame_params* p, int32_t* out);
int rayn_hip_probe_extend(rayn_ctx* ctx, const rayn_frame_params* p, uint32_t depth,
                          const float* org_xyz, const float* dir_xyz, float* out_t,
                          uint32_t* out_obj, uint32_t n);
int rayn_hip_probe_shadow(rayn_ctx* ctx, const rayn_frame_params* p, const float* start_xyz,
                          const float* end_xyz, float* out, uint32_t n);
int rayn_hip_probe_detmath(rayn_ctx* ctx, uint32_t op, const float* a, const float* b, float* out,
                           uint32_t n);
int rayn_hip_probe_shading(rayn_ctx* ctx, const rayn_frame_params* p, uint32_t op, uint32_t index,
                           const float* in, float* out, const float* aux, uint32_t n);
int rayn_hip_probe_queue(rayn_ctx* ctx, uint32_t nclass, uint32_t n_tiles, const uint32_t* tile_groups,
                         const uint32_t* q, const uint8_t* ent_obj, const uint8_t* survive, uint32_t n_refs,
                         uint32_t cap_groups_bin, uint32_t cap_groups_repack, uint32_t max_entries,
                         uint32_t max_slots, uint32_t sentinel, uint32_t out_slots, uint32_t* out_bq,
                         uint32_t* out_qn, uint32_t* out_tile, uint32_t* out_cls_cnt,
                         uint32_t* out_cls_base, uint64_t* ctl_io);
int rayn_hip_probe_resolve(rayn_ctx* ctx, uint32_t width, uint32_t spp, uint32_t n_tiles, const uint32_t* tiles,
                           uint32_t max_tile_pixels, uint32_t n_paths, const uint8_t* term_info,
                           const uint32_t* term_key, const float* col0_rgb, const float* aov_xyz,
                           const uint32_t* aov_obj, const uint32_t* base_hist, uint32_t hist_stride,
                           uint32_t n_depths, uint32_t sentinel, uint32_t out_pixels, float* out_color,
                           float* out_alpha, float* out_background, float* out_normal);

#ifdef __cplusplus
}
#endif
#endif /* RAYN_HIP_H */
