//! rayn_hip.rs — `extern "C"` binding of librayn_hip.so for rayn.  Copy to `src/hip.rs`, copy film_hip.rs to `src/film_hip.rs`
//! and apply bindings/rayn.patch (adds `mod hip; mod film_hip;`, the `describe()` methods of the scene types and three
//! `pub(crate)`s); link with `cargo rustc -- -L <dir of librayn_hip.so>` or a two-line build.rs.
//!
//! Mirrors include/rayn_hip.h field for field.  UNTESTED AS RUST: no Rust toolchain exists in the build environment
//!.  What IS tested (tests/test_bindings.py, every round): the `#[repr(C)]` field lists below — names, order
//! and scalar widths — are parsed and compared with the C header and with the sizes the compiled library reports through
//! `rayn_hip_sizeof`, so this file cannot drift from the ABI unnoticed.  `check_layout()` repeats the size check at start-up.
//!
//! Reference seam: `Film::render_frame_into` (src/film.rs:382-395); the flattened `World` (src/world.rs:7-13).
#![allow(dead_code)]
use std::os::raw::{c_char, c_void};

pub const RAYN_MAX_HITABLES: usize = 16;
pub const RAYN_MAX_MATERIALS: usize = 16;
pub const RAYN_MAX_LIGHTS: usize = 16;
pub const RAYN_FIS_TABLE_SIZE: usize = 512; // FILTER_TABLE_SIZE, src/filter.rs:187

// rayn_hitable_kind / rayn_sdf_kind / rayn_material_kind / rayn_camera_kind of include/rayn_hip.h
pub const RAYN_HITABLE_SPHERE: u32 = 0;
pub const RAYN_HITABLE_TRACED_SDF: u32 = 1;
pub const RAYN_SDF_SPHERE: u32 = 0;
pub const RAYN_SDF_MANDELBOX: u32 = 1;
pub const RAYN_SDF_MANDELBULB: u32 = 2;
pub const RAYN_MAT_LAMBERTIAN: u32 = 0;
pub const RAYN_MAT_DIELECTRIC: u32 = 1;
pub const RAYN_MAT_SKY: u32 = 2;
pub const RAYN_MAT_EMISSIVE: u32 = 3;
pub const RAYN_CAM_PINHOLE: u32 = 0;
pub const RAYN_CAM_THIN_LENS: u32 = 1;
pub const RAYN_CAM_ORTHOGRAPHIC: u32 = 2;

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct RaynVec3 {
    pub x: f32,
    pub y: f32,
    pub z: f32,
}

/// Sphere<TR> (src/sphere.rs:7-87) | TracedSDF<S> (src/sdf.rs:12-102)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct RaynHitable {
    pub kind: u32,     // 0 Sphere, 1 TracedSDF
    pub material: u32, // MaterialHandle(usize), src/material.rs:55-56
    pub center: RaynVec3,
    pub radius: f32,
    pub sdf_kind: u32,   // 0 sdfu::Sphere, 1 MandelBox (src/sdf.rs:104-188), 2 Mandelbulb (extension)
    pub iterations: u32, // MandelBox::new(iterations, ..)
    pub box_side: f32,   // BoxFold::new(side_length), src/sdf.rs:151
    pub min_radius: f32, // SphereFold::new(min_radius, fixed_radius), src/sdf.rs:172
    pub fixed_radius: f32,
    pub scale: f32,
    pub sdf_radius: f32,
    pub animated: u32, // closure transform_seq |t| center + center_vel * t (src/animation.rs:62-68)
    pub center_vel: RaynVec3,
    pub scale_vel: f32, // extension: MandelBox scale = |t| scale + scale_vel * t (0 = the reference's constant)
}

/// Lambertian | Dielectric (exponent = remapped roughness, src/material.rs:167-174) | Sky | Emissive
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct RaynMaterial {
    pub kind: u32,
    pub a: RaynVec3,
    pub b: RaynVec3,
    pub exponent: f32,
}

/// SphereLight::new(pos, rad, emission), src/light.rs:26-34
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct RaynLight {
    pub pos: RaynVec3,
    pub rad: f32,
    pub emission: RaynVec3,
    pub _pad: u32,
}

/// PinholeCamera | ThinLensCamera | OrthographicCamera (src/camera.rs:41-285)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct RaynCamera {
    pub kind: u32,
    pub res_w: f32,
    pub res_h: f32,
    pub vfov_or_size: f32,
    pub origin: RaynVec3,
    pub at: RaynVec3,
    pub up: RaynVec3,
    pub aperture: f32,
    pub focus: RaynVec3,
    pub animated: u32, // bit 0 origin, 1 at, 2 up, 3 focus: the closure |t| base + vel * t
    pub origin_vel: RaynVec3,
    pub at_vel: RaynVec3,
    pub up_vel: RaynVec3,
    pub focus_vel: RaynVec3,
}

/// World (src/world.rs:7-13) + VolumeParams (src/volume.rs:1-5), scene order preserved
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RaynWorldDesc {
    pub n_hitables: u32,
    pub n_materials: u32,
    pub n_lights: u32,
    pub hitables: [RaynHitable; 16],
    pub materials: [RaynMaterial; 16],
    pub lights: [RaynLight; 16],
    pub camera: RaynCamera,
    pub has_scattering: u32,
    pub coeff_scattering: f32,
    pub has_extinction: u32,
    pub coeff_extinction: f32,
}

/// the arguments of Film::render_frame_into + the constants it reads
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct RaynFrameParams {
    pub width: u32,
    pub height: u32,
    pub samples: u32,
    pub tile_w: u32,
    pub tile_h: u32,
    pub max_bounces: u32,
    pub volume_marches: u32,
    pub frame: u32,
    pub time_start: f32,
    pub time_end: f32,
    pub max_marches: u32,
    pub max_vis_marches: u32,
    pub sdf_detail_scale: f32,
    pub world_radius: f32,
    pub tile_first: u32,
    pub tile_step: u32,
}

/// counters + timings of the last render
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct RaynStats {
    pub paths: u64,
    pub segments: u64,
    pub shaded_slots: u64,
    pub tiles: u64,
    pub batches: u64,
    pub ms_total: f64,
    pub ms_raygen: f64,
    pub ms_extend: f64,
    pub ms_bin: f64,
    pub ms_shade: f64,
    pub ms_compact: f64,
    pub ms_resolve: f64,
    pub launches_extend: u64,
    pub launches_shade: u64,
    pub queue_bytes_bin: u64,
    pub ms_shadow: f64,
    pub ms_finish: f64,
    pub queue_bytes_compact: u64,
    pub shadow_jobs: u64,
}

pub enum RaynCtx {}

// The two parameter blocks of the temporal accumulate (extensions; include/rayn_hip.h: rayn_temporal_params,
// rayn_temporal_resample_params).  Plain scalars: 12 and 4 bytes; rayn_hip_sizeof(7) reports the second.
#[repr(C)]
/// `max_history` 1..65536, `depth_tolerance` finite and >= 0, `normal_min` in [-1, 1] (-1: the test is off)
#[derive(Clone, Copy, Debug)]
pub struct RaynTemporalParams {
    pub max_history: u32,
    pub depth_tolerance: f32,
    pub normal_min: f32,
}
#[repr(C)]
/// `resample`: 0 bilinear, 1 Catmull-Rom
#[derive(Clone, Copy, Debug)]
pub struct RaynTemporalResampleParams {
    pub resample: u32,
}

// The parameter block of the HDR display transform (an extension; include/rayn_hip.h: rayn_display_params).  Plain scalars, 36 bytes;
// rayn_hip_sizeof(8) reports it.
#[repr(C)]
/// `tone`: 0 linear, 1 reinhard, 2 aces; `auto_exposure`: 0 manual (`exposure_scale`), 1 auto (`key`, `adapt`); `levels`: bloom levels, 0 = off
#[derive(Clone, Copy, Debug)]
pub struct RaynDisplayParams {
    pub tone: u32,
    pub auto_exposure: u32,
    pub exposure_scale: f32,
    pub key: f32,
    pub adapt: f32,
    pub iw2: f32,
    pub levels: u32,
    pub threshold: f32,
    pub strength: f32,
}

// The parameter block of the guided upscaling (an extension; include/rayn_hip.h: rayn_upscale_params).  Plain scalars, 12 bytes;
// rayn_hip_sizeof(9) reports it.
#[repr(C)]
/// `factor`: 1..8; `sigma_plane`, `sigma_position`: 0 = off, else in [2^-30, 2^30]
#[derive(Clone, Copy, Debug)]
pub struct RaynUpscaleParams {
    pub factor: u32,
    pub sigma_plane: f32,
    pub sigma_position: f32,
}

// The parameter block of the temporal supersampling (an extension; include/rayn_hip.h: rayn_temporal_upscale_params).  One scalar,
// 4 bytes; rayn_hip_sizeof(10) reports it.
#[repr(C)]
/// `confidence`: 0 off, 1 on
#[derive(Clone, Copy, Debug)]
pub struct RaynTemporalUpscaleParams {
    pub confidence: u32,
}

// The parameter block of the preview integrator (an extension; include/rayn_hip.h: rayn_preview_params).  Plain scalars, 12 bytes;
// rayn_hip_sizeof(11) reports it.
#[repr(C)]
/// `samples`: AO rays per pixel, 1..64; `radius`: their length, finite and > 0; `ambient`: in [0, 1]
#[derive(Clone, Copy, Debug)]
pub struct RaynPreviewParams {
    pub samples: u32,
    pub radius: f32,
    pub ambient: f32,
}

// The parameter block of the frame generation (an extension; include/rayn_hip.h: rayn_interpolate_params).  One scalar, 4 bytes;
// rayn_hip_sizeof(12) reports it.
#[repr(C)]
/// `depth_tolerance`: finite, >= 0
#[derive(Clone, Copy, Debug)]
pub struct RaynInterpolateParams {
    pub depth_tolerance: f32,
}

// One key frame of the frame generation (include/rayn_hip.h: rayn_interpolate_key): device pointers to its film planes and G-buffer, a
// host pointer to its camera, and its time_start.  64 bytes; rayn_hip_sizeof(13) reports it.
#[repr(C)]
/// `d_alpha`, `d_background`, `d_normal`: null in both keys and the output together
#[derive(Clone, Copy, Debug)]
pub struct RaynInterpolateKey {
    pub d_color: *const f32,
    pub d_alpha: *const f32,
    pub d_background: *const f32,
    pub d_normal: *const f32,
    pub d_records: *const c_void,
    pub d_object: *const u32,
    pub camera: *const RaynCamera,
    pub time_start: f32,
}

#[link(name = "rayn_hip")]
extern "C" {
    pub fn rayn_hip_create(device: i32, out: *mut *mut RaynCtx) -> i32;
    pub fn rayn_hip_create_multi(devices: *const i32, n_devices: i32, out: *mut *mut RaynCtx) -> i32;
    pub fn rayn_hip_device_count(ctx: *const RaynCtx) -> i32;
    pub fn rayn_hip_destroy(ctx: *mut RaynCtx);
    pub fn rayn_hip_last_error(ctx: *const RaynCtx) -> *const c_char;
    pub fn rayn_hip_upload_world(ctx: *mut RaynCtx, world: *const RaynWorldDesc) -> i32;
    pub fn rayn_hip_render_frame(
        ctx: *mut RaynCtx,
        p: *const RaynFrameParams,
        samples_1d: *const f32,
        samples_2d: *const f32,
        scramble: *const f32,
        fis_table: *const f32,
        out_color: *mut f32,
        out_alpha: *mut f32,
        out_background: *mut f32,
        out_normal: *mut f32,
    ) -> i32;
    pub fn rayn_hip_get_stats(ctx: *const RaynCtx, out: *mut RaynStats) -> i32;
    /// entry 0 .. rayn_hip_device_count() - 1 of a multi-device context: what THAT device did in the last frame
    pub fn rayn_hip_get_entry_stats(ctx: *const RaynCtx, entry: i32, out: *mut RaynStats) -> i32;
    pub fn rayn_hip_set_fma_policy(ctx: *mut RaynCtx, policy: i32) -> i32;
    pub fn rayn_hip_sizeof(which: i32) -> usize;
    /// bytes of the luminance moments beside one temporal history (a float2 per pixel; 0 for a size the entries reject); host only
    pub fn rayn_temporal_moments_bytes(width: u32, height: u32) -> usize;
    /// the variance-guided a-trous filter of a temporally accumulated Color (device pointers; include/rayn_hip.h has the definition)
    pub fn rayn_hip_denoise_temporal_variance_device(
        ctx: *mut RaynCtx,
        width: u32,
        height: u32,
        iterations: u32,
        sigma_luminance: f32,
        sigma_normal: f32,
        sigma_alpha: f32,
        d_color: *const f32,
        d_alpha: *const f32,
        d_normal: *const f32,
        d_gbuffer_object: *const u32,
        d_history: *const c_void,
        history_bytes: usize,
        d_moments: *const c_void,
        moments_bytes: usize,
        d_out_color: *mut f32,
        d_out_variance: *mut f32,
        d_scratch: *mut c_void,
        scratch_bytes: usize,
        hip_stream: *mut c_void,
    ) -> i32;
    /// the temporal accumulate with a choice of the history resampling filter (`rp.resample`: 0 bilinear, 1 Catmull-Rom); both moments
    /// pointers null: no moments (include/rayn_hip.h has the definition)
    pub fn rayn_hip_temporal_accumulate_resample_device(
        ctx: *mut RaynCtx,
        p: *const RaynFrameParams,
        tp: *const RaynTemporalParams,
        rp: *const RaynTemporalResampleParams,
        prev_camera: *const RaynCamera,
        prev_time_start: f32,
        d_color: *const f32,
        d_normal: *const f32,
        d_gbuffer_records: *const c_void,
        d_gbuffer_object: *const u32,
        d_prev_history: *const c_void,
        d_new_history: *mut c_void,
        history_bytes: usize,
        d_prev_moments: *const c_void,
        d_new_moments: *mut c_void,
        moments_bytes: usize,
        d_out_color: *mut f32,
        hip_stream: *mut c_void,
    ) -> i32;
    /// the same filter with SVGF's feedback edge: pass 0 is blended into the history's colour with strength `feedback` (0 = the entry above)
    pub fn rayn_hip_denoise_temporal_variance_feedback_device(
        ctx: *mut RaynCtx,
        width: u32,
        height: u32,
        iterations: u32,
        sigma_luminance: f32,
        sigma_normal: f32,
        sigma_alpha: f32,
        d_color: *const f32,
        d_alpha: *const f32,
        d_normal: *const f32,
        d_gbuffer_object: *const u32,
        d_history: *mut c_void,
        history_bytes: usize,
        d_moments: *const c_void,
        moments_bytes: usize,
        d_out_color: *mut f32,
        d_out_variance: *mut f32,
        d_scratch: *mut c_void,
        scratch_bytes: usize,
        feedback: f32,
        hip_stream: *mut c_void,
    ) -> i32;
    /// bytes of device scratch the display transform needs (0 for a size it rejects or levels > 8); host only
    pub fn rayn_display_scratch_bytes(width: u32, height: u32, levels: u32) -> usize;
    /// the HDR display transform of the Color kind into the 8-bit image (device pointers; `d_state`: two zeroed u32 words, auto exposure
    /// only; `d_out_meter` / `d_out_bloom` may be null; include/rayn_hip.h has the definition)
    pub fn rayn_hip_display_pixels_device(
        ctx: *mut RaynCtx,
        dp: *const RaynDisplayParams,
        have_mask: u32,
        transparent_background: i32,
        width: u32,
        height: u32,
        d_color: *const f32,
        d_alpha: *const f32,
        d_background: *const f32,
        d_state: *mut c_void,
        d_scratch: *mut c_void,
        scratch_bytes: usize,
        d_out: *mut u8,
        d_out_meter: *mut f32,
        d_out_bloom: *mut f32,
        hip_stream: *mut c_void,
    ) -> i32;
    /// the same with the float plane before gamma and quantisation as the output (width * height * 3 floats, film order)
    pub fn rayn_hip_display_color_device(
        ctx: *mut RaynCtx,
        dp: *const RaynDisplayParams,
        have_mask: u32,
        transparent_background: i32,
        width: u32,
        height: u32,
        d_color: *const f32,
        d_alpha: *const f32,
        d_background: *const f32,
        d_state: *mut c_void,
        d_scratch: *mut c_void,
        scratch_bytes: usize,
        d_out_color: *mut f32,
        d_out_meter: *mut f32,
        d_out_bloom: *mut f32,
        hip_stream: *mut c_void,
    ) -> i32;
    /// guided upscaling of the low film (`width` x `height`) to `factor` times its size with the G-buffers of both resolutions (device
    /// pointers; a plane the film lacks is null in input and output together; `d_out_weight` may be null; include/rayn_hip.h has the definition)
    pub fn rayn_hip_upscale_device(
        ctx: *mut RaynCtx,
        width: u32,
        height: u32,
        up: *const RaynUpscaleParams,
        d_color: *const f32,
        d_alpha: *const f32,
        d_background: *const f32,
        d_normal: *const f32,
        d_low_records: *const c_void,
        d_low_object: *const u32,
        d_high_records: *const c_void,
        d_high_object: *const u32,
        d_out_color: *mut f32,
        d_out_alpha: *mut f32,
        d_out_background: *mut f32,
        d_out_normal: *mut f32,
        d_out_weight: *mut f32,
        hip_stream: *mut c_void,
    ) -> i32;
    /// temporal supersampling: the guided upscaling of the low film (`p.width` x `p.height`) fused with the temporal accumulate at
    /// `up.factor` times that size (device pointers; `low_camera`, `d_prev_history` with `prev_camera`, the Alpha / Background pairs and
    /// `d_out_weight` may be null; `d_out_color` receives the accumulated colour; include/rayn_hip.h has the definition)
    pub fn rayn_hip_temporal_upscale_device(
        ctx: *mut RaynCtx,
        p: *const RaynFrameParams,
        up: *const RaynUpscaleParams,
        tp: *const RaynTemporalParams,
        sp: *const RaynTemporalUpscaleParams,
        low_camera: *const RaynCamera,
        prev_camera: *const RaynCamera,
        prev_time_start: f32,
        d_color: *const f32,
        d_alpha: *const f32,
        d_background: *const f32,
        d_normal: *const f32,
        d_low_records: *const c_void,
        d_low_object: *const u32,
        d_high_records: *const c_void,
        d_high_object: *const u32,
        d_prev_history: *const c_void,
        d_new_history: *mut c_void,
        history_bytes: usize,
        d_out_color: *mut f32,
        d_out_alpha: *mut f32,
        d_out_background: *mut f32,
        d_out_normal: *mut f32,
        d_out_weight: *mut f32,
        hip_stream: *mut c_void,
    ) -> i32;
    /// bytes of device scratch the preview integrator needs (0 for a size it rejects and for `samples` outside 1..64); host only
    pub fn rayn_preview_scratch_bytes(width: u32, height: u32, samples: u32) -> usize;
    /// the preview integrator: primary hit, viewer-facing normal and ambient occlusion of the uploaded world (device pointers;
    /// `d_scramble`, `d_out_ao`, `d_out_records` and `d_out_object` may be null; include/rayn_hip.h has the definition)
    pub fn rayn_hip_preview_device(
        ctx: *mut RaynCtx,
        p: *const RaynFrameParams,
        pp: *const RaynPreviewParams,
        d_samples: *const f32,
        d_scramble: *const f32,
        d_out_color: *mut f32,
        d_out_alpha: *mut f32,
        d_out_normal: *mut f32,
        d_out_ao: *mut f32,
        d_out_records: *mut c_void,
        d_out_object: *mut u32,
        d_scratch: *mut c_void,
        scratch_bytes: usize,
        hip_stream: *mut c_void,
    ) -> i32;
    /// frame generation: the planes of the frame `p` (resolution, time_start) between the rendered keys `key_a` and `key_b`, guided by
    /// the frame's own G-buffer (device pointers; the Alpha / Background / WorldNormal outputs are null together with the keys' planes;
    /// `d_out_source` may be null; include/rayn_hip.h has the definition)
    pub fn rayn_hip_interpolate_device(
        ctx: *mut RaynCtx,
        p: *const RaynFrameParams,
        ip: *const RaynInterpolateParams,
        key_a: *const RaynInterpolateKey,
        key_b: *const RaynInterpolateKey,
        d_gbuffer_records: *const c_void,
        d_gbuffer_object: *const u32,
        d_out_color: *mut f32,
        d_out_alpha: *mut f32,
        d_out_background: *mut f32,
        d_out_normal: *mut f32,
        d_out_source: *mut u32,
        hip_stream: *mut c_void,
    ) -> i32;
    /// PNG encoding on the device: the bytes `d_out` / `d_scratch` of rayn_hip_png_encode_device must have for a width x height image of
    /// `bpp` (1, 3 or 4) bytes per pixel; host only, 0 for a geometry the encoder rejects
    pub fn rayn_png_stream_bound(width: u32, height: u32, bpp: u32) -> usize;
    pub fn rayn_png_scratch_bytes(width: u32, height: u32, bpp: u32) -> usize;
    /// the zlib stream of the PNG IDAT chunk of the 8-bit image `d_img` (rows top-down) behind a 16-byte header whose first word is its
    /// length, enqueued on `hip_stream` (device pointers, `d_out` and `d_scratch` 16-byte aligned; include/rayn_hip.h has the definition)
    pub fn rayn_hip_png_encode_device(
        ctx: *mut RaynCtx,
        width: u32,
        height: u32,
        bpp: u32,
        d_img: *const u8,
        d_out: *mut c_void,
        out_bytes: usize,
        d_scratch: *mut c_void,
        scratch_bytes: usize,
        hip_stream: *mut c_void,
    ) -> i32;
    /// the same with LZ77 matches: rayn_hip_png_encode_device's arguments and output, `d_scratch` of rayn_png_scratch_bytes_lz77 bytes
    pub fn rayn_png_scratch_bytes_lz77(width: u32, height: u32, bpp: u32) -> usize;
    pub fn rayn_hip_png_encode_lz77_device(
        ctx: *mut RaynCtx,
        width: u32,
        height: u32,
        bpp: u32,
        d_img: *const u8,
        d_out: *mut c_void,
        out_bytes: usize,
        d_scratch: *mut c_void,
        scratch_bytes: usize,
        hip_stream: *mut c_void,
    ) -> i32;
    /// its deflate stage alone on `n` bytes at `d_data` (1 <= n < 2^31; `stride`: the row candidate's distance, 0 for none): the same
    /// header and a zlib stream; host-only byte counts of `d_out` and `d_scratch`, 0 for a rejected size
    pub fn rayn_deflate_stream_bound(n: usize) -> usize;
    pub fn rayn_deflate_scratch_bytes(n: usize) -> usize;
    pub fn rayn_hip_deflate_lz77_device(
        ctx: *mut RaynCtx,
        d_data: *const c_void,
        n: usize,
        stride: u32,
        d_out: *mut c_void,
        out_bytes: usize,
        d_scratch: *mut c_void,
        scratch_bytes: usize,
        hip_stream: *mut c_void,
    ) -> i32;
    /// OpenEXR chunks on the device: the bytes `d_out` / `d_scratch` of rayn_hip_exr_encode_device must have; `layout` holds (stride,
    /// offset, type) per channel, 3 * n_channels words on the host; host only, 0 for what the entry rejects
    pub fn rayn_exr_stream_bound(width: u32, height: u32, n_channels: u32, layout: *const u32) -> usize;
    pub fn rayn_exr_scratch_bytes(width: u32, height: u32, n_channels: u32, layout: *const u32, matches: u32) -> usize;
    /// the ZIP-compressed scanline chunks of an OpenEXR file from `n_channels` planes in the film's layout (`d_planes`: device pointers in
    /// a host array, channels in the file's order; type 0 UINT, 1 HALF, 2 FLOAT; `matches` 0 run-length blocks, 1 LZ77 blocks) behind
    /// four words and a chunk table, enqueued on `hip_stream` (include/rayn_hip.h has the definition)
    pub fn rayn_hip_exr_encode_device(
        ctx: *mut RaynCtx,
        width: u32,
        height: u32,
        n_channels: u32,
        d_planes: *const *const c_void,
        layout: *const u32,
        matches: u32,
        d_out: *mut c_void,
        out_bytes: usize,
        d_scratch: *mut c_void,
        scratch_bytes: usize,
        hip_stream: *mut c_void,
    ) -> i32;
}

/// Start-up layout check against the library as compiled (indices: include/rayn_hip.h, rayn_hip_sizeof).
pub fn check_layout() -> Result<(), String> {
    use std::mem::size_of;
    let expect = [
        (0, size_of::<RaynWorldDesc>(), "RaynWorldDesc"),
        (1, size_of::<RaynFrameParams>(), "RaynFrameParams"),
        (2, size_of::<RaynStats>(), "RaynStats"),
        (3, size_of::<RaynHitable>(), "RaynHitable"),
        (4, size_of::<RaynMaterial>(), "RaynMaterial"),
        (5, size_of::<RaynLight>(), "RaynLight"),
        (6, size_of::<RaynCamera>(), "RaynCamera"),
    ];
    for (which, size, name) in expect.iter() {
        let lib = unsafe { rayn_hip_sizeof(*which) };
        if lib != *size {
            return Err(format!("{}: binding has {} bytes, librayn_hip.so has {}", name, size, lib));
        }
    }
    Ok(())
}

// ---- glue used by the `describe()` methods bindings/rayn.patch adds to rayn's scene types ---------------------------------

impl From<crate::math::Vec3> for RaynVec3 {
    fn from(v: crate::math::Vec3) -> Self {
        RaynVec3 { x: v.x, y: v.y, z: v.z }
    }
}

/// lane 0 of a wide value (`f32x4::as_ref` -> `[f32; 4]`, the idiom of src/animation.rs:39-41)
pub fn lane0(v: crate::math::f32x4) -> f32 {
    let lanes = v.as_ref();
    lanes[0]
}

fn moves(vel: crate::math::Vec3) -> bool {
    vel.x != 0.0 || vel.y != 0.0 || vel.z != 0.0
}

/// `(base, vel)` of `WSequenced::as_linear` into the descriptor: bit 0 origin, 1 at, 2 up, 3 focus of `animated`
impl RaynCamera {
    pub fn set_origin(&mut self, (base, vel): (crate::math::Vec3, crate::math::Vec3)) {
        self.origin = base.into();
        self.origin_vel = vel.into();
        self.animated |= (moves(vel) as u32) << 0;
    }
    pub fn set_at(&mut self, (base, vel): (crate::math::Vec3, crate::math::Vec3)) {
        self.at = base.into();
        self.at_vel = vel.into();
        self.animated |= (moves(vel) as u32) << 1;
    }
    pub fn set_up(&mut self, (base, vel): (crate::math::Vec3, crate::math::Vec3)) {
        self.up = base.into();
        self.up_vel = vel.into();
        self.animated |= (moves(vel) as u32) << 2;
    }
    pub fn set_focus(&mut self, (base, vel): (crate::math::Vec3, crate::math::Vec3)) {
        self.focus = base.into();
        self.focus_vel = vel.into();
        self.animated |= (moves(vel) as u32) << 3;
    }
}

/// Owning handle of a `rayn_ctx` (one GPU, or several: `rayn_hip_create_multi`).  Every failing call returns the library's
/// message (`rayn_hip_last_error`) as `Err(String)` - the hot path of the reference panics instead (src/film.rs:127,667).
pub struct Context {
    raw: *mut RaynCtx,
}

// the library serialises calls on one ctx itself (include/rayn_hip.h: "not re-entrant per ctx"); the handle is moved, not shared
unsafe impl Send for Context {}

impl Context {
    pub fn new(devices: &[i32]) -> Result<Self, String> {
        check_layout()?;
        let mut raw: *mut RaynCtx = std::ptr::null_mut();
        let rc = unsafe {
            if devices.len() == 1 {
                rayn_hip_create(devices[0], &mut raw)
            } else {
                rayn_hip_create_multi(devices.as_ptr(), devices.len() as i32, &mut raw)
            }
        };
        if rc != 0 || raw.is_null() {
            return Err(format!("rayn_hip_create{:?} failed with status {}", devices, rc));
        }
        Ok(Context { raw })
    }

    pub fn raw(&self) -> *mut RaynCtx {
        self.raw
    }

    /// status -> Result, with the library's text
    pub fn check(&self, rc: i32) -> Result<(), String> {
        if rc == 0 {
            return Ok(());
        }
        let msg = unsafe { std::ffi::CStr::from_ptr(rayn_hip_last_error(self.raw)) };
        Err(format!("librayn_hip status {}: {}", rc, msg.to_string_lossy()))
    }
}

impl Drop for Context {
    fn drop(&mut self) {
        unsafe { rayn_hip_destroy(self.raw) }
    }
}
