// rayn_host.hpp — C++ host-side mirror of rayn's scene/film API on top of the C ABI (rayn_hip.h).
//
// The reference is compiled Rust; its toolchain is absent here, so this header is the compiled-language
// host side: the same type and method names, argument order and meaning as the reference, flattening to
// the POD `rayn_world_desc` exactly where a Rust shim would.  Header-only; link with
// -lrayn_hip.  All construction-time arithmetic is f32 in the reference's operation order (compile with
// -ffp-contract=off if bit-equality of the scene constants with another host matters).
//
//   reference                                              here
//   Srgb::new / * f32 / normalized   src/spectrum.rs        rayn::Srgb
//   Sphere::new(center, r, mat)      src/sphere.rs:14-20    rayn::Sphere
//   TracedSDF::new(sdf, mat)         src/sdf.rs:17-21       rayn::TracedSDF
//   MandelBox::new / BoxFold / SphereFold  src/sdf.rs:114,151,172
//   Lambertian / Dielectric::new_remap / Sky::new / Emissive::new_splat   src/material.rs
//   MaterialStore::add_material -> MaterialHandle            src/material.rs:55-73
//   SphereLight::new                 src/light.rs:27-33
//   Pinhole/ThinLens/OrthographicCamera::new, CameraStore   src/camera.rs
//   VolumeParams, World              src/volume.rs, src/world.rs
//   PathTracingIntegrator            src/integrator.rs:32-45
//   BlackmanHarrisFilter / BoxFilter / MitchellNetravaliFilter / LanczosSincFilter src/filter.rs:12-185
//   Film::new / render_frame_into    src/film.rs:184-203, 382-395
//   setup::setup()                   src/setup.rs:46-170
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <variant>
#include <vector>

#include "rayn_hip.h"

namespace rayn {

struct Vec3 {
    float x = 0, y = 0, z = 0;
    Vec3() = default;
    Vec3(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
    static Vec3 zero() { return Vec3(0, 0, 0); }
    Vec3 operator*(float s) const { return Vec3(x * s, y * s, z * s); }
    // ultraviolet's SCALAR Vec3 (oracle assumption A4/A9): mag_sq = x.mul_add(x, y.mul_add(y, z * z)), v * (1 / mag).  Rust's scalar
    // f32::mul_add is ALWAYS a fused multiply-add (libm fmaf when the target has no FMA unit) - under both build policies of the
    // wide types - so the host mirror uses std::fmaf unconditionally (src/setup.rs:100-101 is the call site of the shipped scene).
    Vec3 normalized() const {
        float m2 = std::fmaf(x, x, std::fmaf(y, y, z * z));
        float r = 1.0f / std::sqrt(m2);
        return Vec3(x * r, y * r, z * r);
    }
    rayn_vec3 pod() const { return rayn_vec3{x, y, z}; }
};
struct Vec2 { float x = 0, y = 0; Vec2() = default; Vec2(float x_, float y_) : x(x_), y(y_) {} };
struct Extent2u { uint32_t w = 0, h = 0; Extent2u() = default; Extent2u(uint32_t w_, uint32_t h_) : w(w_), h(h_) {} };

struct Srgb { // src/spectrum.rs:5-75
    Vec3 v;
    Srgb() = default;
    Srgb(float r, float g, float b) : v(r, g, b) {}
    static Srgb new_(float r, float g, float b) { return Srgb(r, g, b); }
    Srgb operator*(float s) const { Srgb o; o.v = v * s; return o; }
    Srgb normalized() const { Srgb o; o.v = v.normalized(); return o; }
};

struct MaterialHandle { size_t idx = 0; };
struct CameraHandle { size_t idx = 0; };

// ---- materials ---------------------------------------------------------------------------------
struct Lambertian { Srgb albedo; static Lambertian new_(Srgb a) { return Lambertian{a}; } };
struct Dielectric {
    Srgb albedo; float exponent;
    // Roughness between 0.0 (smooth) and 1.0 (rough); src/material.rs:167-174
    static Dielectric new_remap(Srgb albedo, float roughness) {
        float r = 1.0f - roughness;
        float e = 1.0f + r * r * r * r * 300.0f;
        return Dielectric{albedo, e};
    }
};
struct Sky { Srgb top, bottom; static Sky new_(Srgb t, Srgb b) { return Sky{t, b}; } };
struct Emissive { Srgb emission; static Emissive new_splat(Srgb e) { return Emissive{e}; } };
using Material = std::variant<Lambertian, Dielectric, Sky, Emissive>;

class MaterialStore {
  public:
    MaterialHandle add_material(Material m) { mats.push_back(std::move(m)); return MaterialHandle{mats.size() - 1}; }
    size_t len() const { return mats.size(); }
    std::vector<Material> mats;
};

// ---- SDFs + hitables ----------------------------------------------------------------------------
struct BoxFold { float side_length; static BoxFold new_(float s) { return BoxFold{s}; } };
struct SphereFold { float min_radius, fixed_radius; static SphereFold new_(float a, float b) { return SphereFold{a, b}; } };
struct MandelBox {
    uint32_t iterations; BoxFold box_fold; SphereFold sphere_fold; float scale;
    float scale_vel = 0.0f; // EXTENSION: scale(t) = scale + scale_vel * t at lane-0 time (rayn_hip.h); 0 = the reference
    static MandelBox new_(uint32_t it, BoxFold b, SphereFold s, float scale) { MandelBox m{it, b, s, scale}; return m; }
};
struct SphereSDF { float radius; }; // sdfu::Sphere::new(radius)
using SDF = std::variant<MandelBox, SphereSDF>;

// A time-sequenced Vec3 (src/animation.rs): a constant, or the closure `move |t| base + vel * t`
struct Sequenced3 {
    Vec3 base, vel; bool animated = false;
    Sequenced3() = default;
    Sequenced3(Vec3 constant) : base(constant) {}
    static Sequenced3 linear(Vec3 base, Vec3 vel) { Sequenced3 s; s.base = base; s.vel = vel; s.animated = true; return s; }
};

struct Sphere { Sequenced3 transform_seq; float radius; MaterialHandle material;
                static Sphere new_(Sequenced3 c, float r, MaterialHandle m) { return Sphere{c, r, m}; } };
// transform_seq is an EXTENSION (the reference's TracedSDF has none, src/sdf.rs:12-21): Sphere's transform semantics for
// an SDF - constant or |t| base + vel * t sampled at the packet's lane-0 time; default = the reference's behaviour.
struct TracedSDF { SDF sdf; MaterialHandle material; Sequenced3 transform_seq;
                   static TracedSDF new_(SDF s, MaterialHandle m) { return TracedSDF{std::move(s), m, Sequenced3()}; }
                   static TracedSDF new_moving(SDF s, MaterialHandle m, Sequenced3 tr) { return TracedSDF{std::move(s), m, tr}; } };
using Hitable = std::variant<Sphere, TracedSDF>;

class HitableStore {
  public:
    void push(Hitable h) { items.push_back(std::move(h)); }
    size_t len() const { return items.size(); }
    std::vector<Hitable> items;
};

// ---- lights, cameras, volume --------------------------------------------------------------------
struct SphereLight { Vec3 pos; float rad; Srgb emission; static SphereLight new_(Vec3 p, float r, Srgb e) { return SphereLight{p, r, e}; } };

struct PinholeCamera { Vec2 resolution; float vfov; Sequenced3 origin, at, up;
                       static PinholeCamera new_(Vec2 res, float vfov, Sequenced3 o, Sequenced3 a, Sequenced3 u) { return PinholeCamera{res, vfov, o, a, u}; } };
struct ThinLensCamera { Vec2 resolution; float vfov, aperture; Sequenced3 origin, at, up, focus;
                        static ThinLensCamera new_(Vec2 res, float vfov, float ap, Sequenced3 o, Sequenced3 a, Sequenced3 u, Sequenced3 f) { return ThinLensCamera{res, vfov, ap, o, a, u, f}; } };
struct OrthographicCamera { Vec2 resolution; float vertical_size; Sequenced3 origin, at, up;
                            static OrthographicCamera new_(Vec2 res, float vs, Sequenced3 o, Sequenced3 a, Sequenced3 u) { return OrthographicCamera{res, vs, o, a, u}; } };
using Camera = std::variant<PinholeCamera, ThinLensCamera, OrthographicCamera>;
class CameraStore {
  public:
    CameraHandle add_camera(Camera c) { cams.push_back(std::move(c)); return CameraHandle{cams.size() - 1}; }
    const Camera& get(CameraHandle h) const { return cams.at(h.idx); }
    std::vector<Camera> cams;
};

struct VolumeParams { std::optional<float> coeff_scattering, coeff_extinction; };

struct World { // src/world.rs:7-13
    HitableStore hitables;
    std::vector<SphereLight> lights;
    MaterialStore materials;
    CameraStore cameras;
    VolumeParams volume_params;

    // flatten to the C-ABI descriptor; scene order is preserved (it is semantic, src/hitable.rs:170-210)
    rayn_world_desc to_desc(CameraHandle camera) const {
        if (hitables.len() > RAYN_MAX_HITABLES || materials.len() > RAYN_MAX_MATERIALS || lights.size() > RAYN_MAX_LIGHTS)
            throw std::invalid_argument("scene exceeds the C-ABI fixed capacities");
        rayn_world_desc d;
        std::memset(&d, 0, sizeof d);
        d.n_hitables = (uint32_t)hitables.len(); d.n_materials = (uint32_t)materials.len(); d.n_lights = (uint32_t)lights.size();
        for (size_t i = 0; i < hitables.len(); i++) {
            rayn_hitable& o = d.hitables[i];
            if (const Sphere* s = std::get_if<Sphere>(&hitables.items[i])) {
                o.kind = RAYN_HITABLE_SPHERE; o.material = (uint32_t)s->material.idx; o.center = s->transform_seq.base.pod(); o.radius = s->radius;
                if (s->transform_seq.animated) { o.animated = 1; o.center_vel = s->transform_seq.vel.pod(); }
            } else {
                const TracedSDF& t = std::get<TracedSDF>(hitables.items[i]);
                o.kind = RAYN_HITABLE_TRACED_SDF; o.material = (uint32_t)t.material.idx; o.center = t.transform_seq.base.pod();
                if (t.transform_seq.animated) { o.animated = 1; o.center_vel = t.transform_seq.vel.pod(); }
                if (const MandelBox* m = std::get_if<MandelBox>(&t.sdf)) {
                    o.sdf_kind = RAYN_SDF_MANDELBOX; o.iterations = m->iterations; o.box_side = m->box_fold.side_length;
                    o.min_radius = m->sphere_fold.min_radius; o.fixed_radius = m->sphere_fold.fixed_radius; o.scale = m->scale; o.scale_vel = m->scale_vel;
                } else { o.sdf_kind = RAYN_SDF_SPHERE; o.sdf_radius = std::get<SphereSDF>(t.sdf).radius; }
            }
        }
        for (size_t i = 0; i < materials.len(); i++) {
            rayn_material& o = d.materials[i];
            const Material& m = materials.mats[i];
            if (const Lambertian* l = std::get_if<Lambertian>(&m)) { o.kind = RAYN_MAT_LAMBERTIAN; o.a = l->albedo.v.pod(); }
            else if (const Dielectric* di = std::get_if<Dielectric>(&m)) { o.kind = RAYN_MAT_DIELECTRIC; o.a = di->albedo.v.pod(); o.exponent = di->exponent; }
            else if (const Sky* s = std::get_if<Sky>(&m)) { o.kind = RAYN_MAT_SKY; o.a = s->top.v.pod(); o.b = s->bottom.v.pod(); }
            else { o.kind = RAYN_MAT_EMISSIVE; o.a = std::get<Emissive>(m).emission.v.pod(); }
        }
        for (size_t i = 0; i < lights.size(); i++) {
            d.lights[i].pos = lights[i].pos.pod(); d.lights[i].rad = lights[i].rad; d.lights[i].emission = lights[i].emission.v.pod();
        }
        rayn_camera& c = d.camera;
        const Camera& cam = cameras.get(camera);
        auto put = [&c](rayn_vec3& dst, rayn_vec3& vel, uint32_t bit, const Sequenced3& s) { dst = s.base.pod(); if (s.animated) { vel = s.vel.pod(); c.animated |= 1u << bit; } };
        if (const PinholeCamera* p = std::get_if<PinholeCamera>(&cam)) {
            c.kind = RAYN_CAM_PINHOLE; c.res_w = p->resolution.x; c.res_h = p->resolution.y; c.vfov_or_size = p->vfov;
            put(c.origin, c.origin_vel, 0, p->origin); put(c.at, c.at_vel, 1, p->at); put(c.up, c.up_vel, 2, p->up);
        } else if (const ThinLensCamera* t = std::get_if<ThinLensCamera>(&cam)) {
            c.kind = RAYN_CAM_THIN_LENS; c.res_w = t->resolution.x; c.res_h = t->resolution.y; c.vfov_or_size = t->vfov; c.aperture = t->aperture;
            put(c.origin, c.origin_vel, 0, t->origin); put(c.at, c.at_vel, 1, t->at); put(c.up, c.up_vel, 2, t->up); put(c.focus, c.focus_vel, 3, t->focus);
        } else {
            const OrthographicCamera& o = std::get<OrthographicCamera>(cam);
            c.kind = RAYN_CAM_ORTHOGRAPHIC; c.res_w = o.resolution.x; c.res_h = o.resolution.y; c.vfov_or_size = o.vertical_size;
            put(c.origin, c.origin_vel, 0, o.origin); put(c.at, c.at_vel, 1, o.at); put(c.up, c.up_vel, 2, o.up);
        }
        if (volume_params.coeff_scattering) { d.has_scattering = 1; d.coeff_scattering = *volume_params.coeff_scattering; }
        if (volume_params.coeff_extinction) { d.has_extinction = 1; d.coeff_extinction = *volume_params.coeff_extinction; }
        return d;
    }
};

// ---- integrator + filters -----------------------------------------------------------------------
struct PathTracingIntegrator { // src/integrator.rs:32-45
    size_t max_bounces = 3, volume_marches = 2;
    size_t requested_1d_sample_sets() const { return (max_bounces + 1) * (3 + volume_marches); }
    size_t requested_2d_sample_sets() const { return (max_bounces + 1) * (12 + 8 * volume_marches); }
};
struct BlackmanHarrisFilter { float radius_ = 1.5f; static BlackmanHarrisFilter new_(float r) { return BlackmanHarrisFilter{r}; }
                              float radius() const { return radius_; } static constexpr uint32_t kind = 0; };
struct BoxFilter { float radius_ = 0.5f; static BoxFilter new_(float r) { return BoxFilter{r}; }
                   float radius() const { return radius_; } static constexpr uint32_t kind = 1; };
struct MitchellNetravaliFilter { // src/filter.rs:51-108
    float radius_ = 2.0f, b = 1.0f / 3.0f, c = 1.0f / 3.0f;
    static MitchellNetravaliFilter new_(float r, float b, float c) { return MitchellNetravaliFilter{r, b, c}; }
    float radius() const { return radius_; } float param0() const { return b; } float param1() const { return c; }
    static constexpr uint32_t kind = 2;
};
struct LanczosSincFilter { // src/filter.rs:142-185
    float radius_ = 3.0f, tau = 3.0f;
    static LanczosSincFilter new_(float r, float tau) { return LanczosSincFilter{r, tau}; }
    float radius() const { return radius_; } float param0() const { return tau; } float param1() const { return 0.0f; }
    static constexpr uint32_t kind = 3;
};
namespace detail { // parameter-free filters have no param0()/param1()
template <class F> auto filter_p0(const F& f, int) -> decltype(f.param0()) { return f.param0(); }
template <class F> float filter_p0(const F&, long) { return 0.0f; }
template <class F> auto filter_p1(const F& f, int) -> decltype(f.param1()) { return f.param1(); }
template <class F> float filter_p1(const F&, long) { return 0.0f; }
}

// constants the tile closure reads (src/setup.rs:16-44, src/sdf.rs:9-10)
struct RenderConstants { uint32_t max_marches = 256, max_vis_marches = 100; float sdf_detail_scale = 0.5f, world_radius = 100.0f; };

// ---- Film ----------------------------------------------------------------------------------------
enum class ChannelKind { Color, Alpha, Background, WorldNormal }; // src/film.rs:103-120

class Film {
  public:
    // Film::new (src/film.rs:184-203): duplicate channel kinds are an error
    Film(const std::vector<ChannelKind>& channels, Extent2u res, int device = 0) : kinds_(channels), res_(res) {
        for (size_t i = 0; i < channels.size(); i++)
            for (size_t j = i + 1; j < channels.size(); j++)
                if (channels[i] == channels[j]) throw std::invalid_argument("Attempted to create multiple channels of one kind");
        int rc = rayn_hip_create(device, &ctx_);
        if (rc != RAYN_OK) throw std::runtime_error("rayn_hip_create failed: " + std::to_string(rc) + " (no GPU? there is no CPU fallback)");
        const size_t n = (size_t)res.w * res.h;
        color.assign(3 * n, 0.0f); alpha.assign(n, 0.0f); background.assign(3 * n, 0.0f); world_normal.assign(3 * n, 0.0f);
    }
    // the same film rendered by several GPUs of this process (rayn_hip_create_multi: tiles dealt in rotation, one peer copy per GPU)
    Film(const std::vector<ChannelKind>& channels, Extent2u res, const std::vector<int>& devices) : kinds_(channels), res_(res) {
        for (size_t i = 0; i < channels.size(); i++)
            for (size_t j = i + 1; j < channels.size(); j++)
                if (channels[i] == channels[j]) throw std::invalid_argument("Attempted to create multiple channels of one kind");
        int rc = rayn_hip_create_multi(devices.data(), (int)devices.size(), &ctx_);
        if (rc != RAYN_OK) throw std::runtime_error("rayn_hip_create_multi failed: " + std::to_string(rc) + " (no GPU? there is no CPU fallback)");
        const size_t n = (size_t)res.w * res.h;
        color.assign(3 * n, 0.0f); alpha.assign(n, 0.0f); background.assign(3 * n, 0.0f); world_normal.assign(3 * n, 0.0f);
    }
    ~Film() { if (ctx_) rayn_hip_destroy(ctx_); }
    Film(const Film&) = delete;
    Film& operator=(const Film&) = delete;

    // Film::render_frame_into (src/film.rs:382-395); the film is overwritten, not accumulated (src/film.rs:91)
    template <typename F>
    void render_frame_into(const World& world, CameraHandle camera, const PathTracingIntegrator& integrator, const F& filter,
                           Extent2u tile_size, size_t frame, std::pair<float, float> time_range, size_t samples,
                           const RenderConstants& k = RenderConstants()) {
        rayn_world_desc desc = world.to_desc(camera);
        check(rayn_hip_upload_world(ctx_, &desc));
        rayn_frame_params p;
        std::memset(&p, 0, sizeof p);
        p.width = res_.w; p.height = res_.h; p.samples = (uint32_t)samples; p.tile_w = tile_size.w; p.tile_h = tile_size.h;
        p.max_bounces = (uint32_t)integrator.max_bounces; p.volume_marches = (uint32_t)integrator.volume_marches; p.frame = (uint32_t)frame;
        p.time_start = time_range.first; p.time_end = time_range.second;
        p.max_marches = k.max_marches; p.max_vis_marches = k.max_vis_marches; p.sdf_detail_scale = k.sdf_detail_scale; p.world_radius = k.world_radius;
        p.tile_first = 0; p.tile_step = 1;
        const uint32_t spp = 4u * (uint32_t)samples;
        const uint32_t sets_1d = 1 + (uint32_t)integrator.requested_1d_sample_sets(), sets_2d = 2 + (uint32_t)integrator.requested_2d_sample_sets(); // src/film.rs:431-432
        std::vector<float> s1((size_t)spp * sets_1d), s2((size_t)spp * 2 * sets_2d), scr((size_t)res_.w * res_.h), fis(RAYN_FIS_TABLE_SIZE);
        check(rayn_build_rd_tables(spp, sets_1d, sets_2d, frame, s1.data(), s2.data()));   // Samples::new_rd, src/film.rs:434
        check(rayn_build_scramble(res_.w, res_.h, scr.data()));                              // src/film.rs:460-461
        check(rayn_build_fis_table_ex(F::kind, filter.radius(), detail::filter_p0(filter, 0), detail::filter_p1(filter, 0), fis.data()));                   // src/film.rs:429
        check(rayn_hip_render_frame(ctx_, &p, s1.data(), s2.data(), scr.data(), fis.data(), color.data(), alpha.data(), background.data(),
                                    world_normal.data()));
        progressive_epoch++;
    }
    rayn_stats stats() const { rayn_stats s; rayn_hip_get_stats(ctx_, &s); return s; }
    // what GPU `entry` of a multi-device film did in the last frame (its tiles / segments / its own HIP-event time): rayn_hip_get_entry_stats
    int device_count() const { return rayn_hip_device_count(ctx_); }
    rayn_stats device_stats(int entry) const {
        rayn_stats s;
        if (rayn_hip_get_entry_stats(ctx_, entry, &s) != RAYN_OK) throw std::runtime_error("rayn_hip_get_entry_stats: no such entry");
        return s;
    }
    Extent2u res() const { return res_; }
    rayn_ctx* ctx() { return ctx_; }

    // channel storage, bottom-up rows like the reference (the flip happens in save_to, src/film.rs:236)
    std::vector<float> color, alpha, background, world_normal;
    size_t progressive_epoch = 0;

  private:
    void check(int rc) { if (rc != RAYN_OK) throw std::runtime_error(std::string("rayn_hip: ") + rayn_hip_last_error(ctx_)); }
    std::vector<ChannelKind> kinds_;
    Extent2u res_;
    rayn_ctx* ctx_ = nullptr;
};

// Extension (include/rayn_hip.h: temporal accumulate with luminance moments): bytes of the moments beside one temporal history of a film
// of this size, 8 per pixel; 0 for a size the entries reject.  Host only.
inline size_t temporal_moments_bytes(Extent2u res) { return rayn_temporal_moments_bytes(res.w, res.h); }

// Extension (include/rayn_hip.h: rayn_hip_temporal_accumulate_resample_device): the temporal accumulate with a choice of the history
// resampling filter.  Device pointers; the moments pointers may both be null (no moments).  Returns the entry's code.
enum class TemporalResample : uint32_t { Bilinear = 0, CatmullRom = 1 };
inline int temporal_accumulate_resample(rayn_ctx* ctx, const rayn_frame_params& p, const rayn_temporal_params& tp, TemporalResample resample,
                                        const rayn_camera* prev_camera, float prev_time_start, const float* d_color, const float* d_normal,
                                        const void* d_gbuffer_records, const uint32_t* d_gbuffer_object, const void* d_prev_history,
                                        void* d_new_history, size_t history_bytes, const void* d_prev_moments, void* d_new_moments,
                                        size_t moments_bytes, float* d_out_color, void* hip_stream = nullptr) {
    const rayn_temporal_resample_params rp = {static_cast<uint32_t>(resample)};
    return rayn_hip_temporal_accumulate_resample_device(ctx, &p, &tp, &rp, prev_camera, prev_time_start, d_color, d_normal, d_gbuffer_records,
                                                        d_gbuffer_object, d_prev_history, d_new_history, history_bytes, d_prev_moments,
                                                        d_new_moments, moments_bytes, d_out_color, hip_stream);
}

// Extension (include/rayn_hip.h: the HDR display transform): auto exposure, bloom and tone mapping of the Color kind in front of save_to's
// gamma and quantisation.  display_params() fills the block from the terms a user thinks in - an EV (NaN = auto exposure), the Reinhard
// white point, bloom levels (0 = off); display_pixels() is the 8-bit entry.  Device pointers; d_state (two zeroed 32-bit words) is needed
// with auto exposure only, d_scratch (display_scratch_bytes) with auto exposure or bloom.  Returns the entry's code.
enum class Tone : uint32_t { Linear = 0, Reinhard = 1, Aces = 2 };
inline size_t display_scratch_bytes(Extent2u res, uint32_t levels) { return rayn_display_scratch_bytes(res.w, res.h, levels); }
inline rayn_display_params display_params(Tone tone, float ev, float key = 0.18f, float white = 4.0f, uint32_t levels = 0,
                                          float threshold = 1.0f, float strength = 0.5f, float adapt = 1.0f) {
    const bool automatic = ev != ev;
    return rayn_display_params{static_cast<uint32_t>(tone), automatic ? 1u : 0u, automatic ? 1.0f : static_cast<float>(std::exp2(static_cast<double>(ev))),
                               key, adapt, 1.0f / (white * white), levels, threshold, strength};
}
inline int display_pixels(rayn_ctx* ctx, const rayn_display_params& dp, uint32_t have_mask, bool transparent_background, Extent2u res,
                          const float* d_color, const float* d_alpha, const float* d_background, void* d_state, void* d_scratch,
                          size_t scratch_bytes, uint8_t* d_out, void* hip_stream = nullptr) {
    return rayn_hip_display_pixels_device(ctx, &dp, have_mask, transparent_background ? 1 : 0, res.w, res.h, d_color, d_alpha, d_background, d_state,
                                          d_scratch, scratch_bytes, d_out, nullptr, nullptr, hip_stream);
}

// Extension (include/rayn_hip.h: guided upscaling): the low film of `res` and the primary-hit G-buffers of both resolutions -> the planes of
// the film at factor * res.  Device pointers; a plane the film lacks is null in input and output together; d_out_weight may be null.
// Returns the entry's code.
inline int upscale(rayn_ctx* ctx, Extent2u res, uint32_t factor, float sigma_plane, float sigma_position, const float* d_color, const float* d_alpha,
                   const float* d_background, const float* d_normal, const void* d_low_records, const uint32_t* d_low_object,
                   const void* d_high_records, const uint32_t* d_high_object, float* d_out_color, float* d_out_alpha, float* d_out_background,
                   float* d_out_normal, float* d_out_weight = nullptr, void* hip_stream = nullptr) {
    const rayn_upscale_params up = {factor, sigma_plane, sigma_position};
    return rayn_hip_upscale_device(ctx, res.w, res.h, &up, d_color, d_alpha, d_background, d_normal, d_low_records, d_low_object, d_high_records,
                                   d_high_object, d_out_color, d_out_alpha, d_out_background, d_out_normal, d_out_weight, hip_stream);
}

// Extension (include/rayn_hip.h: temporal supersampling): the guided upscaling fused with the temporal accumulate at factor * res, the
// history at the high size.  `res`, p.width and p.height are the LOW film's; low_camera is the (jittered) camera the low film and the low
// G-buffer were traced through, or null.  Device pointers; d_out_color receives the accumulated colour.  Returns the entry's code.
inline int temporal_upscale(rayn_ctx* ctx, const rayn_frame_params& p, const rayn_upscale_params& up, const rayn_temporal_params& tp, bool confidence,
                            const rayn_camera* low_camera, const rayn_camera* prev_camera, float prev_time_start, const float* d_color,
                            const float* d_alpha, const float* d_background, const float* d_normal, const void* d_low_records,
                            const uint32_t* d_low_object, const void* d_high_records, const uint32_t* d_high_object, const void* d_prev_history,
                            void* d_new_history, size_t history_bytes, float* d_out_color, float* d_out_alpha, float* d_out_background,
                            float* d_out_normal, float* d_out_weight = nullptr, void* hip_stream = nullptr) {
    const rayn_temporal_upscale_params sp = {confidence ? 1u : 0u};
    return rayn_hip_temporal_upscale_device(ctx, &p, &up, &tp, &sp, low_camera, prev_camera, prev_time_start, d_color, d_alpha, d_background, d_normal,
                                            d_low_records, d_low_object, d_high_records, d_high_object, d_prev_history, d_new_history, history_bytes,
                                            d_out_color, d_out_alpha, d_out_background, d_out_normal, d_out_weight, hip_stream);
}

// Extension (include/rayn_hip.h: the preview integrator): primary hit, viewer-facing normal and ambient occlusion of the uploaded world under
// p - the geometry alone.  Device pointers; d_samples holds `samples` float pairs; d_scramble (one float per pixel), d_out_ao, d_out_records
// and d_out_object may be null; d_scratch holds at least preview_scratch_bytes.  Returns the entry's code.
inline size_t preview_scratch_bytes(Extent2u res, uint32_t samples) { return rayn_preview_scratch_bytes(res.w, res.h, samples); }
inline int preview(rayn_ctx* ctx, const rayn_frame_params& p, uint32_t samples, float radius, float ambient, const float* d_samples,
                   const float* d_scramble, float* d_out_color, float* d_out_alpha, float* d_out_normal, float* d_out_ao, void* d_out_records,
                   uint32_t* d_out_object, void* d_scratch, size_t scratch_bytes, void* hip_stream = nullptr) {
    const rayn_preview_params pp = {samples, radius, ambient};
    return rayn_hip_preview_device(ctx, &p, &pp, d_samples, d_scramble, d_out_color, d_out_alpha, d_out_normal, d_out_ao, d_out_records, d_out_object,
                                   d_scratch, scratch_bytes, hip_stream);
}

// Extension (include/rayn_hip.h: frame generation): the planes of the frame p (resolution, time_start) between the rendered keys a and b,
// guided by the frame's own G-buffer.  Device pointers; the Alpha / Background / WorldNormal outputs are null together with the keys'
// planes; d_out_source may be null.  Returns the entry's code.
inline int interpolate(rayn_ctx* ctx, const rayn_frame_params& p, float depth_tolerance, const rayn_interpolate_key& a, const rayn_interpolate_key& b,
                       const void* d_gbuffer_records, const uint32_t* d_gbuffer_object, float* d_out_color, float* d_out_alpha,
                       float* d_out_background, float* d_out_normal, uint32_t* d_out_source = nullptr, void* hip_stream = nullptr) {
    const rayn_interpolate_params ip = {depth_tolerance};
    return rayn_hip_interpolate_device(ctx, &p, &ip, &a, &b, d_gbuffer_records, d_gbuffer_object, d_out_color, d_out_alpha, d_out_background,
                                       d_out_normal, d_out_source, hip_stream);
}

// Extension (include/rayn_hip.h: PNG encoding on the device): the zlib stream of the IDAT chunk of the 8-bit image d_img (res.w x res.h
// pixels of bpp bytes, rows top-down) behind a 16-byte header whose first word is its length.  Device pointers; d_out of at least
// png_stream_bound bytes, d_scratch of at least png_scratch_bytes, both 16-byte aligned.  Returns the entry's code.
inline size_t png_stream_bound(Extent2u res, uint32_t bpp) { return rayn_png_stream_bound(res.w, res.h, bpp); }
inline size_t png_scratch_bytes(Extent2u res, uint32_t bpp) { return rayn_png_scratch_bytes(res.w, res.h, bpp); }
inline int png_encode(rayn_ctx* ctx, Extent2u res, uint32_t bpp, const uint8_t* d_img, void* d_out, size_t out_bytes, void* d_scratch,
                      size_t scratch_bytes, void* hip_stream = nullptr) {
    return rayn_hip_png_encode_device(ctx, res.w, res.h, bpp, d_img, d_out, out_bytes, d_scratch, scratch_bytes, hip_stream);
}

// The same with LZ77 matches (include/rayn_hip.h: PNG encoding on the device, with LZ77 matches): png_encode's arguments and output, d_scratch
// of at least png_scratch_bytes_lz77.  deflate_lz77 is its deflate stage on n bytes at d_data (stride: the row candidate's distance, 0 for
// none): the same header and a zlib stream; d_out of at least deflate_stream_bound(n) bytes, d_scratch of deflate_scratch_bytes(n).
inline size_t png_scratch_bytes_lz77(Extent2u res, uint32_t bpp) { return rayn_png_scratch_bytes_lz77(res.w, res.h, bpp); }
inline int png_encode_lz77(rayn_ctx* ctx, Extent2u res, uint32_t bpp, const uint8_t* d_img, void* d_out, size_t out_bytes, void* d_scratch,
                           size_t scratch_bytes, void* hip_stream = nullptr) {
    return rayn_hip_png_encode_lz77_device(ctx, res.w, res.h, bpp, d_img, d_out, out_bytes, d_scratch, scratch_bytes, hip_stream);
}
inline size_t deflate_stream_bound(size_t n) { return rayn_deflate_stream_bound(n); }
inline size_t deflate_scratch_bytes(size_t n) { return rayn_deflate_scratch_bytes(n); }
inline int deflate_lz77(rayn_ctx* ctx, const void* d_data, size_t n, uint32_t stride, void* d_out, size_t out_bytes, void* d_scratch,
                        size_t scratch_bytes, void* hip_stream = nullptr) {
    return rayn_hip_deflate_lz77_device(ctx, d_data, n, stride, d_out, out_bytes, d_scratch, scratch_bytes, hip_stream);
}

// Extension (include/rayn_hip.h: OpenEXR scanline chunks with ZIP compression on the device): the chunks of the EXR file of n_channels
// planes in the film's layout behind four words and a chunk table.  d_planes: device pointers in a host array, in the file's channel
// order; layout: (stride, offset, type) per channel; matches: 0 run-length blocks, 1 LZ77 blocks.  d_out of at least exr_stream_bound
// bytes, d_scratch of at least exr_scratch_bytes, both 16-byte aligned.  Returns the entry's code.
inline size_t exr_stream_bound(Extent2u res, uint32_t n_channels, const uint32_t* layout) { return rayn_exr_stream_bound(res.w, res.h, n_channels, layout); }
inline size_t exr_scratch_bytes(Extent2u res, uint32_t n_channels, const uint32_t* layout, uint32_t matches) {
    return rayn_exr_scratch_bytes(res.w, res.h, n_channels, layout, matches);
}
inline int exr_encode(rayn_ctx* ctx, Extent2u res, uint32_t n_channels, const void* const* d_planes, const uint32_t* layout, uint32_t matches,
                      void* d_out, size_t out_bytes, void* d_scratch, size_t scratch_bytes, void* hip_stream = nullptr) {
    return rayn_hip_exr_encode_device(ctx, res.w, res.h, n_channels, d_planes, layout, matches, d_out, out_bytes, d_scratch, scratch_bytes, hip_stream);
}

// ---- setup::setup() (src/setup.rs:46-170) with the resolution as an argument ---------------------
namespace setup {
constexpr float WORLD_RADIUS = 100.0f;
constexpr uint32_t FRACTAL_ITERATIONS = 12;
inline std::pair<CameraHandle, World> setup(Extent2u resolution = Extent2u(1280, 720), bool volumes = true) {
    World w;
    if (volumes) w.volume_params = VolumeParams{0.25f, 0.035f};
    MaterialHandle sky = w.materials.add_material(Sky::new_(Srgb::new_(0.3f, 0.4f, 0.6f), Srgb::new_(0.2f, 0.3f, 0.6f) * 0.05f));
    w.hitables.push(Sphere::new_(Vec3(0.0f, 0.0f, 0.0f), WORLD_RADIUS, sky));
    MaterialHandle grey = w.materials.add_material(Dielectric::new_remap(Srgb::new_(0.2f, 0.2f, 0.2f), 0.6f));
    w.hitables.push(TracedSDF::new_(MandelBox::new_(FRACTAL_ITERATIONS, BoxFold::new_(1.0f), SphereFold::new_(0.01f, 1.9f), -2.1f), grey));
    Srgb green = Srgb::new_(1.5f, 4.5f, 3.0f).normalized();
    Srgb blue = Srgb::new_(1.5f, 3.0f, 4.5f).normalized();
    MaterialHandle blue_emissive = w.materials.add_material(Emissive::new_splat(blue * 3.0f));
    MaterialHandle green_emissive = w.materials.add_material(Emissive::new_splat(green * 3.0f));
    const std::pair<Vec3, float> light_pairs[2] = {{Vec3(1.2f, -1.2f, 1.2f), 0.15f}, {Vec3(-1.2f, 1.2f, 1.2f), 0.15f}};
    for (const auto& lp : light_pairs) {
        Vec3 pos = lp.first, green_pos = lp.first;
        float rad = lp.second;
        green_pos.y *= -1.0f;
        w.lights.push_back(SphereLight::new_(green_pos, rad, green * 40.0f));
        w.lights.push_back(SphereLight::new_(pos, rad, blue * 40.0f));
        w.hitables.push(Sphere::new_(green_pos, rad - 0.01f, green_emissive));
        w.hitables.push(Sphere::new_(pos, rad - 0.01f, blue_emissive));
    }
    w.lights.push_back(SphereLight::new_(Vec3::zero(), 0.25f, green * 20.0f));
    w.hitables.push(Sphere::new_(Vec3::zero(), 0.24f, green_emissive));
    Vec2 res((float)resolution.w, (float)resolution.h);
    CameraHandle cam = w.cameras.add_camera(PinholeCamera::new_(res, 60.0f, Vec3(-0.45f, 0.2f, 2.0f) * 2.25f, Vec3(0.0f, 0.0f, 0.0f), Vec3(0.0f, 1.0f, 0.0f)));
    return {cam, std::move(w)};
}
} // namespace setup

} // namespace rayn
