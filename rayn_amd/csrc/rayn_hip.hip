// rayn_hip.hip — C ABI (include/rayn_hip.h) and host driver of the wavefront renderer.
//
// Replaces the body of Film::render_frame_into (src/film.rs:382-628): builds the reference's tile
// list, groups tiles into batches that fit the path pool, and for every batch runs
//   ray-gen -> { extend -> bin (scan+scatter) -> shade -> repack (scan+scatter) } per depth -> resolve
// on the worker's HIP stream.  Queue sizes stay on the device (DCtl): a frame share is enqueued without host<->device round
// trips (configurations deeper than 8 bounces peek at the queue size every 4th depth) and the host waits once, at the end.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rayn_detmath.h"
#include "../../include/rayn_hip.h"
#include "driver.h"
#include "frame_layout.h"
#include "tiles.h"
#include "save_to.h"
#include "display.h"
#include "temporal_upscale.h"
#include "upscale.h"
#include "denoise.h"
#include "denoise_variance.h"
#include "post_checks.h"
#include "preview.h"
#include "interpolate.h"
#include "jpeg.h"
#include "png.h"
#include "exr.h"
#include "progressive.h"
#include "temporal.h"

using namespace rayn;

namespace {

enum ProfClass { PC_RAYGEN = 0, PC_EXTEND, PC_BIN, PC_SHADE, PC_COMPACT, PC_RESOLVE, PC_SHADOW, PC_FINISH, PC_COUNT };

int wfail(Worker* w, int code, const std::string& msg) { w->err = msg; w->rc = code; return code; }

#define WCHK(expr)                                                                                            \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) return wfail(w, RAYN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

f3 to3(rayn_vec3 v) { return f3{v.x, v.y, v.z}; }

uint32_t f32_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// DHitable::fast_div == 2 gate: run k_verify_short_div over every denominator max(r2, mrs) with r2 < frs can take, i.e.
// all floats in [mrs, frs) (positive floats are ordered like their bit patterns); cached per (mrs, frs).
bool short_div_is_exact(rayn_ctx* ctx, float mrs, float frs) {
    if (!(mrs > 0.0f) || !(mrs < frs)) return false;
    const std::pair<uint32_t, uint32_t> key(f32_bits(mrs), f32_bits(frs));
    for (const auto& e : ctx->short_div_verdicts) if (e.first == key) return e.second;
    bool ok = false;
    uint32_t* d_bad = nullptr;
    uint32_t bad = 1;
    if (hipSetDevice(ctx->device) == hipSuccess && hipMalloc((void**)&d_bad, 4) == hipSuccess) {
        if (hipMemsetAsync(d_bad, 0, 4, ctx->stream) == hipSuccess) {
            rayn_p0::launch_verify_short_div(ctx->stream, frs, key.first, key.second - key.first, d_bad);
            if (hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess)
                ok = bad == 0;
        }
        hipFree(d_bad);
    }
    ctx->short_div_verdicts.emplace_back(key, ok);
    return ok;
}

} // namespace

namespace rayn { // shared with probes.hip (driver.h)

// rayn_camera -> DCamera: the constants the cameras' ::new derive from resolution and field of view; false for an unknown kind
bool build_camera(const rayn_camera& c, DCamera* out) {
    memset(out, 0, sizeof *out);
    DCamera& dc = *out;
    dc.kind = c.kind; dc.origin = to3(c.origin); dc.at = to3(c.at); dc.up = to3(c.up); dc.focus = to3(c.focus); dc.aperture = c.aperture;
    dc.animated = c.animated & 15u; dc.origin_vel = to3(c.origin_vel); dc.at_vel = to3(c.at_vel); dc.up_vel = to3(c.up_vel); dc.focus_vel = to3(c.focus_vel);
    if (c.kind == RAYN_CAM_ORTHOGRAPHIC) { // OrthographicCamera::new, src/camera.rs:228-240
        float aspect = c.res_w / c.res_h;
        float sx = c.vfov_or_size * aspect, sy = c.vfov_or_size;
        float pixel_size = c.vfov_or_size / c.res_h;
        dc.half_w = sx / 2.0f; dc.half_h = sy / 2.0f; dc.full_w = sx; dc.full_h = sy;
        dc.half_pixel_size = pixel_size / 2.0f;
    } else if (c.kind == RAYN_CAM_PINHOLE || c.kind == RAYN_CAM_THIN_LENS) { // ::new, src/camera.rs:53-72,134-157
        float theta = c.vfov_or_size * 3.14159265358979323846f / 180.0f;
        float half_height = dm_tanf(theta / 2.0f);
        float aspect = c.res_w / c.res_h;
        float half_width = aspect * half_height;
        dc.half_pixel_size = half_height / c.res_h;
        dc.half_w = half_width; dc.half_h = half_height; dc.full_w = half_width; dc.full_h = half_height;
    } else return false;
    return true;
}

int build_scene(rayn_ctx* ctx, const rayn_world_desc& w, const rayn_frame_params& p, DScene* out) {
    DScene& s = *out;
    memset(&s, 0, sizeof s);
    if (w.n_hitables > RAYN_MAX_HITABLES || w.n_materials > RAYN_MAX_MATERIALS || w.n_lights > RAYN_MAX_LIGHTS)
        return fail(ctx, RAYN_ERR_INVALID_ARG, "world exceeds fixed capacities");
    s.n_hitables = w.n_hitables; s.n_materials = w.n_materials; s.n_lights = w.n_lights;
    for (uint32_t i = 0; i < w.n_hitables; i++) {
        const rayn_hitable& h = w.hitables[i];
        DHitable& d = s.h[i];
        if (h.material >= w.n_materials) return fail(ctx, RAYN_ERR_INVALID_ARG, "hitable references a missing material");
        d.kind = h.kind; d.material = h.material; d.sdf_kind = h.sdf_kind; d.iterations = h.iterations;
        d.center = to3(h.center);
        d.animated = h.animated ? 1u : 0u; d.center_vel = to3(h.center_vel); // Sphere::transform_seq; a TracedSDF's origin as an extension
        d.scale_vel = (h.kind == RAYN_HITABLE_TRACED_SDF && h.sdf_kind == RAYN_SDF_MANDELBOX) ? h.scale_vel : 0.0f;
        if (d.animated || d.scale_vel != 0.0f) s.anim_spheres = 1; // the kernels then carry the packet's lane-0 time
        d.radius_sq = h.radius * h.radius;
        d.box_l = h.box_side;
        d.min_rad_sq = h.min_radius * h.min_radius;
        d.fixed_rad_sq = h.fixed_radius * h.fixed_radius;
        d.scale = h.scale;
        d.sdf_radius = h.sdf_radius;
        {   // div_nr is exact while numerator, denominator and quotient stay far from the exponent limits
            const float lo = 8.6736174e-19f /* 2^-60 */, hi = 1.1529215e18f /* 2^60 */;
            // ... and the box fold's 2*clamp(p) is an exact product while |box_side| <= 2^60 (fma == mul, add)
            const float bs = h.box_side < 0.0f ? -h.box_side : h.box_side;
            d.fast_div = (d.min_rad_sq >= lo && d.min_rad_sq <= hi && d.fixed_rad_sq >= lo && d.fixed_rad_sq <= hi && bs <= hi) ? 1u : 0u;
            // ... and the fast arms' box fold is the median of (p, -l, l), which is the reference's min(max(p, -l), l) only for 0 <= l: a negative box side
            // (the reference then returns l for every p, -0 included) and a NaN one (it returns NaN; med3 drops a NaN operand) take the fast_div == 0 arm, which clamps
            // in the reference's own order (device_core.h: clamp_ref)
            if (!(h.box_side >= 0.0f) || std::signbit(h.box_side)) d.fast_div = 0u;
            // ... and the 4-instruction division when the device has verified it for every reachable denominator
            if (d.fast_div && h.kind == RAYN_HITABLE_TRACED_SDF && h.sdf_kind == RAYN_SDF_MANDELBOX && short_div_is_exact(ctx, d.min_rad_sq, d.fixed_rad_sq))
                d.fast_div = 2u;
        }
        if (h.kind == RAYN_HITABLE_TRACED_SDF) {
            s.n_sdf++;
            if (h.sdf_kind != RAYN_SDF_SPHERE && h.sdf_kind != RAYN_SDF_MANDELBOX && h.sdf_kind != RAYN_SDF_MANDELBULB) return fail(ctx, RAYN_ERR_INVALID_ARG, "unknown sdf_kind");
        } else if (h.kind == RAYN_HITABLE_SPHERE) s.sphere_mask |= 1u << i;
        else return fail(ctx, RAYN_ERR_INVALID_ARG, "unknown hitable kind");
    }
    for (uint32_t i = 0; i < w.n_materials; i++) {
        const rayn_material& m = w.materials[i];
        DMaterial& d = s.m[i];
        if (m.kind > RAYN_MAT_EMISSIVE) return fail(ctx, RAYN_ERR_INVALID_ARG, "unknown material kind");
        d.kind = m.kind; d.a = to3(m.a); d.b = to3(m.b); d.exponent = m.exponent;
        d.receives_light = (m.kind == RAYN_MAT_SKY || m.kind == RAYN_MAT_EMISSIVE) ? 0u : 1u; // BSDF::receives_light
    }
    for (uint32_t i = 0; i < w.n_lights; i++) {
        s.l[i].pos = to3(w.lights[i].pos); s.l[i].rad = w.lights[i].rad; s.l[i].emission = to3(w.lights[i].emission);
    }
    if (!build_camera(w.camera, &s.cam)) return fail(ctx, RAYN_ERR_INVALID_ARG, "unknown camera kind");
    s.has_scatter = w.has_scattering; s.has_extinct = w.has_extinction; s.rho_s = w.coeff_scattering; s.rho_t = w.coeff_extinction;
    s.width = p.width; s.height = p.height; s.spp = p.samples * 4; s.max_bounces = p.max_bounces; s.vm = p.volume_marches;
    s.max_marches = p.max_marches; s.max_vis_marches = p.max_vis_marches;
    s.n1 = 3 + p.volume_marches; s.n2 = 12 + 8 * p.volume_marches;
    s.time_start = p.time_start; s.time_range = p.time_end - p.time_start;
    s.detail_scale = p.sdf_detail_scale; s.t_max = p.world_radius * 2.0f;
    s.ndc_x = 1.0f / (float)p.width; s.ndc_y = 1.0f / (float)p.height;
    return RAYN_OK;
}

// which march kernels a scene gets: the index of its TracedSDF when it holds exactly one (single-SDF fast paths), and the context's launch tuning with the
// per-scene decision Tuning::bulb (a single Mandelbulb marches its shadow segments with march_bulb.h's kernel; the march count shares a register with two flags there)
int scene_march_kernels(const rayn_ctx* ctx, const DScene& hs, const rayn_frame_params& p, Tuning* tun) {
    int single_sdf = -1;
    if (hs.n_sdf == 1) for (uint32_t i = 0; i < hs.n_hitables; i++) if (hs.h[i].kind == RAYN_HITABLE_TRACED_SDF) single_sdf = (int)i;
    *tun = ctx->tun;
    tun->sdf_kind = single_sdf >= 0 && ctx->tun.sdf_templates ? (int)hs.h[single_sdf].sdf_kind : -1;
    // the MandelBox in the reference's shipped shape (12 iterations, short division verified for its constants): the instantiation that knows both at compile time
    if (tun->sdf_kind == (int)RAYN_SDF_MANDELBOX && ctx->tun.box12s && hs.h[single_sdf].fast_div == 2u && hs.h[single_sdf].iterations == 12u) tun->sdf_kind = 100; // SDFK_MANDELBOX_12S (device_core.h)
    tun->bulb = ctx->tun.bulb_path && single_sdf >= 0 && hs.h[single_sdf].sdf_kind == RAYN_SDF_MANDELBULB && hs.h[single_sdf].iterations >= 1 &&
                p.max_marches < 0xFFFFu && p.max_vis_marches < 0xFFFFu;
    return single_sdf;
}

int validate(rayn_ctx* ctx, const rayn_frame_params* p) {
    if (!ctx) return RAYN_ERR_INVALID_ARG;
    if (!p) return fail(ctx, RAYN_ERR_INVALID_ARG, "null frame params");
    if (!ctx->cfg->have_world) return fail(ctx, RAYN_ERR_NO_WORLD, "rayn_hip_upload_world has not been called");
    if (!p->width || !p->height || !p->samples || !p->tile_w || !p->tile_h) return fail(ctx, RAYN_ERR_INVALID_ARG, "zero-sized frame, tile or sample count");
    if (p->volume_marches < 2 || p->volume_marches > 4) return fail(ctx, RAYN_ERR_INVALID_ARG, "volume_marches must be in [2,4] (samples_1d[3],[4] are indexed, src/integrator.rs:138,175)");
    if (p->max_bounces > MAX_BOUNCES) return fail(ctx, RAYN_ERR_INVALID_ARG, "max_bounces > 120 does not fit the 7-bit depth field of the termination record");
    if (p->samples > 4096) return fail(ctx, RAYN_ERR_INVALID_ARG, "spp > 16384 unsupported (the film resolve sorts a pixel's samples in the registers of one 1024-thread block)");
    if ((uint64_t)p->tile_w * (uint64_t)p->tile_h > MAX_TILE_PIXELS) return fail(ctx, RAYN_ERR_INVALID_ARG, "tile larger than 1024 pixels unsupported");
    if ((uint64_t)p->width * (uint64_t)p->height >= ((uint64_t)1 << 31)) return fail(ctx, RAYN_ERR_INVALID_ARG, "film larger than 2^31 pixels unsupported (32-bit pixel indices)");
    return RAYN_OK;
}

} // namespace rayn

namespace {

hipEvent_t get_event(Worker* w) {
    if (!w->event_pool.empty()) { hipEvent_t e = w->event_pool.back(); w->event_pool.pop_back(); return e; }
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

// control block, counters, pinned read-back buffers and the 'done' event of a worker (+ its own stream for workers >= 1), created on
// first use.  Worker 0 runs on the caller's stream: a single-worker frame - every small frame, e.g. the reference's shipped 1280x720x8spp
// - needs no stream of its own and no cross-stream fork / join (measured: a second hipStreamCreate costs 12-17 ms of a cold 62 ms frame).
int ensure_worker(rayn_ctx* ctx, Worker* w, bool own_stream) {
    bool ok = hipSetDevice(ctx->device) == hipSuccess;
    if (ok && !w->d_ctl)
        ok = hipMalloc((void**)&w->d_evals, 128) == hipSuccess && hipMalloc((void**)&w->d_ctl, sizeof(DCtl)) == hipSuccess &&
             hipHostMalloc((void**)&w->h_totals, 16) == hipSuccess && hipHostMalloc((void**)&w->h_ctl, sizeof(DCtl)) == hipSuccess &&
             hipEventCreateWithFlags(&w->done, hipEventDisableTiming) == hipSuccess;
    if (ok && own_stream && !w->own) ok = hipStreamCreateWithFlags(&w->own, hipStreamNonBlocking) == hipSuccess;
    return ok ? RAYN_OK : fail(ctx, RAYN_ERR_HIP, std::string("worker resources: ") + hipGetErrorString(hipGetLastError()));
}

struct Timed { // brackets one launch with events when profiling is on
    Worker* w; bool on; hipStream_t s; int cls; hipEvent_t a = nullptr, b = nullptr;
    Timed(Worker* w_, bool on_, int cl) : w(w_), on(on_), s(w_->stream), cls(cl) {
        if (on) { a = get_event(w); b = get_event(w); if (a) (void)hipEventRecord(a, s); }
    }
    ~Timed() {
        if (on && a && b) { (void)hipEventRecord(b, s); w->prof.push_back(ProfRec{cls, a, b}); }
    }
};

// a += b for everything a frame's parts add up to: the workers of a device at the join, the entries of a multi-device frame.  ms_total is
// not a sum (the caller brackets the whole frame on its own clock) and stays a's.  A worker's ms_* are zero at the join - run_worker
// memsets its stats and collect_profile, which fills the context's ms_* from the workers' events, runs after it - so adding them there
// changes nothing; the entries' ms_* are real and do add up.
void add(rayn_stats& a, const rayn_stats& b) {
    a.paths += b.paths; a.segments += b.segments; a.shaded_slots += b.shaded_slots; a.tiles += b.tiles; a.batches += b.batches;
    a.launches_extend += b.launches_extend; a.launches_shade += b.launches_shade; a.shadow_jobs += b.shadow_jobs;
    a.queue_bytes_bin += b.queue_bytes_bin; a.queue_bytes_compact += b.queue_bytes_compact;
    a.ms_raygen += b.ms_raygen; a.ms_extend += b.ms_extend; a.ms_bin += b.ms_bin; a.ms_shade += b.ms_shade; a.ms_compact += b.ms_compact;
    a.ms_resolve += b.ms_resolve; a.ms_shadow += b.ms_shadow; a.ms_finish += b.ms_finish;
}

void collect_profile(rayn_ctx* ctx) {
    double ms[PC_COUNT] = {0};
    for (Worker& w : ctx->workers) {
        for (auto& r : w.prof) {
            float t = 0;
            if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) ms[r.cls] += t;
            w.event_pool.push_back(r.a);
            w.event_pool.push_back(r.b);
        }
        w.prof.clear();
    }
    ctx->stats.ms_raygen = ms[PC_RAYGEN]; ctx->stats.ms_extend = ms[PC_EXTEND]; ctx->stats.ms_bin = ms[PC_BIN];
    ctx->stats.ms_shade = ms[PC_SHADE]; ctx->stats.ms_compact = ms[PC_COMPACT]; ctx->stats.ms_resolve = ms[PC_RESOLVE];
    ctx->stats.ms_shadow = ms[PC_SHADOW]; ctx->stats.ms_finish = ms[PC_FINISH];
}

struct BatchTile { uint32_t tile_index; DTile d; };

struct FrameShared { // read-only for the workers
    const rayn_frame_params* p; DScene hs; Tables tab; const float* d_scr;
    float *d_color, *d_alpha, *d_bg, *d_normal;
    KernelSet K; int single_sdf; uint32_t NS; bool count, profiling;
    size_t batch_paths; // effective per-worker pool capacity of this frame
    Tuning tun;         // the context's launch tuning + what this frame's scene decides (Tuning::bulb)
};

// ---- batches of whole tiles that fit the path pool
struct Plan { std::vector<std::vector<BatchTile>> batches; size_t max_pool = 0, max_tiles = 0; };
Plan make_plan(const std::vector<BatchTile>& mine, size_t cap_paths) { // a worker's tiles cut into batches of <= cap_paths pool slots
    Plan P;
    std::vector<BatchTile> cur;
    size_t pool = 0;
    for (const BatchTile& t : mine) {
        size_t n = t.d.n_paths, na = (n + 63) & ~(size_t)63;
        if (!cur.empty() && pool + na > cap_paths) {
            P.max_pool = std::max(P.max_pool, pool); P.max_tiles = std::max(P.max_tiles, cur.size());
            P.batches.push_back(std::move(cur)); cur.clear(); pool = 0;
        }
        BatchTile bt = t;
        bt.d.pool_base = (uint32_t)pool;
        cur.push_back(bt);
        pool += na;
    }
    if (!cur.empty()) { P.max_pool = std::max(P.max_pool, pool); P.max_tiles = std::max(P.max_tiles, cur.size()); P.batches.push_back(std::move(cur)); }
    return P;
}

// rayn_hip_set_trace_tile, diagnostics only (synchronises): the packet order of the traced tile after the bin stage of 'depth', in HitStore::process_hits order
int dump_trace_tile(rayn_ctx* ctx, Worker* w, const std::vector<BatchTile>& batch, const Layout& L, uint32_t depth, uint32_t width) {
    WCHK(hipStreamSynchronize(w->stream));
    for (uint32_t i = 0; i < (uint32_t)batch.size(); i++) {
        if ((int)batch[i].tile_index != ctx->trace_tile) continue;
        const DTile& td = batch[i].d;
        uint32_t base = 0, total = 0;
        WCHK(hipMemcpy(&base, L.qt.tile_out_base + i, 4, hipMemcpyDeviceToHost));
        WCHK(hipMemcpy(&total, L.qt.tile_total + i, 4, hipMemcpyDeviceToHost));
        std::vector<uint32_t> hq(total);
        std::vector<float4> g1(td.n_paths), c1(td.n_paths);
        WCHK(hipMemcpy(hq.data(), L.bq + base, (size_t)total * 4, hipMemcpyDeviceToHost));
        WCHK(hipMemcpy(g1.data(), L.pool.geo1 + td.pool_base, (size_t)td.n_paths * 16, hipMemcpyDeviceToHost));
        WCHK(hipMemcpy(c1.data(), L.pool.col1 + td.pool_base, (size_t)td.n_paths * 16, hipMemcpyDeviceToHost));
        uint32_t packet_obj = 0;
        for (uint32_t s = 0; s < total; s++) {
            const uint32_t P = hq[s];
            uint32_t rec[6] = {depth, packet_obj, 0, 0, 0, 0};
            if (P != INVALID) {
                uint32_t bits, pix;
                memcpy(&bits, &g1[P - td.pool_base].w, 4);
                memcpy(&pix, &c1[P - td.pool_base].z, 4);
                rec[1] = bits & 0xFFu; rec[2] = pix % width - td.x0; rec[3] = pix / width - td.y0; rec[4] = bits >> 8; rec[5] = 1;
                if ((s & 3u) == 0) packet_obj = rec[1]; // a packet never straddles objects and its padding is at the end
            }
            ctx->trace.insert(ctx->trace.end(), rec, rec + 6);
        }
    }
    return 0;
}

// everything one worker does for its share of the tiles: batches -> per-depth wavefront -> resolve
int run_worker(rayn_ctx* ctx, Worker* w, const FrameShared& F, const std::vector<BatchTile>& mine) {
    w->rc = 0; w->err.clear();
    memset(&w->stats, 0, sizeof w->stats);
    w->counters.clear();
    if (mine.empty()) return 0;
    WCHK(hipSetDevice(ctx->device));
    const DScene& hs = F.hs;
    const uint32_t spp = hs.spp, NS = F.NS;
    const KernelSet& K = F.K;
    hipStream_t stream = w->stream;
    uint32_t max_tile_pixels = 0;
    for (const BatchTile& t : mine) max_tile_pixels = std::max(max_tile_pixels, t.d.ew * t.d.eh);
    const size_t total_tiles = mine.size();
    if (spp > 512 && spp <= MAX_SPP_RESOLVE_BLK && !resolve_keys_fit(max_tile_pixels, spp))
        return wfail(w, RAYN_ERR_INVALID_ARG, "tile x spp too large for the 25-bit slot offset of the film resolve's sort keys (k_resolve_blk)");
    Plan plan = make_plan(mine, F.batch_paths);
    if (!queue_ids_fit(NS, binned_cap(plan.max_pool, plan.max_tiles)))
        return wfail(w, RAYN_ERR_INVALID_ARG, "batch too large for 32-bit queue indices; lower RAYN_HIP_BATCH_PATHS");
    Layout L;
    Arena dry;
    const size_t need = carve(dry, plan.max_pool, plan.max_tiles, total_tiles, NS, F.p->max_bounces, &L);
    if (need > w->arena.cap) {
        // grow: the new arena is obtained BEFORE the old one is released, so that it comes out of memory the driver does not have
        // to wipe first (freshly freed device memory is, see render_device) whenever that much is free
        void* ptr = nullptr;
        if (hipMalloc(&ptr, need) != hipSuccess) {
            (void)hipGetLastError();
            if (w->arena.base) { WCHK(hipFree(w->arena.base)); w->arena = Arena(); }
            if (hipMalloc(&ptr, need) != hipSuccess) return wfail(w, RAYN_ERR_OOM, "hipMalloc of the path pool failed (" + std::to_string(need >> 20) + " MiB)");
        }
        if (w->arena.base) WCHK(hipFree(w->arena.base));
        w->arena.base = (char*)ptr; w->arena.cap = need;
    }
    if (carve(w->arena, plan.max_pool, plan.max_tiles, total_tiles, NS, F.p->max_bounces, &L) > w->arena.cap) return wfail(w, RAYN_ERR_OOM, "internal: arena under-sized");
    DCtl* d_ctl = w->d_ctl;

    // The whole share is ENQUEUED without a single host<->device round trip: queue sizes live in d_ctl,
    // every batch's tile list goes up with one small copy (the staging vector belongs to the worker, is reserved up front and
    // outlives the copies), kernels size themselves.
    w->h_tiles.clear();
    w->h_tiles.reserve(total_tiles);
    WCHK(hipMemsetAsync(d_ctl, 0, sizeof(DCtl), stream));
    WCHK(hipMemsetAsync(w->d_evals, 0, 128, stream));
    const bool count = F.count, prof = F.profiling;
    const Tables& tab = F.tab;
    const uint32_t last_depth = F.p->max_bounces; // a path that reaches depth == max_bounces terminates there (src/integrator.rs:171)
    size_t tile_cursor = 0; // tiles enqueued so far = index into mine / d_all_tiles
    for (size_t bi = 0; bi < plan.batches.size(); bi++) {
        std::vector<BatchTile>& batch = plan.batches[bi];
        const uint32_t nt = (uint32_t)batch.size();
        DTile* d_tiles = L.d_all_tiles + tile_cursor;
        {
            const size_t h0 = w->h_tiles.size();
            for (auto& bt : batch) w->h_tiles.push_back(bt.d);
            WCHK(hipMemcpyAsync(d_tiles, w->h_tiles.data() + h0, (size_t)nt * sizeof(DTile), hipMemcpyHostToDevice, stream));
        }
        tile_cursor += nt;
        size_t n_pool = 0;
        for (uint32_t i = 0; i < nt; i++) {
            n_pool += (size_t)((batch[i].d.n_paths + 63) / 64) * 64;
            w->stats.paths += batch[i].d.n_paths;
        }
        w->stats.tiles += nt; w->stats.batches++;
        // upper bounds of the device-resident queue sizes of this batch (grids are sized for them)
        const uint32_t max_entries = (uint32_t)n_pool, max_slots = (uint32_t)std::min(L.BCAP, binned_cap(n_pool, nt));
        {
            Timed t(w, prof, PC_RAYGEN);
            K.batch_setup(stream, d_tiles, nt, L.pgrp_tile, L.qt.ray_tgb, L.qt.ray_tgc);
            K.raygen(stream, ctx->d_scene, tab, F.d_scr, d_tiles, L.pgrp_tile, L.pool, L.q, (uint32_t)n_pool, d_ctl);
        }
        uint32_t* qcur = L.q; uint32_t* qnext = L.qn;
        for (uint32_t depth = 0; depth <= last_depth; depth++) {
            // deep configurations: look at the queue size now and then, so that a batch whose paths all died early (roulette)
            // does not enqueue dozens of empty depths; <= 8 bounces never synchronise
            if (depth >= 8 && (depth & 3u) == 0) {
                WCHK(hipMemcpyAsync(w->h_totals, &d_ctl->q_groups, 8, hipMemcpyDeviceToHost, stream));
                WCHK(hipStreamSynchronize(stream));
                if (w->h_totals[1] == 0) break;
            }
            { Timed t(w, prof, PC_EXTEND); K.extend(stream, count, ctx->d_scene, depth, qcur, max_entries, L.pool, L.qt.ent_obj, F.single_sdf, d_ctl, w->d_evals, F.tun); }
            w->stats.launches_extend++;
            // k_group_hist is timed with the bin stage it feeds (r1 / r2 timed it with the extend kernel)
            { Timed t(w, prof, PC_BIN); K.bin_stage(stream, L.qt, hs.n_hitables, nt, qcur, max_entries, L.bq, (uint32_t)(L.BCAP / 64), L.base_hist + (size_t)depth * L.hist_stride, d_ctl); }
            if (ctx->trace_tile >= 0 && dump_trace_tile(ctx, w, batch, L, depth, hs.width)) return w->rc;
            {
                static const int cls[3] = {PC_SHADE, PC_SHADOW, PC_FINISH};
                struct HookState { Worker* w; bool on; Timed* cur; } hst{w, prof, nullptr};
                ShadeHooks hooks;
                hooks.user = &hst;
                hooks.before_fn = [](void* u, int i) { HookState* h = (HookState*)u; h->cur = new Timed(h->w, h->on, cls[i]); };
                hooks.after_fn = [](void* u, int) { HookState* h = (HookState*)u; delete h->cur; h->cur = nullptr; };
                K.shade(stream, count, ctx->d_scene, tab, F.d_scr, depth, L.bq, max_slots, L.pool, L.nee, NS, hs.n_sdf > 0, F.single_sdf, L.qt.alive, L.qt.bgrp_cnt, d_ctl, w->d_evals, hooks, F.tun);
            }
            w->stats.launches_shade++;
            if (depth == last_depth) break; // nothing survives the last depth: no repack
            { Timed t(w, prof, PC_COMPACT); K.repack_stage(stream, L.qt, nt, L.bq, max_slots, qnext, (uint32_t)(L.QCAP / 64), d_ctl); }
            std::swap(qcur, qnext);
        }
        { Timed t(w, prof, PC_RESOLVE); K.resolve(stream, ctx->d_scene, d_tiles, nt, max_tile_pixels, spp, L.pool, F.d_color, F.d_alpha, F.d_bg, F.d_normal, L.base_hist, (uint32_t)L.hist_stride); }
    }
    WCHK(hipMemcpyAsync(w->h_ctl, d_ctl, sizeof(DCtl), hipMemcpyDeviceToHost, stream));
    WCHK(hipEventRecord(w->done, stream));
    WCHK(hipStreamSynchronize(stream)); // the only wait of the share
    WCHK(hipGetLastError());
    {
        const DCtl& c = *w->h_ctl;
        if (c.overflow) return wfail(w, RAYN_ERR_HIP, c.overflow & 1u ? "internal: binned queue overflow" : "internal: ray queue overflow");
        w->stats.segments = c.segments; w->stats.shaded_slots = c.shaded_slots; w->stats.shadow_jobs = c.shadow_jobs;
        // algorithmic HBM bytes of the queue stages: bin = hist 1 B/entry + scatter q 4 + ent_obj 1 per entry, bq 4 per slot,
        // ~85 B of scan bookkeeping per group; repack = bq 4 per slot, q' 4 per survivor slot, 17 B per group (survivor ballot 8, count 1, base 4, tile 4)
        w->stats.queue_bytes_bin = c.entries_sum * 6 + c.shaded_slots * 4 + (c.entries_sum / 64) * 85;
        w->stats.queue_bytes_compact = c.shaded_slots * 4 + c.next_sum * 4 + (c.shaded_slots / 64) * 17;
    }
    if (count) {
        unsigned long long h[16];
        WCHK(hipMemcpy(h, w->d_evals, 128, hipMemcpyDeviceToHost));
        w->counters.decode(h);
    }
    return 0;
}

// worker 1's stream + arena for the two-worker schedule of small shares, outside any frame's ev_a..ev_b bracket (see the end of render_device).  Best effort: a
// failure just leaves the work to the frame that needs it.
void prewarm_second_worker(rayn_ctx* ctx) {
    const size_t want = ctx->prewarm_bytes;
    ctx->prewarm_bytes = 0;
    if (!want) return;
    Worker& w1 = ctx->workers[1];
    if (ensure_worker(ctx, &w1, true) == RAYN_OK && !w1.arena.base) {
        void* ptr = nullptr;
        if (hipMalloc(&ptr, want) == hipSuccess) { w1.arena.base = (char*)ptr; w1.arena.cap = want; }
        else (void)hipGetLastError();
    }
    ctx->err.clear();
}

// Where one render_device call resolves to.  Per call and passed by the caller: nothing about a single call is kept in the context.
struct RenderTarget {
    float *color, *alpha, *bg, *normal;
    bool packed = false;               // the planes are those of a packed planar film of the owned tiles (DTile::film_packed), not of a full-resolution film
    const OwnedTiles* tiles = nullptr; // an entry of a multi-device frame: its tiles, already selected and laid out (then 'packed' is theirs);
                                       // nullptr = the context's tile subset, or the share tile_first / tile_step
};

// the four planes of a packed film of px pixels at 'buf' (color 3, alpha 1, background 3, normal 3 floats per pixel)
RenderTarget packed_target(float* buf, size_t px, const OwnedTiles* tiles) { return RenderTarget{buf, buf + 3 * px, buf + 4 * px, buf + 7 * px, true, tiles}; }

hipStream_t pick_stream(const rayn_ctx* ctx, void* hip_stream) { return hip_stream ? (hipStream_t)hip_stream : ctx->stream; }

// the argument check of render_device and render_multi
int check_frame_args(rayn_ctx* ctx, const rayn_frame_params* p, const float* d_s1, const float* d_s2, const float* d_scr, const float* d_fis, const RenderTarget& out) {
    int rc = validate(ctx, p);
    if (rc) return rc;
    if (!d_s1 || !d_s2 || !d_scr || !d_fis || !out.color || !out.alpha || !out.bg || !out.normal) return fail(ctx, RAYN_ERR_INVALID_ARG, "null buffer");
    return RAYN_OK;
}

// the tiles a call on this context owns when nobody dealt them (RenderTarget::tiles == nullptr)
const char* context_tiles(const rayn_ctx* ctx, const rayn_frame_params& p, bool packed, OwnedTiles* out) {
    return owned_tiles(p, ctx->tile_subset.empty() ? nullptr : &ctx->tile_subset, packed, out);
}

int render_device(rayn_ctx* ctx, const rayn_frame_params* p, const float* d_s1, const float* d_s2, const float* d_scr, const float* d_fis,
                  const RenderTarget& out, hipStream_t stream) {
    int rc = check_frame_args(ctx, p, d_s1, d_s2, d_scr, d_fis, out);
    if (rc) return rc;
    if (ctx->prewarm_bytes) { // the second frame of a context under the default first-frame policy: before this frame's bracket
        if (hipSetDevice(ctx->device) == hipSuccess) prewarm_second_worker(ctx);
        else ctx->prewarm_bytes = 0;
    }
    HIPCHK(hipSetDevice(ctx->device));
    FrameShared F;
    F.p = p;
    rc = build_scene(ctx, ctx->cfg->world, *p, &F.hs);
    if (rc) return rc;
    const DScene& hs = F.hs;
    const uint32_t spp = hs.spp;

    // ---- plan: owned tiles, dealt alternately to the workers
    OwnedTiles own;
    if (!out.tiles) if (const char* why = context_tiles(ctx, *p, out.packed, &own)) return fail(ctx, RAYN_ERR_INVALID_ARG, why);
    const OwnedTiles& mine = out.tiles ? *out.tiles : own;
    std::vector<BatchTile> owned(mine.d.size());
    size_t owned_paths = 0;
    for (size_t i = 0; i < owned.size(); i++) {
        owned[i] = BatchTile{mine.index[i], mine.d[i]};
        owned_paths += mine.d[i].n_paths;
    }
    memset(&ctx->stats, 0, sizeof ctx->stats);
    ctx->counters.clear();
    ctx->trace.clear();
    if (owned.empty()) return RAYN_OK;

    // ---- shared, read-only state: scene, tables, packed sample records
    const RecordLayout rec(hs.n2, p->max_bounces);
    const size_t rec_n = rec.count(spp);
    if (rec_n > ctx->rec_cap) {
        if (ctx->d_rec) HIPCHK(hipFree(ctx->d_rec));
        ctx->d_rec = nullptr; ctx->rec_cap = 0;
        if (hipMalloc((void**)&ctx->d_rec, rec_n * 16) != hipSuccess) return fail(ctx, RAYN_ERR_OOM, "hipMalloc of the packed sample records failed");
        ctx->rec_cap = rec_n;
    }
    HIPCHK(hipEventRecord(ctx->ev_a, stream));
    HIPCHK(hipMemcpyAsync(ctx->d_scene, &F.hs, sizeof F.hs, hipMemcpyHostToDevice, stream));
    F.K = kernel_set(ctx->cfg->fma_policy);
    F.single_sdf = scene_march_kernels(ctx, hs, *p, &F.tun);
    F.tab = Tables{d_s1, d_s2, d_fis, ctx->d_rec, rec.stride};
    F.K.pack_tables(stream, F.tab, ctx->d_rec, spp, rec.depths, hs.n1, hs.n2);
    F.d_scr = d_scr; F.d_color = out.color; F.d_alpha = out.alpha; F.d_bg = out.bg; F.d_normal = out.normal;
    F.NS = nee_samples(ctx->cfg->world.has_scattering, p->volume_marches);
    F.count = ctx->cfg->counting; F.profiling = ctx->cfg->profiling;
    // Batch size and worker count.  Bigger batches = fewer launches and tails (2^25 -> 2^27 paths: -9 % frame time), so
    // they are sized for the HBM that is actually free: at most 60 % of it across the workers (the rest stays with the
    // caller: film, tables, torch).  A second/third worker only pays when every worker still gets full-size batches
    // (measured on config 2: whole frame +4 %, a quarter of the frame -4 %, an eighth -10 %).
    int nw = 1;
    {
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        for (const Worker& w : ctx->workers) free_b += w.arena.cap;
        const size_t per_path = arena_bytes_per_path(F.NS);
        // entries of a multi-device context that share one GPU (repeated device ids) size their arenas concurrently from the same
        // free figure: each takes its share of the budget
        const size_t budget_paths = (size_t)(0.6 * (double)free_b / (double)std::max(ctx->budget_share, 1)) / per_path;
        const int max_w = std::min(std::min(ctx->cfg->n_workers, MAX_WORKERS), (int)std::min<size_t>(owned.size(), MAX_WORKERS));
        for (int c = std::max(max_w, 1); c >= 1; c--) {
            // 32-bit [sample][slot] refs: NS * (binned slots of a batch) must stay below 2^32 (5 % slack for bin padding and tile tails)
            const size_t index_cap = (size_t)(0.95 * 4294967296.0 / (double)F.NS);
            // FIRST FRAME of a context: arenas of at most cold_bytes for ALL workers together (44 GB: 2^26-path batches with the
            // volume path's 667 B per path, 2^27 without).  The reference renders ONE frame per process (src/main.rs:47-96) - a
            // render farm runs such processes back to back - and device memory that a process released is wiped by the driver
            // before the next one can use it, at ~20-40 ms per GB: measured (tools/cold_frame.py, profiles/r03_cold_start.txt), a
            // fresh process whose first frame takes a 175 GB arena runs that frame 3.5 s longer when it starts right after a
            // process of the same size (+0.0 s after a 6 s pause; obtaining the arena on a side thread does not hide it - the
            // running kernels stall too).  A quarter of the memory costs 2.5 % of steady-state speed; a context that renders a
            // second frame grows to the full size then.
            const size_t first = (ctx->frames_rendered == 0 && ctx->cfg->cold_bytes) ? ctx->cfg->cold_bytes / per_path / (size_t)c : ~(size_t)0;
            const size_t cap = std::max<size_t>(4096, std::min(first, std::min(std::min(ctx->cfg->batch_paths, index_cap), budget_paths / (size_t)c)));
            // a further worker must not cost batch size: with c workers each still gets >= 3/4 of the batch one worker would get
            // (config 3, 651 B per path: one worker with 2^28-path batches beats two with 2^27; config 2, 331 B: both fit)
            const size_t first1 = first == ~(size_t)0 ? first : first * (size_t)c; // what ONE worker would get of the first-frame budget
            const size_t solo = std::max<size_t>(4096, std::min(first1, std::min(std::min(ctx->cfg->batch_paths, index_cap), budget_paths)));
            // r4: a share that fits ONE batch of a single worker (a rank's eighth of config 2, the reference's shipped 7.4 M-path frame)
            // is split between TWO workers all the same: their persistent march kernels are co-resident, so the tail of one worker's
            // launch (a few long rays; 0.1-0.3 ms per launch) runs under the other worker's kernels.  Measured
            // (profiles/r04_exp_workers_cold_cpu.txt): 1/8 of c2 86.1 -> 84.1 ms, the shipped frame 36.5 -> 35.2 ms; three or four
            // workers, or half-size persistent grids, are slower.
            // (not on the FIRST frame of a context: the second worker's stream alone costs 12-17 ms to create - more than the split gains on a
            // frame this small - and a host that renders one frame per process, the reference's own usage, would only ever pay)
            const bool small_share = c == 2 && ctx->frames_rendered > 0 && owned_paths >= ctx->cfg->two_worker_min_paths && owned_paths <= solo &&
                                     owned_paths <= ctx->small_share_paths;
            if (c == 1 || small_share || (owned_paths >= ctx->cfg->two_worker_min_paths && owned_paths >= (size_t)c * cap && 4 * cap >= 3 * solo) ||
                (ctx->cfg->two_worker_min_paths == 0)) { nw = c; F.batch_paths = cap; break; }
        }
    }
    std::vector<BatchTile> share[MAX_WORKERS];
    for (size_t i = 0; i < owned.size(); i++) share[i % nw].push_back(owned[i]);
    for (int i = 0; i < nw; i++) {
        rc = ensure_worker(ctx, &ctx->workers[i], i > 0);
        if (rc) return rc;
        ctx->workers[i].stream = i == 0 ? stream : ctx->workers[i].own;
    }
    // fork: the worker streams start after everything already queued on the caller's stream
    HIPCHK(hipEventRecord(ctx->ev_fork, stream));
    HIPCHK(hipStreamSynchronize(stream)); // F.hs is on this stack frame: make sure the scene copy has been consumed
    for (int i = 1; i < nw; i++) HIPCHK(hipStreamWaitEvent(ctx->workers[i].stream, ctx->ev_fork, 0));
    {
        std::vector<std::thread> threads;
        for (int i = 1; i < nw; i++) threads.emplace_back([&, i]() { run_worker(ctx, &ctx->workers[i], F, share[i]); });
        run_worker(ctx, &ctx->workers[0], F, share[0]);
        for (auto& t : threads) t.join();
    }
    // join: the caller's stream continues after both workers
    for (int i = 0; i < nw; i++) {
        Worker& w = ctx->workers[i];
        if (w.rc) return fail(ctx, w.rc, w.err);
        if (i > 0 && !share[i].empty()) HIPCHK(hipStreamWaitEvent(stream, w.done, 0));
        add(ctx->stats, w.stats);
        ctx->counters += w.counters;
    }
    HIPCHK(hipEventRecord(ctx->ev_b, stream));
    HIPCHK(hipStreamSynchronize(stream));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ctx->ev_a, ctx->ev_b);
    ctx->stats.ms_total = ms;
    if (ctx->cfg->profiling) collect_profile(ctx);
    ctx->frames_rendered++;
    // A small single-batch share runs TWO co-resident workers from the context's second frame on (above): worker 1 needs a stream (12-17 ms to create) and an
    // arena.  A host that renders ONE frame per process - the reference's own usage, and what the default first-frame policy (cold_bytes != 0) is for - must not
    // pay for them in its only call (+30 ms on the shipped frame's 75): they are then obtained at the START of the second frame, before its ev_a..ev_b
    // bracket (prewarm_second_worker, called from the top of render_device).  A host that has switched the first-frame policy off (rayn_hip_set_cold_bytes(0):
    // bench.py when it measures no cold frame - its second frame is the first timed step) gets them here, after the first frame's bracket.
    if (ctx->frames_rendered == 1 && nw == 1 && ctx->cfg->n_workers >= 2 && owned.size() >= 2 && owned_paths >= ctx->cfg->two_worker_min_paths &&
        owned_paths <= ctx->small_share_paths && owned_paths <= F.batch_paths && ctx->workers[0].arena.cap) {
        ctx->prewarm_bytes = ctx->workers[0].arena.cap / 2 + ((size_t)48 << 20); // half the tiles of the share + the per-batch fixed part
        if (ctx->cfg->cold_bytes == 0) prewarm_second_worker(ctx);
    }
    return RAYN_OK;
}

// grow-only device buffer helper
template <typename T> int ensure(rayn_ctx* ctx, T** ptr, size_t* cap, size_t need) {
    if (need <= *cap) return RAYN_OK;
    if (*ptr) (void)hipFree(*ptr);
    *ptr = nullptr; *cap = 0;
    if (hipMalloc((void**)ptr, need * sizeof(T)) != hipSuccess) return fail(ctx, RAYN_ERR_OOM, "hipMalloc of a multi-device staging buffer failed");
    *cap = need;
    return RAYN_OK;
}

// Film::render_frame_into over several devices.  All pointers are on devices[0] (= ctx->device); the call is blocking.
//  1. the share's tiles (tile_first/tile_step or the tile subset) are dealt to the entries: the j-th tile of the share goes
//     to entry (j + j / N) % N - the same rotating deal the ABI uses between ranks (whole tiles; their cost is very uneven);
//  2. the sample tables / scramble / filter table are copied to every peer (<= tens of MB), scene descriptors are host data;
//  3. one host thread per entry drives that entry's own wavefront renderer on its device;
//  4. every peer resolves its tiles straight into a packed planar film of its owned pixels (10 floats per pixel; no
//     full-resolution film exists on a peer) and sends it to device 0 with ONE hipMemcpyPeerAsync over xGMI; device 0 scatters
//     the blocks into the caller's film.  No other data crosses devices.
int render_multi(rayn_ctx* ctx, const rayn_frame_params* p, const float* d_s1, const float* d_s2, const float* d_scr, const float* d_fis,
                 const RenderTarget& out, hipStream_t stream) {
    int rc = check_frame_args(ctx, p, d_s1, d_s2, d_scr, d_fis, out);
    if (rc) return rc;
    const size_t N = 1 + ctx->peers.size();
    // what each entry renders: entry 0 straight into the caller's film, a peer into a packed film of its tiles.  mine[e] drives the entry's
    // render AND, for a peer, is the tile list device 0 unpacks its block with (DTile::film_base = first pixel of the tile in the peer's
    // packed buffer): one object, so the two layouts cannot differ.
    std::vector<OwnedTiles> mine(N);
    {
        OwnedTiles share;
        if (const char* why = context_tiles(ctx, *p, false, &share)) return fail(ctx, RAYN_ERR_INVALID_ARG, why);
        std::vector<std::vector<uint32_t>> lists(N);
        for (size_t j = 0; j < share.index.size(); j++) lists[(j + j / N) % N].push_back(share.index[j]); // ascending k per entry: the lists are sorted
        for (size_t e = 0; e < N; e++) (void)owned_tiles(*p, &lists[e], e > 0, &mine[e]); // tiles of a valid share: cannot fail
    }
    const size_t spp = (size_t)p->samples * 4, npx = (size_t)p->width * p->height;
    const size_t n1 = spp * rayn_sets_1d(p->max_bounces, p->volume_marches), n2 = spp * 2 * rayn_sets_2d(p->max_bounces, p->volume_marches);
    const size_t n_tab = n1 + n2 + npx + RAYN_FIS_TABLE_SIZE;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(stream)); // the caller's tables are complete before they are copied to the peers
    std::vector<size_t> gather_off(N, 0); // where each peer's block begins in gather_buf, in pixels
    size_t gather_px = 0, gather_nt = 0;
    for (size_t e = 1; e < N; e++) { gather_off[e] = gather_px; gather_px += mine[e].pixels; gather_nt += mine[e].d.size(); }
    rc = ensure(ctx, &ctx->gather_buf, &ctx->gather_cap, gather_px * 10);
    if (rc) return rc;
    rc = ensure(ctx, &ctx->gather_tiles, &ctx->gather_tiles_cap, gather_nt);
    if (rc) return rc;
    if (!ctx->ev_ma) { HIPCHK(hipEventCreate(&ctx->ev_ma)); HIPCHK(hipEventCreate(&ctx->ev_mb)); }
    HIPCHK(hipEventRecord(ctx->ev_ma, stream));
    std::vector<int> rcs(N, 0);
    std::vector<std::string> errs(N);
    auto run_entry = [&](size_t e) {
        rayn_ctx* c = e == 0 ? ctx : ctx->peers[e - 1];
        auto bail = [&](int code, const std::string& m) { rcs[e] = code; errs[e] = m; };
        if (hipSetDevice(c->device) != hipSuccess) return bail(RAYN_ERR_HIP, "hipSetDevice");
        if (e == 0) {
            RenderTarget t = out;
            t.tiles = &mine[0];
            rcs[0] = render_device(ctx, p, d_s1, d_s2, d_scr, d_fis, t, stream);
            if (rcs[0]) errs[0] = ctx->err;
            return;
        }
        rayn_ctx::PeerBuf& B = ctx->peer_bufs[e - 1];
        const size_t px = mine[e].pixels, npk = std::max<size_t>(px, 1);
        if (n_tab > B.tables_cap) B.tab_valid = false; // the buffer is about to be re-allocated
        int r = ensure(c, &B.tables, &B.tables_cap, n_tab);
        if (!r) r = ensure(c, &B.packed, &B.packed_cap, npk * RAYN_FILM_FLOATS_PER_PIXEL);
        if (r) return bail(r, c->err);
        float *t1 = B.tables, *t2 = t1 + n1, *tscr = t2 + n2, *tfis = tscr + npx;
        // the peer's film IS the packed buffer: four planes over its owned pixels (the resolve writes them through DTile::film_base)
        const RenderTarget t = packed_target(B.packed, px, &mine[e]);
        // sample tables / scramble / filter table: broadcast once per (caller buffers, resolution, spp, bounces, volume marches, frame), not once per frame
        const uint64_t key[10] = {(uint64_t)(uintptr_t)d_s1, (uint64_t)(uintptr_t)d_s2, (uint64_t)(uintptr_t)d_scr, (uint64_t)(uintptr_t)d_fis, p->width, p->height,
                                  p->samples, p->max_bounces, p->volume_marches, p->frame};
        hipError_t he = hipSuccess;
        if (!B.tab_valid || memcmp(B.tab_key, key, sizeof key) != 0) {
            B.tab_valid = false;
            he = hipMemcpyPeerAsync(t1, c->device, d_s1, ctx->device, n1 * 4, c->stream);
            if (he == hipSuccess) he = hipMemcpyPeerAsync(t2, c->device, d_s2, ctx->device, n2 * 4, c->stream);
            if (he == hipSuccess) he = hipMemcpyPeerAsync(tscr, c->device, d_scr, ctx->device, npx * 4, c->stream);
            if (he == hipSuccess) he = hipMemcpyPeerAsync(tfis, c->device, d_fis, ctx->device, RAYN_FIS_TABLE_SIZE * 4, c->stream);
            if (he == hipSuccess) { memcpy(B.tab_key, key, sizeof key); B.tab_valid = true; ctx->table_broadcasts++; }
        }
        if (he != hipSuccess) return bail(RAYN_ERR_HIP, std::string("table broadcast: ") + hipGetErrorString(he));
        r = render_device(c, p, t1, t2, tscr, tfis, t, c->stream);
        if (r) return bail(r, c->err);
        if (px) {
            he = hipMemcpyPeerAsync(ctx->gather_buf + gather_off[e] * 10, ctx->device, B.packed, c->device, px * 40, c->stream); // the one gather copy
            if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
            if (he != hipSuccess) return bail(RAYN_ERR_HIP, std::string("film gather: ") + hipGetErrorString(he));
        }
    };
    {
        std::vector<std::thread> threads;
        for (size_t e = 1; e < N; e++) threads.emplace_back(run_entry, e);
        run_entry(0);
        for (auto& t : threads) t.join();
    }
    HIPCHK(hipSetDevice(ctx->device));
    for (size_t e = 0; e < N; e++) if (rcs[e]) return fail(ctx, rcs[e], "device entry " + std::to_string(e) + ": " + errs[e]);
    // scatter the peers' pixels into the caller's film (device 0)
    size_t t_off = 0;
    for (size_t e = 1; e < N; e++) {
        const std::vector<DTile>& pack = mine[e].d;
        if (pack.empty()) continue;
        HIPCHK(hipMemcpyAsync(ctx->gather_tiles + t_off, pack.data(), pack.size() * sizeof(DTile), hipMemcpyHostToDevice, stream));
        rayn_p0::launch_unpack_tiles(stream, ctx->gather_tiles + t_off, (uint32_t)pack.size(), p->width, out.color, out.alpha, out.bg, out.normal,
                                     ctx->gather_buf + gather_off[e] * 10, mine[e].pixels);
        t_off += pack.size();
    }
    HIPCHK(hipEventRecord(ctx->ev_mb, stream));
    HIPCHK(hipStreamSynchronize(stream)); // also keeps 'mine' alive until the tile lists have been copied
    // statistics: sums over the entries; ms_total = the whole multi-device frame on device 0's clock
    ctx->entry0_stats = ctx->stats;
    rayn_stats total = ctx->stats;
    for (rayn_ctx* c : ctx->peers) { add(total, c->stats); ctx->counters += c->counters; }
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ctx->ev_ma, ctx->ev_mb);
    total.ms_total = ms;
    ctx->stats = total;
    return RAYN_OK;
}

int render_any(rayn_ctx* ctx, const rayn_frame_params* p, const float* d_s1, const float* d_s2, const float* d_scr, const float* d_fis,
               const RenderTarget& out, hipStream_t stream) {
    if (ctx && !ctx->peers.empty()) return render_multi(ctx, p, d_s1, d_s2, d_scr, d_fis, out, stream);
    return render_device(ctx, p, d_s1, d_s2, d_scr, d_fis, out, stream);
}

} // namespace

extern "C" {

int rayn_hip_create(int device, rayn_ctx** out) {
    if (!out) return RAYN_ERR_INVALID_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return RAYN_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return RAYN_ERR_INVALID_ARG;
    rayn_ctx* ctx = new rayn_ctx();
    ctx->device = device;
    memset(&ctx->stats, 0, sizeof ctx->stats);
    // Only what EVERY frame needs is created here; worker streams / control blocks / pinned read-back buffers are created when a
    // frame first uses that worker (ensure_worker: a single-frame process - the reference's own usage, src/main.rs:28-45 - runs one
    // or two of the four), the multi-device event pair when a multi-device frame runs.
    bool ok = hipSetDevice(device) == hipSuccess && hipStreamCreate(&ctx->stream) == hipSuccess &&
              hipMalloc((void**)&ctx->d_scene, sizeof(DScene)) == hipSuccess && hipEventCreate(&ctx->ev_a) == hipSuccess &&
              hipEventCreate(&ctx->ev_b) == hipSuccess && hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) == hipSuccess;
    if (!ok) { rayn_hip_destroy(ctx); return RAYN_ERR_HIP; }
    // Launch tuning from the environment is OPT-IN (RAYN_HIP_ENV_TUNING=1; include/rayn_hip.h): a host that merely happens to export one
    // of these names must not change how its frames are scheduled or pay profiling events.  All of them are result-invariant
    // (tests/test_gpu_parity.py::test_tuning_variants_are_invisible); the measurement scripts under tools/ set the switch.
    if (const char* sw = getenv("RAYN_HIP_ENV_TUNING")) if (atoi(sw) != 0) {
        if (const char* e = getenv("RAYN_HIP_WORKERS")) ctx->cfg->n_workers = atoi(e);
        if (const char* e = getenv("RAYN_HIP_WORKER_MIN_PATHS")) ctx->cfg->two_worker_min_paths = (size_t)atoll(e); // 0 forces n_workers
        if (const char* e = getenv("RAYN_HIP_BATCH_PATHS")) { long long v = atoll(e); if (v >= 4096) ctx->cfg->batch_paths = (size_t)v; }
        if (const char* e = getenv("RAYN_HIP_COLD_BYTES")) { long long v = atoll(e); ctx->cfg->cold_bytes = v > 0 ? (size_t)v : 0; }
        if (const char* e = getenv("RAYN_HIP_PROFILE")) ctx->cfg->profiling = atoi(e) != 0;
        if (const char* e = getenv("RAYN_HIP_REFILL_EXTEND")) ctx->tun.refill_min_extend = (uint32_t)std::max(1, atoi(e));
        if (const char* e = getenv("RAYN_HIP_REFILL_SHADOW")) ctx->tun.refill_min_shadow = (uint32_t)std::max(1, atoi(e));
        if (const char* e = getenv("RAYN_HIP_PREFETCH_EXTEND")) ctx->tun.prefetch_min_extend = (uint32_t)std::max(1, atoi(e));
        if (const char* e = getenv("RAYN_HIP_PREFETCH_SHADOW")) ctx->tun.prefetch_min_shadow = (uint32_t)std::max(1, atoi(e));
        if (const char* e = getenv("RAYN_HIP_FAST_PATH")) ctx->tun.fast_path = atoi(e) != 0;
        if (const char* e = getenv("RAYN_HIP_PERSISTENT_BLOCKS")) ctx->tun.persistent_blocks = (uint32_t)std::max(1, atoi(e));
        if (const char* e = getenv("RAYN_HIP_SDF_TEMPLATES")) ctx->tun.sdf_templates = atoi(e) != 0;
        if (const char* e = getenv("RAYN_HIP_BULB_PATH")) ctx->tun.bulb_path = atoi(e) != 0;
        if (const char* e = getenv("RAYN_HIP_BULB_STEPS")) ctx->tun.bulb_steps = atoi(e) == 2 ? 2u : 1u;
        if (const char* e = getenv("RAYN_HIP_BULB_ORBIT_MIN")) ctx->tun.bulb_orbit_min = (uint32_t)std::max(0, atoi(e));
        if (const char* e = getenv("RAYN_HIP_BOX12S")) ctx->tun.box12s = atoi(e) != 0;
        if (const char* e = getenv("RAYN_HIP_BULB_RAYS")) ctx->tun.bulb_rays = (uint32_t)std::min(4, std::max(2, atoi(e)));
        if (const char* e = getenv("RAYN_HIP_BULB_PREFETCH")) ctx->tun.bulb_prefetch_min = (uint32_t)std::max(1, atoi(e));
    }
    *out = ctx;
    return RAYN_OK;
}

int rayn_hip_create_multi(const int* devices, int n_devices, rayn_ctx** out) {
    if (!out) return RAYN_ERR_INVALID_ARG;
    *out = nullptr;
    if (!devices || n_devices < 1 || n_devices > 64) return RAYN_ERR_INVALID_ARG;
    rayn_ctx* ctx = nullptr;
    int rc = rayn_hip_create(devices[0], &ctx);
    if (rc) return rc;
    for (int i = 1; i < n_devices; i++) {
        rayn_ctx* c = nullptr;
        rc = rayn_hip_create(devices[i], &c);
        if (rc) { rayn_hip_destroy(ctx); return rc; }
        c->cfg = &ctx->own_cfg; // one settings block for all entries
        ctx->peers.push_back(c);
        if (devices[i] != devices[0]) { // direct xGMI copies; "already enabled" is fine, and without access the runtime stages the copy
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, devices[0], devices[i]) == hipSuccess && can) {
                (void)hipSetDevice(devices[0]); (void)hipDeviceEnablePeerAccess(devices[i], 0);
                (void)hipSetDevice(devices[i]); (void)hipDeviceEnablePeerAccess(devices[0], 0);
                (void)hipGetLastError();
            }
        }
    }
    ctx->peer_bufs.resize(ctx->peers.size());
    for (int i = 0; i < n_devices; i++) { // entries sharing a GPU split its HBM budget
        int share = 0;
        for (int j = 0; j < n_devices; j++) share += devices[j] == devices[i];
        (i == 0 ? ctx : ctx->peers[i - 1])->budget_share = share;
    }
    (void)hipSetDevice(devices[0]);
    *out = ctx;
    return RAYN_OK;
}

int rayn_hip_device_count(const rayn_ctx* ctx) { return ctx ? (int)(1 + ctx->peers.size()) : 0; }
uint64_t rayn_hip_table_broadcasts(const rayn_ctx* ctx) { return ctx ? ctx->table_broadcasts : 0; }

void rayn_hip_destroy(rayn_ctx* ctx) {
    if (!ctx) return;
    for (size_t i = 0; i < ctx->peers.size(); i++) {
        rayn_ctx* c = ctx->peers[i];
        (void)hipSetDevice(c->device);
        if (i < ctx->peer_bufs.size()) {
            rayn_ctx::PeerBuf& B = ctx->peer_bufs[i];
            if (B.tables) (void)hipFree(B.tables);
            if (B.packed) (void)hipFree(B.packed);
        }
        rayn_hip_destroy(c);
    }
    ctx->peers.clear();
    (void)hipSetDevice(ctx->device);
    if (ctx->gather_buf) (void)hipFree(ctx->gather_buf);
    if (ctx->gather_tiles) (void)hipFree(ctx->gather_tiles);
    for (auto& up : ctx->unpack_plans) if (up.d_tiles) (void)hipFree(up.d_tiles);
    ctx->unpack_plans.clear();
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (Worker& w : ctx->workers) {
        if (w.own) (void)hipStreamSynchronize(w.own);
        for (auto e : w.event_pool) (void)hipEventDestroy(e);
        if (w.d_ctl) (void)hipFree(w.d_ctl);
        if (w.arena.base) (void)hipFree(w.arena.base);
        if (w.d_evals) (void)hipFree(w.d_evals);
        if (w.h_totals) (void)hipHostFree(w.h_totals);
        if (w.h_ctl) (void)hipHostFree(w.h_ctl);
        if (w.done) (void)hipEventDestroy(w.done);
        if (w.own) (void)hipStreamDestroy(w.own);
    }
    if (ctx->d_rec) (void)hipFree(ctx->d_rec);
    if (ctx->host_stage) (void)hipFree(ctx->host_stage);
    if (ctx->d_scene) (void)hipFree(ctx->d_scene);
    if (ctx->ev_a) (void)hipEventDestroy(ctx->ev_a);
    if (ctx->ev_b) (void)hipEventDestroy(ctx->ev_b);
    if (ctx->ev_ma) (void)hipEventDestroy(ctx->ev_ma);
    if (ctx->ev_mb) (void)hipEventDestroy(ctx->ev_mb);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char* rayn_hip_last_error(const rayn_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int rayn_hip_upload_world(rayn_ctx* ctx, const rayn_world_desc* world) {
    if (!ctx) return RAYN_ERR_INVALID_ARG;
    if (!world) return fail(ctx, RAYN_ERR_INVALID_ARG, "null world");
    if (world->n_hitables == 0 || world->n_hitables > RAYN_MAX_HITABLES || world->n_materials == 0 || world->n_materials > RAYN_MAX_MATERIALS ||
        world->n_lights > RAYN_MAX_LIGHTS)
        return fail(ctx, RAYN_ERR_INVALID_ARG, "world counts out of range");
    ctx->cfg->world = *world;
    ctx->cfg->have_world = true;
    for (auto& B : ctx->peer_bufs) B.tab_valid = false; // a host that rewrites its tables IN PLACE re-uploads the world (or passes other buffers): see rayn_hip.h
    return RAYN_OK;
}

int rayn_hip_render_frame_device(rayn_ctx* ctx, const rayn_frame_params* p, const float* d_samples_1d, const float* d_samples_2d,
                                 const float* d_scramble, const float* d_fis_table, float* d_out_color, float* d_out_alpha,
                                 float* d_out_background, float* d_out_normal, void* hip_stream) {
    if (!ctx) return RAYN_ERR_INVALID_ARG;
    return render_any(ctx, p, d_samples_1d, d_samples_2d, d_scramble, d_fis_table, RenderTarget{d_out_color, d_out_alpha, d_out_background, d_out_normal},
                      pick_stream(ctx, hip_stream));
}

/* the packed film of the share tile_first / tile_step of p (no tile subset); a zero-sized frame or tile has no tiles, a bad share gives 0 */
uint64_t rayn_share_pixels(const rayn_frame_params* p) {
    OwnedTiles share;
    if (!p || owned_tiles(*p, nullptr, true, &share)) return 0;
    return (uint64_t)share.pixels;
}

int rayn_hip_render_frame_packed_device(rayn_ctx* ctx, const rayn_frame_params* p, const float* d_samples_1d, const float* d_samples_2d,
                                        const float* d_scramble, const float* d_fis_table, float* d_packed, void* hip_stream) {
    if (!ctx) return RAYN_ERR_INVALID_ARG;
    if (!ctx->peers.empty()) return fail(ctx, RAYN_ERR_INVALID_ARG, "rayn_hip_render_frame_packed_device is a single-device entry (a multi-device context gathers by itself)");
    if (!ctx->tile_subset.empty()) return fail(ctx, RAYN_ERR_INVALID_ARG, "a packed film is defined for a tile_first / tile_step share, not for a tile subset");
    if (!p || !d_packed) return fail(ctx, RAYN_ERR_INVALID_ARG, "null frame params or packed film");
    // the four planes of the share's packed film: the resolve kernels write them through DTile::film_base (DTile::film_packed)
    return render_device(ctx, p, d_samples_1d, d_samples_2d, d_scramble, d_fis_table, packed_target(d_packed, (size_t)rayn_share_pixels(p), nullptr),
                         pick_stream(ctx, hip_stream));
}

int rayn_hip_unpack_share_device(rayn_ctx* ctx, const rayn_frame_params* p, const float* d_packed, float* d_out_color, float* d_out_alpha,
                                 float* d_out_background, float* d_out_normal, void* hip_stream) {
    if (!ctx) return RAYN_ERR_INVALID_ARG;
    if (!p || !d_packed || !d_out_color || !d_out_alpha || !d_out_background || !d_out_normal) return fail(ctx, RAYN_ERR_INVALID_ARG, "null buffer");
    if (!p->width || !p->height || !p->tile_w || !p->tile_h) return fail(ctx, RAYN_ERR_INVALID_ARG, "zero-sized frame or tile");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, hip_stream);
    const uint32_t key[6] = {p->width, p->height, p->tile_w, p->tile_h, p->tile_first, p->tile_step ? p->tile_step : 1};
    const rayn_ctx::UnpackPlan* plan = nullptr;
    for (const auto& up : ctx->unpack_plans) if (memcmp(up.key, key, sizeof key) == 0) { plan = &up; break; }
    if (!plan) { // first use of this share: build + upload its tile list (synchronous, once); an invalid share is never kept
        rayn_ctx::UnpackPlan up;
        memcpy(up.key, key, sizeof key);
        OwnedTiles share; // of tile_first / tile_step, no tile subset
        if (const char* why = owned_tiles(*p, nullptr, true, &share)) return fail(ctx, RAYN_ERR_INVALID_ARG, why);
        const std::vector<DTile>& tiles = share.d;
        up.pixels = share.pixels;
        up.n_tiles = (uint32_t)tiles.size();
        up.d_tiles = nullptr;
        if (up.n_tiles) {
            if (hipMalloc((void**)&up.d_tiles, tiles.size() * sizeof(DTile)) != hipSuccess) return fail(ctx, RAYN_ERR_OOM, "hipMalloc of a share's tile list failed");
            hipError_t e = hipMemcpy(up.d_tiles, tiles.data(), tiles.size() * sizeof(DTile), hipMemcpyHostToDevice);
            if (e != hipSuccess) { (void)hipFree(up.d_tiles); return fail(ctx, RAYN_ERR_HIP, std::string("tile list upload: ") + hipGetErrorString(e)); }
        }
        ctx->unpack_plans.push_back(up);
        plan = &ctx->unpack_plans.back();
    }
    if (plan->n_tiles)
        rayn_p0::launch_unpack_tiles(s, plan->d_tiles, plan->n_tiles, p->width, d_out_color, d_out_alpha, d_out_background, d_out_normal, d_packed, plan->pixels);
    HIPCHK(hipGetLastError());
    return RAYN_OK; // enqueued on the stream, not waited for
}

// What the post-process entries (save_to_pixels, denoise, denoise_variance, progressive_*) share around their own argument checks.  post_enter: 'why' is
// the entry's verdict on its arguments (nullptr = valid); on RAYN_OK the context's device is current - a multi-device ctx is entry 0: its
// device is devices[0], where the film lives - and *s is the stream to enqueue on.
static int post_enter(rayn_ctx* ctx, const char* why, void* hip_stream, hipStream_t* s) {
    if (!ctx) return RAYN_ERR_INVALID_ARG;
    if (why) return fail(ctx, RAYN_ERR_INVALID_ARG, why);
    HIPCHK(hipSetDevice(ctx->device));
    *s = pick_stream(ctx, hip_stream);
    return RAYN_OK;
}
static int post_enqueued(rayn_ctx* ctx) {
    HIPCHK(hipGetLastError());
    return RAYN_OK; // enqueued on the stream, not waited for
}

int rayn_hip_save_to_pixels_device(rayn_ctx* ctx, uint32_t kind, uint32_t have_mask, int transparent_background, uint32_t width, uint32_t height,
                                   const float* d_color, const float* d_alpha, const float* d_background, const float* d_normal, uint8_t* d_out,
                                   void* hip_stream) {
    const char* why = nullptr;
    const int arm = save_to_arm(kind, have_mask, transparent_background, &why); // < 0: why = the reference's Err text
    if (arm >= 0) {
        const uint32_t reads = save_to_arm_reads(arm);
        why = check_size(width, height);
        if (!why && (!d_out || ((reads & 1u) && !d_color) || ((reads & 2u) && !d_alpha) || ((reads & 4u) && !d_background) || ((reads & 8u) && !d_normal)))
            why = "null buffer";
    }
    hipStream_t s;
    if (int rc = post_enter(ctx, why, hip_stream, &s)) return rc;
    launch_save_to(s, arm, width, height, d_color, d_alpha, d_background, d_normal, d_out);
    return post_enqueued(ctx);
}

// The HDR display transform (display.hip): both entries differ only in which output the final kernel writes.
static int display_entry(rayn_ctx* ctx, const rayn_display_params* dp, uint32_t have_mask, int transparent_background, uint32_t width, uint32_t height,
                         const float* d_color, const float* d_alpha, const float* d_background, void* d_state, void* d_scratch, size_t scratch_bytes,
                         uint8_t* d_out8, float* d_out_color, bool want_color, float* d_out_meter, float* d_out_bloom, void* hip_stream) {
    int arm = -1;
    const char* why = display_check_args(dp, have_mask, transparent_background, width, height, d_color, d_alpha, d_background, d_state, d_scratch,
                                         scratch_bytes, &arm);
    if (!why && !(want_color ? (const void*)d_out_color : (const void*)d_out8)) why = "null buffer";
    if (!why && want_color && (d_out_color == d_color || d_out_color == d_background)) why = "d_out_color must not be d_color or d_background";
    hipStream_t s;
    if (int rc = post_enter(ctx, why, hip_stream, &s)) return rc;
    launch_display(s, arm, *dp, width, height, d_color, d_alpha, d_background, d_state, d_scratch, d_out8, d_out_color, d_out_meter, d_out_bloom);
    return post_enqueued(ctx);
}

int rayn_hip_display_pixels_device(rayn_ctx* ctx, const rayn_display_params* dp, uint32_t have_mask, int transparent_background, uint32_t width,
                                   uint32_t height, const float* d_color, const float* d_alpha, const float* d_background, void* d_state,
                                   void* d_scratch, size_t scratch_bytes, uint8_t* d_out, float* d_out_meter, float* d_out_bloom, void* hip_stream) {
    return display_entry(ctx, dp, have_mask, transparent_background, width, height, d_color, d_alpha, d_background, d_state, d_scratch, scratch_bytes,
                         d_out, nullptr, false, d_out_meter, d_out_bloom, hip_stream);
}

int rayn_hip_display_color_device(rayn_ctx* ctx, const rayn_display_params* dp, uint32_t have_mask, int transparent_background, uint32_t width,
                                  uint32_t height, const float* d_color, const float* d_alpha, const float* d_background, void* d_state,
                                  void* d_scratch, size_t scratch_bytes, float* d_out_color, float* d_out_meter, float* d_out_bloom, void* hip_stream) {
    return display_entry(ctx, dp, have_mask, transparent_background, width, height, d_color, d_alpha, d_background, d_state, d_scratch, scratch_bytes,
                         nullptr, d_out_color, true, d_out_meter, d_out_bloom, hip_stream);
}

int rayn_hip_denoise_device(rayn_ctx* ctx, uint32_t width, uint32_t height, uint32_t iterations, float sigma_color, float sigma_normal,
                            float sigma_alpha, const float* d_color, const float* d_alpha, const float* d_normal, float* d_out_color,
                            void* d_scratch, size_t scratch_bytes, void* hip_stream) {
    hipStream_t s;
    if (int rc = post_enter(ctx, denoise_check_args(width, height, iterations, sigma_color, sigma_normal, sigma_alpha, d_color, d_alpha, d_normal, d_out_color,
                                                    d_scratch, scratch_bytes), hip_stream, &s)) return rc;
    launch_denoise(s, width, height, iterations, sigma_color, sigma_normal, sigma_alpha, d_color, d_alpha, d_normal, d_out_color, d_scratch);
    return post_enqueued(ctx);
}

int rayn_hip_denoise_variance_device(rayn_ctx* ctx, const rayn_frame_params* p, uint32_t iterations, float sigma_luminance, float sigma_normal,
                                     float sigma_alpha, const float* d_color, const float* d_alpha, const float* d_normal, const void* d_state,
                                     size_t state_bytes, float* d_out_color, float* d_out_variance, void* d_scratch, size_t scratch_bytes,
                                     void* hip_stream) {
    hipStream_t s;
    if (int rc = post_enter(ctx, denoise_variance_check_args(p, iterations, sigma_luminance, sigma_normal, sigma_alpha, d_color, d_alpha, d_normal, d_state,
                                                             state_bytes, d_out_color, d_out_variance, d_scratch, scratch_bytes), hip_stream, &s)) return rc;
    launch_denoise_variance(s, *p, iterations, sigma_luminance, sigma_normal, sigma_alpha, d_color, d_alpha, d_normal, d_state, d_out_color, d_out_variance,
                            d_scratch);
    return post_enqueued(ctx);
}

// Guided upscaling (upscale.hip): the low film and the G-buffers of both resolutions -> the planes of the high film.
int rayn_hip_upscale_device(rayn_ctx* ctx, uint32_t width, uint32_t height, const rayn_upscale_params* up, const float* d_color,
                            const float* d_alpha, const float* d_background, const float* d_normal, const void* d_low_records,
                            const uint32_t* d_low_object, const void* d_high_records, const uint32_t* d_high_object, float* d_out_color,
                            float* d_out_alpha, float* d_out_background, float* d_out_normal, float* d_out_weight, void* hip_stream) {
    const UpscalePlanes pl = {d_color, d_alpha, d_background, d_normal, d_low_records, d_low_object, d_high_records, d_high_object,
                              d_out_color, d_out_alpha, d_out_background, d_out_normal, d_out_weight};
    hipStream_t s;
    if (int rc = post_enter(ctx, upscale_check_args(width, height, up, pl), hip_stream, &s)) return rc;
    launch_upscale(s, width, height, *up, pl);
    return post_enqueued(ctx);
}

// The primary-hit pass of rayn_hip_gbuffer_device and rayn_hip_preview_device over the scratch g: one centre ray per pixel through the scene's
// PRODUCT extend kernel at depth 0, selected as rayn_hip_probe_extend selects it, then (P, t) records and object indices.  The scene of (uploaded
// world, p) goes to ctx->d_scene on the stream, as a render's does (a pageable source is staged before hipMemcpyAsync returns, so the stack copy
// may go away).  What the scene decided comes back for the kernels a caller launches afterwards.
struct PrimaryHit { DScene hs; int single_sdf; Tuning tun; KernelSet K; };
static int primary_hit_pass(rayn_ctx* ctx, const rayn_frame_params* p, hipStream_t s, const GbufScratch& g, void* d_out_records, uint32_t* d_out_object,
                            PrimaryHit* out) {
    if (int rc = build_scene(ctx, ctx->cfg->world, *p, &out->hs)) return rc;
    HIPCHK(hipMemcpyAsync(ctx->d_scene, &out->hs, sizeof out->hs, hipMemcpyHostToDevice, s));
    out->single_sdf = scene_march_kernels(ctx, out->hs, *p, &out->tun);
    out->K = kernel_set(ctx->cfg->fma_policy);
    if (ctx->cfg->fma_policy) rayn_p1::launch_gbuffer_rays(s, ctx->d_scene, g);
    else rayn_p0::launch_gbuffer_rays(s, ctx->d_scene, g);
    out->K.extend(s, false, ctx->d_scene, 0, g.q, g.npad, g.pool, g.ent_obj, out->single_sdf, g.ctl, g.evals, out->tun);
    launch_gbuffer_finish(s, g, d_out_records, d_out_object);
    return RAYN_OK;
}

// The primary-hit G-buffer (temporal.hip).
int rayn_hip_gbuffer_device(rayn_ctx* ctx, const rayn_frame_params* p, void* d_out_records, uint32_t* d_out_object, void* d_scratch,
                            size_t scratch_bytes, void* hip_stream) {
    const char* why = gbuffer_check_args(p, d_out_records, d_out_object, d_scratch, scratch_bytes);
    if (!why && ctx && !ctx->cfg->have_world) why = "rayn_hip_upload_world has not been called";
    hipStream_t s;
    if (int rc = post_enter(ctx, why, hip_stream, &s)) return rc;
    PrimaryHit ph;
    if (int rc = primary_hit_pass(ctx, p, s, gbuffer_scratch(p->width, p->height, d_scratch), d_out_records, d_out_object, &ph)) return rc;
    return post_enqueued(ctx);
}

// The preview integrator (preview.hip): the G-buffer pass above into the entry's scratch, then per round of AO rays the job-generating kernel, the
// scene's PRODUCT shadow-march kernel over the jobs it parked (none without a TracedSDF, as launch_shade decides) and the resolve.
int rayn_hip_preview_device(rayn_ctx* ctx, const rayn_frame_params* p, const rayn_preview_params* pp, const float* d_samples, const float* d_scramble,
                            float* d_out_color, float* d_out_alpha, float* d_out_normal, float* d_out_ao, void* d_out_records, uint32_t* d_out_object,
                            void* d_scratch, size_t scratch_bytes, void* hip_stream) {
    const char* why = preview_check_args(p, pp, d_samples, d_scramble, d_out_color, d_out_alpha, d_out_normal, d_out_ao, d_out_records, d_out_object,
                                         d_scratch, scratch_bytes);
    if (!why && ctx && !ctx->cfg->have_world) why = "rayn_hip_upload_world has not been called";
    hipStream_t s;
    if (int rc = post_enter(ctx, why, hip_stream, &s)) return rc;
    const PreviewScratch ps = preview_scratch(p->width, p->height, pp->samples, d_scratch, d_out_records, d_out_object);
    PrimaryHit ph;
    if (int rc = primary_hit_pass(ctx, p, s, ps.g, ps.records, ps.object, &ph)) return rc;
    const Nee nee = preview_nee(ps);
    for (uint32_t k0 = 0; k0 < pp->samples; k0 += ps.round) {
        const uint32_t kn = std::min(ps.round, pp->samples - k0);
        if (ctx->cfg->fma_policy) rayn_p1::launch_preview_jobs(s, ctx->d_scene, ps, k0, kn, pp->radius, pp->ambient, d_samples, d_scramble, d_out_normal);
        else rayn_p0::launch_preview_jobs(s, ctx->d_scene, ps, k0, kn, pp->radius, pp->ambient, d_samples, d_scramble, d_out_normal);
        if (ph.hs.n_sdf > 0) ph.K.shadow_march(s, false, ctx->d_scene, nee, kn * ps.g.npad, ph.single_sdf, ps.g.ctl, ps.g.evals, ph.tun);
        launch_preview_resolve(s, ps, kn, pp->samples, k0 + kn >= pp->samples, d_out_color, d_out_alpha, d_out_ao);
    }
    return post_enqueued(ctx);
}

// Frame generation (interpolate.hip): two rendered keys and the frame's own G-buffer -> the planes of the frame between them.  The hitable
// velocities come from the world as uploaded at the time of the call, by value, as for the accumulate entries.
int rayn_hip_interpolate_device(rayn_ctx* ctx, const rayn_frame_params* p, const rayn_interpolate_params* ip, const rayn_interpolate_key* key_a,
                                const rayn_interpolate_key* key_b, const void* d_gbuffer_records, const uint32_t* d_gbuffer_object,
                                float* d_out_color, float* d_out_alpha, float* d_out_background, float* d_out_normal, uint32_t* d_out_source,
                                void* hip_stream) {
    const char* why = interpolate_check_args(p, ip, key_a, key_b, d_gbuffer_records, d_gbuffer_object, d_out_color, d_out_alpha, d_out_background,
                                             d_out_normal, d_out_source);
    if (!why && ctx && !ctx->cfg->have_world) why = "rayn_hip_upload_world has not been called";
    InterpolateCall c;
    memset(&c, 0, sizeof c);
    if (!why && (!build_camera(*key_a->camera, &c.a.cam) || !build_camera(*key_b->camera, &c.b.cam))) why = "unknown camera kind";
    hipStream_t s;
    if (int rc = post_enter(ctx, why, hip_stream, &s)) return rc;
    c.width = p->width;
    c.height = p->height;
    c.depth_tolerance = ip->depth_tolerance;
    c.time = p->time_start;
    const rayn_interpolate_key* keys[2] = {key_a, key_b};
    InterpolateKey* dst[2] = {&c.a, &c.b};
    for (int k = 0; k < 2; k++) {
        dst[k]->color = keys[k]->d_color;
        dst[k]->alpha = keys[k]->d_alpha;
        dst[k]->background = keys[k]->d_background;
        dst[k]->normal = keys[k]->d_normal;
        dst[k]->records = keys[k]->d_records;
        dst[k]->object = keys[k]->d_object;
        dst[k]->time = keys[k]->time_start;
    }
    c.records = d_gbuffer_records;
    c.object = d_gbuffer_object;
    c.out_color = d_out_color;
    c.out_alpha = d_out_alpha;
    c.out_background = d_out_background;
    c.out_normal = d_out_normal;
    c.out_source = d_out_source;
    const rayn_world_desc& w = ctx->cfg->world;
    c.n_hitables = w.n_hitables < RAYN_MAX_HITABLES ? w.n_hitables : RAYN_MAX_HITABLES;
    for (uint32_t i = 0; i < c.n_hitables; i++)
        c.hvel[i] = make_float4(w.hitables[i].center_vel.x, w.hitables[i].center_vel.y, w.hitables[i].center_vel.z, w.hitables[i].animated ? 1.0f : 0.0f);
    launch_interpolate(s, c);
    return post_enqueued(ctx);
}

// The PNG encoder (png.hip): the 8-bit image of save_to_pixels / display_pixels -> the zlib stream of its IDAT chunk behind a 16-byte header.
int rayn_hip_png_encode_device(rayn_ctx* ctx, uint32_t w, uint32_t h, uint32_t bpp, const uint8_t* d_img, void* d_out, size_t out_bytes, void* d_scratch,
                               size_t scratch_bytes, void* hip_stream) {
    const char* why = png_check_args(w, h, bpp, d_img, d_out, out_bytes, d_scratch, scratch_bytes);
    hipStream_t s;
    if (int rc = post_enter(ctx, why, hip_stream, &s)) return rc;
    HIPCHK(launch_png_encode(s, w, h, bpp, d_img, d_out, d_scratch));
    return post_enqueued(ctx);
}

// The PNG encoder with LZ77 matches (png_lz.hip): rayn_hip_png_encode_device's arguments and output, smaller streams.
int rayn_hip_png_encode_lz77_device(rayn_ctx* ctx, uint32_t w, uint32_t h, uint32_t bpp, const uint8_t* d_img, void* d_out, size_t out_bytes,
                                    void* d_scratch, size_t scratch_bytes, void* hip_stream) {
    const char* why = png_lz_check_args(w, h, bpp, d_img, d_out, out_bytes, d_scratch, scratch_bytes);
    hipStream_t s;
    if (int rc = post_enter(ctx, why, hip_stream, &s)) return rc;
    HIPCHK(launch_png_encode_lz77(s, w, h, bpp, d_img, d_out, d_scratch));
    return post_enqueued(ctx);
}

// Its deflate stage alone on n bytes of the caller's: a zlib stream behind the same 16-byte header.
int rayn_hip_deflate_lz77_device(rayn_ctx* ctx, const void* d_data, size_t n, uint32_t stride, void* d_out, size_t out_bytes, void* d_scratch,
                                 size_t scratch_bytes, void* hip_stream) {
    const char* why = deflate_check_args(d_data, n, d_out, out_bytes, d_scratch, scratch_bytes);
    hipStream_t s;
    if (int rc = post_enter(ctx, why, hip_stream, &s)) return rc;
    HIPCHK(launch_deflate_lz77(s, d_data, (uint32_t)n, stride, d_out, d_scratch));
    return post_enqueued(ctx);
}

// The EXR chunk encoder (exr.hip): planes in the film's layout -> the ZIP-compressed scanline chunks of an OpenEXR file behind a chunk table.
int rayn_hip_exr_encode_device(rayn_ctx* ctx, uint32_t w, uint32_t h, uint32_t n_channels, const void* const* d_planes, const uint32_t* layout,
                               uint32_t matches, void* d_out, size_t out_bytes, void* d_scratch, size_t scratch_bytes, void* hip_stream) {
    const char* why = exr_check_args(w, h, n_channels, d_planes, layout, matches, d_out, out_bytes, d_scratch, scratch_bytes);
    hipStream_t s;
    if (int rc = post_enter(ctx, why, hip_stream, &s)) return rc;
    HIPCHK(launch_exr_encode(s, w, h, n_channels, d_planes, layout, matches, d_out, d_scratch));
    return post_enqueued(ctx);
}

// The JPEG scan encoder (jpeg.hip): the 8-bit image of save_to_pixels / display_pixels -> the entropy-coded scan behind a 16-byte header.
int rayn_hip_jpeg_encode_device(rayn_ctx* ctx, uint32_t w, uint32_t h, uint32_t bpp, uint32_t quality, uint32_t subsampling, uint32_t restart_interval,
                                const uint8_t* d_img, void* d_out, size_t out_bytes, void* d_scratch, size_t scratch_bytes, void* hip_stream) {
    const char* why = jpeg_check_args(w, h, bpp, quality, subsampling, restart_interval, d_img, d_out, out_bytes, d_scratch, scratch_bytes);
    hipStream_t s;
    if (int rc = post_enter(ctx, why, hip_stream, &s)) return rc;
    launch_jpeg_encode(s, jpeg_geometry(w, h, bpp, subsampling, restart_interval), quality, d_img, d_out, d_scratch);
    return post_enqueued(ctx);
}

// The temporal accumulate entries: moments == false is the plain one (the moments arguments are then not looked at); resample is step 4's
// filter (0: the two older entries), bad_resample the resample entry's own complaint about its rp, reported after the shared checks.
static int temporal_accumulate(rayn_ctx* ctx, const rayn_frame_params* p, const rayn_temporal_params* tp, const rayn_camera* prev_camera,
                               float prev_time_start, const float* d_color, const float* d_normal, const void* d_gbuffer_records,
                               const uint32_t* d_gbuffer_object, const void* d_prev_history, void* d_new_history, size_t history_bytes,
                               bool moments, const void* d_prev_moments, void* d_new_moments, size_t moments_bytes, float* d_out_color,
                               void* hip_stream, uint32_t resample, const char* bad_resample) {
    const char* why = temporal_check_args(p, tp, prev_camera, d_color, d_normal, d_gbuffer_records, d_gbuffer_object, d_prev_history, d_new_history,
                                          history_bytes, d_out_color);
    if (!why && moments)
        why = temporal_moments_check_args(p, d_color, d_normal, d_gbuffer_records, d_gbuffer_object, d_prev_history, d_new_history, d_prev_moments,
                                          d_new_moments, moments_bytes, d_out_color);
    if (!why) why = bad_resample;
    if (!why && ctx && !ctx->cfg->have_world) why = "rayn_hip_upload_world has not been called";
    TemporalScene ts;
    memset(&ts, 0, sizeof ts);
    if (!why && prev_camera && !build_camera(*prev_camera, &ts.cam)) why = "unknown camera kind";
    hipStream_t s;
    if (int rc = post_enter(ctx, why, hip_stream, &s)) return rc;
    fill_temporal_scene(&ts, ctx->cfg->world, prev_time_start, p->time_start);
    launch_temporal_accumulate(s, p->width, p->height, *tp, ts, d_color, d_normal, d_gbuffer_records, d_gbuffer_object, d_prev_history, d_new_history,
                               d_out_color, moments ? d_prev_moments : nullptr, moments ? d_new_moments : nullptr, resample);
    return post_enqueued(ctx);
}

int rayn_hip_temporal_accumulate_device(rayn_ctx* ctx, const rayn_frame_params* p, const rayn_temporal_params* tp, const rayn_camera* prev_camera,
                                        float prev_time_start, const float* d_color, const float* d_normal, const void* d_gbuffer_records,
                                        const uint32_t* d_gbuffer_object, const void* d_prev_history, void* d_new_history, size_t history_bytes,
                                        float* d_out_color, void* hip_stream) {
    return temporal_accumulate(ctx, p, tp, prev_camera, prev_time_start, d_color, d_normal, d_gbuffer_records, d_gbuffer_object, d_prev_history,
                               d_new_history, history_bytes, false, nullptr, nullptr, 0, d_out_color, hip_stream, 0, nullptr);
}

int rayn_hip_temporal_accumulate_moments_device(rayn_ctx* ctx, const rayn_frame_params* p, const rayn_temporal_params* tp,
                                                const rayn_camera* prev_camera, float prev_time_start, const float* d_color, const float* d_normal,
                                                const void* d_gbuffer_records, const uint32_t* d_gbuffer_object, const void* d_prev_history,
                                                void* d_new_history, size_t history_bytes, const void* d_prev_moments, void* d_new_moments,
                                                size_t moments_bytes, float* d_out_color, void* hip_stream) {
    return temporal_accumulate(ctx, p, tp, prev_camera, prev_time_start, d_color, d_normal, d_gbuffer_records, d_gbuffer_object, d_prev_history,
                               d_new_history, history_bytes, true, d_prev_moments, d_new_moments, moments_bytes, d_out_color, hip_stream, 0, nullptr);
}

int rayn_hip_temporal_accumulate_resample_device(rayn_ctx* ctx, const rayn_frame_params* p, const rayn_temporal_params* tp,
                                                 const rayn_temporal_resample_params* rp, const rayn_camera* prev_camera, float prev_time_start,
                                                 const float* d_color, const float* d_normal, const void* d_gbuffer_records,
                                                 const uint32_t* d_gbuffer_object, const void* d_prev_history, void* d_new_history,
                                                 size_t history_bytes, const void* d_prev_moments, void* d_new_moments, size_t moments_bytes,
                                                 float* d_out_color, void* hip_stream) {
    const bool moments = d_prev_moments || d_new_moments; // both NULL: no moments; one alone: the moments entry's error
    const char* bad = temporal_resample_check_args(rp);
    return temporal_accumulate(ctx, p, tp, prev_camera, prev_time_start, d_color, d_normal, d_gbuffer_records, d_gbuffer_object, d_prev_history,
                               d_new_history, history_bytes, moments, d_prev_moments, d_new_moments, moments_bytes, d_out_color, hip_stream,
                               bad ? 0u : rp->resample, bad);
}

// Temporal supersampling (temporal_upscale.hip): the guided upscaling and the temporal accumulate at the high size in one kernel.  The
// hitable velocities come from the world as uploaded at the time of the call, by value, as for the accumulate entries.
int rayn_hip_temporal_upscale_device(rayn_ctx* ctx, const rayn_frame_params* p, const rayn_upscale_params* up, const rayn_temporal_params* tp,
                                     const rayn_temporal_upscale_params* sp, const rayn_camera* low_camera, const rayn_camera* prev_camera,
                                     float prev_time_start, const float* d_color, const float* d_alpha, const float* d_background,
                                     const float* d_normal, const void* d_low_records, const uint32_t* d_low_object, const void* d_high_records,
                                     const uint32_t* d_high_object, const void* d_prev_history, void* d_new_history, size_t history_bytes,
                                     float* d_out_color, float* d_out_alpha, float* d_out_background, float* d_out_normal, float* d_out_weight,
                                     void* hip_stream) {
    const TemporalUpscaleCall c = {{d_color, d_alpha, d_background, d_normal, d_low_records, d_low_object, d_high_records, d_high_object,
                                    d_out_color, d_out_alpha, d_out_background, d_out_normal, d_out_weight},
                                   d_prev_history, d_new_history, history_bytes};
    const char* why = temporal_upscale_check_args(p, up, tp, sp, low_camera, prev_camera, c);
    if (!why && ctx && !ctx->cfg->have_world) why = "rayn_hip_upload_world has not been called";
    TemporalScene ts;
    memset(&ts, 0, sizeof ts);
    DCamera low;
    if (!why && prev_camera && !build_camera(*prev_camera, &ts.cam)) why = "unknown camera kind";
    if (!why && low_camera && !build_camera(*low_camera, &low)) why = "unknown camera kind";
    hipStream_t s;
    if (int rc = post_enter(ctx, why, hip_stream, &s)) return rc;
    fill_temporal_scene(&ts, ctx->cfg->world, prev_time_start, p->time_start);
    launch_temporal_upscale(s, p->width, p->height, *up, *tp, sp->confidence, low_camera ? &low : nullptr, ts, c);
    return post_enqueued(ctx);
}

int rayn_hip_denoise_temporal_variance_device(rayn_ctx* ctx, uint32_t width, uint32_t height, uint32_t iterations, float sigma_luminance,
                                              float sigma_normal, float sigma_alpha, const float* d_color, const float* d_alpha, const float* d_normal,
                                              const uint32_t* d_gbuffer_object, const void* d_history, size_t history_bytes, const void* d_moments,
                                              size_t moments_bytes, float* d_out_color, float* d_out_variance, void* d_scratch, size_t scratch_bytes,
                                              void* hip_stream) {
    hipStream_t s;
    if (int rc = post_enter(ctx, denoise_temporal_check_args(width, height, iterations, sigma_luminance, sigma_normal, sigma_alpha, d_color, d_alpha, d_normal,
                                                             d_gbuffer_object, d_history, history_bytes, d_moments, moments_bytes, d_out_color, d_out_variance,
                                                             d_scratch, scratch_bytes), hip_stream, &s)) return rc;
    launch_denoise_temporal_variance(s, width, height, iterations, sigma_luminance, sigma_normal, sigma_alpha, d_color, d_alpha, d_normal, d_gbuffer_object,
                                     d_history, d_moments, d_out_color, d_out_variance, d_scratch);
    return post_enqueued(ctx);
}

int rayn_hip_denoise_temporal_variance_feedback_device(rayn_ctx* ctx, uint32_t width, uint32_t height, uint32_t iterations, float sigma_luminance,
                                                       float sigma_normal, float sigma_alpha, const float* d_color, const float* d_alpha,
                                                       const float* d_normal, const uint32_t* d_gbuffer_object, void* d_history, size_t history_bytes,
                                                       const void* d_moments, size_t moments_bytes, float* d_out_color, float* d_out_variance,
                                                       void* d_scratch, size_t scratch_bytes, float feedback, void* hip_stream) {
    hipStream_t s;
    if (int rc = post_enter(ctx, denoise_temporal_feedback_check_args(width, height, iterations, sigma_luminance, sigma_normal, sigma_alpha, d_color, d_alpha,
                                                                      d_normal, d_gbuffer_object, d_history, history_bytes, d_moments, moments_bytes, d_out_color,
                                                                      d_out_variance, d_scratch, scratch_bytes, feedback), hip_stream, &s)) return rc;
    launch_denoise_temporal_variance_feedback(s, width, height, iterations, sigma_luminance, sigma_normal, sigma_alpha, d_color, d_alpha, d_normal,
                                              d_gbuffer_object, d_history, d_moments, d_out_color, d_out_variance, d_scratch, feedback);
    return post_enqueued(ctx);
}

// the checks every rayn_hip_progressive_* entry shares; on success *L is the state's layout
static const char* progressive_geometry(const rayn_frame_params* p, const void* d_state, size_t state_bytes, ProgLayout* L) {
    const char* why = progressive_check_geometry(p, d_state, state_bytes);
    if (!why) *L = progressive_layout(p->width, p->height, p->tile_w, p->tile_h);
    return why;
}

int rayn_hip_progressive_reset_device(rayn_ctx* ctx, const rayn_frame_params* p, void* d_state, size_t state_bytes, void* hip_stream) {
    ProgLayout L;
    hipStream_t s;
    if (int rc = post_enter(ctx, progressive_geometry(p, d_state, state_bytes, &L), hip_stream, &s)) return rc;
    launch_progressive_reset(s, L, d_state);
    return post_enqueued(ctx);
}

int rayn_hip_progressive_accumulate_device(rayn_ctx* ctx, const rayn_frame_params* p, const rayn_progressive_params* pp, const uint32_t* tiles,
                                           uint32_t n_tiles, const float* d_color, const float* d_alpha, const float* d_background,
                                           const float* d_normal, void* d_state, size_t state_bytes, float* d_out_color, float* d_out_alpha,
                                           float* d_out_background, float* d_out_normal, void* hip_stream) {
    ProgLayout L;
    const char* why = progressive_geometry(p, d_state, state_bytes, &L);
    if (!why) why = progressive_check_params(pp);
    if (!why && (!d_color || !d_alpha || !d_background || !d_normal || !d_out_color || !d_out_alpha || !d_out_background || !d_out_normal)) why = "null buffer";
    if (!why) {
        const float* in[4] = {d_color, d_alpha, d_background, d_normal};
        const float* out[4] = {d_out_color, d_out_alpha, d_out_background, d_out_normal};
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++)
                if (out[i] == in[j]) why = "the output film must not alias the epoch film";
    }
    if (!why) why = progressive_check_tiles(L, tiles, n_tiles);
    hipStream_t s;
    if (int rc = post_enter(ctx, why, hip_stream, &s)) return rc;
    uint32_t* d_list = nullptr;
    if (tiles) {
        d_list = (uint32_t*)((char*)d_state + L.off_listed);
        ctx->prog_host.assign(tiles, tiles + n_tiles); // the caller's array may go away once this returns
        HIPCHK(hipMemcpyAsync(d_list, ctx->prog_host.data(), (size_t)n_tiles * 4u, hipMemcpyHostToDevice, s));
    }
    launch_progressive_accumulate(s, L, *pp, d_list, n_tiles, d_color, d_alpha, d_background, d_normal, d_state, d_out_color, d_out_alpha,
                                  d_out_background, d_out_normal);
    launch_progressive_compact(s, L, d_state);
    return post_enqueued(ctx);
}

int64_t rayn_hip_progressive_fetch_active(rayn_ctx* ctx, const rayn_frame_params* p, const void* d_state, size_t state_bytes, uint32_t* out_tiles,
                                          uint32_t cap, rayn_progressive_totals* out_totals, void* hip_stream) {
    ProgLayout L;
    const char* why = progressive_geometry(p, d_state, state_bytes, &L);
    if (!why && out_tiles && cap < L.n_tiles) why = "out_tiles holds fewer entries than the film has tiles";
    hipStream_t s;
    if (int rc = post_enter(ctx, why, hip_stream, &s)) return rc;
    const size_t words = 4u + (out_tiles ? (size_t)L.n_tiles : 0u); // totals, then the list: adjacent in the state, ONE copy
    ctx->prog_host.resize(words);
    HIPCHK(hipMemcpyAsync(ctx->prog_host.data(), (const char*)d_state + L.off_totals, words * 4u, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const uint32_t* h = ctx->prog_host.data();
    if (h[0] > L.n_tiles) return fail(ctx, RAYN_ERR_INVALID_ARG, "the state holds more active tiles than the film has tiles (not a state of this film?)");
    if (out_totals) {
        out_totals->active_tiles = h[0];
        memcpy(&out_totals->max_e, &h[1], 4);
        out_totals->outlier_pixels = (uint64_t)h[2] | ((uint64_t)h[3] << 32);
    }
    if (out_tiles) memcpy(out_tiles, h + 4, (size_t)h[0] * 4u);
    return (int64_t)h[0];
}

int rayn_hip_progressive_tile_report(rayn_ctx* ctx, const rayn_frame_params* p, const void* d_state, size_t state_bytes, uint32_t* out_epochs,
                                     uint32_t* out_retired, uint32_t* out_outliers, float* out_max_e, void* hip_stream) {
    ProgLayout L;
    hipStream_t s;
    if (int rc = post_enter(ctx, progressive_geometry(p, d_state, state_bytes, &L), hip_stream, &s)) return rc;
    ctx->prog_host.resize((size_t)L.n_tiles * 4u);
    HIPCHK(hipMemcpyAsync(ctx->prog_host.data(), (const char*)d_state + L.off_records, (size_t)L.n_tiles * 16u, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (uint32_t k = 0; k < L.n_tiles; k++) {
        const uint32_t* r = ctx->prog_host.data() + (size_t)k * 4u;
        if (out_epochs) out_epochs[k] = r[0];
        if (out_retired) out_retired[k] = r[1];
        if (out_outliers) out_outliers[k] = r[2];
        if (out_max_e) memcpy(&out_max_e[k], &r[3], 4);
    }
    return RAYN_OK;
}

int rayn_hip_get_entry_stats(const rayn_ctx* ctx, int entry, rayn_stats* out) {
    if (!ctx || !out || entry < 0 || entry > (int)ctx->peers.size()) return RAYN_ERR_INVALID_ARG;
    if (ctx->peers.empty()) *out = ctx->stats;
    else *out = entry == 0 ? ctx->entry0_stats : ctx->peers[(size_t)entry - 1]->stats;
    return RAYN_OK;
}

int rayn_hip_render_frame(rayn_ctx* ctx, const rayn_frame_params* p, const float* samples_1d, const float* samples_2d, const float* scramble,
                          const float* fis_table, float* out_color, float* out_alpha, float* out_background, float* out_normal) {
    int rc = check_frame_args(ctx, p, samples_1d, samples_2d, scramble, fis_table, RenderTarget{out_color, out_alpha, out_background, out_normal});
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t spp = (size_t)p->samples * 4, npx = (size_t)p->width * p->height;
    const size_t n1 = spp * rayn_sets_1d(p->max_bounces, p->volume_marches), n2 = spp * 2 * rayn_sets_2d(p->max_bounces, p->volume_marches);
    // device copies of the caller's buffers: one grow-only allocation kept by the context (no hipMalloc / hipFree per frame)
    const size_t total = n1 + n2 + npx + RAYN_FIS_TABLE_SIZE + npx * RAYN_FILM_FLOATS_PER_PIXEL;
    rc = ensure(ctx, &ctx->host_stage, &ctx->host_stage_cap, total);
    if (rc) return rc;
    float* d = ctx->host_stage;
    float *d1 = d, *d2 = d1 + n1, *dscr = d2 + n2, *dfis = dscr + npx, *dc = dfis + RAYN_FIS_TABLE_SIZE, *da = dc + 3 * npx, *db = da + npx, *dn = db + 3 * npx;
    hipError_t e = hipSuccess;
    auto up = [&](float* dst, const float* src, size_t n) { if (e == hipSuccess) e = hipMemcpyAsync(dst, src, n * 4, hipMemcpyHostToDevice, ctx->stream); };
    up(d1, samples_1d, n1); up(d2, samples_2d, n2); up(dscr, scramble, npx); up(dfis, fis_table, RAYN_FIS_TABLE_SIZE);
    // The film goes up first only when the call leaves some of its pixels alone (a tile share, a tile subset, or a resolution the
    // reference's tile grid under-covers, src/film.rs:399-427): Film::render_frame_into overwrites every pixel of every tile it runs
    // (src/film.rs:82-98), so a whole-frame call - what src/main.rs does - has nothing to preserve (82.9 MB at 1920x1080, 1.33 GB at 8K).
    const bool covers = TileGrid(p->width, p->height, p->tile_w, p->tile_h).covers(p->width, p->height, p->tile_w, p->tile_h);
    const bool owns_all = covers && p->tile_step <= 1 && ctx->tile_subset.empty();
    if (!owns_all) { up(dc, out_color, 3 * npx); up(da, out_alpha, npx); up(db, out_background, 3 * npx); up(dn, out_normal, 3 * npx); }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream); // the host tables may change as soon as this call returns; pageable sources are staged by the runtime
    if (e != hipSuccess) return fail(ctx, RAYN_ERR_HIP, std::string("upload: ") + hipGetErrorString(e));
    rc = render_any(ctx, p, d1, d2, dscr, dfis, RenderTarget{dc, da, db, dn}, ctx->stream);
    if (rc == RAYN_OK) {
        auto down = [&](float* dst, const float* src, size_t n) { if (e == hipSuccess) e = hipMemcpy(dst, src, n * 4, hipMemcpyDeviceToHost); };
        down(out_color, dc, 3 * npx); down(out_alpha, da, npx); down(out_background, db, 3 * npx); down(out_normal, dn, 3 * npx);
        if (e != hipSuccess) rc = fail(ctx, RAYN_ERR_HIP, std::string("download: ") + hipGetErrorString(e));
    }
    return rc;
}

int rayn_hip_get_stats(const rayn_ctx* ctx, rayn_stats* out) {
    if (!ctx || !out) return RAYN_ERR_INVALID_ARG;
    *out = ctx->stats;
    return RAYN_OK;
}

/* profiling controls: per-kernel-class HIP-event timing (stats.ms_*) and SDF-evaluation counting
 * (instrumented kernel variants; slower — for roofline accounting only). */
int rayn_hip_set_profiling(rayn_ctx* ctx, int timing, int count_evals) {
    if (!ctx) return RAYN_ERR_INVALID_ARG;
    ctx->cfg->profiling = timing != 0;
    ctx->cfg->counting = count_evals != 0;
    return RAYN_OK;
}
static int get_counts(const rayn_ctx* ctx, const unsigned long long* counts, int n, uint64_t* out) {
    if (!ctx || !out) return RAYN_ERR_INVALID_ARG;
    for (int i = 0; i < n; i++) out[i] = counts[i];
    return RAYN_OK;
}
int rayn_hip_get_eval_counts(const rayn_ctx* ctx, uint64_t out[3]) { return get_counts(ctx, ctx ? ctx->counters.evals : nullptr, 3, out); }
int rayn_hip_get_sdf_iterations(const rayn_ctx* ctx, uint64_t out[3]) { return get_counts(ctx, ctx ? ctx->counters.iters : nullptr, 3, out); }
int rayn_hip_get_elision_counts(const rayn_ctx* ctx, uint64_t out[3]) { return get_counts(ctx, ctx ? ctx->counters.elided : nullptr, 3, out); }
int rayn_hip_get_stage_slots(const rayn_ctx* ctx, uint64_t out[2]) { return get_counts(ctx, ctx ? ctx->counters.stage_slots : nullptr, 2, out); }
int rayn_hip_set_batch_paths(rayn_ctx* ctx, uint64_t paths) {
    if (!ctx || paths < 4096) return RAYN_ERR_INVALID_ARG;
    ctx->cfg->batch_paths = (size_t)paths;
    return RAYN_OK;
}

int rayn_hip_set_cold_bytes(rayn_ctx* ctx, uint64_t bytes) {
    if (!ctx) return RAYN_ERR_INVALID_ARG;
    ctx->cfg->cold_bytes = (size_t)bytes;
    return RAYN_OK;
}

int rayn_hip_set_workers(rayn_ctx* ctx, int n_workers, uint64_t min_paths) {
    if (!ctx || n_workers < 1 || n_workers > MAX_WORKERS) return RAYN_ERR_INVALID_ARG;
    ctx->cfg->n_workers = n_workers;
    ctx->cfg->two_worker_min_paths = (size_t)min_paths;
    return RAYN_OK;
}
int rayn_hip_set_tile_subset(rayn_ctx* ctx, const uint32_t* tiles, uint32_t n) {
    if (!ctx || (n && !tiles)) return RAYN_ERR_INVALID_ARG;
    std::vector<uint32_t> v(tiles, tiles + n);
    std::sort(v.begin(), v.end());
    if (std::adjacent_find(v.begin(), v.end()) != v.end()) return fail(ctx, RAYN_ERR_INVALID_ARG, "duplicate tile index in the subset");
    ctx->tile_subset.swap(v);
    return RAYN_OK;
}
int rayn_hip_set_trace_tile(rayn_ctx* ctx, int tile_index) {
    if (!ctx) return RAYN_ERR_INVALID_ARG;
    if (!ctx->peers.empty()) return fail(ctx, RAYN_ERR_INVALID_ARG, "rayn_hip_set_trace_tile is not supported on a multi-device context");
    ctx->trace_tile = tile_index;
    return RAYN_OK;
}
int64_t rayn_hip_get_trace(const rayn_ctx* ctx, uint32_t* out, uint64_t cap_records) {
    if (!ctx) return RAYN_ERR_INVALID_ARG;
    const uint64_t n = ctx->trace.size() / 6;
    if (out) memcpy(out, ctx->trace.data(), (size_t)std::min(n, cap_records) * 24);
    return (int64_t)n;
}
int rayn_hip_fma_policy(void) { return 0; }
#ifndef RAYN_BUILD_VARIANT
#define RAYN_BUILD_VARIANT ""
#endif
const char* rayn_hip_build_variant(void) { return RAYN_BUILD_VARIANT; }
int rayn_hip_set_fma_policy(rayn_ctx* ctx, int policy) {
    if (!ctx || (policy != 0 && policy != 1)) return RAYN_ERR_INVALID_ARG;
    ctx->cfg->fma_policy = policy;
    return RAYN_OK;
}
size_t rayn_hip_sizeof(int which) {
    switch (which) {
    case 0: return sizeof(rayn_world_desc);
    case 1: return sizeof(rayn_frame_params);
    case 2: return sizeof(rayn_stats);
    case 3: return sizeof(rayn_hitable);
    case 4: return sizeof(rayn_material);
    case 5: return sizeof(rayn_light);
    case 6: return sizeof(rayn_camera);
    case 7: return sizeof(rayn_temporal_resample_params);
    case 8: return sizeof(rayn_display_params);
    case 9: return sizeof(rayn_upscale_params);
    case 10: return sizeof(rayn_temporal_upscale_params);
    case 11: return sizeof(rayn_preview_params);
    case 12: return sizeof(rayn_interpolate_params);
    case 13: return sizeof(rayn_interpolate_key);
    default: return 0;
    }
}

} // extern "C"
