// probes.hip — the test probes of the C ABI (rayn_hip_probe_*): per-lane device primitives, the PRODUCT march kernels, the PRODUCT queue stages, the PRODUCT shade and ray-generation stages and the PRODUCT film resolve on caller data.
// Test infrastructure; the one kernel defined here is k_probe_huffman, a shell around huffman_code of png_device.h (kernels.hip holds the other probe kernels; the JPEG probes launch jpeg.hip's own).
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "driver.h"
#include "frame_layout.h"
#include "jpeg.h"
#include "png_device.h"

using namespace rayn;

namespace {
struct DevBuf { // hipMalloc'ed scratch of a probe call, released on every exit path
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 4); }
    template <typename T> T* as() const { return (T*)p; }
};
struct ProbeArena : Arena { // the one device allocation of a stage probe call, released on every exit path
    ~ProbeArena() { if (base) (void)hipFree(base); }
    template <typename F> hipError_t alloc(F carve) { // run_worker's pattern: a dry run of `carve` sizes the allocation, then the same carve hands it out
        Arena dry; carve(dry);
        const hipError_t e = hipMalloc((void**)&base, dry.off);
        if (e != hipSuccess) { base = nullptr; return e; }
        cap = dry.off; carve(*this);
        return hipSuccess;
    }
};

// One workgroup of PNG_BT threads per count set: huffman_code<N> of png_device.h as the block kernels call it - the counts in LDS, published by its first
// barrier - and the lengths and table entries it leaves
template <uint32_t N>
__global__ __launch_bounds__(PNG_BT) void k_probe_huffman(const uint32_t* __restrict__ counts, uint32_t* __restrict__ clen, uint32_t* __restrict__ tab) {
    __shared__ uint32_t hist[N];
    __shared__ HuffmanLds<N> h;
    const size_t at = (size_t)blockIdx.x * N;
    for (uint32_t s = threadIdx.x; s < N; s += PNG_BT) hist[s] = counts[at + s];
    huffman_code(hist, h);
    for (uint32_t s = threadIdx.x; s < N; s += PNG_BT) clen[at + s] = h.clen[s], tab[at + s] = h.tab[s];
}
} // namespace

extern "C" {

/* ---- test probes: per-lane device primitives on caller data (HOST pointers) ---- */

// builds the scene of (uploaded world, p), uploads it to ctx->d_scene and hands the host copy back when the caller wants it
static int probe_common(rayn_ctx* ctx, const rayn_frame_params* p, DScene* out_hs = nullptr) {
    int rc = validate(ctx, p);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    DScene hs;
    rc = build_scene(ctx, ctx->cfg->world, *p, &hs);
    if (rc) return rc;
    HIPCHK(hipMemcpy(ctx->d_scene, &hs, sizeof hs, hipMemcpyHostToDevice));
    if (out_hs) *out_hs = hs;
    return RAYN_OK;
}
// count_evals on (rayn_hip_set_profiling): what a probe's instrumented launch left in its d_ev[16], decoded into the context's counters as a frame's
// read-back is (Counters::decode) - the four getters then report that probe call
static int probe_counters(rayn_ctx* ctx, const unsigned long long* d_ev) {
    unsigned long long h[16];
    HIPCHK(hipMemcpy(h, d_ev, sizeof h, hipMemcpyDeviceToHost));
    ctx->counters.decode(h);
    return RAYN_OK;
}
// the first n slots of a device pool into the seven host arrays of a stage probe
static int probe_pool_out(rayn_ctx* ctx, const Pool& pool, size_t n, float* geo0, float* geo1, float* col0, float* col1, float* aov, uint32_t* term_key, uint8_t* term_info) {
    HIPCHK(hipMemcpy(geo0, pool.geo0, n * 16, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(geo1, pool.geo1, n * 16, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(col0, pool.col0, n * 16, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(col1, pool.col1, n * 16, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(aov, pool.aov, n * 16, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(term_key, pool.term_key, n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(term_info, pool.term_info, n, hipMemcpyDeviceToHost));
    return RAYN_OK;
}
int rayn_hip_probe_sdf_dist(rayn_ctx* ctx, const rayn_frame_params* p, uint32_t hitable_index, const float* pts, float* out, uint32_t n) {
    int rc = probe_common(ctx, p);
    if (rc) return rc;
    if (hitable_index >= ctx->cfg->world.n_hitables || ctx->cfg->world.hitables[hitable_index].kind != RAYN_HITABLE_TRACED_SDF)
        return fail(ctx, RAYN_ERR_INVALID_ARG, "hitable_index does not name a TracedSDF of the uploaded world");
    if (!pts || !out) return fail(ctx, RAYN_ERR_INVALID_ARG, "null buffer");
    const KernelSet K = kernel_set(ctx->cfg->fma_policy);
    DevBuf d_in, d_out;
    HIPCHK(d_in.alloc((size_t)n * 12)); HIPCHK(d_out.alloc((size_t)n * 4));
    HIPCHK(hipMemcpy(d_in.p, pts, (size_t)n * 12, hipMemcpyHostToDevice));
    K.probe_dist(ctx->stream, ctx->d_scene, hitable_index, d_in.as<float>(), d_out.as<float>(), n);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(out, d_out.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RAYN_OK;
}
// sdf_dist<false, sdfk> of one TracedSDF in the division arm fast_div (at most the object's own) with the scale of a packet whose lane-0 time is t0.  The scene
// copy that carries the lowered fast_div lives in a buffer of this call: ctx->d_scene keeps what the upload decided.
int rayn_hip_probe_sdf_dist_as(rayn_ctx* ctx, const rayn_frame_params* p, uint32_t hitable_index, int32_t sdfk, uint32_t fast_div, float t0, const float* pts,
                               float* out, uint32_t n) {
    int rc = validate(ctx, p);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    DScene hs;
    rc = build_scene(ctx, ctx->cfg->world, *p, &hs);
    if (rc) return rc;
    if (hitable_index >= ctx->cfg->world.n_hitables || ctx->cfg->world.hitables[hitable_index].kind != RAYN_HITABLE_TRACED_SDF)
        return fail(ctx, RAYN_ERR_INVALID_ARG, "hitable_index does not name a TracedSDF of the uploaded world");
    if (!pts || !out) return fail(ctx, RAYN_ERR_INVALID_ARG, "null buffer");
    if (n == 0 || n > (1u << 26)) return fail(ctx, RAYN_ERR_INVALID_ARG, "probe size out of range");
    DHitable& h = hs.h[hitable_index];
    if (sdfk != -1 && sdfk != (int32_t)RAYN_SDF_SPHERE && sdfk != (int32_t)RAYN_SDF_MANDELBOX && sdfk != (int32_t)RAYN_SDF_MANDELBULB && sdfk != 100)
        return fail(ctx, RAYN_ERR_INVALID_ARG, "sdfk names no instantiation of sdf_dist (-1, a RAYN_SDF_* kind or 100)");
    if (sdfk >= 0 && sdfk != 100 && (uint32_t)sdfk != h.sdf_kind) return fail(ctx, RAYN_ERR_INVALID_ARG, "sdfk is not the SDF kind of the object");
    if (sdfk == 100 && (h.sdf_kind != RAYN_SDF_MANDELBOX || h.fast_div != 2u || h.iterations != 12u))
        return fail(ctx, RAYN_ERR_INVALID_ARG, "sdfk 100 needs a 12-iteration MandelBox whose short division the upload verified (fast_div 2)");
    if (fast_div > h.fast_div) return fail(ctx, RAYN_ERR_INVALID_ARG, "fast_div may only lower the object's own division arm");
    if (sdfk == 100 && fast_div != 2u) return fail(ctx, RAYN_ERR_INVALID_ARG, "sdfk 100 has the short division compiled in: fast_div must be 2");
    h.fast_div = fast_div;
    const KernelSet K = kernel_set(ctx->cfg->fma_policy);
    DevBuf d_sc, d_in, d_out;
    HIPCHK(d_sc.alloc(sizeof hs)); HIPCHK(d_in.alloc((size_t)n * 12)); HIPCHK(d_out.alloc((size_t)n * 4));
    HIPCHK(hipMemcpy(d_sc.p, &hs, sizeof hs, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_in.p, pts, (size_t)n * 12, hipMemcpyHostToDevice));
    K.probe_dist_as(ctx->stream, d_sc.as<DScene>(), hitable_index, sdfk, t0, d_in.as<float>(), d_out.as<float>(), n);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, d_out.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RAYN_OK;
}
// what the values of (uploaded world, p) decide: the same build_scene and scene_march_kernels a render calls, nothing uploaded and nothing launched
// beyond build_scene's own verdict kernel (short_div_is_exact)
int rayn_hip_probe_scene_dispatch(rayn_ctx* ctx, const rayn_frame_params* p, int32_t* out) {
    int rc = validate(ctx, p);
    if (rc) return rc;
    if (!out) return fail(ctx, RAYN_ERR_INVALID_ARG, "null buffer");
    HIPCHK(hipSetDevice(ctx->device));
    DScene hs;
    rc = build_scene(ctx, ctx->cfg->world, *p, &hs);
    if (rc) return rc;
    Tuning tun;
    out[0] = scene_march_kernels(ctx, hs, *p, &tun);
    out[1] = tun.sdf_kind; out[2] = tun.bulb ? 1 : 0; out[3] = (int32_t)hs.anim_spheres;
    for (uint32_t i = 0; i < RAYN_MAX_HITABLES; i++) out[4 + i] = i < hs.n_hitables ? (int32_t)hs.h[i].fast_div : -1;
    return RAYN_OK;
}
// HitableStore::add_hits for caller-supplied rays through the PRODUCT extend kernel of the uploaded scene (k_extend1, or the generic k_extend of a
// multi-SDF scene): one synthetic ray queue - pool slot i = ray i, queue entry i = i, padded to whole 64-slot groups - one launch, then hit_t / object read back.
int rayn_hip_probe_extend(rayn_ctx* ctx, const rayn_frame_params* p, uint32_t depth, const float* org, const float* dir, float* out_t,
                          uint32_t* out_obj, uint32_t n) {
    DScene hs;
    int rc = probe_common(ctx, p, &hs);
    if (rc) return rc;
    if (!org || !dir || !out_t || !out_obj) return fail(ctx, RAYN_ERR_INVALID_ARG, "null buffer");
    if (n == 0 || n > (1u << 26)) return fail(ctx, RAYN_ERR_INVALID_ARG, "probe size out of range");
    Tuning tun;
    const int single_sdf = scene_march_kernels(ctx, hs, *p, &tun);
    const KernelSet K = kernel_set(ctx->cfg->fma_policy);
    const uint32_t npad = (n + 63u) & ~63u;
    std::vector<float4> g0(n), g1(n);
    std::vector<uint32_t> q(npad, INVALID);
    uint32_t none_bits = OBJ_NONE;
    float none_f; memcpy(&none_f, &none_bits, 4);
    for (uint32_t i = 0; i < n; i++) {
        g0[i] = make_float4(org[3 * i], org[3 * i + 1], org[3 * i + 2], dir[3 * i]);
        g1[i] = make_float4(dir[3 * i + 1], dir[3 * i + 2], 0.0f, none_f);
        q[i] = i;
    }
    DCtl hc;
    memset(&hc, 0, sizeof hc);
    hc.q_groups = npad / 64; hc.q_valid = n;
    DevBuf d_g0, d_g1, d_c1, d_q, d_obj, d_ctl, d_ev;
    HIPCHK(d_g0.alloc((size_t)n * 16)); HIPCHK(d_g1.alloc((size_t)n * 16)); HIPCHK(d_c1.alloc((size_t)n * 16)); HIPCHK(d_q.alloc((size_t)npad * 4));
    HIPCHK(d_obj.alloc(npad)); HIPCHK(d_ctl.alloc(sizeof(DCtl))); HIPCHK(d_ev.alloc(128));
    HIPCHK(hipMemcpy(d_g0.p, g0.data(), (size_t)n * 16, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(d_g1.p, g1.data(), (size_t)n * 16, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_c1.p, 0, (size_t)n * 16)); // ray time 0 (the packet time of closure-sequenced hitables)
    HIPCHK(hipMemcpy(d_q.p, q.data(), (size_t)npad * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemset(d_obj.p, 0xEE, npad));
    HIPCHK(hipMemcpy(d_ctl.p, &hc, sizeof hc, hipMemcpyHostToDevice)); HIPCHK(hipMemset(d_ev.p, 0, 128));
    Pool pool;
    memset(&pool, 0, sizeof pool);
    pool.geo0 = d_g0.as<float4>(); pool.geo1 = d_g1.as<float4>(); pool.col1 = d_c1.as<float4>();
    const bool count = ctx->cfg->counting; // the instrumented instantiation; the context's counters then report this call
    K.extend(ctx->stream, count, ctx->d_scene, depth, d_q.as<uint32_t>(), npad, pool, d_obj.as<uint8_t>(), single_sdf, d_ctl.as<DCtl>(), d_ev.as<unsigned long long>(), tun);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    if (count) { rc = probe_counters(ctx, d_ev.as<unsigned long long>()); if (rc) return rc; }
    std::vector<uint8_t> obj(npad);
    HIPCHK(hipMemcpy(g1.data(), d_g1.p, (size_t)n * 16, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(obj.data(), d_obj.p, npad, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++) {
        uint32_t bits; memcpy(&bits, &g1[i].w, 4);
        if ((bits & 0xFFu) != obj[i]) return fail(ctx, RAYN_ERR_HIP, "internal: the pool's hit object and the per-entry object byte disagree");
        out_t[i] = g1[i].z;
        out_obj[i] = obj[i] == OBJ_NONE ? INVALID : obj[i];
    }
    for (uint32_t i = n; i < npad; i++) if (obj[i] != OBJ_NONE) return fail(ctx, RAYN_ERR_HIP, "internal: a padding entry of the queue was not marked empty");
    return RAYN_OK;
}
// TracedSDF::occluded of every TracedSDF of the uploaded scene (the SDF factors of HitableStore::test_occluded; the analytic spheres are k_shade_setup's part)
// for caller-supplied segments through the PRODUCT shadow-march kernel (k_shadow1 / k_shadow_bulb / the generic k_shadow): one synthetic job list, one launch.
int rayn_hip_probe_shadow(rayn_ctx* ctx, const rayn_frame_params* p, const float* start, const float* end, float* out, uint32_t n) {
    DScene hs;
    int rc = probe_common(ctx, p, &hs);
    if (rc) return rc;
    if (!start || !end || !out) return fail(ctx, RAYN_ERR_INVALID_ARG, "null buffer");
    if (n == 0 || n > (1u << 26)) return fail(ctx, RAYN_ERR_INVALID_ARG, "probe size out of range");
    if (hs.n_sdf == 0) return fail(ctx, RAYN_ERR_INVALID_ARG, "the uploaded world holds no TracedSDF: nothing to march");
    Tuning tun;
    const int single_sdf = scene_march_kernels(ctx, hs, *p, &tun);
    const KernelSet K = kernel_set(ctx->cfg->fma_policy);
    std::vector<float2> geo(3 * (size_t)n);
    std::vector<uint32_t> ref(n);
    for (uint32_t i = 0; i < n; i++) {
        geo[3 * (size_t)i] = make_float2(start[3 * i], start[3 * i + 1]);
        geo[3 * (size_t)i + 1] = make_float2(start[3 * i + 2], end[3 * i]);
        geo[3 * (size_t)i + 2] = make_float2(end[3 * i + 1], end[3 * i + 2]);
        ref[i] = i;
    }
    DCtl hc;
    memset(&hc, 0, sizeof hc);
    hc.job_count = n;
    DevBuf d_geo, d_ref, d_vis, d_t0, d_ctl, d_ev;
    HIPCHK(d_geo.alloc((size_t)n * 24)); HIPCHK(d_ref.alloc((size_t)n * 4)); HIPCHK(d_vis.alloc(n)); HIPCHK(d_t0.alloc((size_t)n * 4));
    HIPCHK(d_ctl.alloc(sizeof(DCtl))); HIPCHK(d_ev.alloc(128));
    HIPCHK(hipMemcpy(d_geo.p, geo.data(), (size_t)n * 24, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(d_ref.p, ref.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_vis.p, 2, n)); // every segment pending; the kernels write 1 for a visible one and leave the mark otherwise (= occluded, Nee::vis)
    HIPCHK(hipMemset(d_t0.p, 0, (size_t)n * 4)); HIPCHK(hipMemcpy(d_ctl.p, &hc, sizeof hc, hipMemcpyHostToDevice)); HIPCHK(hipMemset(d_ev.p, 0, 128));
    Nee nee;
    memset(&nee, 0, sizeof nee);
    nee.vis = d_vis.as<uint8_t>(); nee.t0 = d_t0.as<float>(); nee.cap = n; nee.job_ref = d_ref.as<uint32_t>(); nee.job_geo = d_geo.as<float2>(); nee.jobcap = n;
    const bool count = ctx->cfg->counting; // the instrumented instantiation; the context's counters then report this call
    K.shadow_march(ctx->stream, count, ctx->d_scene, nee, n, single_sdf, d_ctl.as<DCtl>(), d_ev.as<unsigned long long>(), tun);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    if (count) { rc = probe_counters(ctx, d_ev.as<unsigned long long>()); if (rc) return rc; }
    std::vector<uint8_t> vis(n);
    HIPCHK(hipMemcpy(vis.data(), d_vis.p, n, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++) out[i] = vis[i] == 1 ? 1.0f : 0.0f;
    return RAYN_OK;
}
// the sizes that decide whether a launch of the march kernels reaches its steady state (kernels.h) + the two launch-tuning values of this context that enter them
int rayn_hip_probe_march_limits(const rayn_ctx* ctx, uint32_t* chunk, uint32_t* endgame_entries, uint32_t* persistent_blocks, uint32_t* bulb_rays) {
    if (!ctx || !chunk || !endgame_entries || !persistent_blocks || !bulb_rays) return RAYN_ERR_INVALID_ARG;
    *chunk = CHUNK; *endgame_entries = ENDGAME_ENTRIES;
    *persistent_blocks = ctx->tun.persistent_blocks; *bulb_rays = ctx->tun.bulb_rays;
    return RAYN_OK;
}
int rayn_hip_probe_detmath(rayn_ctx* ctx, uint32_t op, const float* a, const float* b, float* out, uint32_t n) {
    if (!ctx) return RAYN_ERR_INVALID_ARG;
    if (!a || !b || !out) return fail(ctx, RAYN_ERR_INVALID_ARG, "null buffer");
    const KernelSet K = kernel_set(ctx->cfg->fma_policy);
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf d_a, d_b, d_out;
    const size_t na = ((op >= 9 && op <= 12) || (op >= 17 && op <= 19)) ? (size_t)n * 3 : (size_t)n; // ops 9..12 and 17..19 read xyz triples from a
    HIPCHK(d_a.alloc(na * 4)); HIPCHK(d_b.alloc((size_t)n * 4)); HIPCHK(d_out.alloc((size_t)n * 4));
    HIPCHK(hipMemcpy(d_a.p, a, na * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(d_b.p, b, (size_t)n * 4, hipMemcpyHostToDevice));
    K.probe_detmath(ctx->stream, op, d_a.as<float>(), d_b.as<float>(), d_out.as<float>(), n);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(out, d_out.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RAYN_OK;
}
int rayn_hip_probe_shading(rayn_ctx* ctx, const rayn_frame_params* p, uint32_t op, uint32_t index, const float* in, float* out, const float* aux, uint32_t n) {
    int rc = probe_common(ctx, p);
    if (rc) return rc;
    if (!in || !out) return fail(ctx, RAYN_ERR_INVALID_ARG, "null buffer");
    if (op >= PROBE_SHADING_OPS) return fail(ctx, RAYN_ERR_INVALID_ARG, "unknown shading probe op");
    if (n == 0 || n > (1u << 26)) return fail(ctx, RAYN_ERR_INVALID_ARG, "probe size out of range");
    const rayn_world_desc& w = ctx->cfg->world;
    if (op >= 6 && op <= 8) {
        if (index >= w.n_materials) return fail(ctx, RAYN_ERR_INVALID_ARG, "index does not name a material of the uploaded world");
        const uint32_t k = w.materials[index].kind;
        if (op == 6 && k == RAYN_MAT_SKY) return fail(ctx, RAYN_ERR_INVALID_ARG, "Sky's BSDF::f panics in the reference: not probed");
        if (op == 8 && k != RAYN_MAT_LAMBERTIAN && k != RAYN_MAT_DIELECTRIC) return fail(ctx, RAYN_ERR_INVALID_ARG, "only Lambertian and Dielectric scatter");
    }
    if ((op == 9 || op == 10) && index >= w.n_lights) return fail(ctx, RAYN_ERR_INVALID_ARG, "index does not name a light of the uploaded world");
    if (op == 11 && index == 0) return fail(ctx, RAYN_ERR_INVALID_ARG, "light_index needs at least one light");
    if (op == 12 && !aux) return fail(ctx, RAYN_ERR_INVALID_ARG, "fis_sample needs the inverse-CDF table in aux");
    if ((op == 13 || op == 14) && (index >= w.n_hitables || w.hitables[index].kind != RAYN_HITABLE_SPHERE))
        return fail(ctx, RAYN_ERR_INVALID_ARG, "index does not name an analytic Sphere of the uploaded world");
    const size_t nin = (size_t)n * probe_shading_in(op), nout = (size_t)n * probe_shading_out(op);
    const KernelSet K = kernel_set(ctx->cfg->fma_policy);
    DevBuf d_in, d_out, d_aux;
    HIPCHK(d_in.alloc(nin * 4)); HIPCHK(d_out.alloc(nout * 4)); HIPCHK(d_aux.alloc(RAYN_FIS_TABLE_SIZE * 4));
    HIPCHK(hipMemcpy(d_in.p, in, nin * 4, hipMemcpyHostToDevice));
    if (op == 12) HIPCHK(hipMemcpy(d_aux.p, aux, RAYN_FIS_TABLE_SIZE * 4, hipMemcpyHostToDevice));
    K.probe_shading(ctx->stream, ctx->d_scene, op, index, d_in.as<float>(), d_out.as<float>(), d_aux.as<float>(), n);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, d_out.p, nout * 4, hipMemcpyDeviceToHost));
    return RAYN_OK;
}
// The two queue stages of one depth (bin: k_group_hist, k_scan_tile, k_tile_prefix, k_bin_scatter; repack: k_scan_tile, k_tile_prefix, k_compact_scatter) on a
// caller-built ray queue: the two stage launchers run_worker's depth loop calls (launch_bin_stage, launch_repack_stage) over tables from the carve function
// its arena is carved by.  The survivor ballots and counts k_shade_setup would write between the stages are built here on the host from the binned queue as
// the device left it.  Both output queues hold out_slots slots (>= the input's full need, whatever the
// cap_groups arguments say) and start filled with `sentinel`, so the overflow guard runs without an address leaving its buffer and a stray write shows.
int rayn_hip_probe_queue(rayn_ctx* ctx, uint32_t nclass, uint32_t n_tiles, const uint32_t* tile_groups, const uint32_t* q, const uint8_t* ent_obj,
                         const uint8_t* survive, uint32_t n_refs, uint32_t cap_groups_bin, uint32_t cap_groups_repack, uint32_t max_entries,
                         uint32_t max_slots, uint32_t sentinel, uint32_t out_slots, uint32_t* out_bq, uint32_t* out_qn, uint32_t* out_tile,
                         uint32_t* out_cls_cnt, uint32_t* out_cls_base, uint64_t* ctl_io) {
    if (!ctx) return RAYN_ERR_INVALID_ARG;
    if (!tile_groups || !q || !ent_obj || !survive || !out_bq || !out_qn || !out_tile || !out_cls_cnt || !out_cls_base || !ctl_io)
        return fail(ctx, RAYN_ERR_INVALID_ARG, "null buffer");
    if (nclass == 0 || nclass > SCAN_NC_BIN) return fail(ctx, RAYN_ERR_INVALID_ARG, "nclass outside 1..16");
    if (n_tiles == 0 || n_tiles > (1u << 20)) return fail(ctx, RAYN_ERR_INVALID_ARG, "n_tiles outside 1..2^20");
    if (max_entries > (1u << 27) || max_slots > (1u << 27) || out_slots > (1u << 27)) return fail(ctx, RAYN_ERR_INVALID_ARG, "probe size out of range");
    if (sentinel == INVALID || sentinel < n_refs) return fail(ctx, RAYN_ERR_INVALID_ARG, "the sentinel must be neither INVALID nor a queue reference");
    for (int k = 0; k < 12; k++) if (k != 5 && k != 6 && k != 7 && k != 8 && ctl_io[k] > 0xFFFFFFFFull) return fail(ctx, RAYN_ERR_INVALID_ARG, "a 32-bit field of ctl_io is out of range");
    size_t groups = 0;
    for (uint32_t k = 0; k < n_tiles; k++) {
        groups += tile_groups[k];
        if (groups > (1u << 20)) return fail(ctx, RAYN_ERR_INVALID_ARG, "more than 2^26 queue entries");
    }
    const size_t n_entries = groups * 64;
    // the full need of the bin stage (the repack's is at most that: survivors of a tile's segment, unpadded) - and every entry must be binnable
    size_t need_groups = 0;
    {
        size_t e = 0;
        for (uint32_t k = 0; k < n_tiles; k++) {
            uint32_t cnt[SCAN_NC_BIN] = {0};
            for (size_t end = e + (size_t)tile_groups[k] * 64; e < end; e++) {
                const uint32_t o = ent_obj[e];
                if (o != OBJ_NONE && o >= nclass) return fail(ctx, RAYN_ERR_INVALID_ARG, "an object byte is neither a class below nclass nor OBJ_NONE");
                if (q[e] == INVALID ? o != OBJ_NONE : q[e] >= n_refs) return fail(ctx, RAYN_ERR_INVALID_ARG, "a queue entry is a padding entry with an object, or a reference >= n_refs");
                if (o != OBJ_NONE) cnt[o]++;
            }
            size_t total = 0;
            for (uint32_t c = 0; c < nclass; c++) total += (cnt[c] + 3u) & ~3u;
            need_groups += (total + 63) / 64;
        }
    }
    if (out_slots < need_groups * 64) return fail(ctx, RAYN_ERR_INVALID_ARG, "out_slots is smaller than the binned queue the input needs");
    const KernelSet K = kernel_set(ctx->cfg->fma_policy);
    HIPCHK(hipSetDevice(ctx->device));
    const size_t BG = out_slots / 64 + 1, NT = n_tiles;
    uint32_t *d_q, *d_bq, *d_qn, *d_hist; QueueTables T; DCtl* ctl;
    ProbeArena arena;
    const auto carve = [&](Arena& A) {
        d_q = A.take<uint32_t>(n_entries); d_bq = A.take<uint32_t>(out_slots); d_qn = A.take<uint32_t>(out_slots);
        T = carve_queue_tables(A, groups + 1, BG, NT);
        d_hist = A.take<uint32_t>(NT); ctl = A.take<DCtl>(1);
    };
    HIPCHK(arena.alloc(carve));
    std::vector<uint32_t> tgb(n_tiles), fill(out_slots, sentinel);
    { uint32_t g = 0; for (uint32_t k = 0; k < n_tiles; k++) { tgb[k] = g; g += tile_groups[k]; } } // back to back, as k_batch_setup lays the tiles out
    DCtl hc;
    memset(&hc, 0, sizeof hc);
    hc.q_groups = (uint32_t)groups; hc.q_valid = (uint32_t)ctl_io[1]; hc.b_groups = (uint32_t)ctl_io[2]; hc.b_valid = (uint32_t)ctl_io[3]; hc.overflow = (uint32_t)ctl_io[4];
    hc.segments = ctl_io[5]; hc.shaded_slots = ctl_io[6]; hc.entries_sum = ctl_io[7]; hc.next_sum = ctl_io[8];
    hc.job_count = (uint32_t)ctl_io[9]; hc.head_shadow = (uint32_t)ctl_io[10]; hc.head_extend = (uint32_t)ctl_io[11];
    HIPCHK(hipMemset(arena.base, 0, arena.cap)); // the binned queue's tile group table, the per-tile tables and the base_hist row start as zero
    HIPCHK(hipMemcpy(d_q, q, n_entries * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(T.ent_obj, ent_obj, n_entries, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_bq, fill.data(), (size_t)out_slots * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(d_qn, fill.data(), (size_t)out_slots * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(T.ray_tgb, tgb.data(), NT * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(T.ray_tgc, tile_groups, NT * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ctl, &hc, sizeof hc, hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize()); // the fills above ran on the null stream
    hipStream_t s = ctx->stream;
    K.bin_stage(s, T, nclass, n_tiles, d_q, max_entries, d_bq, cap_groups_bin, d_hist, ctl);
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    std::vector<uint32_t> tmp(n_tiles);
    HIPCHK(hipMemcpy(&hc, ctl, sizeof hc, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_bq, d_bq, (size_t)out_slots * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_cls_cnt, T.tile_cls_cnt, NT * SCAN_NC_BIN * 4, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(out_cls_base, T.tile_cls_base, NT * SCAN_NC_BIN * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(tmp.data(), T.bin_tgb, NT * 4, hipMemcpyDeviceToHost)); for (uint32_t k = 0; k < n_tiles; k++) out_tile[5 * (size_t)k] = tmp[k];
    HIPCHK(hipMemcpy(tmp.data(), T.bin_tgc, NT * 4, hipMemcpyDeviceToHost)); for (uint32_t k = 0; k < n_tiles; k++) out_tile[5 * (size_t)k + 1] = tmp[k];
    HIPCHK(hipMemcpy(tmp.data(), d_hist, NT * 4, hipMemcpyDeviceToHost)); for (uint32_t k = 0; k < n_tiles; k++) out_tile[5 * (size_t)k + 4] = tmp[k];
    if ((size_t)hc.b_groups * 64 > out_slots) return fail(ctx, RAYN_ERR_HIP, "internal: the bin stage reports a binned queue larger than the input's full need");
    // what k_shade_setup would leave: one survivor ballot and one survivor count per binned group
    std::vector<unsigned long long> alive(BG, 0ull);
    std::vector<uint8_t> bcnt(BG, 0);
    for (uint32_t g = 0; g < hc.b_groups; g++) {
        unsigned long long m = 0;
        for (uint32_t j = 0; j < 64; j++) {
            const uint32_t r = out_bq[(size_t)g * 64 + j];
            if (r < n_refs && survive[r]) m |= 1ull << j; // INVALID (and an unwritten slot's sentinel) are dead
        }
        alive[g] = m; bcnt[g] = (uint8_t)__builtin_popcountll(m);
    }
    HIPCHK(hipMemcpy(T.alive, alive.data(), BG * 8, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(T.bgrp_cnt, bcnt.data(), BG, hipMemcpyHostToDevice));
    K.repack_stage(s, T, n_tiles, d_bq, max_slots, d_qn, cap_groups_repack, ctl);
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(&hc, ctl, sizeof hc, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_qn, d_qn, (size_t)out_slots * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(tmp.data(), T.ray_tgb, NT * 4, hipMemcpyDeviceToHost)); for (uint32_t k = 0; k < n_tiles; k++) out_tile[5 * (size_t)k + 2] = tmp[k];
    HIPCHK(hipMemcpy(tmp.data(), T.ray_tgc, NT * 4, hipMemcpyDeviceToHost)); for (uint32_t k = 0; k < n_tiles; k++) out_tile[5 * (size_t)k + 3] = tmp[k];
    const uint64_t fin[12] = {hc.q_groups, hc.q_valid, hc.b_groups, hc.b_valid, hc.overflow, hc.segments, hc.shaded_slots, hc.entries_sum, hc.next_sum,
                              hc.job_count, hc.head_shadow, hc.head_extend};
    memcpy(ctl_io, fin, sizeof fin);
    return RAYN_OK;
}
// the sizes that decide the grid-stride trips of the shade stage's streaming kernels (kernels.h)
int rayn_hip_probe_shade_limits(const rayn_ctx* ctx, uint32_t* stream_blocks, uint32_t* list_ids_per_block, uint32_t* setup_threads) {
    if (!ctx || !stream_blocks || !list_ids_per_block || !setup_threads) return RAYN_ERR_INVALID_ARG;
    *stream_blocks = STREAM_BLOCKS; *list_ids_per_block = 256 * SCAN_ITEMS; *setup_threads = SHADE_SETUP_THREADS;
    return RAYN_OK;
}
// The shade stage of ONE depth through launch_shade (k_shade_setup, k_shadow_list, the scene's shadow-march kernel, k_shade_finish) on a caller-built binned
// queue and pool; the pool and the NEE records come from the carve functions run_worker's arena is carved by (frame_layout.h).  The probe owns every device
// buffer: the pool, the NEE records, the survivor ballots and the control block; what the kernels must not read before they write it starts as the worst stale value (header: rayn_hip.h).
// Everything the kernels would index is checked here first, and so are their preconditions.
int rayn_hip_probe_shade(rayn_ctx* ctx, const rayn_frame_params* p, const float* samples_1d, const float* samples_2d, const float* scramble, const float* fis_table,
                         uint32_t depth, uint32_t n_slots, uint32_t max_slots, uint32_t nee_cap, const uint32_t* ref, uint32_t n_pool, const float* geo0,
                         const float* geo1, const float* col0, const float* col1, uint32_t sentinel, float* out_geo0, float* out_geo1, float* out_col0,
                         float* out_col1, float* out_aov, uint32_t* out_term_key, uint8_t* out_term_info, uint64_t* out_alive_mask, uint8_t* out_bgrp_cnt,
                         uint64_t* out_jobs) {
    int rc = validate(ctx, p);
    if (rc) return rc;
    if (!samples_1d || !samples_2d || !scramble || !fis_table || !ref || !geo0 || !geo1 || !col0 || !col1 || !out_geo0 || !out_geo1 || !out_col0 || !out_col1 ||
        !out_aov || !out_term_key || !out_term_info || !out_alive_mask || !out_bgrp_cnt || !out_jobs)
        return fail(ctx, RAYN_ERR_INVALID_ARG, "null buffer");
    if (n_slots == 0 || n_slots % 64) return fail(ctx, RAYN_ERR_INVALID_ARG, "n_slots is 0 or not a multiple of 64 (the kernels work on whole 64-slot groups)");
    if (max_slots < n_slots || nee_cap < n_slots) return fail(ctx, RAYN_ERR_INVALID_ARG, "max_slots or nee_cap below n_slots");
    if (depth > p->max_bounces) return fail(ctx, RAYN_ERR_INVALID_ARG, "depth above max_bounces (the packed sample records end there)");
    if (n_pool == 0 || n_pool > (1u << 27) || max_slots > (1u << 27)) return fail(ctx, RAYN_ERR_INVALID_ARG, "probe size out of range");
    const rayn_world_desc& w = ctx->cfg->world;
    const uint32_t NS = nee_samples(w.has_scattering, p->volume_marches);
    if (!queue_ids_fit(NS, nee_cap) || !queue_ids_fit(NS, max_slots)) // run_worker's check, on the probe's strides
        return fail(ctx, RAYN_ERR_INVALID_ARG, "ns * nee_cap or ns * max_slots does not fit the 32-bit [sample][slot] ids");
    const uint32_t spp = p->samples * 4;
    const uint64_t n_pixels = (uint64_t)p->width * p->height;
    {
        std::vector<uint8_t> named(n_pool, 0);
        for (uint32_t k = 0; k < n_slots; k += 4) {
            uint32_t obj0 = 0;
            bool any = false;
            for (uint32_t i = 0; i < 4; i++) {
                const uint32_t P = ref[k + i];
                if (P == INVALID) continue;
                if (P >= n_pool) return fail(ctx, RAYN_ERR_INVALID_ARG, "a ref that is neither 0xFFFFFFFF nor below n_pool");
                if (named[P]) return fail(ctx, RAYN_ERR_INVALID_ARG, "a pool slot is referenced twice");
                named[P] = 1;
                uint32_t ow, pix;
                memcpy(&ow, &geo1[4 * (size_t)P + 3], 4); memcpy(&pix, &col1[4 * (size_t)P + 2], 4);
                const uint32_t obj = ow & 0xFFu;
                if (obj >= w.n_hitables) return fail(ctx, RAYN_ERR_INVALID_ARG, "an object at or beyond n_hitables");
                if ((ow >> 8) >= spp) return fail(ctx, RAYN_ERR_INVALID_ARG, "a sample index at or beyond 4 * samples");
                if (pix >= n_pixels) return fail(ctx, RAYN_ERR_INVALID_ARG, "a pixel index at or beyond width * height");
                if (!any && i != 0) return fail(ctx, RAYN_ERR_INVALID_ARG, "lane 0 of a packet is invalid while a later lane is not (lane 0 of a bin packet is always a real hit)");
                if (any && obj != obj0) return fail(ctx, RAYN_ERR_INVALID_ARG, "the valid lanes of a packet name different objects");
                any = true; obj0 = obj;
            }
        }
    }
    HIPCHK(hipSetDevice(ctx->device));
    DScene hs;
    rc = build_scene(ctx, w, *p, &hs);
    if (rc) return rc;
    Tuning tun;
    const int single_sdf = scene_march_kernels(ctx, hs, *p, &tun);
    const KernelSet K = kernel_set(ctx->cfg->fma_policy);
    const size_t n1 = (size_t)spp * rayn_sets_1d(p->max_bounces, p->volume_marches), n2 = (size_t)spp * 2 * rayn_sets_2d(p->max_bounces, p->volume_marches);
    const RecordLayout rec(hs.n2, p->max_bounces);
    const size_t CAP = nee_cap, NV = NS - 4 + 1, G = n_slots / 64, NP = n_pool;
    float *d_s1, *d_s2, *d_scr, *d_fis; float4* d_rec; uint32_t* d_bq; Pool pool; Nee nee; unsigned long long *d_alive, *d_ev; uint8_t* d_cnt; DCtl* d_ctl;
    ProbeArena arena;
    const auto carve = [&](Arena& A) {
        d_s1 = A.take<float>(n1); d_s2 = A.take<float>(n2); d_scr = A.take<float>(n_pixels); d_fis = A.take<float>(RAYN_FIS_TABLE_SIZE);
        d_rec = A.take<float4>(rec.count(spp)); d_bq = A.take<uint32_t>(n_slots);
        pool = carve_pool(A, NP); nee = carve_nee(A, NS, CAP);
        d_alive = A.take<unsigned long long>(G); d_cnt = A.take<uint8_t>(G); d_ctl = A.take<DCtl>(1); d_ev = A.take<unsigned long long>(16);
    };
    if (arena.alloc(carve) != hipSuccess) { (void)hipGetLastError(); return fail(ctx, RAYN_ERR_OOM, "hipMalloc of the shade probe's buffers failed"); }
    // the float planes of the NEE records, in the order the guard below walks them
    const struct Plane { float* p; size_t planes; } fplanes[] = {{nee.x, 12}, {nee.vtr, NV}, {nee.pdf, NS}, {nee.aux, NV}, {nee.T, 1}, {nee.t0, 1}, {nee.nthr, 3}};
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpy(d_s1, samples_1d, n1 * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(d_s2, samples_2d, n2 * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_scr, scramble, n_pixels * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(d_fis, fis_table, RAYN_FIS_TABLE_SIZE * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_bq, ref, (size_t)n_slots * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(pool.geo0, geo0, NP * 16, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(pool.geo1, geo1, NP * 16, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(pool.col0, col0, NP * 16, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(pool.col1, col1, NP * 16, hipMemcpyHostToDevice));
    HIPCHK(hipMemsetD32((hipDeviceptr_t)pool.aov, (int)sentinel, NP * 4)); HIPCHK(hipMemsetD32((hipDeviceptr_t)pool.term_key, (int)sentinel, NP));
    HIPCHK(hipMemset(pool.term_info, (int)TERM_NONE, NP));
    for (const Plane& pl : fplanes) HIPCHK(hipMemsetD32((hipDeviceptr_t)pl.p, (int)sentinel, pl.planes * CAP));
    HIPCHK(hipMemset(nee.vis, 2, NS * CAP)); // "march pending" everywhere: a (sample, slot) the setup forgets becomes a job and an occluded sample
    HIPCHK(hipMemset(nee.vpicks, 0xFF, CAP * 8)); HIPCHK(hipMemset(nee.flags, 0xFF, CAP));
    HIPCHK(hipMemset(nee.job_ref, 0xFF, nee.jobcap * 4)); HIPCHK(hipMemset(nee.job_geo, 0, 3 * nee.jobcap * 8));
    HIPCHK(hipMemset(d_alive, 0xA5, G * 8)); HIPCHK(hipMemset(d_cnt, 0xA5, G)); HIPCHK(hipMemset(d_ev, 0, 128));
    DCtl hc;
    memset(&hc, 0, sizeof hc);
    hc.b_groups = (uint32_t)G;
    for (uint32_t k = 0; k < n_slots; k++) hc.b_valid += ref[k] != INVALID;
    HIPCHK(hipMemcpy(d_ctl, &hc, sizeof hc, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ctx->d_scene, &hs, sizeof hs, hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize()); // the fills above ran on the null stream
    const Tables tab{d_s1, d_s2, d_fis, d_rec, rec.stride};
    K.pack_tables(s, tab, d_rec, spp, rec.depths, hs.n1, hs.n2);
    const bool count = ctx->cfg->counting; // the instrumented instantiations; the context's counters then report this call
    K.shade(s, count, ctx->d_scene, tab, d_scr, depth, d_bq, max_slots, pool, nee, NS, hs.n_sdf > 0, single_sdf, d_alive, d_cnt, d_ctl, d_ev,
            ShadeHooks{nullptr, nullptr, nullptr}, tun);
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    if (count) { rc = probe_counters(ctx, d_ev); if (rc) return rc; }
    HIPCHK(hipMemcpy(&hc, d_ctl, sizeof hc, hipMemcpyDeviceToHost));
    if ((uint64_t)hc.job_count > (uint64_t)NS * n_slots) return fail(ctx, RAYN_ERR_HIP, "internal: job_count exceeds ns * n_slots");
    if (CAP > n_slots) { // the surplus of every NEE plane: no word at a slot index in [n_slots, nee_cap) may have changed
        const size_t extra = CAP - n_slots;
        std::vector<uint32_t> words(extra);
        std::vector<uint8_t> bytes(extra);
        for (const Plane& pl : fplanes)
            for (size_t k = 0; k < pl.planes; k++) {
                HIPCHK(hipMemcpy(words.data(), pl.p + k * CAP + n_slots, extra * 4, hipMemcpyDeviceToHost));
                for (uint32_t v : words) if (v != sentinel) return fail(ctx, RAYN_ERR_HIP, "internal: a float plane of the NEE records was written at a slot index in [n_slots, nee_cap)");
            }
        for (size_t k = 0; k < NS; k++) {
            HIPCHK(hipMemcpy(bytes.data(), nee.vis + k * CAP + n_slots, extra, hipMemcpyDeviceToHost));
            for (uint8_t v : bytes) if (v != 2) return fail(ctx, RAYN_ERR_HIP, "internal: the visibility plane was written at a slot index in [n_slots, nee_cap)");
        }
        HIPCHK(hipMemcpy(bytes.data(), nee.flags + n_slots, extra, hipMemcpyDeviceToHost));
        for (uint8_t v : bytes) if (v != 0xFF) return fail(ctx, RAYN_ERR_HIP, "internal: the flag plane was written at a slot index in [n_slots, nee_cap)");
        std::vector<unsigned long long> picks(extra);
        HIPCHK(hipMemcpy(picks.data(), nee.vpicks + n_slots, extra * 8, hipMemcpyDeviceToHost));
        for (unsigned long long v : picks) if (v != ~0ull) return fail(ctx, RAYN_ERR_HIP, "internal: the volume picks were written at a slot index in [n_slots, nee_cap)");
    }
    if ((rc = probe_pool_out(ctx, pool, NP, out_geo0, out_geo1, out_col0, out_col1, out_aov, out_term_key, out_term_info))) return rc;
    HIPCHK(hipMemcpy(out_alive_mask, d_alive, G * 8, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(out_bgrp_cnt, d_cnt, G, hipMemcpyDeviceToHost));
    out_jobs[0] = hc.job_count; out_jobs[1] = hc.shadow_jobs;
    // the shadow-march kernel launch_shadow_march launched, by the decision it shares with this probe (kernels.h); 0: launch_shade skips the march without a TracedSDF
    out_jobs[2] = hs.n_sdf == 0 ? 0 : (uint64_t)shadow_march_kernel(single_sdf, tun);
    return RAYN_OK;
}
// The film resolve on caller-built tiles and termination records, through launch_resolve (so the variant is the product's choice for spp).  The resolve
// reads spp and width of the scene and term_info / term_key / col0 / aov of the pool; everything else of both stays zero / null.  The four planes start
// filled with `sentinel`.  Everything the kernels would index is checked here first, and so are their preconditions (rayn_hip.h lists them).
int rayn_hip_probe_resolve(rayn_ctx* ctx, uint32_t width, uint32_t spp, uint32_t n_tiles, const uint32_t* tiles, uint32_t max_tile_pixels, uint32_t n_paths,
                           const uint8_t* term_info, const uint32_t* term_key, const float* col0_rgb, const float* aov_xyz, const uint32_t* aov_obj,
                           const uint32_t* base_hist, uint32_t hist_stride, uint32_t n_depths, uint32_t sentinel, uint32_t out_pixels, float* out_color,
                           float* out_alpha, float* out_background, float* out_normal) {
    if (!ctx) return RAYN_ERR_INVALID_ARG;
    if (!tiles || !term_info || !term_key || !col0_rgb || !aov_xyz || !aov_obj || !out_color || !out_alpha || !out_background || !out_normal)
        return fail(ctx, RAYN_ERR_INVALID_ARG, "null buffer");
    if (spp < 4 || spp > 16384 || spp % 4) return fail(ctx, RAYN_ERR_INVALID_ARG, "spp is not a multiple of 4 in 4..16384");
    if (n_tiles == 0 || n_tiles > 65535) return fail(ctx, RAYN_ERR_INVALID_ARG, "n_tiles outside 1..65535 (the grid's y size)");
    if (max_tile_pixels == 0 || max_tile_pixels > (1u << 16)) return fail(ctx, RAYN_ERR_INVALID_ARG, "max_tile_pixels outside 1..2^16");
    if (n_paths == 0 || n_paths > (1u << 27) || out_pixels == 0 || out_pixels > (1u << 24) || width == 0) return fail(ctx, RAYN_ERR_INVALID_ARG, "probe size out of range");
    const bool blk = spp > 512 && spp <= MAX_SPP_RESOLVE_BLK; // k_resolve_blk: the only variant that reads base_hist
    if (blk && (!base_hist || hist_stride < n_tiles || n_depths == 0 || n_depths > MAX_BOUNCES + 1))
        return fail(ctx, RAYN_ERR_INVALID_ARG, "512 < spp <= 4096 needs base_hist[n_depths][hist_stride] with hist_stride >= n_tiles and n_depths in 1..121");
    std::vector<DTile> ht(n_tiles);
    std::vector<uint8_t> owned(out_pixels, 0);
    std::vector<unsigned long long> keys(spp);
    for (uint32_t t = 0; t < n_tiles; t++) {
        const uint32_t* w = tiles + 8 * (size_t)t;
        DTile& T = ht[t];
        T.x0 = w[0]; T.y0 = w[1]; T.ew = w[2]; T.eh = w[3]; T.pool_base = w[4]; T.n_paths = w[5]; T.film_base = w[6]; T.film_packed = w[7];
        const uint64_t npx = (uint64_t)T.ew * T.eh;
        if (npx == 0 || npx > MAX_TILE_PIXELS || npx > max_tile_pixels) return fail(ctx, RAYN_ERR_INVALID_ARG, "a tile has no pixel, more than 1024 pixels or more than max_tile_pixels");
        if ((uint64_t)T.pool_base + npx * spp > n_paths) return fail(ctx, RAYN_ERR_INVALID_ARG, "a tile's paths end beyond the path arrays");
        for (uint32_t lpix = 0; lpix < (uint32_t)npx; lpix++) {
            const uint64_t fi = T.film_packed ? (uint64_t)T.film_base + lpix : (uint64_t)T.x0 + lpix / T.eh + ((uint64_t)T.y0 + lpix % T.eh) * width;
            if (fi >= out_pixels) return fail(ctx, RAYN_ERR_INVALID_ARG, "a film index at or beyond out_pixels");
            if (owned[fi]) return fail(ctx, RAYN_ERR_INVALID_ARG, "two tile pixels share a film index");
            owned[fi] = 1;
            const size_t P0 = (size_t)T.pool_base + (size_t)lpix * spp;
            uint32_t nk = 0;
            for (uint32_t i = 0; i < spp; i++) {
                const uint32_t ob = aov_obj[P0 + i], info = term_info[P0 + i];
                if (ob > OBJ_NONE) return fail(ctx, RAYN_ERR_INVALID_ARG, "an object word is neither below 0xFF nor OBJ_NONE");
                if (info == TERM_NONE) continue;
                const uint32_t d = info & 0x7Fu, slot = term_key[P0 + i];
                if (d > MAX_BOUNCES) return fail(ctx, RAYN_ERR_INVALID_ARG, "a contributing sample is deeper than max_bounces can be (120)");
                if (blk) {
                    if (d >= n_depths) return fail(ctx, RAYN_ERR_INVALID_ARG, "a depth at or beyond n_depths");
                    const uint32_t base = base_hist[(size_t)d * hist_stride + t];
                    if (slot < base || slot - base >= (1u << RESOLVE_KEY_SHIFT)) return fail(ctx, RAYN_ERR_INVALID_ARG, "a slot below its base_hist entry, or 2^25 or more above it");
                }
                keys[nk++] = ((unsigned long long)d << 32) | slot;
            }
            std::sort(keys.begin(), keys.begin() + nk);
            if (std::adjacent_find(keys.begin(), keys.begin() + nk) != keys.begin() + nk)
                return fail(ctx, RAYN_ERR_INVALID_ARG, "two contributing samples of one pixel have equal (depth, slot)");
        }
    }
    const KernelSet K = kernel_set(ctx->cfg->fma_policy);
    HIPCHK(hipSetDevice(ctx->device));
    DScene hs;
    memset(&hs, 0, sizeof hs);
    hs.spp = spp; hs.width = width;
    HIPCHK(hipMemcpy(ctx->d_scene, &hs, sizeof hs, hipMemcpyHostToDevice));
    std::vector<float4> c0(n_paths), av(n_paths);
    for (size_t i = 0; i < n_paths; i++) {
        float obf; memcpy(&obf, &aov_obj[i], 4);
        c0[i] = make_float4(col0_rgb[3 * i], col0_rgb[3 * i + 1], col0_rgb[3 * i + 2], 0.0f);
        av[i] = make_float4(aov_xyz[3 * i], aov_xyz[3 * i + 1], aov_xyz[3 * i + 2], obf);
    }
    const size_t NP = out_pixels, hist_words = blk ? (size_t)n_depths * hist_stride : 0;
    DevBuf d_tiles, d_info, d_key, d_c0, d_av, d_hist, d_out;
    HIPCHK(d_tiles.alloc((size_t)n_tiles * sizeof(DTile))); HIPCHK(d_info.alloc(n_paths)); HIPCHK(d_key.alloc((size_t)n_paths * 4));
    HIPCHK(d_c0.alloc((size_t)n_paths * 16)); HIPCHK(d_av.alloc((size_t)n_paths * 16)); HIPCHK(d_hist.alloc(hist_words * 4)); HIPCHK(d_out.alloc(NP * 40));
    std::vector<uint32_t> fill(NP * 10, sentinel);
    HIPCHK(hipMemcpy(d_tiles.p, ht.data(), (size_t)n_tiles * sizeof(DTile), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_info.p, term_info, n_paths, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(d_key.p, term_key, (size_t)n_paths * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_c0.p, c0.data(), (size_t)n_paths * 16, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(d_av.p, av.data(), (size_t)n_paths * 16, hipMemcpyHostToDevice));
    if (hist_words) HIPCHK(hipMemcpy(d_hist.p, base_hist, hist_words * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_out.p, fill.data(), NP * 40, hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize()); // the uploads above ran on the null stream
    Pool pool;
    memset(&pool, 0, sizeof pool);
    pool.col0 = d_c0.as<float4>(); pool.aov = d_av.as<float4>(); pool.term_key = d_key.as<uint32_t>(); pool.term_info = d_info.as<uint8_t>();
    float *o_color = d_out.as<float>(), *o_alpha = o_color + 3 * NP, *o_bg = o_alpha + NP, *o_normal = o_bg + 3 * NP;
    K.resolve(ctx->stream, ctx->d_scene, d_tiles.as<DTile>(), n_tiles, max_tile_pixels, spp, pool, o_color, o_alpha, o_bg, o_normal, d_hist.as<uint32_t>(), hist_stride);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out_color, o_color, NP * 12, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(out_alpha, o_alpha, NP * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_background, o_bg, NP * 12, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(out_normal, o_normal, NP * 12, hipMemcpyDeviceToHost));
    return RAYN_OK;
}

// The ray-generation stage (k_pack_tables, k_batch_setup, k_raygen) through the product launchers, with the pool and the record geometry of frame_layout.h, on
// caller-built tables and a caller-built tile list.  The probe owns every device buffer; every output buffer starts filled with `sentinel` (term_info with its low byte)
// and is `surplus` slots longer than the pool (the group tables surplus / 64 words, the tile tables 2 words, the records 64 floats), so a write beyond the
// pool, into a padding slot or into term_key shows.  Everything the kernels would index is checked here first (rayn_hip.h lists it).
int rayn_hip_probe_raygen(rayn_ctx* ctx, const rayn_frame_params* p, const float* samples_1d, uint64_t n_samples_1d, const float* samples_2d, uint64_t n_samples_2d,
                          const float* scramble, uint64_t n_scramble, const float* fis_table, uint32_t n_tiles, const uint32_t* tiles, uint32_t n_pool,
                          uint32_t surplus, uint32_t sentinel, float* out_geo0, float* out_geo1, float* out_col0, float* out_col1, float* out_aov,
                          uint32_t* out_term_key, uint8_t* out_term_info, uint32_t* out_q, uint32_t* out_pgrp_tile, uint32_t* out_tgb, uint32_t* out_tgc,
                          uint32_t* out_ctl, float* out_records) {
    int rc = validate(ctx, p);
    if (rc) return rc;
    if (!samples_1d || !samples_2d || !scramble || !fis_table || !tiles || !out_geo0 || !out_geo1 || !out_col0 || !out_col1 || !out_aov || !out_term_key ||
        !out_term_info || !out_q || !out_pgrp_tile || !out_tgb || !out_tgc || !out_ctl || !out_records)
        return fail(ctx, RAYN_ERR_INVALID_ARG, "null buffer");
    const uint32_t spp = p->samples * 4; // validate: samples in 1..4096, so spp is a multiple of 4 in 4..16384
    const uint64_t n_pixels = (uint64_t)p->width * p->height;
    const size_t n1 = (size_t)spp * rayn_sets_1d(p->max_bounces, p->volume_marches), n2 = (size_t)spp * 2 * rayn_sets_2d(p->max_bounces, p->volume_marches);
    if (n_samples_1d != n1 || n_samples_2d != n2) return fail(ctx, RAYN_ERR_INVALID_ARG, "a sample table is not sized by rayn_sets_1d / rayn_sets_2d for the frame's bounces and volume marches");
    if (n_scramble != n_pixels) return fail(ctx, RAYN_ERR_INVALID_ARG, "the scramble does not hold width * height entries");
    if (n_tiles == 0 || n_tiles > (1u << 20)) return fail(ctx, RAYN_ERR_INVALID_ARG, "n_tiles outside 1..2^20");
    if (n_pool == 0 || n_pool % 64 || n_pool > (1u << 27)) return fail(ctx, RAYN_ERR_INVALID_ARG, "n_pool is 0, not a multiple of 64 or above 2^27");
    if (surplus < 128 || surplus % 64 || surplus > (1u << 20)) return fail(ctx, RAYN_ERR_INVALID_ARG, "surplus is not a multiple of 64 in 128..2^20");
    if (sentinel == INVALID || sentinel < n_pool || (sentinel & 0xFFu) == TERM_NONE)
        return fail(ctx, RAYN_ERR_INVALID_ARG, "the sentinel must be neither INVALID nor a pool index, and its low byte not TERM_NONE");
    std::vector<DTile> ht(n_tiles);
    {
        std::vector<uint8_t> owned(n_pool / 64, 0);
        size_t covered = 0;
        for (uint32_t t = 0; t < n_tiles; t++) {
            const uint32_t* w = tiles + 8 * (size_t)t;
            DTile& T = ht[t];
            T.x0 = w[0]; T.y0 = w[1]; T.ew = w[2]; T.eh = w[3]; T.pool_base = w[4]; T.n_paths = w[5]; T.film_base = w[6]; T.film_packed = w[7];
            const uint64_t npx = (uint64_t)T.ew * T.eh;
            if (npx == 0 || npx > MAX_TILE_PIXELS) return fail(ctx, RAYN_ERR_INVALID_ARG, "a tile has no pixel or more than 1024 pixels");
            if ((uint64_t)T.x0 + T.ew > p->width || (uint64_t)T.y0 + T.eh > p->height) return fail(ctx, RAYN_ERR_INVALID_ARG, "a tile does not lie inside width x height");
            if (T.n_paths != npx * spp) return fail(ctx, RAYN_ERR_INVALID_ARG, "a tile's n_paths is not ew * eh * spp");
            if (T.pool_base % 64) return fail(ctx, RAYN_ERR_INVALID_ARG, "a tile's pool_base is not a multiple of 64");
            const uint64_t g0 = T.pool_base / 64, groups = ((uint64_t)T.n_paths + 63) / 64;
            if (g0 + groups > n_pool / 64) return fail(ctx, RAYN_ERR_INVALID_ARG, "a tile's 64-padded segment ends beyond n_pool");
            for (uint64_t g = g0; g < g0 + groups; g++) {
                if (owned[g]) return fail(ctx, RAYN_ERR_INVALID_ARG, "the 64-padded segments of two tiles overlap");
                owned[g] = 1;
            }
            covered += groups;
        }
        if (covered != n_pool / 64) return fail(ctx, RAYN_ERR_INVALID_ARG, "the tiles' 64-padded segments do not cover [0, n_pool): k_raygen would read an unwritten pgrp_tile word");
    }
    HIPCHK(hipSetDevice(ctx->device));
    DScene hs;
    rc = build_scene(ctx, ctx->cfg->world, *p, &hs);
    if (rc) return rc;
    const KernelSet K = kernel_set(ctx->cfg->fma_policy);
    const RecordLayout rec(hs.n2, p->max_bounces);
    const size_t rec_words = rec.count(spp) * 4 + 64, NP = (size_t)n_pool + surplus, NG = NP / 64, NT = (size_t)n_tiles + 2;
    float *d_s1, *d_s2, *d_scr, *d_fis, *d_rec; DTile* d_tiles; Pool pool; uint32_t *d_q, *d_pgrp, *d_tgb, *d_tgc; DCtl* d_ctl;
    ProbeArena arena;
    const auto carve = [&](Arena& A) {
        d_s1 = A.take<float>(n1); d_s2 = A.take<float>(n2); d_scr = A.take<float>(n_pixels); d_fis = A.take<float>(RAYN_FIS_TABLE_SIZE);
        d_rec = A.take<float>(rec_words); d_tiles = A.take<DTile>(n_tiles); pool = carve_pool(A, NP);
        d_q = A.take<uint32_t>(NP); d_pgrp = A.take<uint32_t>(NG); d_tgb = A.take<uint32_t>(NT); d_tgc = A.take<uint32_t>(NT); d_ctl = A.take<DCtl>(1);
    };
    if (arena.alloc(carve) != hipSuccess) { (void)hipGetLastError(); return fail(ctx, RAYN_ERR_OOM, "hipMalloc of the ray-gen probe's buffers failed"); }
    HIPCHK(hipMemcpy(d_s1, samples_1d, n1 * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(d_s2, samples_2d, n2 * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_scr, scramble, n_pixels * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(d_fis, fis_table, RAYN_FIS_TABLE_SIZE * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_tiles, ht.data(), (size_t)n_tiles * sizeof(DTile), hipMemcpyHostToDevice));
    const struct Fill { void* p; size_t words; } fills[] = {{d_rec, rec_words}, {pool.geo0, NP * 4}, {pool.geo1, NP * 4}, {pool.col0, NP * 4}, {pool.col1, NP * 4},
                                                            {pool.aov, NP * 4}, {pool.term_key, NP}, {d_q, NP}, {d_pgrp, NG}, {d_tgb, NT}, {d_tgc, NT}, {d_ctl, sizeof(DCtl) / 4}};
    for (const Fill& f : fills) HIPCHK(hipMemsetD32((hipDeviceptr_t)f.p, (int)sentinel, f.words));
    HIPCHK(hipMemset(pool.term_info, (int)(sentinel & 0xFFu), NP));
    HIPCHK(hipMemcpy(ctx->d_scene, &hs, sizeof hs, hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize()); // the fills above ran on the null stream
    hipStream_t s = ctx->stream;
    const Tables tab{d_s1, d_s2, d_fis, (float4*)d_rec, rec.stride};
    K.pack_tables(s, tab, (float4*)d_rec, spp, rec.depths, hs.n1, hs.n2);
    K.batch_setup(s, d_tiles, n_tiles, d_pgrp, d_tgb, d_tgc);
    K.raygen(s, ctx->d_scene, tab, d_scr, d_tiles, d_pgrp, pool, d_q, n_pool, d_ctl);
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    if ((rc = probe_pool_out(ctx, pool, NP, out_geo0, out_geo1, out_col0, out_col1, out_aov, out_term_key, out_term_info))) return rc;
    HIPCHK(hipMemcpy(out_q, d_q, NP * 4, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(out_pgrp_tile, d_pgrp, NG * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_tgb, d_tgb, NT * 4, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(out_tgc, d_tgc, NT * 4, hipMemcpyDeviceToHost));
    static_assert(sizeof(DCtl) >= 32, "the eight 32-bit words of DCtl");
    HIPCHK(hipMemcpy(out_ctl, d_ctl, 32, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_records, d_rec, rec_words * 4, hipMemcpyDeviceToHost));
    return RAYN_OK;
}

// huffman_code<286> / huffman_code<30> (png_device.h) on n_sets count sets of n_symbols words each
int rayn_hip_probe_huffman(rayn_ctx* ctx, uint32_t n_symbols, uint32_t n_sets, const uint32_t* counts, uint32_t* out_clen, uint32_t* out_tab) {
    if (!ctx) return RAYN_ERR_INVALID_ARG;
    if (n_symbols != PNG_NSYM && n_symbols != PNG_NDIST) return fail(ctx, RAYN_ERR_INVALID_ARG, "n_symbols must be 286 or 30");
    if (n_sets == 0 || n_sets > (1u << 16)) return fail(ctx, RAYN_ERR_INVALID_ARG, "probe size out of range");
    if (!counts || !out_clen || !out_tab) return fail(ctx, RAYN_ERR_INVALID_ARG, "null buffer");
    const size_t words = (size_t)n_sets * n_symbols;
    for (uint32_t k = 0; k < n_sets; k++) {
        uint64_t sum = 0;
        for (uint32_t s = 0; s < n_symbols; s++) sum += counts[(size_t)k * n_symbols + s];
        if (sum >> 32) return fail(ctx, RAYN_ERR_INVALID_ARG, "a count set sums to 2^32 or more (32-bit node weights)");
    }
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf d_in, d_clen, d_tab;
    HIPCHK(d_in.alloc(words * 4)); HIPCHK(d_clen.alloc(words * 4)); HIPCHK(d_tab.alloc(words * 4));
    HIPCHK(hipMemcpy(d_in.p, counts, words * 4, hipMemcpyHostToDevice));
    if (n_symbols == PNG_NSYM) k_probe_huffman<PNG_NSYM><<<n_sets, PNG_BT, 0, ctx->stream>>>(d_in.as<uint32_t>(), d_clen.as<uint32_t>(), d_tab.as<uint32_t>());
    else k_probe_huffman<PNG_NDIST><<<n_sets, PNG_BT, 0, ctx->stream>>>(d_in.as<uint32_t>(), d_clen.as<uint32_t>(), d_tab.as<uint32_t>());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out_clen, d_clen.p, words * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_tab, d_tab.p, words * 4, hipMemcpyDeviceToHost));
    return RAYN_OK;
}

// ---- the two halves of the JPEG encoder (jpeg.hip) alone.  Both own their device buffers, with PROBE_GUARD bytes of the fill's complement behind each
// buffer a kernel writes, looked at after the run.
constexpr size_t PROBE_GUARD = 64;
constexpr uint32_t PROBE_JPEG_BLOCKS = 1u << 20; // the probes' own size limit
static int probe_guard_intact(rayn_ctx* ctx, const void* d_buf, size_t bytes, uint8_t guard, const char* what) {
    uint8_t h[PROBE_GUARD];
    HIPCHK(hipMemcpy(h, (const uint8_t*)d_buf + bytes, PROBE_GUARD, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < PROBE_GUARD; k++)
        if (h[k] != guard) return fail(ctx, RAYN_ERR_HIP, std::string("a kernel wrote behind ") + what);
    return RAYN_OK;
}

// k_jpeg_transform alone: the image -> out_coef[blocks][64], int16, zigzag, the blocks in the order of the scan
int rayn_hip_probe_jpeg_transform(rayn_ctx* ctx, uint32_t w, uint32_t h, uint32_t bpp, uint32_t quality, uint32_t subsampling, const uint8_t* img, int16_t* out_coef) {
    if (!ctx) return RAYN_ERR_INVALID_ARG;
    const JpegGeometry g = jpeg_geometry(w, h, bpp, subsampling, 65535u); // the transform does not look at the restart interval
    if (!g.ok) return fail(ctx, RAYN_ERR_INVALID_ARG, g.why);
    if (quality < 1u || quality > 100u) return fail(ctx, RAYN_ERR_INVALID_ARG, "quality must be in 1..100");
    if (g.blocks > PROBE_JPEG_BLOCKS) return fail(ctx, RAYN_ERR_INVALID_ARG, "probe size out of range");
    if (!img || !out_coef) return fail(ctx, RAYN_ERR_INVALID_ARG, "null buffer");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t img_bytes = (size_t)w * h * bpp, coef_bytes = (size_t)g.blocks * 128u;
    DevBuf d_img, d_coef;
    HIPCHK(d_img.alloc(img_bytes)); HIPCHK(d_coef.alloc(coef_bytes + PROBE_GUARD));
    HIPCHK(hipMemcpy(d_img.p, img, img_bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_coef.p, 0xA5, coef_bytes)); HIPCHK(hipMemset(d_coef.as<uint8_t>() + coef_bytes, 0x5A, PROBE_GUARD));
    HIPCHK(hipDeviceSynchronize()); // the fills above ran on the null stream
    launch_jpeg_transform(ctx->stream, g, quality, d_img.as<uint8_t>(), d_coef.p);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    if (int rc = probe_guard_intact(ctx, d_coef.p, coef_bytes, 0x5A, "the coefficients")) return rc;
    HIPCHK(hipMemcpy(out_coef, d_coef.p, coef_bytes, hipMemcpyDeviceToHost));
    return RAYN_OK;
}

// k_jpeg_segment, k_jpeg_layout and k_jpeg_compact on caller coefficients: coef[blocks][64] as the transform leaves them -> the first
// rayn_jpeg_scan_bound bytes of d_out (header words, scan, and fill_byte where nothing was written).  The whole scratch and the output
// hold fill_byte when the kernels start.  Rejected on the host: a DC outside [-1024, 1023] or an |AC| above 1023 - the reach of the 13-bit
// transform at Q = 1 (|F| < 2^25, so |m| <= 1024 and only a DC of -1024 is met).  Inside it a DC difference stays within +-2047, category
// 11, and an AC within size 10, the last symbols the Annex K tables have: beyond it walk_block would index past d_tables.dc or read the 0
// of a symbol that has no code, and the scan bound would no longer hold.
int rayn_hip_probe_jpeg_entropy(rayn_ctx* ctx, uint32_t w, uint32_t h, uint32_t bpp, uint32_t subsampling, uint32_t restart_interval, const int16_t* coef,
                                uint32_t fill_byte, uint8_t* out, size_t out_bytes) {
    if (!ctx) return RAYN_ERR_INVALID_ARG;
    const JpegGeometry g = jpeg_geometry(w, h, bpp, subsampling, restart_interval);
    if (!g.ok) return fail(ctx, RAYN_ERR_INVALID_ARG, g.why);
    if (g.blocks > PROBE_JPEG_BLOCKS) return fail(ctx, RAYN_ERR_INVALID_ARG, "probe size out of range");
    if (fill_byte > 255u) return fail(ctx, RAYN_ERR_INVALID_ARG, "fill_byte must be in 0..255");
    if (!coef || !out) return fail(ctx, RAYN_ERR_INVALID_ARG, "null buffer");
    if (out_bytes < g.bound) return fail(ctx, RAYN_ERR_INVALID_ARG, "out smaller than rayn_jpeg_scan_bound");
    for (size_t k = 0; k < (size_t)g.blocks * 64u; k++) {
        const int v = coef[k];
        if ((k & 63u) == 0u ? (v < -1024 || v > 1023) : (v < -1023 || v > 1023))
            return fail(ctx, RAYN_ERR_INVALID_ARG, "a coefficient the encoder cannot produce (DC in -1024..1023, |AC| <= 1023)");
    }
    HIPCHK(hipSetDevice(ctx->device));
    const uint8_t guard = (uint8_t)~fill_byte;
    DevBuf d_out, d_scr;
    HIPCHK(d_out.alloc(g.bound + PROBE_GUARD)); HIPCHK(d_scr.alloc(g.scratch_bytes + PROBE_GUARD));
    HIPCHK(hipMemset(d_out.p, (int)fill_byte, g.bound)); HIPCHK(hipMemset(d_out.as<uint8_t>() + g.bound, guard, PROBE_GUARD));
    HIPCHK(hipMemset(d_scr.p, (int)fill_byte, g.scratch_bytes)); HIPCHK(hipMemset(d_scr.as<uint8_t>() + g.scratch_bytes, guard, PROBE_GUARD));
    HIPCHK(hipMemcpy(d_scr.p, coef, (size_t)g.blocks * 128u, hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize()); // the fills above ran on the null stream
    launch_jpeg_entropy(ctx->stream, g, d_out.p, d_scr.p);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    if (int rc = probe_guard_intact(ctx, d_out.p, g.bound, guard, "the output")) return rc;
    if (int rc = probe_guard_intact(ctx, d_scr.p, g.scratch_bytes, guard, "the scratch")) return rc;
    HIPCHK(hipMemcpy(out, d_out.p, g.bound, hipMemcpyDeviceToHost));
    return RAYN_OK;
}

} // extern "C"
