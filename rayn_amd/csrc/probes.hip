// probes.hip — the test probes of the C ABI (rayn_hip_probe_*): per-lane device primitives and the PRODUCT march kernels on caller data.
// Test infrastructure; defines no kernels (kernels.hip holds the probe kernels).
#include <hip/hip_runtime.h>
#include <string.h>

#include <string>
#include <vector>

#include "driver.h"

using namespace rayn;

namespace {
struct DevBuf { // hipMalloc'ed scratch of a probe call, released on every exit path
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 4); }
    template <typename T> T* as() const { return (T*)p; }
};
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
    K.extend(ctx->stream, false, ctx->d_scene, depth, d_q.as<uint32_t>(), npad, pool, d_obj.as<uint8_t>(), single_sdf, d_ctl.as<DCtl>(), d_ev.as<unsigned long long>(), tun);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
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
    K.shadow_march(ctx->stream, false, ctx->d_scene, nee, n, single_sdf, d_ctl.as<DCtl>(), d_ev.as<unsigned long long>(), tun);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    std::vector<uint8_t> vis(n);
    HIPCHK(hipMemcpy(vis.data(), d_vis.p, n, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++) out[i] = vis[i] == 1 ? 1.0f : 0.0f;
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

} // extern "C"
