// preview.hip — the preview integrator (rayn_hip_preview_device): primary hit, viewer-facing normal and ambient occlusion, an image of the
// geometry alone for look-dev, camera placement and as an AO AOV.  An extension: rayn has one integrator, the path tracer.  It runs beside
// the film path and touches none of its kernels: the primary hit is the G-buffer pass (temporal.hip), the occlusion of the TracedSDFs goes
// through the scene's PRODUCT shadow-march kernel (k_shadow1 / k_shadow_bulb / k_shadow, launch_shadow_march) on a job list this file builds.
//
// Definition (include/rayn_hip.h has the same text; tests/preview_np.py restates it in numpy and the tests compare bit for bit).  All
// arithmetic f32 under the context's mul_add policy where the film's own functions honour it (dot, mag_sq, cross, concentric_circle_map,
// the fold's box step: device_core.h); everything written out below as a product and a sum is a separate multiply and add.  For pixel
// p = x + y * width, bottom-up rows:
//   1. Primary hit: the G-buffer pass - same ray (direction d), same product extend kernel at depth 0, same record (P, t) and object index;
//      records and objects are bit for bit those of rayn_hip_gbuffer_device for the same p.  Every closure time is p->time_start (ts).
//   2. Background: a miss, or a hit object whose material kind is Sky: colour (0, 0, 0), alpha 0, normal (0, 0, 0), ao 1.  Every other pixel
//      is a surface, alpha 1.
//   3. Surface normal at depth 0 as k_shade_setup takes it, with h the hit object: a Sphere has n = normalized(P - sphere_center(h, ts)) and
//      offset = 0; a TracedSDF has hps = max(0.0001f, detail_scale * thr_at(make_thr(scene, 0), t)), n = sdf_normal(h, P - sphere_center(h, ts),
//      hps, ...) - four sdf_dist evaluations with the MandelBox scale taken at ts - and offset = hps.
//   4. Viewer side: wo = -d, nf = n * signum(dot(n, wo)).
//   5. AO rays, k = 0..K-1 (K = samples, 1..64): u = dm_fractf(s[k].x + r_p), v = dm_fractf(s[k].y + r_p) with s the caller's table of K
//      float pairs and r_p the pixel's entry of the caller's scramble table (0 without one); l = cosine_weighted_in_hemisphere(u, v);
//      w = basis.c0 * l.x + basis.c1 * l.y + basis.c2 * l.z with basis = orthonormal_basis(nf); a = P + nf * offset, b = a + w * radius;
//      vis_k = HitableStore::test_occluded(a, b): the analytic spheres in index order by sphere_occluded_dir (here), the TracedSDFs by the
//      product shadow-march kernel.  A segment a sphere occludes parks no job; a scene without a TracedSDF launches no march.
//   6. Resolve: ao = (float)(number of k with vis_k == 1) / (float)K; hl = ambient + (1.0f - ambient) * max(0.0f, dot(nf, wo));
//      colour = ao * hl in all three channels.  The normal output is nf.
//
// Kernels.  k_preview_jobs, one thread per pixel, built once per mul_add policy: the normal (first round only; later rounds read it back
// from the normal output), the sphere tests, and the surviving segments parked in the layout the shadow kernels read (Nee: 24-byte
// segments at [sample][slot], a pending mark in vis, the slot's packet time in t0).  The job references are written directly, dense: a
// wave scans its lanes' pending counts with shuffles and takes its range with ONE atomic on DCtl::job_count - k_shadow_list would scan
// every visibility byte again for a list this kernel already knows.  k_preview_resolve (policy-free) counts a round's visible bytes per
// pixel and, after the last round, writes colour, alpha and ao.
// Rounds.  The job store is 29 bytes per AO ray and pixel, 1.7 GB for 64 rays at 1280x720, so the rays go in rounds of PREVIEW_ROUND = 8:
// park 8, march, count, repeat; the visible count is an integer, so the split changes nothing.  8 is the largest count the tests and the
// shipped look-dev use in one go, and 214 MB at 1280x720.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "device_core.h"
#include "post_checks.h"
#include "preview.h"

namespace RAYN_KNS {

#include "march_queue.h" // store_job: the segment layout the shadow kernels read

// One thread per padded pixel slot, whole waves.  k0 == 0 is the first round.
__global__ void __launch_bounds__(256) k_preview_jobs(const DScene* __restrict__ scp, uint32_t n, uint32_t npad, uint32_t k0, uint32_t kn, float radius,
                                                       float ambient, const float2* __restrict__ samples, const float* __restrict__ scramble,
                                                       const float4* __restrict__ geo0, const float4* __restrict__ geo1,
                                                       const float4* __restrict__ records, const uint32_t* __restrict__ object,
                                                       float* __restrict__ out_normal, float* __restrict__ hl, uint32_t* __restrict__ count,
                                                       float* __restrict__ t0s, uint8_t* __restrict__ vis, uint32_t* __restrict__ job_ref,
                                                       float2* __restrict__ job_geo, DCtl* __restrict__ ctl) {
    // the slot index as an ordinary value that no out-of-line call (bulb_logf inside sdf_normal) touches: see k_shade_setup on threadIdx.x in v0
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    asm volatile("" : "+v"(i));
    if (i >= npad) return; // npad % 64 == 0: whole waves
    const DScene& sc = *scp;
    const uint32_t lane = i & 63u;
    const bool first = k0 == 0;
    const float ts = sc.time_start;
    const uint32_t obj = i < n ? object[i] : INVALID;
    const DHitable& h = sc.h[obj < sc.n_hitables ? obj : 0u];
    const bool surface = obj < sc.n_hitables && sc.m[h.material].kind != RAYN_MAT_SKY;
    f3 P = f3{0, 0, 0}, nf = f3{0, 0, 0};
    float offset = 0.0f;
    if (surface) {
        const float4 rec = records[i], g0 = geo0[i], g1 = geo1[i];
        P = f3{rec.x, rec.y, rec.z};
        const f3 wo = -f3{g0.w, g1.x, g1.y};
        float hps = 0.0f;
        if (h.kind != RAYN_HITABLE_SPHERE) {
            const Thr th = make_thr(sc, 0);
            hps = fmaxs(0.0001f, sc.detail_scale * thr_at(th, rec.w));
            offset = hps;
        }
        if (first) {
            f3 nrm;
            if (h.kind == RAYN_HITABLE_SPHERE) nrm = normalized(P - sphere_center(h, ts));
            else {
                EvalCtr evals;
                nrm = sdf_normal<false>(h, P - sphere_center(h, ts), hps, evals, sdf_scale(h, ts));
            }
            nf = nrm * signum(dot(nrm, wo));
            hl[i] = ambient + (1.0f - ambient) * fmaxs(0.0f, dot(nf, wo));
        } else nf = f3{out_normal[3u * (size_t)i], out_normal[3u * (size_t)i + 1u], out_normal[3u * (size_t)i + 2u]};
    }
    if (first) {
        t0s[i] = ts;
        if (i < n) {
            out_normal[3u * (size_t)i] = nf.x; out_normal[3u * (size_t)i + 1u] = nf.y; out_normal[3u * (size_t)i + 2u] = nf.z;
            count[i] = surface ? 0u : INVALID;
        }
    }
    uint32_t pend = 0; // bit kk: sample k0 + kk of this pixel waits for the SDF march (kn <= PREVIEW_ROUND <= 32)
    if (surface) {
        const Basis basis = orthonormal_basis(nf);
        const f3 a = P + nf * offset;
        const float r_p = scramble ? scramble[i] : 0.0f;
        const bool scene_has_sdf = sc.n_sdf > 0;
        for (uint32_t kk = 0; kk < kn; kk++) {
            const float2 s = samples[k0 + kk];
            const float u = dm_fractf(s.x + r_p), v = dm_fractf(s.y + r_p);
            const f3 l = cosine_weighted_in_hemisphere(u, v);
            const f3 b = a + mul(basis, l) * radius;
            // the analytic spheres of test_occluded, as k_shade_setup tests them (every factor is exactly 0 or 1 -> order independent)
            f3 dir = b - a;
            const float dist = mag(dir);
            dir = div_by_mag(dir, dist);
            bool open = true;
            for (uint32_t m = sc.sphere_mask; m && open; m &= m - 1u)
                if (sphere_occluded_dir(sc.h[__builtin_ctz(m)], a, dir, dist, ts) == 0.0f) open = false;
            const size_t idx = (size_t)kk * npad + i; // < 2^32: the host sizes the round
            uint8_t vb = open ? 1 : 0;
            if (open && scene_has_sdf) {
                vb = 2;
                pend |= 1u << kk;
                store_job(job_geo, idx, a, b);
            }
            vis[idx] = vb;
        }
    }
    // the wave's pending references, dense and in lane order: inclusive scan of the lanes' counts, one atomic for the wave's range
    const uint32_t mine = (uint32_t)__popc(pend);
    uint32_t incl = mine;
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, off);
        if (lane >= off) incl += up;
    }
    const uint32_t total = (uint32_t)__shfl((int)incl, 63);
    if (total == 0) return; // wave-uniform
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&ctl->job_count, total);
    base = (uint32_t)__shfl((int)base, 0);
    uint32_t w = base + (incl - mine);
    for (uint32_t m = pend; m; m &= m - 1u) job_ref[w++] = (uint32_t)__builtin_ctz(m) * npad + i;
}

void launch_preview_jobs(hipStream_t s, const DScene* sc, const PreviewScratch& ps, uint32_t k0, uint32_t kn, float radius, float ambient, const float* samples,
                         const float* scramble, float* out_normal) {
    hipLaunchKernelGGL(k_preview_jobs, dim3(ps.g.npad / 256u + (ps.g.npad % 256u ? 1u : 0u)), dim3(256), 0, s, sc, ps.g.n, ps.g.npad, k0, kn, radius, ambient,
                       (const float2*)samples, scramble, ps.g.pool.geo0, ps.g.pool.geo1, ps.records, ps.object, out_normal, ps.hl, ps.count, ps.t0, ps.vis,
                       ps.job_ref, ps.job_geo, ps.g.ctl);
}

} // namespace RAYN_KNS

#if RAYN_FMA_POLICY == 0
namespace rayn {
namespace {

// One thread per pixel: add the round's visible rays to the pixel's count; last: the outputs.  Thread 0 empties the job list for the next round.
__global__ void __launch_bounds__(256) k_preview_resolve(uint32_t n, uint32_t npad, uint32_t kn, float samples, int last, const uint8_t* __restrict__ vis,
                                                          const float* __restrict__ hl, uint32_t* __restrict__ count, float* __restrict__ out_color,
                                                          float* __restrict__ out_alpha, float* __restrict__ out_ao, DCtl* __restrict__ ctl) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0) { ctl->job_count = 0; ctl->head_shadow = 0; }
    if (i >= n) return;
    uint32_t c = count[i];
    const bool surface = c != INVALID;
    if (surface) {
        for (uint32_t kk = 0; kk < kn; kk++) c += vis[(size_t)kk * npad + i] == 1 ? 1u : 0u;
        if (!last) count[i] = c;
    }
    if (!last) return;
    const float ao = surface ? (float)c / samples : 1.0f;
    const float col = surface ? ao * hl[i] : 0.0f;
    out_color[3u * (size_t)i] = col; out_color[3u * (size_t)i + 1u] = col; out_color[3u * (size_t)i + 2u] = col;
    out_alpha[i] = surface ? 1.0f : 0.0f;
    if (out_ao) out_ao[i] = ao;
}

} // namespace

size_t preview_scratch_bytes(uint32_t width, uint32_t height, uint32_t samples) {
    if (check_size(width, height) || samples < 1 || samples > PREVIEW_MAX_SAMPLES) return 0;
    const uint64_t npad = ((uint64_t)width * height + 63u) & ~(uint64_t)63u;
    const uint64_t round = samples < PREVIEW_ROUND ? samples : PREVIEW_ROUND;
    return (size_t)(gbuffer_scratch_bytes(width, height) + 32u * npad + 29u * round * npad);
}

PreviewScratch preview_scratch(uint32_t width, uint32_t height, uint32_t samples, void* scratch, void* out_records, uint32_t* out_object) {
    PreviewScratch ps;
    memset(&ps, 0, sizeof ps);
    ps.g = gbuffer_scratch(width, height, scratch);
    const size_t np = ps.g.npad;
    uint32_t round = samples < PREVIEW_ROUND ? samples : PREVIEW_ROUND;
    const size_t room = round; // the layout is that of preview_scratch_bytes whatever the round becomes
    while (round > 1 && (uint64_t)round * np >= ((uint64_t)1 << 32)) round >>= 1; // 32-bit [sample][slot] references
    ps.round = round;
    char* b = (char*)scratch + gbuffer_scratch_bytes(width, height);
    ps.records = out_records ? (float4*)out_records : (float4*)b;
    ps.object = out_object ? out_object : (uint32_t*)(b + 16u * np);
    ps.hl = (float*)(b + 20u * np);
    ps.count = (uint32_t*)(b + 24u * np);
    ps.t0 = (float*)(b + 28u * np);
    ps.vis = (uint8_t*)(b + 32u * np);
    ps.job_ref = (uint32_t*)(b + 32u * np + room * np);
    ps.job_geo = (float2*)(b + 32u * np + 5u * room * np);
    return ps;
}

const char* preview_check_args(const rayn_frame_params* p, const rayn_preview_params* pp, const float* samples, const float* scramble, const float* out_color,
                               const float* out_alpha, const float* out_normal, const float* out_ao, const void* out_records, const uint32_t* out_object,
                               const void* scratch, size_t scratch_bytes) {
    if (!p) return "null frame params";
    if (!pp) return "null preview params";
    if (const char* why = check_size(p->width, p->height)) return why;
    if (pp->samples < 1 || pp->samples > PREVIEW_MAX_SAMPLES) return "samples must be in 1..64";
    if (!(pp->radius > 0.0f) || !(pp->radius <= 3.40282347e+38f)) return "radius must be finite and > 0";
    if (!(pp->ambient >= 0.0f && pp->ambient <= 1.0f)) return "ambient must be in [0, 1]";
    if (!samples || !out_color || !out_alpha || !out_normal || !scratch) return "null buffer";
    if (scratch_bytes < preview_scratch_bytes(p->width, p->height, pp->samples)) return "scratch smaller than rayn_preview_scratch_bytes(width, height, samples)";
    if ((uintptr_t)scratch % 16u) return "scratch not 16-byte aligned";
    if ((uintptr_t)samples % 8u) return "d_samples not 8-byte aligned";
    if ((uintptr_t)out_records % 16u) return "d_out_records not 16-byte aligned";
    if ((uintptr_t)scramble % 4u || (uintptr_t)out_color % 4u || (uintptr_t)out_alpha % 4u || (uintptr_t)out_normal % 4u || (uintptr_t)out_ao % 4u ||
        (uintptr_t)out_object % 4u)
        return "a float or u32 plane is not 4-byte aligned";
    const size_t n = (size_t)p->width * p->height;
    const Span out[7] = {{out_color, 12u * n}, {out_alpha, 4u * n}, {out_normal, 12u * n}, {out_ao, 4u * n}, {out_records, 16u * n}, {out_object, 4u * n},
                         {scratch, scratch_bytes}};
    const Span in[2] = {{samples, 8u * (size_t)pp->samples}, {scramble, 4u * n}};
    if (first_overlap(out, 7, in, 2)) return "an output or the scratch must not alias an input";
    for (int i = 0; i < 7; i++)
        if (first_overlap(out + i, 1, out + i + 1, 6 - i)) return "the outputs must not overlap each other or the scratch";
    return nullptr;
}

Nee preview_nee(const PreviewScratch& ps) {
    Nee nee;
    memset(&nee, 0, sizeof nee);
    nee.vis = ps.vis; nee.t0 = ps.t0; nee.cap = ps.g.npad;
    nee.job_ref = ps.job_ref; nee.job_geo = ps.job_geo; nee.jobcap = (size_t)ps.round * ps.g.npad;
    return nee;
}

void launch_preview_resolve(hipStream_t s, const PreviewScratch& ps, uint32_t kn, uint32_t samples, bool last, float* out_color, float* out_alpha, float* out_ao) {
    hipLaunchKernelGGL(k_preview_resolve, dim3((ps.g.n + 255u) / 256u), dim3(256), 0, s, ps.g.n, ps.g.npad, kn, (float)samples, last ? 1 : 0, ps.vis, ps.hl, ps.count,
                       out_color, out_alpha, out_ao, ps.g.ctl);
}

} // namespace rayn

extern "C" size_t rayn_preview_scratch_bytes(uint32_t width, uint32_t height, uint32_t samples) { return rayn::preview_scratch_bytes(width, height, samples); }
#endif // RAYN_FMA_POLICY == 0
