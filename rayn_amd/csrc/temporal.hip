// temporal.hip — temporal accumulation for frame sequences, the temporal half of SVGF (Schied et al., HPG 2017): a primary-hit G-buffer
// pass (rayn_hip_gbuffer_device) and the reprojection + blend of the film's Color channel (rayn_hip_temporal_accumulate_device).
// Extensions: rayn has neither.  Both run downstream of the film; the film and the integrator are not touched.
//
// G-buffer.  k_gbuffer_rays writes one ray per pixel p = x + y * width (bottom-up rows) into a pool-shaped scratch: uv = (ndc_x (x + 0.5f),
// ndc_y (y + 0.5f)) - k_raygen's expression with a filter offset of 0 - lens sample (0.5, 0.5), ray time = closure time = time_start,
// through camera_ray (device_core.h) under the build's mul_add policy; and the identity queue padded to whole 64-slot groups.  (0.5, 0.5)
// is the point concentric_circle_map nudges off its singular centre (b = 0.0001, src/math.rs:205): a thin lens's G-buffer ray leaves the
// lens 0.0001 * aperture beside the centre, far below a pixel.  The scene's PRODUCT extend kernel then runs at depth 0 (launch glue in
// rayn_hip.hip, as rayn_hip_probe_extend selects it), and k_gbuffer_finish writes (P, t) with P = o + t d as a separate multiply and add,
// and the object index; a miss writes (0, 0, 0, +inf) and 0xFFFFFFFF.  This file is built once per mul_add policy for k_gbuffer_rays;
// everything else is policy-free and built with the RAYN_FMA_POLICY=0 object only.
//
// Accumulate (include/rayn_hip.h has the same text; tests/temporal_np.py restates it in numpy and the tests compare bit for bit).  All f32,
// -ffp-contract=off, IEEE '/' and sqrtf.  dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z; cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z,
// a.x b.y - a.y b.x); nz(a) = a * (1.0f / sqrtf(dot(a, a))); a vector +, -, * scalar acts per component; "a - b * s" is a multiply, then
// a subtraction.  Per pixel p with colour c, normal nrm, G-buffer record (P, t) and object obj:
//   reset (out = c, n' = 1; n' = 0 when c has a non-finite component) when obj = 0xFFFFFFFF, c is not finite, or there is no previous history
//   Pp = P - center_vel[obj] * (time_start_cur - time_start_prev) when hitable obj is animated, else P
//   camera at ts = time_start_prev: o = origin + origin_vel * ts (bit 0 of animated; else origin), at and up likewise
//   pinhole, thin lens:  w = nz(o - at), u = nz(cross(up, w)), v = cross(w, u);  q = Pp - o;  zc = -dot(q, w), rejected unless zc > 0;
//                        uvx = (dot(q, u) / (zc * half_w) + 1.0f) * 0.5f, uvy = (dot(q, v) / (zc * half_h) + 1.0f) * 0.5f;  te = sqrtf(dot(q, q))
//   orthographic:        w = nz(at - o), u = nz(cross(w, up)), v = cross(u, w);  ll = (o - u * half_w) - v * half_h;  q = Pp - ll;
//                        uvx = dot(q, u) / full_w, uvy = dot(q, v) / full_h;  te = dot(q, w), rejected unless te > 0
//   fx = uvx * (float)width - 0.5f, fy = uvy * (float)height - 0.5f, rejected unless both are finite
//   x0f = floorf(fx), y0f = floorf(fy); wx1 = fx - x0f, wx0 = 1.0f - wx1, wy1 = fy - y0f, wy0 = 1.0f - wy1;
//   x0 = (integer) min(max(x0f, -2), 2^31), y0 likewise (the clamp only keeps the conversion defined: such taps are outside anyway)
//   taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) with w = wx0 wy0, wx1 wy0, wx0 wy1, wx1 wy1; a tap counts when it is inside
//   the image, n_tap >= 1, obj_tap = obj, fabsf(t_tap - te) <= depth_tolerance * te and, with normal_min > -1, dot(nrm, nrm_tap) >= normal_min
//   (every comparison false for a NaN):   W += w, S += w * c_tap, N += w * n_tap
//   W > 0:  h = S / W, nh = N / W, n' = fminf(nh + 1.0f, (float)max_history), a = 1.0f / n', out = h + a * (c - h); out is taken when its
//   three components are finite.  A rejected projection, W <= 0 and a non-finite out reset the pixel.
//   History out: A' = (out, n'), B' = (P, t), the object and (nrm, 0).
// Moments (rayn_hip_temporal_accumulate_moments_device; k_temporal_accumulate<true>): 8 more bytes per pixel, a float2 (m1, m2) in film pixel
// order beside the history, carried through the same taps.  y = (0.2126f c.r + 0.7152f c.g) + 0.0722f c.b, y2 = y * y.  A pixel that resets
// writes (y, y2), and (0, 0) when c is not finite.  Otherwise S1 += w * m1_tap, S2 += w * m2_tap over the colour's taps in its loop order,
// h1 = S1 / W, h2 = S2 / W, m1' = h1 + a * (y - h1), m2' = h2 + a * (y2 - h2) with the colour's a; a non-finite m1' or m2' writes (y, y2)
// while the colour keeps its blend.  The colour and the 52 B history are the bits of the plain entry.
// Catmull-Rom (rayn_hip_temporal_accumulate_resample_device with resample = 1; k_temporal_accumulate<*, 1>): step 4 reads the 4x4 footprint
// (x0 - 1 .. x0 + 2) x (y0 - 1 .. y0 + 2).  With t = wx1 (and wy1) the weights of the offsets -1, 0, 1, 2 are ((-0.5f t + 1.0f) t - 0.5f) t,
// ((1.5f t - 2.5f) t) t + 1.0f, ((-1.5f t + 2.0f) t + 0.5f) t, ((0.5f t - 0.5f) t) t.  When all 16 taps count (the predicate above), in
// raster order with w = kx_i * ky_j: W += w, S += w * c_tap, N += w * n_tap (S1, S2 likewise); h = S / W, nh = N / W, h1, h2; every
// component of h, and h1 and h2, is clamped with fminf(fmaxf(v, lo), hi) to the range of the four inner taps (anti-ringing; fminf / fmaxf
// drop a NaN operand and order -0 below +0, as v_min_f32 / v_max_f32 do), nh = fmaxf(nh, 1.0f), then step 5.  Any tap outside the image or
// rejected: the bilinear step 4 above, exactly.  The kernel checks the 16 taps first (4 + 4 + 4 [+ 16] bytes each) and re-reads the colours
// (and moments) of a full footprint in a second loop: no 16 live float4.
// One thread per pixel in 16x16 blocks, 16-byte record loads, as denoise.hip; at most 4 x 3 record loads per pixel: bandwidth-trivial.
// Step 3 (project), step 4's predicate (history_tap_counts) and step 5 (blend_history) are in post_device.h: k_temporal_upscale's phase C
// calls the same functions.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "device_core.h"
#include "post_checks.h"
#include "post_device.h"
#include "temporal.h"

namespace RAYN_KNS {

// One thread per padded slot.  n = width * height < 2^31, npad = n rounded up to 64.
__global__ void __launch_bounds__(256) k_gbuffer_rays(const DScene* __restrict__ scp, uint32_t n, uint32_t npad, float4* __restrict__ geo0,
                                                       float4* __restrict__ geo1, float4* __restrict__ col1, uint32_t* __restrict__ q,
                                                       DCtl* __restrict__ ctl) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= npad) return;
    if (i == 0) {
        DCtl c = {};
        c.q_groups = npad >> 6; c.q_valid = n;
        *ctl = c;
    }
    if (i >= n) { q[i] = INVALID; return; }
    const DScene& sc = *scp;
    const uint32_t y = i / sc.width, x = i - y * sc.width;
    const float uvx = sc.ndc_x * ((float)x + 0.5f), uvy = sc.ndc_y * ((float)y + 0.5f);
    f3 o, d;
    camera_ray(sc.cam, uvx, uvy, 0.5f, 0.5f, sc.time_start, &o, &d);
    geo0[i] = make_float4(o.x, o.y, o.z, d.x);
    geo1[i] = make_float4(d.y, d.z, 0.0f, __uint_as_float(OBJ_NONE));
    col1[i] = make_float4(0.0f, 0.0f, __uint_as_float(i), sc.time_start);
    q[i] = i;
}

void launch_gbuffer_rays(hipStream_t s, const DScene* sc, const GbufScratch& g) {
    hipLaunchKernelGGL(k_gbuffer_rays, dim3((g.npad + 255u) / 256u), dim3(256), 0, s, sc, g.n, g.npad, g.pool.geo0, g.pool.geo1, g.pool.col1, g.q, g.ctl);
}

} // namespace RAYN_KNS

#if RAYN_FMA_POLICY == 0
namespace rayn {
namespace {

constexpr size_t GBUF_CTL_BYTES = 256, GBUF_EVALS_BYTES = 128;
static_assert(sizeof(DCtl) <= GBUF_CTL_BYTES, "the G-buffer scratch reserves 256 bytes for the control block");

// One thread per pixel: the pool's ray + the hit the extend kernel left in geo1 -> record and object index.
__global__ void __launch_bounds__(256) k_gbuffer_finish(uint32_t n, const float4* __restrict__ geo0, const float4* __restrict__ geo1,
                                                         float4* __restrict__ out, uint32_t* __restrict__ out_obj) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 g0 = geo0[i], g1 = geo1[i];
    const uint32_t id = __float_as_uint(g1.w) & 0xFFu;
    if (id == OBJ_NONE) {
        out[i] = make_float4(0.0f, 0.0f, 0.0f, __builtin_inff());
        out_obj[i] = INVALID;
        return;
    }
    const float t = g1.z;
    const float mx = t * g0.w, my = t * g1.x, mz = t * g1.y;
    out[i] = make_float4(g0.x + mx, g0.y + my, g0.z + mz, t);
    out_obj[i] = id;
}

// One Catmull-Rom weight set: the offsets -1, 0, 1, 2 at the fraction t in [0, 1)
__device__ inline void cubic_weights(float t, float k[4]) {
    k[0] = ((-0.5f * t + 1.0f) * t - 0.5f) * t;
    k[1] = ((1.5f * t - 2.5f) * t) * t + 1.0f;
    k[2] = ((-1.5f * t + 2.0f) * t + 0.5f) * t;
    k[3] = ((0.5f * t - 0.5f) * t) * t;
}
__device__ inline float clampf(float v, float lo, float hi) { return __builtin_fminf(__builtin_fmaxf(v, lo), hi); }

// Step 4's result: the resampled history colour, length and moments
struct Resampled { float r, g, b, n, m1, m2; };

// The Catmull-Rom arm of step 4.  False - nothing written - unless all 16 taps of the footprint count; the caller then takes the bilinear
// arm.  The first loop reads what the predicate needs (the length, object and depth dwords, the normal when its test is on), the second
// re-reads the colours (and moments) of a full footprint from L2: at most one float4 (+ float2) is live per tap.
template <bool MOMENTS>
__device__ inline bool cubic_history(long long x0, long long y0, uint32_t width, uint32_t height, float tx, float ty, uint32_t obj, float te, float tol,
                                     float normal_min, v3 nrm, const float4* __restrict__ pA, const float4* __restrict__ pB,
                                     const float4* __restrict__ pN, const uint32_t* __restrict__ pO, const float2* __restrict__ pM, Resampled* out) {
    if (x0 < 1 || x0 + 2 >= (long long)width || y0 < 1 || y0 + 2 >= (long long)height) return false;
    const uint32_t q0 = (uint32_t)(x0 - 1) + (uint32_t)(y0 - 1) * width; // every tap is a pixel of the image: its index is < 2^31
    // one row of the footprint per trip, not unrolled, in both loops: four taps in flight instead of sixteen
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
        bool row = true;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t q = q0 + (uint32_t)i + (uint32_t)j * width;
            // history_tap_counts' four tests, but every plane read before any is looked at: a row's twelve loads are in flight together
            bool counts = pA[q].w >= 1.0f;
            counts &= pO[q] == obj;
            counts &= __builtin_fabsf(pB[q].w - te) <= tol;
            if (normal_min > -1.0f) {
                const float4 nq = pN[q];
                counts &= dot3(nrm, v3{nq.x, nq.y, nq.z}) >= normal_min;
            }
            row &= counts;
        }
        if (!row) return false;
    }
    float kx[4], ky[4];
    cubic_weights(tx, kx);
    cubic_weights(ty, ky);
    float W = 0.0f, S[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, lo[6], hi[6]; // r, g, b, n, m1, m2
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
        const float kyj = j == 0 ? ky[0] : j == 1 ? ky[1] : j == 2 ? ky[2] : ky[3];
        const bool inner_row = j == 1 || j == 2;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t q = q0 + (uint32_t)i + (uint32_t)j * width;
            const float4 a = pA[q];
            const float2 m = MOMENTS ? pM[q] : make_float2(0.0f, 0.0f);
            const float v[6] = {a.x, a.y, a.z, a.w, m.x, m.y};
            const float w = kx[i] * kyj;
            W += w;
#pragma unroll
            for (int c = 0; c < (MOMENTS ? 6 : 4); c++) {
                S[c] += w * v[c];
                // the four inner taps, raster order: the range of the anti-ringing clamp
                if (i == 1 && j == 1) lo[c] = hi[c] = v[c];
                else if ((i == 1 || i == 2) && inner_row) { lo[c] = __builtin_fminf(lo[c], v[c]); hi[c] = __builtin_fmaxf(hi[c], v[c]); }
            }
        }
    }
    out->r = clampf(S[0] / W, lo[0], hi[0]);
    out->g = clampf(S[1] / W, lo[1], hi[1]);
    out->b = clampf(S[2] / W, lo[2], hi[2]);
    out->n = __builtin_fmaxf(S[3] / W, 1.0f);
    if (MOMENTS) {
        out->m1 = clampf(S[4] / W, lo[4], hi[4]);
        out->m2 = clampf(S[5] / W, lo[5], hi[5]);
    }
    return true;
}

// MOMENTS: also carry the first and second moment of the luminance through the same taps (rayn_hip_temporal_accumulate_moments_device);
// the false instantiation reads and writes exactly what the kernel did before the moments existed.
// RESAMPLE: 0 the bilinear step 4, the instruction streams of the kernel before the option existed; 1 Catmull-Rom over a full 4x4
// footprint, bilinear otherwise (rayn_hip_temporal_accumulate_resample_device).
template <bool MOMENTS, int RESAMPLE>
__global__ void __launch_bounds__(256) k_temporal_accumulate(uint32_t width, uint32_t height, uint32_t tiles_x, float max_history, float depth_tolerance,
                                                              float normal_min, TemporalScene ts, const float* __restrict__ color,
                                                              const float* __restrict__ normal, const float4* __restrict__ grec,
                                                              const uint32_t* __restrict__ gobj, const float4* __restrict__ pA,
                                                              const float4* __restrict__ pB, const float4* __restrict__ pN,
                                                              const uint32_t* __restrict__ pO, float4* __restrict__ nA, float4* __restrict__ nB,
                                                              float4* __restrict__ nN, uint32_t* __restrict__ nO, float* __restrict__ out_color,
                                                              const float2* __restrict__ pM, float2* __restrict__ nM) {
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const uint32_t x = tx * 16u + threadIdx.x, y = ty * 16u + threadIdx.y;
    if (x >= width || y >= height) return;
    const uint32_t p = x + y * width; // < 2^31
    const size_t f = (size_t)p * 3u;
    const v3 c = v3{color[f], color[f + 1], color[f + 2]};
    const v3 nrm = v3{normal[f], normal[f + 1], normal[f + 2]};
    const float4 g = grec[p];
    const uint32_t obj = gobj[p];
    const bool cfin = fin(c.x) && fin(c.y) && fin(c.z);
    v3 out = c;
    float nn = cfin ? 1.0f : 0.0f;
    const float lum = luminance(c.x, c.y, c.z), lum2 = lum * lum; // the definition's y, y2
    float m1 = cfin ? lum : 0.0f, m2 = cfin ? lum2 : 0.0f;
    if (cfin && obj != MISS_OBJECT && pA) {
        v3 Pp = v3{g.x, g.y, g.z};
        const float dt = ts.cur_time - ts.prev_time;
#pragma unroll
        for (uint32_t k = 0; k < RAYN_MAX_HITABLES; k++)
            if (k < ts.n_hitables && obj == k && ts.hvel[k].w != 0.0f) Pp = v3{g.x - ts.hvel[k].x * dt, g.y - ts.hvel[k].y * dt, g.z - ts.hvel[k].z * dt};
        float fx, fy, te;
        if (project(ts.cam, ts.prev_time, Pp, width, height, &fx, &fy, &te)) {
            const float x0f = __builtin_floorf(fx), y0f = __builtin_floorf(fy);
            const float wx1 = fx - x0f, wx0 = 1.0f - wx1, wy1 = fy - y0f, wy0 = 1.0f - wy1;
            const long long x0 = (long long)__builtin_fminf(__builtin_fmaxf(x0f, -2.0f), 2147483648.0f);
            const long long y0 = (long long)__builtin_fminf(__builtin_fmaxf(y0f, -2.0f), 2147483648.0f);
            const float tol = depth_tolerance * te;
            float W = 0.0f, Sr = 0.0f, Sg = 0.0f, Sb = 0.0f, N = 0.0f, S1 = 0.0f, S2 = 0.0f;
            Resampled hs = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            bool have = false;
            if (RESAMPLE == 1) have = cubic_history<MOMENTS>(x0, y0, width, height, wx1, wy1, obj, te, tol, normal_min, nrm, pA, pB, pN, pO, pM, &hs);
            if (!have) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const long long qx = x0 + (k & 1), qy = y0 + (k >> 1);
                    if (qx < 0 || qx >= (long long)width || qy < 0 || qy >= (long long)height) continue;
                    const uint32_t q = (uint32_t)qx + (uint32_t)qy * width;
                    const float4 a = pA[q];
                    if (!history_tap_counts(a.w, q, obj, te, tol, normal_min, nrm, pB, pN, pO)) continue;
                    const float w = ((k & 1) ? wx1 : wx0) * ((k >> 1) ? wy1 : wy0);
                    W += w;
                    Sr += w * a.x;
                    Sg += w * a.y;
                    Sb += w * a.z;
                    N += w * a.w;
                    if (MOMENTS) {
                        const float2 m = pM[q];
                        S1 += w * m.x;
                        S2 += w * m.y;
                    }
                }
                if (W > 0.0f) {
                    hs = Resampled{Sr / W, Sg / W, Sb / W, N / W, 0.0f, 0.0f};
                    if (MOMENTS) { hs.m1 = S1 / W; hs.m2 = S2 / W; }
                    have = true;
                }
            }
            if (have) {
                const Blend b = blend_history(c, v3{hs.r, hs.g, hs.b}, hs.n, 1.0f, max_history);
                if (b.ok) {
                    out = b.out; nn = b.n1;
                    if (MOMENTS) {
                        const float h1 = hs.m1, h2 = hs.m2;
                        const float d1 = lum - h1, d2 = lum2 - h2;
                        const float b1 = h1 + b.a * d1, b2 = h2 + b.a * d2;
                        if (fin(b1) && fin(b2)) { m1 = b1; m2 = b2; } // else (y, y2): an overflow heals on the next frame
                    }
                }
            }
        }
    }
    out_color[f] = out.x;
    out_color[f + 1] = out.y;
    out_color[f + 2] = out.z;
    nA[p] = make_float4(out.x, out.y, out.z, nn);
    nB[p] = g;
    nN[p] = make_float4(nrm.x, nrm.y, nrm.z, 0.0f);
    nO[p] = obj;
    if (MOMENTS) nM[p] = make_float2(m1, m2);
}

} // namespace

size_t gbuffer_scratch_bytes(uint32_t width, uint32_t height) {
    if (check_size(width, height)) return 0;
    const uint64_t npad = ((uint64_t)width * height + 63u) & ~(uint64_t)63u;
    return (size_t)(53u * npad + GBUF_CTL_BYTES + GBUF_EVALS_BYTES);
}

GbufScratch gbuffer_scratch(uint32_t width, uint32_t height, void* scratch) {
    GbufScratch g;
    memset(&g, 0, sizeof g);
    g.n = width * height;
    g.npad = (g.n + 63u) & ~63u;
    char* b = (char*)scratch;
    const size_t np = g.npad;
    g.pool.geo0 = (float4*)b;
    g.pool.geo1 = (float4*)(b + 16u * np);
    g.pool.col1 = (float4*)(b + 32u * np);
    g.q = (uint32_t*)(b + 48u * np);
    g.ent_obj = (uint8_t*)(b + 52u * np);
    g.ctl = (DCtl*)(b + 53u * np);
    g.evals = (unsigned long long*)(b + 53u * np + GBUF_CTL_BYTES);
    return g;
}

const char* gbuffer_check_args(const rayn_frame_params* p, const void* out_records, const uint32_t* out_object, const void* scratch, size_t scratch_bytes) {
    if (!p) return "null frame params";
    if (const char* why = check_size(p->width, p->height)) return why;
    if (!out_records || !out_object || !scratch) return "null buffer";
    if (scratch_bytes < gbuffer_scratch_bytes(p->width, p->height)) return "scratch smaller than rayn_gbuffer_scratch_bytes(width, height)";
    if ((uintptr_t)scratch % 16u) return "scratch not 16-byte aligned";
    if ((uintptr_t)out_records % 16u) return "d_out_records not 16-byte aligned";
    if ((uintptr_t)out_object % 4u) return "d_out_object not 4-byte aligned";
    const size_t n = (size_t)p->width * p->height;
    if (overlap(out_records, 16u * n, scratch, scratch_bytes) || overlap(out_object, 4u * n, scratch, scratch_bytes) || overlap(out_records, 16u * n, out_object, 4u * n))
        return "the outputs must not overlap each other or the scratch";
    return nullptr;
}

void launch_gbuffer_finish(hipStream_t s, const GbufScratch& g, void* out_records, uint32_t* out_object) {
    hipLaunchKernelGGL(k_gbuffer_finish, dim3((g.n + 255u) / 256u), dim3(256), 0, s, g.n, g.pool.geo0, g.pool.geo1, (float4*)out_records, out_object);
}

size_t temporal_history_bytes(uint32_t width, uint32_t height) {
    if (check_size(width, height)) return 0;
    return (size_t)(52u * (uint64_t)width * height);
}

const char* temporal_check_args(const rayn_frame_params* p, const rayn_temporal_params* tp, const rayn_camera* prev_camera, const float* color,
                                const float* normal, const void* g_records, const uint32_t* g_object, const void* prev_history,
                                const void* new_history, size_t history_bytes, const float* out_color) {
    if (!p) return "null frame params";
    if (const char* why = check_size(p->width, p->height)) return why;
    if (const char* why = check_temporal_params(tp)) return why;
    if (!color || !normal || !g_records || !g_object || !new_history || !out_color) return "null buffer";
    if (prev_history && !prev_camera) return "a previous history needs the previous camera";
    if (prev_camera && prev_camera->kind > RAYN_CAM_ORTHOGRAPHIC) return "unknown camera kind";
    const size_t need = temporal_history_bytes(p->width, p->height);
    if (history_bytes < need) return "history smaller than rayn_temporal_history_bytes(width, height)";
    if ((uintptr_t)new_history % 16u || (uintptr_t)prev_history % 16u) return "history not 16-byte aligned";
    if ((uintptr_t)g_records % 16u) return "d_gbuffer_records not 16-byte aligned";
    if ((uintptr_t)g_object % 4u) return "d_gbuffer_object not 4-byte aligned";
    const size_t n = (size_t)p->width * p->height;
    if (overlap(new_history, need, prev_history, need)) return "the new history must not alias the previous one";
    const Span in[5] = {{color, 12u * n}, {normal, 12u * n}, {g_records, 16u * n}, {g_object, 4u * n}, {prev_history, need}};
    const Span out[2] = {{out_color, 12u * n}, {new_history, need}};
    if (first_overlap(out, 2, in, 5)) return "an output must not alias an input";
    if (overlap(out_color, 12u * n, new_history, need)) return "d_out_color must not alias the new history";
    return nullptr;
}

size_t temporal_moments_bytes(uint32_t width, uint32_t height) {
    if (check_size(width, height)) return 0;
    return (size_t)(8u * (uint64_t)width * height);
}

const char* temporal_moments_check_args(const rayn_frame_params* p, const float* color, const float* normal, const void* g_records,
                                        const uint32_t* g_object, const void* prev_history, const void* new_history, const void* prev_moments,
                                        const void* new_moments, size_t moments_bytes, const float* out_color) {
    if (!new_moments) return "null buffer";
    if (prev_moments && !prev_history) return "previous moments without a previous history";
    if (prev_history && !prev_moments) return "a previous history needs the previous moments";
    const size_t need = temporal_moments_bytes(p->width, p->height), hist = temporal_history_bytes(p->width, p->height);
    if (moments_bytes < need) return "moments smaller than rayn_temporal_moments_bytes(width, height)";
    if ((uintptr_t)new_moments % 16u || (uintptr_t)prev_moments % 16u) return "moments not 16-byte aligned";
    const size_t n = (size_t)p->width * p->height;
    if (overlap(new_moments, need, prev_moments, need)) return "the new moments must not alias the previous ones";
    const Span in[6] = {{color, 12u * n}, {normal, 12u * n}, {g_records, 16u * n}, {g_object, 4u * n}, {prev_history, hist}, {prev_moments, need}};
    const Span mom = {new_moments, need};
    if (first_overlap(&mom, 1, in, 6)) return "an output must not alias an input";
    if (overlap(out_color, 12u * n, prev_moments, need) || overlap(new_history, hist, prev_moments, need)) return "an output must not alias an input";
    if (overlap(new_moments, need, new_history, hist) || overlap(new_moments, need, out_color, 12u * n)) return "the new moments must not alias another output";
    return nullptr;
}

const char* temporal_resample_check_args(const rayn_temporal_resample_params* rp) {
    if (!rp) return "null resample params";
    if (rp->resample > 1u) return "resample must be 0 (bilinear) or 1 (Catmull-Rom)";
    return nullptr;
}

void launch_temporal_accumulate(hipStream_t s, uint32_t width, uint32_t height, const rayn_temporal_params& tp, const TemporalScene& ts,
                                const float* color, const float* normal, const void* g_records, const uint32_t* g_object,
                                const void* prev_history, void* new_history, float* out_color, const void* prev_moments, void* new_moments, uint32_t resample) {
    const size_t n = (size_t)width * height;
    const float4* pA = (const float4*)prev_history; // null: no previous history
    float4* nA = (float4*)new_history;
    const uint32_t tiles_x = (width + 15u) / 16u, tiles_y = (height + 15u) / 16u;
#define RAYN_TACC(M, R) hipLaunchKernelGGL((k_temporal_accumulate<M, R>), dim3(tiles_x * tiles_y), dim3(16, 16), 0, s, width, height, tiles_x, (float)tp.max_history, \
                       tp.depth_tolerance, tp.normal_min, ts, color, normal, (const float4*)g_records, g_object, pA, pA ? pA + n : nullptr,           \
                       pA ? pA + 2u * n : nullptr, pA ? (const uint32_t*)(pA + 3u * n) : nullptr, nA, nA + n, nA + 2u * n, (uint32_t*)(nA + 3u * n), \
                       out_color, (const float2*)prev_moments, (float2*)new_moments)
    if (resample == 1) {
        if (new_moments) RAYN_TACC(true, 1);
        else RAYN_TACC(false, 1);
    } else if (new_moments) RAYN_TACC(true, 0); // the moments entry
    else RAYN_TACC(false, 0);
#undef RAYN_TACC
}

} // namespace rayn

extern "C" size_t rayn_gbuffer_scratch_bytes(uint32_t width, uint32_t height) { return rayn::gbuffer_scratch_bytes(width, height); }
extern "C" size_t rayn_temporal_history_bytes(uint32_t width, uint32_t height) { return rayn::temporal_history_bytes(width, height); }
extern "C" size_t rayn_temporal_moments_bytes(uint32_t width, uint32_t height) { return rayn::temporal_moments_bytes(width, height); }
#endif // RAYN_FMA_POLICY == 0
