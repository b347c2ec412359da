// temporal_upscale.hip — temporal supersampling (rayn_hip_temporal_upscale_device): the guided upscaling of upscale.hip and the temporal
// accumulation of temporal.hip in ONE kernel whose history lives at the high resolution.  Low frames rendered with different sub-pixel
// camera offsets then meet in a full-size history: over s * s frames every high pixel has had a low sample at its own centre (temporal
// upsampling as in TAAU / FSR2).  An extension: rayn renders at one resolution and every frame on its own.  Downstream of the film: the
// low film, both G-buffers and the previous history are read; the high planes and the new history are written.
//
// The definition (include/rayn_hip.h; tests/temporal_upscale_np.py restates it in numpy and the tests compare bit
// for bit).  Per high pixel (X, Y) with the high G-buffer's (P, t) and o:
//   A. footprint in the low film: fx = ((float)X + 0.5f) / s - 0.5f (upscale step 1), or - with a low camera and a hit pixel - P projected
//      through that camera at the frame's time_start by the temporal entry's step 3 (project(), post_device.h) at the LOW size; a
//      rejected projection and a miss pixel keep the default.  x0, y0 by the temporal entry's step 4.
//   B. this frame's value: steps 2 and 3 of the upscale on that footprint (three tiers, sums from -0.0f, tap order), every plane -
//      upscale_gather() of post_device.h, the function k_upscale calls; conf = 1, or with confidence on the largest bilinear weight b_k
//      among the taps that were added in the tier that gave the value (what upscale_gather returns).
//   C. steps 1 to 5 of the temporal accumulate at the high size on B's Color and WorldNormal, with n' = fminf(nh + conf, max_history)
//      and a = conf / n': project(), history_tap_counts() and blend_history() of post_device.h, the functions k_temporal_accumulate calls.
// With no low camera and confidence off the outputs are, bit for bit, those of k_upscale followed by k_temporal_accumulate - without the
// 24 bytes per high pixel of Color and WorldNormal written by the one and read back by the other.  f32 throughout, built with
// -ffp-contract=off and IEEE division; nothing depends on the mul_add policy: the file is built once.
//
// Layout: one thread per high pixel in 16x16 tiles (the taps of both footprints are 2-D neighbourhoods).  A pixel reads 20 bytes of its
// own guide and writes 40 + 52 (+ 4); the low taps are shared by s x s pixels and the history taps by their neighbours, both from L2.
// The phases run one after another, so the eleven sums of B are dead - Alpha and Background already stored - before C's five begin; the
// two fallback tiers re-read their taps in a branch few pixels take.  The uniform choices (low camera, confidence, a first frame) are
// uniform branches; only the two sigma terms are template parameters, as in upscale.hip.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "post_checks.h"
#include "post_device.h"
#include "temporal_upscale.h"

namespace rayn {
namespace {

struct TUArgs {
    uint32_t w, h, W, H, tiles_x, factor, confidence, have_low_cam; // the low size, the high size, 16x16 tiles per high row
    float sigma_plane, sigma_position, max_history, depth_tolerance, normal_min;
    UpscalePlanes pl;
    const float4 *pA, *pB, *pN; // the previous history's planes; pA null: none
    const uint32_t* pO;
    float4 *nA, *nB, *nN;
    uint32_t* nO;
    DCamera low_cam; // looked at only with have_low_cam
    TemporalScene ts;
};

// Step 4's integer tap origin.  The definition clamps to [-2, 2^31]; images are at most 2^23 wide and high here (the upscale's limit), so
// every origin above 2^24 is as far outside as one at 2^31 and the narrower clamp, which fits an int, changes no result.
__device__ inline int tap_origin(float x0f) { return (int)__builtin_fminf(__builtin_fmaxf(x0f, -2.0f), 16777216.0f); }

// TERMS: which of the plane / position terms of B are on.  Every index is bounded by its plane: a low tap is used only with qx < w and
// qy < h, the tier-3 source is clamped to the low image, a history tap only with qx < W and qy < H, and P < W * H by the guards on X, Y.
template <uint32_t TERMS>
__global__ void __launch_bounds__(256) k_temporal_upscale(const TUArgs A) {
    const uint32_t tyi = blockIdx.x / A.tiles_x, txi = blockIdx.x - tyi * A.tiles_x;
    const uint32_t X = txi * 16u + threadIdx.x, Y = tyi * 16u + threadIdx.y;
    if (X >= A.W || Y >= A.H) return;
    const UpscalePlanes& pl = A.pl;
    const uint32_t P = X + Y * A.W; // < 2^31
    const uint32_t o = pl.high_object[P];
    const float4 G = ((const float4*)pl.high_records)[P];

    // ---- A: the footprint in the low film
    const float sf = (float)A.factor;
    float fx = ((float)X + 0.5f) / sf - 0.5f, fy = ((float)Y + 0.5f) / sf - 0.5f; // exact pixel centres (W, H <= 2^23)
    if (A.have_low_cam && o != MISS_OBJECT) {
        float pfx, pfy, pte;
        if (project(A.low_cam, A.ts.cur_time, v3{G.x, G.y, G.z}, A.w, A.h, &pfx, &pfy, &pte)) { fx = pfx; fy = pfy; }
    }
    float conf = 1.0f, weight;
    v3 c, nrm;
    {
        const float x0f = __builtin_floorf(fx), y0f = __builtin_floorf(fy);
        const float wx1 = fx - x0f, wy1 = fy - y0f;
        const float wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
        const int x0 = tap_origin(x0f), y0 = tap_origin(y0f);

        // ---- B: this frame's value (steps 2 and 3 of the upscale)
        const UpscaleGuide u = upscale_guide<TERMS>(o, TERMS != 0u && o != MISS_OBJECT, G, A.sigma_plane, A.sigma_position);
        Sums S;
        float bmax = upscale_gather<TERMS, true, true>(S, x0, y0, wx0, wx1, wy0, wy1, A.w, A.h, u, pl);
        weight = S.W;
        if (!(S.W > 0.0f)) {
            // tier 2: the plain bilinear weights over the usable taps, whatever they show
            weight = 0.0f;
            S = Sums();
            bmax = upscale_gather<TERMS, false, true>(S, x0, y0, wx0, wx1, wy0, wy1, A.w, A.h, u, pl);
        }
        const size_t F = (size_t)P * 3u;
        if (S.W > 0.0f) {
            c = v3{S.c[0] / S.W, S.c[1] / S.W, S.c[2] / S.W};
            nrm = v3{S.n[0] / S.W, S.n[1] / S.W, S.n[2] / S.W};
            if (pl.alpha) pl.out_alpha[P] = S.a / S.W;
            if (pl.background) {
#pragma unroll
                for (int i = 0; i < 3; i++) pl.out_background[F + i] = S.b[i] / S.W;
            }
            if (A.confidence) conf = bmax;
        } else {
            // tier 3: the low pixel this one falls into, verbatim; conf stays 1
            const uint32_t sx = min(X / A.factor, A.w - 1u), sy = min(Y / A.factor, A.h - 1u);
            const size_t q = (size_t)sx + (size_t)sy * A.w;
            c = v3{pl.color[3u * q], pl.color[3u * q + 1], pl.color[3u * q + 2]};
            nrm = v3{pl.normal[3u * q], pl.normal[3u * q + 1], pl.normal[3u * q + 2]};
            if (pl.alpha) pl.out_alpha[P] = pl.alpha[q];
            if (pl.background) {
#pragma unroll
                for (int i = 0; i < 3; i++) pl.out_background[F + i] = pl.background[3u * q + i];
            }
        }
        pl.out_normal[F] = nrm.x;
        pl.out_normal[F + 1] = nrm.y;
        pl.out_normal[F + 2] = nrm.z;
        if (pl.out_weight) pl.out_weight[P] = weight;
    }

    // ---- C: accumulate at the high size (steps 1 to 5 of the temporal accumulate, with conf in step 5)
    const bool cfin = fin(c.x) && fin(c.y) && fin(c.z);
    v3 out = c;
    float nn = cfin ? 1.0f : 0.0f;
    if (cfin && o != MISS_OBJECT && A.pA) {
        const TemporalScene& ts = A.ts;
        v3 Pp = v3{G.x, G.y, G.z};
        const float dt = ts.cur_time - ts.prev_time;
#pragma unroll
        for (uint32_t k = 0; k < RAYN_MAX_HITABLES; k++)
            if (k < ts.n_hitables && o == k && ts.hvel[k].w != 0.0f) Pp = v3{G.x - ts.hvel[k].x * dt, G.y - ts.hvel[k].y * dt, G.z - ts.hvel[k].z * dt};
        float hx, hy, te;
        if (project(ts.cam, ts.prev_time, Pp, A.W, A.H, &hx, &hy, &te)) {
            const float x0f = __builtin_floorf(hx), y0f = __builtin_floorf(hy);
            const float wx1 = hx - x0f, wx0 = 1.0f - wx1, wy1 = hy - y0f, wy0 = 1.0f - wy1;
            const int x0 = tap_origin(x0f), y0 = tap_origin(y0f);
            const float tol = A.depth_tolerance * te;
            float Wh = 0.0f, Sr = 0.0f, Sg = 0.0f, Sb = 0.0f, N = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t qx = (uint32_t)(x0 + (k & 1)), qy = (uint32_t)(y0 + (k >> 1));
                if (qx >= A.W || qy >= A.H) continue;
                const uint32_t q = qx + qy * A.W;
                const float4 a = A.pA[q];
                if (!history_tap_counts(a.w, q, o, te, tol, A.normal_min, nrm, A.pB, A.pN, A.pO)) continue;
                const float w = ((k & 1) ? wx1 : wx0) * ((k >> 1) ? wy1 : wy0);
                Wh += w;
                Sr += w * a.x;
                Sg += w * a.y;
                Sb += w * a.z;
                N += w * a.w;
            }
            if (Wh > 0.0f) {
                const Blend b = blend_history(c, v3{Sr / Wh, Sg / Wh, Sb / Wh}, N / Wh, conf, A.max_history);
                if (b.ok) { out = b.out; nn = b.n1; }
            }
        }
    }
    const size_t F = (size_t)P * 3u;
    pl.out_color[F] = out.x;
    pl.out_color[F + 1] = out.y;
    pl.out_color[F + 2] = out.z;
    A.nA[P] = make_float4(out.x, out.y, out.z, nn);
    A.nB[P] = G;
    A.nN[P] = make_float4(nrm.x, nrm.y, nrm.z, 0.0f);
    A.nO[P] = o;
}

} // namespace

const char* temporal_upscale_check_args(const rayn_frame_params* p, const rayn_upscale_params* up, const rayn_temporal_params* tp,
                                        const rayn_temporal_upscale_params* sp, const rayn_camera* low_camera, const rayn_camera* prev_camera,
                                        const TemporalUpscaleCall& c) {
    const UpscalePlanes& pl = c.pl;
    if (!p) return "null frame params";
    // the upscale's own rules: the factor, both sizes, the sigmas, the planes, the G-buffers and every overlap among them
    if (const char* why = upscale_check_args(p->width, p->height, up, pl)) return why;
    // the temporal accumulate's, at the high size
    if (const char* why = check_temporal_params(tp)) return why;
    if (!sp) return "null temporal upscale params";
    if (sp->confidence > 1u) return "confidence must be 0 (off) or 1 (on)";
    if (!pl.normal || !c.new_history) return "null buffer"; // the accumulate needs the WorldNormal
    if (c.prev_history && !prev_camera) return "a previous history needs the previous camera";
    if ((prev_camera && prev_camera->kind > RAYN_CAM_ORTHOGRAPHIC) || (low_camera && low_camera->kind > RAYN_CAM_ORTHOGRAPHIC)) return "unknown camera kind";
    const uint32_t W = p->width * up->factor, H = p->height * up->factor;
    const size_t need = temporal_history_bytes(W, H);
    if (c.history_bytes < need) return "history smaller than rayn_temporal_history_bytes(width, height)";
    if ((uintptr_t)c.new_history % 16u || (uintptr_t)c.prev_history % 16u) return "history not 16-byte aligned";
    if (overlap(c.new_history, need, c.prev_history, need)) return "the new history must not alias the previous one";
    const size_t n = (size_t)p->width * p->height, N = (size_t)W * H;
    const UpscaleSpans us = upscale_spans(pl, n, N);
    const Span prev = {c.prev_history, need}, next = {c.new_history, need};
    if (first_overlap(&next, 1, us.in, 8)) return "an output must not alias an input";
    for (int i = 0; i < 5; i++) {
        if (first_overlap(us.out + i, 1, &prev, 1)) return "an output must not alias an input";
        if (first_overlap(us.out + i, 1, &next, 1)) return i == 0 ? "d_out_color must not alias the new history" : "the outputs must not alias each other";
    }
    return nullptr;
}

void launch_temporal_upscale(hipStream_t s, uint32_t width, uint32_t height, const rayn_upscale_params& up, const rayn_temporal_params& tp,
                             uint32_t confidence, const DCamera* low_cam, const TemporalScene& ts, const TemporalUpscaleCall& c) {
    TUArgs A;
    A.w = width;
    A.h = height;
    A.W = width * up.factor;
    A.H = height * up.factor;
    A.tiles_x = (A.W + 15u) / 16u;
    A.factor = up.factor;
    A.confidence = confidence;
    A.have_low_cam = low_cam ? 1u : 0u;
    A.sigma_plane = up.sigma_plane;
    A.sigma_position = up.sigma_position;
    A.max_history = (float)tp.max_history;
    A.depth_tolerance = tp.depth_tolerance;
    A.normal_min = tp.normal_min;
    A.pl = c.pl;
    const size_t N = (size_t)A.W * A.H;
    const float4* pA = (const float4*)c.prev_history;
    float4* nA = (float4*)c.new_history;
    A.pA = pA;
    A.pB = pA ? pA + N : nullptr;
    A.pN = pA ? pA + 2u * N : nullptr;
    A.pO = pA ? (const uint32_t*)(pA + 3u * N) : nullptr;
    A.nA = nA;
    A.nB = nA + N;
    A.nN = nA + 2u * N;
    A.nO = (uint32_t*)(nA + 3u * N);
    A.low_cam = low_cam ? *low_cam : ts.cam;
    A.ts = ts;
    const uint32_t terms = (up.sigma_plane != 0.0f ? UPSCALE_PLANE : 0u) | (up.sigma_position != 0.0f ? UPSCALE_POSITION : 0u);
    const dim3 grid(A.tiles_x * ((A.H + 15u) / 16u)), block(16, 16);
    with_terms<2>(terms, [&](auto T) { hipLaunchKernelGGL((k_temporal_upscale<decltype(T)::value>), grid, block, 0, s, A); });
}

} // namespace rayn
