// post_device.h — the device-side definitions the post-process kernels share (denoise.hip, denoise_variance.hip, denoise_temporal.hip,
// temporal.hip, upscale.hip, temporal_upscale.hip, display.hip): each exists once, here, so that two kernels that the definitions in
// include/rayn_hip.h call equal are equal by construction.  Everything is f32, built with -ffp-contract=off and IEEE '/' and sqrtf, and
// inlines into its caller.  Host-side checks: post_checks.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rayn_detmath_fast.h"
#include "../../include/rayn_hip.h"
#include "kernels.h"
#include "upscale.h"

namespace rayn {

// the object index of a G-buffer pixel whose primary ray hit nothing
constexpr uint32_t MISS_OBJECT = 0xFFFFFFFFu;

// finite3 is spelled with the builtin and not as fin(x) && fin(y) && fin(z): the compiler turns the two spellings into different (equivalent)
// instruction sequences, and the places that test three components one by one (the accumulates' own colour, blend_history) keep theirs.
__device__ inline bool fin(float v) { return __builtin_isfinite(v); }
__device__ inline bool finite3(float x, float y, float z) { return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z); }
__device__ inline float luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
__device__ inline float quiet_nan() { return __uint_as_float(0x7FC00000u); }

// ---- vectors, as the accumulate's definition writes them ---------------------------------------------------------------------------
struct v3 { float x, y, z; };
__device__ inline v3 sub3(v3 a, v3 b) { return v3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline v3 scale3(v3 a, float s) { return v3{a.x * s, a.y * s, a.z * s}; }
__device__ inline float dot3(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ inline v3 cross3(v3 a, v3 b) { return v3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ inline v3 nz3(v3 a) { return scale3(a, 1.0f / __builtin_sqrtf(dot3(a, a))); }
// a camera closure at time t: base + vel * t when animated, else base
__device__ inline v3 closure3(f3 base, f3 vel, bool on, float t) {
    return on ? v3{base.x + vel.x * t, base.y + vel.y * t, base.z + vel.z * t} : v3{base.x, base.y, base.z};
}

// ---- the temporal accumulate's steps 3 to 5 ----------------------------------------------------------------------------------------
// Step 3: the point Pp through the camera at the closure time ts onto a width x height image, both camera families.  False for a
// rejected projection (behind the camera, or a position that is not finite).
__device__ inline bool project(const DCamera& cam, float ts, v3 Pp, uint32_t width, uint32_t height, float* fx, float* fy, float* te) {
    const v3 o = closure3(cam.origin, cam.origin_vel, cam.animated & 1u, ts);
    const v3 at = closure3(cam.at, cam.at_vel, cam.animated & 2u, ts);
    const v3 up = closure3(cam.up, cam.up_vel, cam.animated & 4u, ts);
    float uvx, uvy;
    bool ok;
    if (cam.kind == RAYN_CAM_ORTHOGRAPHIC) {
        const v3 w = nz3(sub3(at, o)), u = nz3(cross3(w, up)), v = cross3(u, w);
        const v3 ll = sub3(sub3(o, scale3(u, cam.half_w)), scale3(v, cam.half_h));
        const v3 q = sub3(Pp, ll);
        uvx = dot3(q, u) / cam.full_w;
        uvy = dot3(q, v) / cam.full_h;
        *te = dot3(q, w);
        ok = *te > 0.0f;
    } else {
        const v3 w = nz3(sub3(o, at)), u = nz3(cross3(up, w)), v = cross3(w, u);
        const v3 q = sub3(Pp, o);
        const float zc = -dot3(q, w);
        ok = zc > 0.0f;
        uvx = (dot3(q, u) / (zc * cam.half_w) + 1.0f) * 0.5f;
        uvy = (dot3(q, v) / (zc * cam.half_h) + 1.0f) * 0.5f;
        *te = __builtin_sqrtf(dot3(q, q));
    }
    *fx = uvx * (float)width - 0.5f;
    *fy = uvy * (float)height - 0.5f;
    return ok && fin(*fx) && fin(*fy);
}

// Step 4's predicate on the history tap q (a pixel of the image) whose length n_tap the caller has read with the colour: n_tap >= 1, the
// pixel's object, a depth within tol = depth_tolerance * te of te and, with normal_min > -1, a normal within normal_min of nrm; every
// comparison is false for a NaN.  A test is only reached - its plane only read - when the ones before it hold.
__device__ inline bool history_tap_counts(float n_tap, uint32_t q, uint32_t obj, float te, float tol, float normal_min, v3 nrm,
                                          const float4* __restrict__ pB, const float4* __restrict__ pN, const uint32_t* __restrict__ pO) {
    if (!(n_tap >= 1.0f)) return false;
    if (pO[q] != obj) return false;
    if (!(__builtin_fabsf(pB[q].w - te) <= tol)) return false;
    if (normal_min > -1.0f) {
        const float4 nq = pN[q];
        if (!(dot3(nrm, v3{nq.x, nq.y, nq.z}) >= normal_min)) return false;
    }
    return true;
}

// Step 5: the colour c blended into the resampled history (h, nh) with the confidence conf (1 in the plain accumulate): n' = fminf(nh +
// conf, max_history), a = conf / n', out = h + a * (c - h).  ok is false - the pixel resets - when out has a non-finite component.
struct Blend {
    v3 out;
    float n1, a;
    bool ok;
};
__device__ inline Blend blend_history(v3 c, v3 h, float nh, float conf, float max_history) {
    const float n1 = __builtin_fminf(nh + conf, max_history);
    const float a = conf / n1;
    const float dr = c.x - h.x, dg = c.y - h.y, db = c.z - h.z;
    const v3 b = v3{h.x + a * dr, h.y + a * dg, h.z + a * db};
    return Blend{b, n1, a, fin(b.x) && fin(b.y) && fin(b.z)};
}

// ---- the upscale's footprint (steps 2 and 3 of rayn_hip_upscale_device) --------------------------------------------------------------
constexpr uint32_t UPSCALE_PLANE = 1u, UPSCALE_POSITION = 2u; // the TERMS of the guided tier

// the sums of one weight set: every one starts at -0.0f, the identity of + for both zeros, so that a single tap of weight 1 gives the
// tap's own bits back (0.0f + -0.0f would be +0.0f)
struct Sums {
    float W = -0.0f, c[3] = {-0.0f, -0.0f, -0.0f}, a = -0.0f, b[3] = {-0.0f, -0.0f, -0.0f}, n[3] = {-0.0f, -0.0f, -0.0f};
};

// NORMAL: the entry requires the WorldNormal plane (rayn_hip_temporal_upscale_device), so pl.normal is not tested; else it is optional
// like Alpha and Background (rayn_hip_upscale_device).
template <bool NORMAL>
__device__ inline void add_tap(Sums& S, float g, size_t q, float cr, float cg, float cb, const UpscalePlanes& pl) {
    S.W += g;
    S.c[0] += g * cr;
    S.c[1] += g * cg;
    S.c[2] += g * cb;
    if (pl.alpha) S.a += g * pl.alpha[q];
    if (pl.background) {
#pragma unroll
        for (int i = 0; i < 3; i++) S.b[i] += g * pl.background[3u * q + i];
    }
    if (NORMAL || pl.normal) {
#pragma unroll
        for (int i = 0; i < 3; i++) S.n[i] += g * pl.normal[3u * q + i];
    }
}

// what the guided tier knows of the high pixel: its object, its G-buffer record G = (P, t) and the terms' constants
struct UpscaleGuide {
    uint32_t o;
    bool on; // a hit pixel with a term on; else the guided weight is the bilinear one: e = 0 and dm_expf(-0) = 1
    float4 G;
    float inv_t, kp, ks;
};
template <uint32_t TERMS>
__device__ inline UpscaleGuide upscale_guide(uint32_t o, bool on, float4 G, float sigma_plane, float sigma_position) {
    UpscaleGuide u;
    u.o = o;
    u.on = on;
    u.G = G;
    u.inv_t = 1.0f / (G.w + 1e-8f);
    u.kp = (TERMS & UPSCALE_PLANE) ? 1.0f / (sigma_plane * sigma_plane) : 0.0f;
    u.ks = (TERMS & UPSCALE_POSITION) ? 1.0f / (sigma_position * sigma_position) : 0.0f;
    return u;
}

// One tier's gather over the four taps (x0, y0) .. (x0 + 1, y0 + 1) of a w x h low film, in that order, into S.  A tap is used when it
// is inside, its bilinear weight b is > 0 and its colour is finite.  TIER1: the guided tier - the tap must also show the pixel's object,
// and its weight is b * expf(-e) of the TERMS that are on (a NaN weight skips it); else tier 2, the plain b whatever the tap shows.
// NORMAL: add_tap's.  Returns the largest b among the taps that were added (0: none).
template <uint32_t TERMS, bool TIER1, bool NORMAL>
__device__ inline float upscale_gather(Sums& S, int x0, int y0, float wx0, float wx1, float wy0, float wy1, uint32_t w, uint32_t h,
                                       const UpscaleGuide& u, const UpscalePlanes& pl) {
    float bmax = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        // unsigned wrap: a negative coordinate becomes >= w (w < 2^31)
        const uint32_t qx = (uint32_t)(x0 + (k & 1)), qy = (uint32_t)(y0 + (k >> 1));
        if (qx >= w || qy >= h) continue;
        const float b = ((k & 1) ? wx1 : wx0) * ((k >> 1) ? wy1 : wy0);
        if (!(b > 0.0f)) continue;
        const size_t q = (size_t)qx + (size_t)qy * w;
        if (TIER1 && pl.low_object[q] != u.o) continue;
        const float cr = pl.color[3u * q], cg = pl.color[3u * q + 1], cb = pl.color[3u * q + 2];
        if (!finite3(cr, cg, cb)) continue;
        float g = b;
        if (TIER1 && u.on) {
            const float4 Q = ((const float4*)pl.low_records)[q];
            const float dx = u.G.x - Q.x, dy = u.G.y - Q.y, dz = u.G.z - Q.z;
            float e = 0.0f;
            if (TERMS & UPSCALE_PLANE) {
                const float nx = pl.normal[3u * q], ny = pl.normal[3u * q + 1], nz = pl.normal[3u * q + 2];
                const float dpl = fabsf((nx * dx + ny * dy) + nz * dz) * u.inv_t;
                e = (dpl * dpl) * u.kp;
            }
            if (TERMS & UPSCALE_POSITION) {
                const float dps = ((dx * dx + dy * dy) + dz * dz) * (u.inv_t * u.inv_t);
                e = (TERMS & UPSCALE_PLANE) ? e + dps * u.ks : dps * u.ks;
            }
            g = b * dmf_expf(-e);
            if (g != g) continue;
        }
        add_tap<NORMAL>(S, g, q, cr, cg, cb, pl);
        bmax = __builtin_fmaxf(bmax, b);
    }
    return bmax;
}

// ---- the variance pack kernels' guide record ------------------------------------------------------------------------------------------
// b[p] = (nx, ny, nz, alpha) of film pixel p, whose normal starts at float f = 3 p of its plane (the index the caller read the colour
// with).  A guide that is switched off is not read (its pointer is null) and reads as 0; b is null when both are off.
__device__ inline void write_guide_record(float4* b, uint32_t p, size_t f, const float* normal, const float* alpha) {
    if (!b) return;
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (normal) { nx = normal[f]; ny = normal[f + 1]; nz = normal[f + 2]; }
    b[p] = make_float4(nx, ny, nz, alpha ? alpha[p] : 0.0f);
}

} // namespace rayn
