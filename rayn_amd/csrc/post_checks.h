// post_checks.h — the host-side checks and launch helpers the post-process entries share (the *_check_args and launch_* of denoise.hip,
// denoise_variance.hip, denoise_temporal.hip, temporal.hip, upscale.hip, temporal_upscale.hip, display.hip and their glue in
// rayn_hip.hip).  A check returns nullptr when its arguments are valid, else the entry's error text.  Device side: post_device.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>

#include "../../include/rayn_hip.h"
#include "temporal.h"
#include "upscale.h"

namespace rayn {

// the size every post-process entry accepts: not empty, and pixel indices that fit 32 bits
inline const char* check_size(uint32_t width, uint32_t height) {
    if (!width || !height) return "zero-sized image";
    if ((uint64_t)width * height >= ((uint64_t)1 << 31)) return "image larger than 2^31 pixels unsupported (32-bit pixel indices)";
    return nullptr;
}

// a sigma of the a-trous and upscale entries: 0 = off; else finite and in [2^-30, 2^30]
inline bool sigma_ok(float sigma) { return sigma == 0.0f || (sigma >= 0x1p-30f && sigma <= 0x1p30f); }

// ---- aliasing ------------------------------------------------------------------------------------------------------------------------
// do [a, a + na) and [b, b + nb) share a byte?  A null pointer is an absent buffer and overlaps nothing.
inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + nb && y < x + na;
}
struct Span {
    const void* p;
    size_t bytes;
};
// The first pair (a[i], b[j]) that overlaps, a outer and b inner; false when none does.  ia / ib (null-able) receive i and j.
inline bool first_overlap(const Span* a, int na, const Span* b, int nb, int* ia = nullptr, int* ib = nullptr) {
    for (int i = 0; i < na; i++)
        for (int j = 0; j < nb; j++)
            if (overlap(a[i].p, a[i].bytes, b[j].p, b[j].bytes)) {
                if (ia) *ia = i;
                if (ib) *ib = j;
                return true;
            }
    return false;
}
// the inputs and outputs of an upscale of n low to N high pixels
struct UpscaleSpans {
    Span in[8], out[5];
};
inline UpscaleSpans upscale_spans(const UpscalePlanes& pl, size_t n, size_t N) {
    return UpscaleSpans{{{pl.color, 12u * n}, {pl.alpha, 4u * n}, {pl.background, 12u * n}, {pl.normal, 12u * n}, {pl.low_records, 16u * n},
                         {pl.low_object, 4u * n}, {pl.high_records, 16u * N}, {pl.high_object, 4u * N}},
                        {{pl.out_color, 12u * N}, {pl.out_alpha, 4u * N}, {pl.out_background, 12u * N}, {pl.out_normal, 12u * N}, {pl.out_weight, 4u * N}}};
}

// ---- parameter blocks ----------------------------------------------------------------------------------------------------------------
inline const char* check_temporal_params(const rayn_temporal_params* tp) {
    if (!tp) return "null temporal params";
    if (tp->max_history < 1 || tp->max_history > 65536) return "max_history must be in 1..65536";
    if (!(tp->depth_tolerance >= 0.0f) || !(tp->depth_tolerance <= 3.40282347e+38f)) return "depth_tolerance must be finite and >= 0";
    if (!(tp->normal_min >= -1.0f && tp->normal_min <= 1.0f)) return "normal_min must be in [-1, 1]";
    return nullptr;
}

// What the three a-trous entries ask of their filter arguments, in their order: the iterations, the three sigmas (bad_first: the text for
// the first one, sigma_color or sigma_luminance), the entry's own required buffers (buffers: all present), the guides of the terms that
// are on.
inline const char* check_atrous_params(uint32_t iterations, float sigma_first, const char* bad_first, float sigma_normal, float sigma_alpha, bool buffers,
                                       const float* normal, const float* alpha) {
    if (iterations < 1 || iterations > 8) return "iterations must be in 1..8";
    if (!sigma_ok(sigma_first)) return bad_first;
    if (!sigma_ok(sigma_normal)) return "sigma_normal must be 0 (off) or in [2^-30, 2^30]";
    if (!sigma_ok(sigma_alpha)) return "sigma_alpha must be 0 (off) or in [2^-30, 2^30]";
    if (!buffers) return "null buffer";
    if (!normal && sigma_normal != 0.0f) return "null normal guide with sigma_normal != 0";
    if (!alpha && sigma_alpha != 0.0f) return "null alpha guide with sigma_alpha != 0";
    return nullptr;
}

// Device scratch of an a-trous entry: three planes of 16-byte records; 0 for a size the entries reject.
inline size_t atrous_scratch_bytes(uint32_t width, uint32_t height) {
    if (check_size(width, height)) return 0;
    return (size_t)(3u * sizeof(float4) * (uint64_t)width * height);
}

// ---- launch helpers ------------------------------------------------------------------------------------------------------------------
// ts (its camera aside): both time_starts and the velocities of the uploaded world's hitables
inline void fill_temporal_scene(TemporalScene* ts, const rayn_world_desc& w, float prev_time_start, float cur_time_start) {
    ts->prev_time = prev_time_start;
    ts->cur_time = cur_time_start;
    ts->n_hitables = w.n_hitables < RAYN_MAX_HITABLES ? w.n_hitables : RAYN_MAX_HITABLES;
    for (uint32_t i = 0; i < ts->n_hitables; i++)
        ts->hvel[i] = make_float4(w.hitables[i].center_vel.x, w.hitables[i].center_vel.y, w.hitables[i].center_vel.z, w.hitables[i].animated ? 1.0f : 0.0f);
}

// Calls f(std::integral_constant<uint32_t, T>()) with T = terms, a set of N_TERMS one-bit terms (terms < 2^N_TERMS), so that f can name
// the kernel instantiated for exactly that set: [&](auto T) { launch(k<decltype(T)::value>) }.
template <uint32_t N_TERMS, uint32_t T = 0, class F>
inline void with_terms(uint32_t terms, F&& f) {
    if constexpr (T + 1u == (1u << N_TERMS)) f(std::integral_constant<uint32_t, T>());
    else if (terms == T) f(std::integral_constant<uint32_t, T>());
    else with_terms<N_TERMS, T + 1u>(terms, f);
}

} // namespace rayn
