// denoise_variance.h — host-visible side of denoise_variance.hip: the a-trous filter of the film's Color channel whose luminance
// edge-stop is scaled by the local standard deviation a progressive render measured (the spatial half of SVGF, Schied et al., HPG
// 2017).  An extension: rayn has neither a denoiser nor a progressive render.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rayn_hip.h"

namespace rayn {

// Device scratch of launch_denoise_variance: two (colour, variance) record planes (ping-pong) and one (normal, alpha) record plane,
// 16 bytes per pixel each.  0 for a size the entry rejects (zero, or width * height >= 2^31).
size_t denoise_variance_scratch_bytes(uint32_t width, uint32_t height);
// nullptr when the arguments are valid, else the reason (the entry's last error text).  Checks everything but the stream.
const char* denoise_variance_check_args(const rayn_frame_params* p, uint32_t iterations, float sigma_luminance, float sigma_normal,
                                        float sigma_alpha, const float* color, const float* alpha, const float* normal, const void* state,
                                        size_t state_bytes, const float* out_color, const float* out_variance, const void* scratch,
                                        size_t scratch_bytes);
// Enqueue the pack kernel and the `iterations` passes on stream s (arguments checked by denoise_variance_check_args).
void launch_denoise_variance(hipStream_t s, const rayn_frame_params& p, uint32_t iterations, float sigma_luminance, float sigma_normal,
                             float sigma_alpha, const float* color, const float* alpha, const float* normal, const void* state, float* out_color,
                             float* out_variance, void* scratch);


// ---- what the entries that pack a variance of their own share (denoise_temporal.hip) ----------------------------------------------------
// which of k_vatrous's terms are on: a sigma of 0 switches its term off
constexpr uint32_t VATROUS_LUMINANCE = 1u, VATROUS_NORMAL = 2u, VATROUS_ALPHA = 4u;
inline uint32_t vatrous_terms(float sigma_luminance, float sigma_normal, float sigma_alpha) {
    return (sigma_luminance != 0.0f ? VATROUS_LUMINANCE : 0u) | (sigma_normal != 0.0f ? VATROUS_NORMAL : 0u) | (sigma_alpha != 0.0f ? VATROUS_ALPHA : 0u);
}
// the (normal, alpha) record plane of the scratch, nullptr when both guides are off (it is then neither written nor read)
inline float4* vatrous_guides(uint32_t terms, uint32_t width, uint32_t height, void* scratch) {
    return (terms & (VATROUS_NORMAL | VATROUS_ALPHA)) ? (float4*)scratch + 2u * ((size_t)width * height) : nullptr;
}
// Enqueue the `iterations` passes on records a pack kernel has written: A = (r, g, b, v or NaN) in plane 0 of the scratch, B = (nx, ny,
// nz, alpha) in vatrous_guides.  The last pass writes out_color and, when given, out_variance.  With `history` (a temporal history, plane A
// first) and feedback != 0, pass 0 also blends its colour into plane A's (r, g, b) with that strength; the outputs do not depend on it.
void launch_vatrous_passes(hipStream_t s, uint32_t width, uint32_t height, uint32_t iterations, float sigma_luminance, float sigma_normal,
                           float sigma_alpha, float* out_color, float* out_variance, void* scratch, void* history = nullptr, float feedback = 0.0f);

// ---- the same filter on a temporally accumulated colour (denoise_temporal.hip; rayn_hip_denoise_temporal_variance_device) -----------------
const char* denoise_temporal_check_args(uint32_t width, uint32_t height, uint32_t iterations, float sigma_luminance, float sigma_normal,
                                        float sigma_alpha, const float* color, const float* alpha, const float* normal, const uint32_t* g_object,
                                        const void* history, size_t history_bytes, const void* moments, size_t moments_bytes,
                                        const float* out_color, const float* out_variance, const void* scratch, size_t scratch_bytes);
void launch_denoise_temporal_variance(hipStream_t s, uint32_t width, uint32_t height, uint32_t iterations, float sigma_luminance,
                                      float sigma_normal, float sigma_alpha, const float* color, const float* alpha, const float* normal,
                                      const uint32_t* g_object, const void* history, const void* moments, float* out_color, float* out_variance,
                                      void* scratch);
// rayn_hip_denoise_temporal_variance_feedback_device: the checks above, the strength, and the history as an output that overlaps nothing
const char* denoise_temporal_feedback_check_args(uint32_t width, uint32_t height, uint32_t iterations, float sigma_luminance, float sigma_normal,
                                                 float sigma_alpha, const float* color, const float* alpha, const float* normal,
                                                 const uint32_t* g_object, const void* history, size_t history_bytes, const void* moments,
                                                 size_t moments_bytes, const float* out_color, const float* out_variance, const void* scratch,
                                                 size_t scratch_bytes, float feedback);
// the same kernels; with feedback != 0 pass 0 writes plane A's colour of `history` (feedback == 0: nothing writes it)
void launch_denoise_temporal_variance_feedback(hipStream_t s, uint32_t width, uint32_t height, uint32_t iterations, float sigma_luminance,
                                               float sigma_normal, float sigma_alpha, const float* color, const float* alpha, const float* normal,
                                               const uint32_t* g_object, void* history, const void* moments, float* out_color, float* out_variance,
                                               void* scratch, float feedback);

} // namespace rayn
