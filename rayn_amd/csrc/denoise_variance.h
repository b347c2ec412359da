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

} // namespace rayn
