// denoise.h — host-visible side of denoise.hip: the edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010) of the film's
// Color channel, guided by WorldNormal and Alpha.  An extension: rayn has no denoiser.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rayn {

// Device scratch of launch_denoise: two colour + alpha record planes (ping-pong) and one normal record plane, 16 bytes per pixel
// each.  0 for a size the entry rejects (zero, or width * height >= 2^31).
size_t denoise_scratch_bytes(uint32_t width, uint32_t height);
// nullptr when the arguments are valid, else the reason (the entry's last error text).  Checks everything but the stream.
const char* denoise_check_args(uint32_t width, uint32_t height, uint32_t iterations, float sigma_color, float sigma_normal, float sigma_alpha,
                               const float* color, const float* alpha, const float* normal, const float* out_color, const void* scratch,
                               size_t scratch_bytes);
// Enqueue the pack kernel and the `iterations` a-trous passes on stream s (arguments checked by denoise_check_args).
void launch_denoise(hipStream_t s, uint32_t width, uint32_t height, uint32_t iterations, float sigma_color, float sigma_normal, float sigma_alpha,
                    const float* color, const float* alpha, const float* normal, float* out_color, void* scratch);

} // namespace rayn
