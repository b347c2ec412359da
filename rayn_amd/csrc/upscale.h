// upscale.h — host-visible side of upscale.hip: guided upscaling of a low-resolution film to s times its size with the primary-hit
// G-buffers of both resolutions as the guide (rayn_hip_upscale_device; joint bilateral upsampling, Kopf et al., SIGGRAPH 2007).  An
// extension: rayn renders at one resolution.  include/rayn_hip.h holds the definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rayn_hip.h"

namespace rayn {

// The planes of one call: the low film (width x height) and its G-buffer, the high G-buffer (factor * width x factor * height) and the
// outputs.  alpha / background / normal are null together with their outputs when the film lacks the channel; out_weight may be null.
struct UpscalePlanes {
    const float *color, *alpha, *background, *normal;
    const void* low_records;
    const uint32_t* low_object;
    const void* high_records;
    const uint32_t* high_object;
    float *out_color, *out_alpha, *out_background, *out_normal, *out_weight;
};
// nullptr when the arguments are valid, else the reason (the entry's last error text).  Checks everything but ctx and stream.
const char* upscale_check_args(uint32_t width, uint32_t height, const rayn_upscale_params* up, const UpscalePlanes& pl);
// Enqueue the kernel on stream s (arguments checked by upscale_check_args).
void launch_upscale(hipStream_t s, uint32_t width, uint32_t height, const rayn_upscale_params& up, const UpscalePlanes& pl);

} // namespace rayn
