// interpolate.h — host-visible side of interpolate.hip: a frame of a sequence generated from two rendered key frames and its own
// primary-hit G-buffer (rayn_hip_interpolate_device), motion-compensated by projecting every pixel's hit into both keys.  An extension:
// rayn renders every frame.  include/rayn_hip.h holds the definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rayn_hip.h"
#include "kernels.h"

namespace rayn {

// One key as the kernel takes it: its planes, its G-buffer, its camera (build_camera) and its time_start, by value
struct InterpolateKey {
    const float *color, *alpha, *background, *normal;
    const void* records;
    const uint32_t* object;
    DCamera cam;
    float time;
};
// One call: both keys, the generated frame's G-buffer and time, the outputs and the uploaded world's hitable velocities.  alpha /
// background / normal are null in both keys and the output together; out_source may be null.
struct InterpolateCall {
    uint32_t width, height;
    float depth_tolerance, time;
    InterpolateKey a, b;
    const void* records;
    const uint32_t* object;
    float *out_color, *out_alpha, *out_background, *out_normal;
    uint32_t* out_source;
    uint32_t n_hitables, _pad;
    float4 hvel[RAYN_MAX_HITABLES]; // center_vel, w != 0: animated
};
// nullptr when the arguments are valid, else the reason (the entry's last error text).  Checks everything but ctx, world, the camera
// kinds and the stream.
const char* interpolate_check_args(const rayn_frame_params* p, const rayn_interpolate_params* ip, const rayn_interpolate_key* key_a,
                                   const rayn_interpolate_key* key_b, const void* g_records, const uint32_t* g_object, const float* out_color,
                                   const float* out_alpha, const float* out_background, const float* out_normal, const uint32_t* out_source);
// Enqueue the kernel on stream s (arguments checked by interpolate_check_args).
void launch_interpolate(hipStream_t s, const InterpolateCall& c);

} // namespace rayn
