// temporal_upscale.h — host-visible side of temporal_upscale.hip: temporal supersampling (rayn_hip_temporal_upscale_device), the guided
// upscaling of a low film fused with the temporal accumulation at the high resolution, so that low frames rendered with different
// sub-pixel offsets meet in one full-size history (temporal upsampling as in TAAU / FSR2).  An extension: rayn renders at one resolution
// and every frame on its own.  include/rayn_hip.h holds the definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rayn_hip.h"
#include "temporal.h"
#include "upscale.h"

namespace rayn {

// What one call works on.  pl: the low film (width x height), the G-buffers of both sizes and the outputs of the high size, where
// out_color receives the ACCUMULATED colour and the other planes this frame's upscaled values; normal / out_normal are required.
struct TemporalUpscaleCall {
    UpscalePlanes pl;
    const void* prev_history; // null: no previous history
    void* new_history;
    size_t history_bytes;     // of EACH history, at the HIGH size
};
// nullptr when the arguments are valid, else the reason (the entry's last error text).  Checks everything but ctx, world and stream.
const char* temporal_upscale_check_args(const rayn_frame_params* p, const rayn_upscale_params* up, const rayn_temporal_params* tp,
                                        const rayn_temporal_upscale_params* sp, const rayn_camera* low_camera, const rayn_camera* prev_camera,
                                        const TemporalUpscaleCall& c);
// Enqueue the kernel on stream s (arguments checked by temporal_upscale_check_args).  low_cam: null = the default footprint everywhere;
// ts: the previous camera (looked at only with a previous history), both time_starts and the hitable velocities.
void launch_temporal_upscale(hipStream_t s, uint32_t width, uint32_t height, const rayn_upscale_params& up, const rayn_temporal_params& tp,
                             uint32_t confidence, const DCamera* low_cam, const TemporalScene& ts, const TemporalUpscaleCall& c);

} // namespace rayn
