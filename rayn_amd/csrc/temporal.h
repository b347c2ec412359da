// temporal.h — host-visible side of temporal.hip: the primary-hit G-buffer pass (rayn_hip_gbuffer_device) and the temporal accumulation of
// the film's Color channel by reprojection (rayn_hip_temporal_accumulate_device), the temporal half of SVGF (Schied et al., HPG 2017).
// Extensions: rayn has neither.  include/rayn_hip.h holds the definitions.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rayn_hip.h"
#include "kernels.h"

namespace rayn {

// ---- G-buffer ----------------------------------------------------------------------------------------------------------------------
// The caller's scratch as the pass carves it: a pool-shaped ray store (geo0, geo1, col1 of npad = width * height rounded up to whole
// 64-slot groups), the identity queue, the per-entry object bytes, a control block and the (unused: no counting) evaluation counters.
struct GbufScratch {
    uint32_t n, npad;
    Pool pool;          // geo0, geo1, col1 set; the rest null (the extend kernels touch nothing else)
    uint32_t* q;        // [npad]
    uint8_t* ent_obj;   // [npad]
    DCtl* ctl;
    unsigned long long* evals; // [16]
};
// 53 bytes per padded slot + 384; 0 for a size the entry rejects (zero, or width * height >= 2^31)
size_t gbuffer_scratch_bytes(uint32_t width, uint32_t height);
GbufScratch gbuffer_scratch(uint32_t width, uint32_t height, void* scratch);
// nullptr when the arguments are valid, else the reason (the entry's last error text).  Checks everything but ctx, world and stream.
const char* gbuffer_check_args(const rayn_frame_params* p, const void* out_records, const uint32_t* out_object, const void* scratch, size_t scratch_bytes);
// the last kernel of the pass: pool + hit -> (P, t) records and object indices
void launch_gbuffer_finish(hipStream_t s, const GbufScratch& g, void* out_records, uint32_t* out_object);

// ---- temporal accumulate -----------------------------------------------------------------------------------------------------------
// One history of a width x height film: plane A (r, g, b, n) | plane B (Px, Py, Pz, t) | WorldNormal (nx, ny, nz, 0) | object u32,
// 52 bytes per pixel, in that order; 0 for a size the entry rejects.
size_t temporal_history_bytes(uint32_t width, uint32_t height);
// what the kernel needs of the previous camera and of the uploaded world's hitables, by value
struct TemporalScene {
    DCamera cam;          // the PREVIOUS frame's camera (build_camera)
    float prev_time, cur_time;
    uint32_t n_hitables, _pad;
    float4 hvel[RAYN_MAX_HITABLES]; // center_vel, w != 0: animated
};
const char* temporal_check_args(const rayn_frame_params* p, const rayn_temporal_params* tp, const rayn_camera* prev_camera, const float* color,
                                const float* normal, const void* g_records, const uint32_t* g_object, const void* prev_history,
                                const void* new_history, size_t history_bytes, const float* out_color);
// The luminance moments beside a history: a float2 (m1, m2) per pixel in film pixel order, 8 bytes per pixel; 0 for a size the entry rejects.
size_t temporal_moments_bytes(uint32_t width, uint32_t height);
// what rayn_hip_temporal_accumulate_moments_device checks on top of temporal_check_args (call that first: p is valid here)
const char* temporal_moments_check_args(const rayn_frame_params* p, const float* color, const float* normal, const void* g_records,
                                        const uint32_t* g_object, const void* prev_history, const void* new_history, const void* prev_moments,
                                        const void* new_moments, size_t moments_bytes, const float* out_color);
// what rayn_hip_temporal_accumulate_resample_device checks on top of the two above
const char* temporal_resample_check_args(const rayn_temporal_resample_params* rp);
// new_moments == nullptr: the plain accumulate (k_temporal_accumulate<false, *>); else the moments are carried too.  resample: 0 the
// bilinear step 4 (<*, 0>, the kernels of the two older entries), 1 Catmull-Rom over a full 4x4 footprint (<*, 1>).
void launch_temporal_accumulate(hipStream_t s, uint32_t width, uint32_t height, const rayn_temporal_params& tp, const TemporalScene& ts,
                                const float* color, const float* normal, const void* g_records, const uint32_t* g_object,
                                const void* prev_history, void* new_history, float* out_color, const void* prev_moments = nullptr,
                                void* new_moments = nullptr, uint32_t resample = 0);

} // namespace rayn

// the ray kernel of the G-buffer pass calls camera_ray (device_core.h) and is therefore built once per mul_add policy, like kernels.hip
namespace rayn_p0 { void launch_gbuffer_rays(hipStream_t s, const rayn::DScene* sc, const rayn::GbufScratch& g); }
namespace rayn_p1 { void launch_gbuffer_rays(hipStream_t s, const rayn::DScene* sc, const rayn::GbufScratch& g); }
