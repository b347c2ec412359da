// preview.h — host-visible side of preview.hip: the preview integrator (rayn_hip_preview_device), an image of the geometry alone - primary
// hit, viewer-facing normal and ambient occlusion - that runs on the G-buffer pass and the product shadow-march kernels.  An extension: rayn
// has no such mode.  include/rayn_hip.h holds the definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rayn_hip.h"
#include "kernels.h"
#include "temporal.h"

namespace rayn {

constexpr uint32_t PREVIEW_MAX_SAMPLES = 64;
// AO rays of one pixel that are parked, marched and counted together: a round's job store is 29 bytes per ray and pixel
constexpr uint32_t PREVIEW_ROUND = 8;

// The caller's scratch as the entry carves it.  cap = npad: the job store is laid out [round sample][pixel] like Nee's [sample][slot].
struct PreviewScratch {
    GbufScratch g;       // the G-buffer pass's own scratch, at the front
    float4* records;     // [npad] (P, t): the caller's d_out_records when given, else here
    uint32_t* object;    // [npad] likewise
    float* hl;           // [npad] the headlight term of a surface pixel
    uint32_t* count;     // [npad] visible AO rays so far; 0xFFFFFFFF: background
    float* t0;           // [npad] time_start: the packet time the march kernels read per slot
    uint8_t* vis;        // [round][npad] 0 occluded by a sphere, 1 visible, 2 SDF march pending
    uint32_t* job_ref;   // [round * npad]
    float2* job_geo;     // [round * npad][3]
    uint32_t round;      // samples per round: min(samples, PREVIEW_ROUND), less while round * npad would not fit the 32-bit job references
};
// 0 for a size the entry rejects (zero, width * height >= 2^31) and for samples outside 1..64
size_t preview_scratch_bytes(uint32_t width, uint32_t height, uint32_t samples);
PreviewScratch preview_scratch(uint32_t width, uint32_t height, uint32_t samples, void* scratch, void* out_records, uint32_t* out_object);
// nullptr when the arguments are valid, else the reason (the entry's last error text).  Checks everything but ctx, world and stream.
const char* preview_check_args(const rayn_frame_params* p, const rayn_preview_params* pp, const float* samples, const float* scramble, const float* out_color,
                               const float* out_alpha, const float* out_normal, const float* out_ao, const void* out_records, const uint32_t* out_object,
                               const void* scratch, size_t scratch_bytes);
// Nee as the shadow-march kernels read it: the round's job store
Nee preview_nee(const PreviewScratch& ps);
// after a round's march: count its visible rays; last: write colour, alpha and ao
void launch_preview_resolve(hipStream_t s, const PreviewScratch& ps, uint32_t kn, uint32_t samples, bool last, float* out_color, float* out_alpha, float* out_ao);

} // namespace rayn

// the job-generating kernel estimates normals and tests spheres with device_core.h's functions and is therefore built once per mul_add policy
#define RAYN_DECLARE_PREVIEW(NS)                                                                                                                \
    namespace NS {                                                                                                                              \
    void launch_preview_jobs(hipStream_t s, const rayn::DScene* sc, const rayn::PreviewScratch& ps, uint32_t k0, uint32_t kn, float radius, float ambient, \
                             const float* samples, const float* scramble, float* out_normal);                                                  \
    }
RAYN_DECLARE_PREVIEW(rayn_p0)
RAYN_DECLARE_PREVIEW(rayn_p1)
#undef RAYN_DECLARE_PREVIEW
