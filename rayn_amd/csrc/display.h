// display.h — host-visible side of display.hip: the HDR display transform of the film's Color channel (auto exposure, bloom, tone
// mapping) in front of save_to's gamma and 8-bit quantisation.  An extension: rayn clamps its film to [0, 1].
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rayn_hip.h"

namespace rayn {

// Device scratch of launch_display: a 256-byte header ({e, m} in its first two floats), the metering partials (a float and a u32 per
// block of 256 pixels) and bloom levels 1 .. levels as 16-byte records.  0 for a size the entries reject (zero, width * height >= 2^31,
// levels > 8).
size_t display_scratch_bytes(uint32_t width, uint32_t height, uint32_t levels);
// nullptr when the arguments are valid, else the reason (the entry's last error text); *arm receives the save_to arm of the Color kind.
// Checks everything but the stream and the entry's own output pointer.
const char* display_check_args(const rayn_display_params* dp, uint32_t have_mask, int transparent_background, uint32_t width, uint32_t height,
                               const float* color, const float* alpha, const float* background, const void* state, const void* scratch,
                               size_t scratch_bytes, int* arm);
// Enqueue the transform on stream s (arguments checked by display_check_args).  Exactly one of out8 (width * height * bpp bytes, rows
// top-down) and out_color (width * height * 3 floats, film order) is non-null; out_meter (2 floats: m, e) and out_bloom (width * height * 3
// floats, film order; written only with bloom on) may be null.
void launch_display(hipStream_t s, int arm, const rayn_display_params& dp, uint32_t width, uint32_t height, const float* color, const float* alpha,
                    const float* background, void* state, void* scratch, uint8_t* out8, float* out_color, float* out_meter, float* out_bloom);

} // namespace rayn
