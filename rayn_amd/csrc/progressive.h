// progressive.h — host-visible side of progressive.hip: epoch accumulation of finished films with a per-pixel error estimate and
// tile-adaptive retirement (rayn_hip_progressive_*).  An extension: rayn only carries an unused progressive_epoch counter.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rayn_hip.h"

namespace rayn {

// Where the pieces of the caller's state buffer lie (byte offsets from its 16-byte aligned start) for a width x height film cut into
// tile_w x tile_h tiles.  n_tiles == 0 marks a geometry the entries reject.
struct ProgLayout {
    uint32_t width, height, tile_w, tile_h, tiles_y, n_tiles;
    uint64_t pixels;
    size_t off_s0, off_s1, off_s2; // float4 per pixel (film pixel order): (sum color rgb, sum alpha), (sum background rgb, mean_y), (sum normal xyz, m2)
    size_t off_records;            // uint4 per tile: epochs, retired, outliers, bits of max_e
    size_t off_totals;             // 4 u32: active tiles, bits of max_e, outlier pixels lo / hi; the active list follows it directly (one read-back)
    size_t off_active;             // u32 per tile: the active tiles, ascending (the first totals[0] entries)
    size_t off_listed;             // u32 per tile: the tile list of the accumulate in flight
    size_t bytes;
};
ProgLayout progressive_layout(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h);

// nullptr when valid, else the reason (the entries' last error text)
const char* progressive_check_geometry(const rayn_frame_params* p, const void* state, size_t state_bytes);
const char* progressive_check_params(const rayn_progressive_params* pp);
const char* progressive_check_tiles(const ProgLayout& L, const uint32_t* tiles, uint32_t n_tiles);

// Enqueue on stream s (arguments checked by the functions above).  d_list: the tile list on the device (nullptr = every tile).
void launch_progressive_reset(hipStream_t s, const ProgLayout& L, void* state);
void launch_progressive_accumulate(hipStream_t s, const ProgLayout& L, const rayn_progressive_params& pp, const uint32_t* d_list, uint32_t n_listed,
                                   const float* color, const float* alpha, const float* background, const float* normal, void* state,
                                   float* out_color, float* out_alpha, float* out_background, float* out_normal);
void launch_progressive_compact(hipStream_t s, const ProgLayout& L, void* state);

} // namespace rayn
