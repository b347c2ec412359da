// png.h — host-visible side of png.hip: the zlib stream of a PNG's IDAT chunk encoded on the device from the 8-bit image the save_to and
// display entries write (rayn_hip_png_encode_device).  An extension: rayn encodes on the host.  include/rayn_hip.h holds the definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rayn_hip.h"

namespace rayn {

constexpr uint32_t PNG_BLOCK = 32768u;            // bytes of the filtered stream per deflate block: part of the format
constexpr uint32_t PNG_SLOT = PNG_BLOCK + 16u;    // bytes of scratch an encoded block may take before the compaction (len + 5 + alignment <= len + 10)
constexpr uint32_t PNG_HEADER_BYTES = 16u;        // the four words in front of the zlib stream

// The geometry of one call, from (w, h, bpp); ok = false for what the entry rejects (why: the reason)
struct PngGeometry {
    bool ok;
    const char* why;
    uint32_t stride;   // bytes of a row of the filtered stream: 1 + w * bpp
    uint32_t n;        // bytes of the filtered stream
    uint32_t blocks;
    size_t off_meta, off_offsets, off_totals, off_slots, scratch_bytes, bound;
};
PngGeometry png_geometry(uint32_t w, uint32_t h, uint32_t bpp);
// nullptr when the arguments are valid, else the reason (the entry's last error text).  Checks everything but ctx and the stream.
const char* png_check_args(uint32_t w, uint32_t h, uint32_t bpp, const uint8_t* d_img, const void* d_out, size_t out_bytes, const void* d_scratch,
                           size_t scratch_bytes);
// Enqueue the encoder on stream s (arguments checked by png_check_args); the first HIP error of the memset, else hipSuccess.
hipError_t launch_png_encode(hipStream_t s, uint32_t w, uint32_t h, uint32_t bpp, const uint8_t* d_img, void* d_out, void* d_scratch);

} // namespace rayn
