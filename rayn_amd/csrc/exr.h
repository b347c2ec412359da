// exr.h — host-visible side of exr.hip: the ZIP-compressed scanline chunks of an OpenEXR file encoded on the device from planes in the
// film's layout (rayn_hip_exr_encode_device).  An extension: rayn writes no EXR.  include/rayn_hip.h holds the definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "png.h"

namespace rayn {

constexpr uint32_t EXR_MAX_CHANNELS = 16u;
constexpr uint32_t EXR_ROWS = 16u;         // scanlines per ZIP chunk: part of the file format
constexpr uint32_t EXR_HEADER_BYTES = 16u; // the four words in front of the chunk table

// The geometry of one call, from (w, h, layout); ok = false for what the entry rejects (why: the reason)
struct ExrGeometry {
    bool ok;
    const char* why;
    uint32_t row_bytes;   // S
    uint32_t n;           // bytes of all rows: the sum of the n_k
    uint32_t chunks;
    PngSegments seg;      // a full chunk's bytes (16 * S, a multiple of 32) and blocks
    uint32_t blocks;      // over all chunks
    size_t body_at;       // align16(16 + 4 * chunks): where the body starts in d_out
    size_t bound;
    // d_scratch: P at 0 (the block kernels' R), then
    size_t off_raw, off_meta, off_block_at, off_starts, off_sizes, off_adler, off_slots, scratch_bytes;
};
ExrGeometry exr_geometry(uint32_t w, uint32_t h, uint32_t n_channels, const uint32_t* layout, uint32_t matches);
// nullptr when the arguments are valid, else the reason (the entry's last error text).  Checks everything but ctx and the stream.
const char* exr_check_args(uint32_t w, uint32_t h, uint32_t n_channels, const void* const* d_planes, const uint32_t* layout, uint32_t matches,
                           const void* d_out, size_t out_bytes, const void* d_scratch, size_t scratch_bytes);
// Enqueue the encoder on stream s (arguments checked by exr_check_args): one memset and four kernels, whatever the height.  The first HIP
// error of the memset, else hipSuccess.
hipError_t launch_exr_encode(hipStream_t s, uint32_t w, uint32_t h, uint32_t n_channels, const void* const* d_planes, const uint32_t* layout,
                             uint32_t matches, void* d_out, void* d_scratch);

} // namespace rayn
