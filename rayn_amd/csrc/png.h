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

struct PngMeta { // one per block
    uint32_t bytes;  // of the encoded block in its slot, the alignment block included
    uint32_t a, b;   // Adler-32 partial sums mod 65521: sum of the bytes, sum of (len - i) * byte i
    uint32_t stored;
};

// The segmented form of the block kernels (exr.hip): R is segments of `bytes` bytes, a multiple of 16, the last one possibly shorter; each
// is a stream of its own, cut into blocks from its own start - `blocks` of them per segment, also where the last one has fewer.
struct PngSegments {
    uint32_t bytes, blocks;
};

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
// The same for n bytes that are deflated as they are (stride 0); ok = false for n == 0 and n >= 2^31
PngGeometry stream_geometry(uint64_t n);
// nullptr when the arguments are valid, else the reason (the entry's last error text).  Checks everything but ctx and the stream.
const char* png_check_args(uint32_t w, uint32_t h, uint32_t bpp, const uint8_t* d_img, const void* d_out, size_t out_bytes, const void* d_scratch,
                           size_t scratch_bytes);
// Enqueue the encoder on stream s (arguments checked by png_check_args); the first HIP error of the memset, else hipSuccess.
hipError_t launch_png_encode(hipStream_t s, uint32_t w, uint32_t h, uint32_t bpp, const uint8_t* d_img, void* d_out, void* d_scratch);

// The steps the encoders share: the row filter into R; the layout and the compaction of the blocks a block kernel left in their slots
void launch_png_filter(hipStream_t s, uint32_t w, uint32_t h, uint32_t bpp, const uint8_t* d_img, uint8_t* R);
void launch_png_finish(hipStream_t s, const PngGeometry& g, void* d_out, void* d_scratch);

// k_png_block on the segments of R (n bytes in all, nblocks blocks over all segments): block b of segment k leaves meta[k * seg.blocks + b]
// and that slot of `slots`
void launch_png_block_segmented(hipStream_t s, const uint8_t* R, uint32_t n, uint32_t nblocks, PngSegments seg, PngMeta* meta, uint8_t* slots);

// ---- png_lz.hip: the encoder with LZ77 matches (rayn_hip_png_encode_lz77_device, rayn_hip_deflate_lz77_device) --------------------------
constexpr uint32_t PNG_LZ_POSITIONS = 2u * PNG_BLOCK; // bytes of scratch per block behind the slots: one array of 16-bit positions of the sort
// scratch of n filtered bytes: the run-only encoder's, then PNG_LZ_POSITIONS per block
size_t png_lz_scratch_bytes(const PngGeometry& g);
const char* png_lz_check_args(uint32_t w, uint32_t h, uint32_t bpp, const uint8_t* d_img, const void* d_out, size_t out_bytes, const void* d_scratch,
                              size_t scratch_bytes);
const char* deflate_check_args(const void* d_data, size_t n, const void* d_out, size_t out_bytes, const void* d_scratch, size_t scratch_bytes);
hipError_t launch_png_encode_lz77(hipStream_t s, uint32_t w, uint32_t h, uint32_t bpp, const uint8_t* d_img, void* d_out, void* d_scratch);
hipError_t launch_deflate_lz77(hipStream_t s, const void* d_data, uint32_t n, uint32_t stride, void* d_out, void* d_scratch);
// k_png_lz_block on the segments of R, as launch_png_block_segmented; positions: PNG_LZ_POSITIONS bytes per block
void launch_png_lz_block_segmented(hipStream_t s, const uint8_t* R, uint32_t n, uint32_t nblocks, PngSegments seg, uint32_t stride, PngMeta* meta,
                                   uint8_t* slots, uint16_t* positions);

} // namespace rayn
