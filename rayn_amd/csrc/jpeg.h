// jpeg.h — host-visible side of jpeg.hip: the entropy-coded scan of a baseline JPEG encoded on the device from the 8-bit image the save_to
// and display entries write (rayn_hip_jpeg_encode_device).  An extension: rayn writes PNG only.  include/rayn_hip.h holds the definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rayn_hip.h"

namespace rayn {

constexpr uint32_t JPEG_HEADER_BYTES = 16u; // the four words in front of the scan

// The worst case of one block in bits, from the longest codes of the Annex K tables (jpeg.hip asserts them): a DC code and its 11 value
// bits (the largest DC difference is 2047), then 63 non-zero AC coefficients, each the longest AC code and 10 value bits (|AC| < 1024: no
// run, so no ZRL, and a non-zero last coefficient, so no EOB; a run only removes coefficients, and a ZRL replaces 16 of them by 16 bits).
//   luminance    9 + 11 + 63 * (16 + 10) = 1658
//   chrominance 11 + 11 + 63 * (16 + 10) = 1660
// A segment of n MCUs is at most ceil(n * mcu_bits / 8) bytes before the stuffing, which at worst doubles them (every byte 0xFF); the
// padding is inside the ceil.  rayn_jpeg_scan_bound: 16 + the sum of that over the segments + 2 per marker, rounded up to 16.
constexpr uint32_t JPEG_LUMA_BLOCK_BITS = 1658u, JPEG_CHROMA_BLOCK_BITS = 1660u;

// The geometry of one call; ok = false for what the entry rejects (why: the reason)
struct JpegGeometry {
    bool ok;
    const char* why;
    uint32_t width, height, bpp, subsampling;
    uint32_t bpm;              // blocks per MCU: 1 grey, 3 for 4:4:4, 6 for 4:2:0
    uint32_t mcus_x, mcus;     // MCUs per row, in all
    uint32_t blocks;
    uint32_t ri, segments;     // the restart interval as given; ceil(mcus / ri)
    uint32_t raw_words;        // 32-bit words of a segment's unstuffed bits in the scratch
    uint32_t slot_bytes;       // bytes of a segment's stuffed bytes in the scratch
    size_t off_bits, off_meta, off_offsets, off_totals, off_raw, off_slots, scratch_bytes, bound;
};
JpegGeometry jpeg_geometry(uint32_t w, uint32_t h, uint32_t bpp, uint32_t subsampling, uint32_t restart_interval);
// nullptr when the arguments are valid, else the reason (the entry's last error text).  Checks everything but ctx and the stream.
const char* jpeg_check_args(uint32_t w, uint32_t h, uint32_t bpp, uint32_t quality, uint32_t subsampling, uint32_t restart_interval, const uint8_t* d_img,
                            const void* d_out, size_t out_bytes, const void* d_scratch, size_t scratch_bytes);
// The two halves of the encoder, which rayn_hip_probe_jpeg_transform and rayn_hip_probe_jpeg_entropy (probes.hip) run alone.
// launch_jpeg_transform: k_jpeg_transform, the image -> the int16 coefficients at the start of the scratch (64 per block, zigzag, scan order).
// launch_jpeg_entropy: the segment, layout and compaction kernels, those coefficients -> the header words and the scan in d_out.
void launch_jpeg_transform(hipStream_t s, const JpegGeometry& g, uint32_t quality, const uint8_t* d_img, void* d_scratch);
void launch_jpeg_entropy(hipStream_t s, const JpegGeometry& g, void* d_out, void* d_scratch);
// Enqueue the four kernels on stream s (arguments checked by jpeg_check_args): the two launches above
void launch_jpeg_encode(hipStream_t s, const JpegGeometry& g, uint32_t quality, const uint8_t* d_img, void* d_out, void* d_scratch);

} // namespace rayn
