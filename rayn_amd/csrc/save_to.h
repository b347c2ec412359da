// save_to.h — host-visible side of save_to.hip: Film::save_to's per-pixel post-process (src/film.rs:205-378) on the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rayn {

// The arms of save_to (src/film.rs:222-362) a (kind, channels, transparent_background) combination selects.
enum SaveArm : int {
    SAVE_COLOR_RGBA = 0,   // Color + Alpha, transparent_background: RGBA                    (:231-254)
    SAVE_COLOR_BG = 1,     // Color + Background, not transparent: RGB of (color + bg)         (:255-277)
    SAVE_COLOR_ONLY = 2,   // Color without Background, not transparent: RGB, NOT saturated   (:274-293)
    SAVE_BACKGROUND = 3,   // (:290-313)
    SAVE_NORMAL = 4,       // (:314-338)
    SAVE_ALPHA = 5         // (:339-362)
};

// kind: ChannelKind (0 Color, 1 Alpha, 2 Background, 3 WorldNormal); bit k of have_mask = ChannelKind k is present.
// Returns the arm, or -1 with *err (if err is non-null) set to the reference's Err text.
int save_to_arm(uint32_t kind, uint32_t have_mask, int transparent_background, const char** err);
int save_to_arm_bpp(int arm); // 4, 3 or 1 bytes per pixel
// Which film channels the arm reads (bit k = ChannelKind k).
uint32_t save_to_arm_reads(int arm);
// One thread per output pixel on stream s; the film is bottom-up (Color / Background / WorldNormal 3 interleaved floats per pixel,
// Alpha 1), out is width * height * bpp bytes, rows top-down.  width * height < 2^31 (the caller checks).
void launch_save_to(hipStream_t s, int arm, uint32_t width, uint32_t height, const float* color, const float* alpha,
                    const float* background, const float* normal, uint8_t* out);

} // namespace rayn
