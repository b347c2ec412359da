// save_to.hip — Film::save_to's per-pixel post-process (src/film.rs:205-378) on the device: saturate, gamma 2.2, the Color +
// Background composite, Color + Alpha RGBA, normal -> RGB, the y-flip and the 8-bit quantisation, arm by arm.  The arithmetic is
// the oracle's (oracle_save_to_pixels, oracle/rayn_oracle.cpp) and rayn_amd/image.py's: f32 throughout, Rust's f32::min / max (a NaN
// operand yields the OTHER operand), powf = the pinned dm_powf (binary64 inside, the same bits on the host and on gfx950), and
// `(v * 255.0).min(255.0).max(0.0) as u8`.  Built with -ffp-contract=off like the rest: n * 0.5 + 0.5 must not be fused.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rayn_detmath.h"
#include "../../include/rayn_hip.h"
#include "save_to.h"

namespace rayn {
namespace {

// the oracle's rust_min / rust_max / quant8 / saturate1 / gamma1, written the same way so that no min/max instruction with other
// NaN or signed-zero conventions is substituted
__device__ inline float rmin(float a, float b) { return a != a ? b : (b != b ? a : (a < b ? a : b)); }
__device__ inline float rmax(float a, float b) { return a != a ? b : (b != b ? a : (a > b ? a : b)); }
__device__ inline uint8_t quant8(float v) { return (uint8_t)rmax(rmin(v * 255.0f, 255.0f), 0.0f); }
__device__ inline float saturate1(float x) { return rmin(rmax(x, 0.0f), 1.0f); }
__device__ inline float gamma22(float x) { return dm_powf(x, 1.0f / 2.2f); }

// One thread per output pixel.  i = x + y * width is the top-down output pixel; it reads film pixel x + (height - 1 - y) * width
// (src/film.rs:236).  n = width * height < 2^31.
template <int ARM>
__global__ void __launch_bounds__(256) k_save_to(uint32_t width, uint32_t height, const float* __restrict__ color,
                                                 const float* __restrict__ alpha, const float* __restrict__ background,
                                                 const float* __restrict__ normal, uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= width * height) return;
    const uint32_t y = i / width, x = i - y * width;
    const size_t o = i, f = (size_t)x + (size_t)(height - 1u - y) * width; // 3 or 4 bytes / floats per pixel need 64-bit offsets
    if (ARM == SAVE_COLOR_RGBA) {
        for (int c = 0; c < 3; c++) out[4 * o + c] = quant8(gamma22(saturate1(color[3 * f + c])));
        out[4 * o + 3] = quant8(alpha[f]);
    } else if (ARM == SAVE_COLOR_BG) {
        for (int c = 0; c < 3; c++) out[3 * o + c] = quant8(gamma22(saturate1(color[3 * f + c] + background[3 * f + c])));
    } else if (ARM == SAVE_COLOR_ONLY) {
        for (int c = 0; c < 3; c++) out[3 * o + c] = quant8(gamma22(color[3 * f + c]));
    } else if (ARM == SAVE_BACKGROUND) {
        for (int c = 0; c < 3; c++) out[3 * o + c] = quant8(gamma22(saturate1(background[3 * f + c])));
    } else if (ARM == SAVE_NORMAL) {
        for (int c = 0; c < 3; c++) out[3 * o + c] = quant8(normal[3 * f + c] * 0.5f + 0.5f);
    } else {
        out[o] = quant8(alpha[f]);
    }
}

} // namespace

int save_to_arm(uint32_t kind, uint32_t have_mask, int transparent_background, const char** err) {
    const bool color = have_mask & 1u, alpha = have_mask & 2u, background = have_mask & 4u, normal = have_mask & 8u;
    const char* why = nullptr;
    int arm = -1;
    switch (kind) {
    case 0: // src/film.rs:222-298: the match on (color, alpha, background, transparent_background)
        if (color && alpha && transparent_background) arm = SAVE_COLOR_RGBA;
        else if (color && background && !transparent_background) arm = SAVE_COLOR_BG;
        else if (color && !background && !transparent_background) arm = SAVE_COLOR_ONLY;
        else why = "Attempted to write Color channel with insufficient channels";
        break;
    case 1:
        if (alpha) arm = SAVE_ALPHA;
        else why = "Attempted to write Alpha channel but it didn't exist";
        break;
    case 2:
        if (background) arm = SAVE_BACKGROUND;
        else why = "Attempted to write Background channel but it didn't exist";
        break;
    case 3:
        if (normal) arm = SAVE_NORMAL;
        else why = "Attempted to write WorldNormal channel but it didn't exist";
        break;
    default:
        why = "unknown ChannelKind (0 Color, 1 Alpha, 2 Background, 3 WorldNormal)";
    }
    if (err) *err = why;
    return arm;
}

int save_to_arm_bpp(int arm) { return arm == SAVE_COLOR_RGBA ? 4 : arm == SAVE_ALPHA ? 1 : 3; }

uint32_t save_to_arm_reads(int arm) {
    switch (arm) {
    case SAVE_COLOR_RGBA: return 1u | 2u;
    case SAVE_COLOR_BG: return 1u | 4u;
    case SAVE_COLOR_ONLY: return 1u;
    case SAVE_BACKGROUND: return 4u;
    case SAVE_NORMAL: return 8u;
    default: return 2u;
    }
}

void launch_save_to(hipStream_t s, int arm, uint32_t width, uint32_t height, const float* color, const float* alpha,
                    const float* background, const float* normal, uint8_t* out) {
    const uint32_t n = width * height;
    const dim3 grid((n + 255u) / 256u), block(256);
    switch (arm) {
    case SAVE_COLOR_RGBA: hipLaunchKernelGGL(k_save_to<SAVE_COLOR_RGBA>, grid, block, 0, s, width, height, color, alpha, background, normal, out); break;
    case SAVE_COLOR_BG: hipLaunchKernelGGL(k_save_to<SAVE_COLOR_BG>, grid, block, 0, s, width, height, color, alpha, background, normal, out); break;
    case SAVE_COLOR_ONLY: hipLaunchKernelGGL(k_save_to<SAVE_COLOR_ONLY>, grid, block, 0, s, width, height, color, alpha, background, normal, out); break;
    case SAVE_BACKGROUND: hipLaunchKernelGGL(k_save_to<SAVE_BACKGROUND>, grid, block, 0, s, width, height, color, alpha, background, normal, out); break;
    case SAVE_NORMAL: hipLaunchKernelGGL(k_save_to<SAVE_NORMAL>, grid, block, 0, s, width, height, color, alpha, background, normal, out); break;
    default: hipLaunchKernelGGL(k_save_to<SAVE_ALPHA>, grid, block, 0, s, width, height, color, alpha, background, normal, out); break;
    }
}

} // namespace rayn

extern "C" int rayn_save_to_bpp(uint32_t kind, uint32_t have_mask, int transparent_background) {
    const int arm = rayn::save_to_arm(kind, have_mask, transparent_background, nullptr);
    return arm < 0 ? -1 : rayn::save_to_arm_bpp(arm);
}
