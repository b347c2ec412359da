// upscale.hip — guided upscaling of a film rendered at width x height to factor * width x factor * height (rayn_hip_upscale_device):
// joint bilateral upsampling (Kopf et al., SIGGRAPH 2007) whose guide is traced, not interpolated - the primary-hit G-buffer of the same
// camera at both resolutions (rayn_hip_gbuffer_device).  An extension: rayn renders at one resolution.  It runs downstream of the film:
// it reads the low film's planes and writes new planes of the high size; nothing it reads is touched.
//
// The definition (include/rayn_hip.h; tests/upscale_np.py restates it in numpy and the tests compare bit for bit):
// per high pixel the four taps of the bilinear footprint in the low film, each weighted by its bilinear weight b times
// expf(-(plane distance^2 / sigma_plane^2 + position distance^2 / sigma_position^2)), distances relative to the pixel's hit distance,
// over the taps that show the pixel's object and hold a finite colour; where that sum is empty the plain bilinear weights over the taps
// with a finite colour; where that is empty too, the low pixel the high one falls into, verbatim.  One weight set serves every plane.
// f32 throughout, built with -ffp-contract=off and IEEE division; expf is the pinned dm_expf of rayn_detmath.h, evaluated through dmf_expf
// (rayn_detmath_fast.h: the same bits, cheaper).  Nothing here depends on the mul_add policy: the file is built once.
//
// Layout: one thread per high pixel, blocks of 128 threads over contiguous runs of a row, rows x runs in a 1-D grid.  A pixel reads 20
// bytes of its own guide (one 128-bit record load and the object index) and writes up to 44; its taps are shared with the s x s pixels
// around it and come from L2.  The guided pass keeps eleven sums; the two fallback tiers re-read the taps in a branch few pixels take,
// which keeps their sums out of the common path's registers.  The sums and the gather of one tier (Sums, add_tap, upscale_gather) are in
// post_device.h: k_temporal_upscale runs the same function on its own footprint.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "post_checks.h"
#include "post_device.h"
#include "upscale.h"

namespace rayn {
namespace {

constexpr uint32_t BLOCK = 128u;

struct UpscaleArgs {
    uint32_t w, h, W, blocks_x, factor; // the low size, the high width, blocks per high row
    float sigma_plane, sigma_position;
    UpscalePlanes pl;
};

__device__ inline void write_mean(const Sums& S, size_t P, const UpscalePlanes& pl) {
#pragma unroll
    for (int i = 0; i < 3; i++) pl.out_color[3u * P + i] = S.c[i] / S.W;
    if (pl.alpha) pl.out_alpha[P] = S.a / S.W;
    if (pl.background) {
#pragma unroll
        for (int i = 0; i < 3; i++) pl.out_background[3u * P + i] = S.b[i] / S.W;
    }
    if (pl.normal) {
#pragma unroll
        for (int i = 0; i < 3; i++) pl.out_normal[3u * P + i] = S.n[i] / S.W;
    }
}

// TERMS: which of the plane / position terms are on.  Every index is bounded by its plane: a tap is used only with qx < w and qy < h
// (q < w * h), the tier-3 source is clamped to the low image, and P < W * H by the two guards on X and the grid (blocks_x * H blocks).
template <uint32_t TERMS>
__global__ void __launch_bounds__(BLOCK) k_upscale(const UpscaleArgs A) {
    const uint32_t Y = blockIdx.x / A.blocks_x, xb = blockIdx.x - Y * A.blocks_x;
    const uint32_t X = xb * BLOCK + threadIdx.x;
    if (X >= A.W) return;
    const UpscalePlanes& pl = A.pl;
    const size_t P = (size_t)X + (size_t)Y * A.W; // < 2^31
    const float sf = (float)A.factor;
    const float fx = ((float)X + 0.5f) / sf - 0.5f, fy = ((float)Y + 0.5f) / sf - 0.5f; // in (-0.5, w - 0.5), exact pixel centres (W, H <= 2^23)
    const float x0f = floorf(fx), y0f = floorf(fy);
    const float wx1 = fx - x0f, wy1 = fy - y0f;
    const float wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
    const int x0 = (int)x0f, y0 = (int)y0f; // -1 .. w - 1
    const uint32_t o = pl.high_object[P];
    const bool guided = TERMS != 0u && o != MISS_OBJECT;
    float4 G = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (guided) G = ((const float4*)pl.high_records)[P];
    const UpscaleGuide u = upscale_guide<TERMS>(o, guided, G, A.sigma_plane, A.sigma_position);

    Sums S;
    upscale_gather<TERMS, true, false>(S, x0, y0, wx0, wx1, wy0, wy1, A.w, A.h, u, pl);
    float weight = S.W;
    if (!(S.W > 0.0f)) {
        // tier 2: the plain bilinear weights over the usable taps, whatever they show
        weight = 0.0f;
        S = Sums();
        upscale_gather<TERMS, false, false>(S, x0, y0, wx0, wx1, wy0, wy1, A.w, A.h, u, pl);
    }
    if (S.W > 0.0f) {
        write_mean(S, P, pl);
    } else {
        // tier 3: the low pixel this one falls into, verbatim
        const uint32_t sx = min(X / A.factor, A.w - 1u), sy = min(Y / A.factor, A.h - 1u);
        const size_t q = (size_t)sx + (size_t)sy * A.w;
#pragma unroll
        for (int i = 0; i < 3; i++) pl.out_color[3u * P + i] = pl.color[3u * q + i];
        if (pl.alpha) pl.out_alpha[P] = pl.alpha[q];
        if (pl.background) {
#pragma unroll
            for (int i = 0; i < 3; i++) pl.out_background[3u * P + i] = pl.background[3u * q + i];
        }
        if (pl.normal) {
#pragma unroll
            for (int i = 0; i < 3; i++) pl.out_normal[3u * P + i] = pl.normal[3u * q + i];
        }
    }
    if (pl.out_weight) pl.out_weight[P] = weight;
}

} // namespace

const char* upscale_check_args(uint32_t width, uint32_t height, const rayn_upscale_params* up, const UpscalePlanes& pl) {
    if (!up) return "null upscale params";
    if (up->factor < 1u || up->factor > 8u) return "factor must be in 1..8";
    if (!width || !height) return "zero-sized image";
    const uint64_t W = (uint64_t)width * up->factor, H = (uint64_t)height * up->factor;
    if (W * H >= ((uint64_t)1 << 31)) return "upscaled image larger than 2^31 pixels unsupported (32-bit pixel indices)";
    if (W > ((uint64_t)1 << 23) || H > ((uint64_t)1 << 23)) return "upscaled image wider or taller than 2^23 pixels unsupported (pixel centres exact in f32)";
    if (!sigma_ok(up->sigma_plane)) return "sigma_plane must be 0 (off) or in [2^-30, 2^30]";
    if (!sigma_ok(up->sigma_position)) return "sigma_position must be 0 (off) or in [2^-30, 2^30]";
    if (!pl.color || !pl.out_color) return "null Color buffer";
    if (!pl.low_records || !pl.low_object || !pl.high_records || !pl.high_object) return "null G-buffer";
    if ((pl.alpha && !pl.out_alpha) || (pl.background && !pl.out_background) || (pl.normal && !pl.out_normal)) return "null output for a present input plane";
    if ((!pl.alpha && pl.out_alpha) || (!pl.background && pl.out_background) || (!pl.normal && pl.out_normal)) return "null input for a present output plane";
    if (!pl.normal && up->sigma_plane != 0.0f) return "null normal guide with sigma_plane != 0";
    if ((uintptr_t)pl.low_records % 16u || (uintptr_t)pl.high_records % 16u) return "G-buffer records not 16-byte aligned";
    if ((uintptr_t)pl.low_object % 4u || (uintptr_t)pl.high_object % 4u) return "G-buffer objects not 4-byte aligned";
    const size_t n = (size_t)width * height, N = (size_t)(W * H);
    const UpscaleSpans sp = upscale_spans(pl, n, N);
    for (int i = 0; i < 5; i++) {
        if (first_overlap(sp.out + i, 1, sp.in, 8)) return "an output must not alias an input";
        if (first_overlap(sp.out + i, 1, sp.out + i + 1, 4 - i)) return "the outputs must not alias each other";
    }
    return nullptr;
}

void launch_upscale(hipStream_t s, uint32_t width, uint32_t height, const rayn_upscale_params& up, const UpscalePlanes& pl) {
    UpscaleArgs A;
    A.w = width;
    A.h = height;
    A.W = width * up.factor;
    A.blocks_x = (A.W + BLOCK - 1u) / BLOCK;
    A.factor = up.factor;
    A.sigma_plane = up.sigma_plane;
    A.sigma_position = up.sigma_position;
    A.pl = pl;
    const uint32_t terms = (up.sigma_plane != 0.0f ? UPSCALE_PLANE : 0u) | (up.sigma_position != 0.0f ? UPSCALE_POSITION : 0u);
    const dim3 grid(A.blocks_x * (height * up.factor)), block(BLOCK); // blocks_x * H <= W * H < 2^31
    with_terms<2>(terms, [&](auto T) { hipLaunchKernelGGL((k_upscale<decltype(T)::value>), grid, block, 0, s, A); });
}

} // namespace rayn
