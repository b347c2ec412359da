// denoise.hip — the edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010) of the film's Color channel, guided by the film's
// WorldNormal and Alpha (rayn_hip_denoise_device).  An extension: rayn has no denoiser.  It runs downstream of the film: it reads the
// finished Color / Alpha / WorldNormal planes and writes a new Color plane; the film itself is not touched.
//
// The definition (include/rayn_hip.h; tests/denoise_np.py restates it in numpy and the tests compare bit for bit):
// iteration i = 0 .. L-1 with step s = 2^i reads the previous iteration's colour (iteration 0 the film's).  A pixel whose colour has a
// non-finite component passes through.  Otherwise W = 9/64, S = (9/64) c_p (the centre tap, h[2] h[2]), then the 24 other taps of the
// 5x5 B3-spline stencil in raster order (ky outer, kx inner), tap q = p + (kx, ky) s, skipped outside the image or where c_q has a
// non-finite component:
//     e = (d_c kc 4^i + d_n kn) + d_a ka     (d_* = squared distances, k* = 1 / sigma*^2; a term whose sigma is 0 is left out)
//     w = (h[ky+2] h[kx+2]) expf(-e),        h = {1/16, 1/4, 3/8, 1/4, 1/16}; a NaN w skips the tap
//     W += w, S += w c_q
// and out_p = S / W.  f32 throughout, built with -ffp-contract=off and IEEE division; expf is the pinned dm_expf of rayn_detmath.h,
// evaluated through dmf_expf (rayn_detmath_fast.h: the same bits, cheaper).
//
// Layout: a pack kernel turns the planar inputs into 16-byte records (colour + alpha, normal + 0), so that a tap costs one 128-bit
// load per guide; the passes ping-pong between two colour + alpha record planes in the caller's scratch and the last one writes the
// planar 3-float colour.  One thread per pixel in 16x16 blocks; every tap is a plain global load served by L2 / the Infinity Cache
// (a 1280x720 record plane is 15 MB).  A tap is about 80 VALU instructions, 22 of them binary64 (dmf_expf), against 3 loads: the
// passes are bound by VALU, not by memory, so no LDS tile is staged.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "denoise.h"
#include "post_checks.h"
#include "post_device.h"

namespace rayn {
namespace {

constexpr uint32_t TERM_COLOR = 1u, TERM_NORMAL = 2u, TERM_ALPHA = 4u;

// One thread per pixel: planar colour (3 floats), alpha (1) and normal (3) -> ca[p] = (r, g, b, alpha), nrm[p] = (nx, ny, nz, 0).
// A guide that is switched off is not read (its pointer may be null): alpha 0, no normal record.  n < 2^31.
__global__ void __launch_bounds__(256) k_denoise_pack(uint32_t n, const float* __restrict__ color, const float* __restrict__ alpha,
                                                      const float* __restrict__ normal, float4* __restrict__ ca, float4* __restrict__ nrm) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const size_t f = (size_t)p * 3u;
    ca[p] = make_float4(color[f], color[f + 1], color[f + 2], alpha ? alpha[p] : 0.0f);
    if (normal) nrm[p] = make_float4(normal[f], normal[f + 1], normal[f + 2], 0.0f);
}

// One a-trous pass with step `step` (a power of two <= 128).  Blocks of 16x16 threads, one per 16x16 tile of the image, tiles in a
// 1-D grid (row-major, tiles_x per row) so that tall images do not run into the grid's y limit.  TERMS: which of the colour / normal /
// alpha terms are on.  LAST: write the planar colour instead of the next record plane.
template <uint32_t TERMS, bool LAST>
__global__ void __launch_bounds__(256) k_atrous(uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t step, float sigma_color,
                                                float sigma_normal, float sigma_alpha, const float4* __restrict__ ca,
                                                const float4* __restrict__ nrm, float4* __restrict__ ca_out, float* __restrict__ out_color) {
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const uint32_t x = tx * 16u + threadIdx.x, y = ty * 16u + threadIdx.y;
    if (x >= width || y >= height) return;
    const uint32_t p = x + y * width; // < 2^31
    const float4 cp = ca[p];
    float r = cp.x, g = cp.y, b = cp.z;
    if (finite3(cp.x, cp.y, cp.z)) {
        // kc 4^i: 4^i = step^2 <= 2^14 is exact in f32, and sigma in [2^-30, 2^30] keeps the product finite
        const float kc = (TERMS & TERM_COLOR) ? (1.0f / (sigma_color * sigma_color)) * (float)(step * step) : 0.0f;
        const float kn = (TERMS & TERM_NORMAL) ? 1.0f / (sigma_normal * sigma_normal) : 0.0f;
        const float ka = (TERMS & TERM_ALPHA) ? 1.0f / (sigma_alpha * sigma_alpha) : 0.0f;
        const float4 np = (TERMS & TERM_NORMAL) ? nrm[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
        float W = 9.0f / 64.0f, Sr = W * r, Sg = W * g, Sb = W * b;
#pragma unroll
        for (int ky = -2; ky <= 2; ky++) {
            // unsigned wrap: a negative offset past the edge becomes >= height (height < 2^31), a positive one stays below 2^32
            const uint32_t qy = y + (uint32_t)(ky * (int)step);
            if (qy >= height) continue;
#pragma unroll
            for (int kx = -2; kx <= 2; kx++) {
                if (kx == 0 && ky == 0) continue;
                const uint32_t qx = x + (uint32_t)(kx * (int)step);
                if (qx >= width) continue;
                const uint32_t q = qx + qy * width;
                const float4 cq = ca[q];
                if (!finite3(cq.x, cq.y, cq.z)) continue;
                float e = 0.0f; // 0 + t == t for every term t (t >= +0, inf or NaN): the same bits as the definition's sum
                if (TERMS & TERM_COLOR) {
                    const float dr = r - cq.x, dg = g - cq.y, db = b - cq.z;
                    e = e + (dr * dr + dg * dg + db * db) * kc;
                }
                if (TERMS & TERM_NORMAL) {
                    const float4 nq = nrm[q];
                    const float dx = np.x - nq.x, dy = np.y - nq.y, dz = np.z - nq.z;
                    e = e + (dx * dx + dy * dy + dz * dz) * kn;
                }
                if (TERMS & TERM_ALPHA) {
                    const float da = cp.w - cq.w;
                    e = e + (da * da) * ka;
                }
                const float w = (h[ky + 2] * h[kx + 2]) * dmf_expf(-e);
                if (w != w) continue;
                W += w;
                Sr += w * cq.x;
                Sg += w * cq.y;
                Sb += w * cq.z;
            }
        }
        r = Sr / W; // W >= 9/64
        g = Sg / W;
        b = Sb / W;
    }
    if (LAST) {
        const size_t f = (size_t)p * 3u;
        out_color[f] = r;
        out_color[f + 1] = g;
        out_color[f + 2] = b;
    } else {
        ca_out[p] = make_float4(r, g, b, cp.w);
    }
}

template <uint32_t TERMS>
void launch_pass(hipStream_t s, bool last, dim3 grid, uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t step, float sc, float sn,
                 float sa, const float4* ca, const float4* nrm, float4* ca_out, float* out_color) {
    const dim3 block(16, 16);
    if (last)
        hipLaunchKernelGGL((k_atrous<TERMS, true>), grid, block, 0, s, width, height, tiles_x, step, sc, sn, sa, ca, nrm, ca_out, out_color);
    else
        hipLaunchKernelGGL((k_atrous<TERMS, false>), grid, block, 0, s, width, height, tiles_x, step, sc, sn, sa, ca, nrm, ca_out, out_color);
}

} // namespace

size_t denoise_scratch_bytes(uint32_t width, uint32_t height) {
    return atrous_scratch_bytes(width, height);
}

const char* denoise_check_args(uint32_t width, uint32_t height, uint32_t iterations, float sigma_color, float sigma_normal, float sigma_alpha,
                               const float* color, const float* alpha, const float* normal, const float* out_color, const void* scratch,
                               size_t scratch_bytes) {
    if (const char* why = check_size(width, height)) return why;
    if (const char* why = check_atrous_params(iterations, sigma_color, "sigma_color must be 0 (off) or in [2^-30, 2^30]", sigma_normal, sigma_alpha,
                                              color && out_color && scratch, normal, alpha))
        return why;
    if (scratch_bytes < denoise_scratch_bytes(width, height)) return "scratch smaller than rayn_denoise_scratch_bytes(width, height)";
    if ((uintptr_t)scratch % 16u) return "scratch not 16-byte aligned";
    if (out_color == color) return "d_out_color must not be d_color";
    return nullptr;
}

void launch_denoise(hipStream_t s, uint32_t width, uint32_t height, uint32_t iterations, float sigma_color, float sigma_normal, float sigma_alpha,
                    const float* color, const float* alpha, const float* normal, float* out_color, void* scratch) {
    const uint32_t n = width * height;
    const uint32_t terms = (sigma_color != 0.0f ? TERM_COLOR : 0u) | (sigma_normal != 0.0f ? TERM_NORMAL : 0u) | (sigma_alpha != 0.0f ? TERM_ALPHA : 0u);
    float4* plane[2] = {(float4*)scratch, (float4*)scratch + n};
    float4* nrm = (float4*)scratch + 2u * (size_t)n;
    hipLaunchKernelGGL(k_denoise_pack, dim3((n + 255u) / 256u), dim3(256), 0, s, n, color, (terms & TERM_ALPHA) ? alpha : nullptr,
                       (terms & TERM_NORMAL) ? normal : nullptr, plane[0], nrm);
    const uint32_t tiles_x = (width + 15u) / 16u, tiles_y = (height + 15u) / 16u;
    const dim3 grid(tiles_x * tiles_y); // < 2^27 tiles
    for (uint32_t i = 0; i < iterations; i++) {
        const bool last = i + 1 == iterations;
        const float4* in = plane[i & 1u];
        float4* out = plane[(i + 1u) & 1u];
        const uint32_t step = 1u << i;
        with_terms<3>(terms, [&](auto T) {
            launch_pass<decltype(T)::value>(s, last, grid, width, height, tiles_x, step, sigma_color, sigma_normal, sigma_alpha, in, nrm, out, out_color);
        });
    }
}

} // namespace rayn

extern "C" size_t rayn_denoise_scratch_bytes(uint32_t width, uint32_t height) { return rayn::denoise_scratch_bytes(width, height); }
