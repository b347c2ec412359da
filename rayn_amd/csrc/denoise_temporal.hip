// denoise_temporal.hip — the variance-guided a-trous filter on a temporally accumulated colour (rayn_hip_denoise_temporal_variance_device):
// SVGF's variance estimate for sequences (Schied et al., HPG 2017, section 4.2) in front of the passes of denoise_variance.hip.  An
// extension: rayn has neither.  It runs downstream of the temporal accumulate: it reads the accumulated colour, the film's Alpha and
// WorldNormal, the frame's G-buffer objects, the new history (for the history length n' in A.w) and the new luminance moments, and
// writes a new Color plane and, optionally, the filtered variance.  That entry does not touch the history: the filtered colour is not fed
// back.  rayn_hip_denoise_temporal_variance_feedback_device is the same filter with SVGF's feedback edge: pass 0 (k_vatrous<.., true>,
// denoise_variance.hip) also blends its colour into plane A of the history, which the next frame's accumulate reprojects.
//
// The definition (include/rayn_hip.h; tests/temporal_variance_np.py restates it in numpy and the tests compare bit
// for bit).  l_x = (0.2126f c_x.r + 0.7152f c_x.g) + 0.0722f c_x.b of the accumulated colour.  Pixel p is NOT GUIDED (v = NaN: it passes
// through every pass and is never a tap) when its object is a miss, c_p has a non-finite component or !(n'_p >= 1).  Else
//     n'_p >= 4.0f (the temporal estimate):  d = m2 - m1 * m1,  v = (d > 0 ? d : 0.0f) / n'_p      - the variance of the accumulated mean
//     else (the spatial estimate):  over the 7x7 window at unit spacing in raster order, centre included, the taps q inside the image with
//         obj_q = obj_p, n'_q >= 1 and a finite c_q:  k += 1.0f, s1 += l_q, s2 += l_q * l_q;  mu = s1 / k, d = s2 / k - mu * mu,
//         v = d > 0 ? d : 0.0f
// and a v that is not finite makes p not guided.  Then the passes of k_vatrous, unchanged.  f32, -ffp-contract=off, IEEE division.
//
// Layout: one thread per pixel in 16x16 blocks.  Only a block that holds a short-history pixel stages its 22x22 halo of (luminance,
// object) in LDS (3872 B; a tap that cannot count - outside, n' < 1, a non-finite colour - is stored with the miss object, which a
// guided p never has, so the window test is one compare) and only those pixels walk it; once a sequence runs, that is the disocclusions.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "denoise_variance.h"
#include "post_checks.h"
#include "post_device.h"
#include "temporal.h"

namespace rayn {
namespace {

constexpr int HALO = 3, TILE = 16, SPAN = TILE + 2 * HALO; // 22

// hA: plane A of the history, (r, g, b, n'); only n' is read - the colour is the caller's planar one.  a / b as k_vdenoise_pack writes
// them (b by the same write_guide_record); a guide that is switched off is not read (its pointer may be null), b is null when both are off.  width * height < 2^31.
__global__ void __launch_bounds__(256) k_tvdenoise_pack(uint32_t width, uint32_t height, uint32_t blocks_x, const float* __restrict__ color,
                                                        const float* __restrict__ alpha, const float* __restrict__ normal,
                                                        const uint32_t* __restrict__ gobj, const float4* __restrict__ hA,
                                                        const float2* __restrict__ mom, float4* __restrict__ a, float4* __restrict__ b) {
    __shared__ float s_lum[SPAN][SPAN];
    __shared__ uint32_t s_obj[SPAN][SPAN];
    const uint32_t by = blockIdx.x / blocks_x, bx = blockIdx.x - by * blocks_x;
    const uint32_t x = bx * TILE + threadIdx.x, y = by * TILE + threadIdx.y;
    const bool inside = x < width && y < height;
    const uint32_t p = inside ? x + y * width : 0u; // < 2^31
    const size_t f = (size_t)p * 3u;
    float cr = 0.0f, cg = 0.0f, cb = 0.0f, v = quiet_nan();
    uint32_t obj = MISS_OBJECT;
    bool spatial = false;
    if (inside) {
        cr = color[f]; cg = color[f + 1]; cb = color[f + 2];
        obj = gobj[p];
        const float n1 = hA[p].w;
        if (obj != MISS_OBJECT && finite3(cr, cg, cb) && n1 >= 1.0f) {
            if (n1 >= 4.0f) {
                const float2 m = mom[p];
                const float d = m.y - m.x * m.x;
                v = (d > 0.0f ? d : 0.0f) / n1;
            } else {
                spatial = true;
            }
        }
    }
    if (__syncthreads_or(spatial)) { // block-uniform
        const int x0 = (int)(bx * TILE) - HALO, y0 = (int)(by * TILE) - HALO;
        for (uint32_t i = threadIdx.y * TILE + threadIdx.x; i < (uint32_t)(SPAN * SPAN); i += 256u) {
            const uint32_t ly = i / SPAN, lx = i - ly * SPAN;
            const int qx = x0 + (int)lx, qy = y0 + (int)ly;
            float l = 0.0f;
            uint32_t o = MISS_OBJECT;
            if (qx >= 0 && qx < (int)width && qy >= 0 && qy < (int)height) {
                const uint32_t q = (uint32_t)qx + (uint32_t)qy * width;
                const size_t fq = (size_t)q * 3u;
                const float qr = color[fq], qg = color[fq + 1], qb = color[fq + 2];
                if (hA[q].w >= 1.0f && finite3(qr, qg, qb)) {
                    l = luminance(qr, qg, qb);
                    o = gobj[q];
                }
            }
            s_lum[ly][lx] = l;
            s_obj[ly][lx] = o;
        }
        __syncthreads();
        if (spatial) {
            float k = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
            for (int dy = 0; dy < 2 * HALO + 1; dy++) {
#pragma unroll
                for (int dx = 0; dx < 2 * HALO + 1; dx++) {
                    if (s_obj[threadIdx.y + dy][threadIdx.x + dx] != obj) continue;
                    const float l = s_lum[threadIdx.y + dy][threadIdx.x + dx];
                    k += 1.0f;
                    s1 += l;
                    s2 += l * l;
                }
            }
            // k >= 1: the centre counts
            const float mu = s1 / k;
            const float d = s2 / k - mu * mu;
            v = d > 0.0f ? d : 0.0f;
        }
    }
    if (!inside) return;
    if (!__builtin_isfinite(v)) v = quiet_nan();
    a[p] = make_float4(cr, cg, cb, v);
    write_guide_record(b, p, f, normal, alpha);
}

} // namespace

const char* denoise_temporal_check_args(uint32_t width, uint32_t height, uint32_t iterations, float sigma_luminance, float sigma_normal,
                                        float sigma_alpha, const float* color, const float* alpha, const float* normal, const uint32_t* g_object,
                                        const void* history, size_t history_bytes, const void* moments, size_t moments_bytes,
                                        const float* out_color, const float* out_variance, const void* scratch, size_t scratch_bytes) {
    if (const char* why = check_size(width, height)) return why;
    if (const char* why = check_atrous_params(iterations, sigma_luminance, "sigma_luminance must be 0 (off) or in [2^-30, 2^30]", sigma_normal, sigma_alpha,
                                              color && g_object && history && moments && out_color && scratch, normal, alpha))
        return why;
    const size_t n = (size_t)width * height, hist = temporal_history_bytes(width, height), mom = temporal_moments_bytes(width, height);
    if (history_bytes < hist) return "history smaller than rayn_temporal_history_bytes(width, height)";
    if (moments_bytes < mom) return "moments smaller than rayn_temporal_moments_bytes(width, height)";
    if (scratch_bytes < denoise_variance_scratch_bytes(width, height)) return "scratch smaller than rayn_denoise_variance_scratch_bytes(width, height)";
    if ((uintptr_t)scratch % 16u) return "scratch not 16-byte aligned";
    if ((uintptr_t)history % 16u) return "history not 16-byte aligned";
    if ((uintptr_t)moments % 16u) return "moments not 16-byte aligned";
    if ((uintptr_t)g_object % 4u) return "d_gbuffer_object not 4-byte aligned";
    const Span in[6] = {{color, 12u * n}, {alpha, 4u * n}, {normal, 12u * n}, {g_object, 4u * n}, {history, hist}, {moments, mom}};
    const Span work[3] = {{out_color, 12u * n}, {out_variance, 4u * n}, {scratch, scratch_bytes}};
    int j;
    if (first_overlap(in, 6, work, 3, nullptr, &j)) return j < 2 ? "an output must not alias an input" : "the scratch must not alias an input";
    if (overlap(out_variance, 4u * n, out_color, 12u * n)) return "d_out_variance must not alias d_out_color";
    if (overlap(scratch, scratch_bytes, out_color, 12u * n) || overlap(scratch, scratch_bytes, out_variance, 4u * n)) return "the scratch must not alias an output";
    return nullptr;
}

// history: read by the pack kernel (n'), written by pass 0 when feedback != 0 - kernels of one stream, in that order
static void launch_tvdenoise(hipStream_t s, uint32_t width, uint32_t height, uint32_t iterations, float sigma_luminance, float sigma_normal, float sigma_alpha,
                             const float* color, const float* alpha, const float* normal, const uint32_t* g_object, const void* history,
                             void* history_out, const void* moments, float* out_color, float* out_variance, void* scratch, float feedback) {
    const uint32_t terms = vatrous_terms(sigma_luminance, sigma_normal, sigma_alpha);
    const uint32_t blocks_x = (width + 15u) / 16u, blocks_y = (height + 15u) / 16u;
    hipLaunchKernelGGL(k_tvdenoise_pack, dim3(blocks_x * blocks_y), dim3(TILE, TILE), 0, s, width, height, blocks_x, color,
                       (terms & VATROUS_ALPHA) ? alpha : nullptr, (terms & VATROUS_NORMAL) ? normal : nullptr, g_object, (const float4*)history,
                       (const float2*)moments, (float4*)scratch, vatrous_guides(terms, width, height, scratch));
    launch_vatrous_passes(s, width, height, iterations, sigma_luminance, sigma_normal, sigma_alpha, out_color, out_variance, scratch, history_out, feedback);
}

void launch_denoise_temporal_variance(hipStream_t s, uint32_t width, uint32_t height, uint32_t iterations, float sigma_luminance,
                                      float sigma_normal, float sigma_alpha, const float* color, const float* alpha, const float* normal,
                                      const uint32_t* g_object, const void* history, const void* moments, float* out_color, float* out_variance,
                                      void* scratch) {
    launch_tvdenoise(s, width, height, iterations, sigma_luminance, sigma_normal, sigma_alpha, color, alpha, normal, g_object, history, nullptr, moments,
                     out_color, out_variance, scratch, 0.0f);
}

const char* denoise_temporal_feedback_check_args(uint32_t width, uint32_t height, uint32_t iterations, float sigma_luminance, float sigma_normal,
                                                 float sigma_alpha, const float* color, const float* alpha, const float* normal,
                                                 const uint32_t* g_object, const void* history, size_t history_bytes, const void* moments,
                                                 size_t moments_bytes, const float* out_color, const float* out_variance, const void* scratch,
                                                 size_t scratch_bytes, float feedback) {
    if (const char* why = denoise_temporal_check_args(width, height, iterations, sigma_luminance, sigma_normal, sigma_alpha, color, alpha, normal, g_object,
                                                      history, history_bytes, moments, moments_bytes, out_color, out_variance, scratch, scratch_bytes))
        return why;
    if (!(feedback >= 0.0f && feedback <= 1.0f)) return "feedback must be finite and in [0, 1]";
    // the history is an output here: the checks above keep it off the outputs and the scratch; these keep it off the other inputs
    const size_t n = (size_t)width * height, hist = temporal_history_bytes(width, height);
    const Span in[5] = {{color, 12u * n}, {alpha, 4u * n}, {normal, 12u * n}, {g_object, 4u * n}, {moments, temporal_moments_bytes(width, height)}};
    const Span hs = {history, hist};
    if (first_overlap(&hs, 1, in, 5)) return "the history must not alias an input";
    return nullptr;
}

void launch_denoise_temporal_variance_feedback(hipStream_t s, uint32_t width, uint32_t height, uint32_t iterations, float sigma_luminance,
                                               float sigma_normal, float sigma_alpha, const float* color, const float* alpha, const float* normal,
                                               const uint32_t* g_object, void* history, const void* moments, float* out_color, float* out_variance,
                                               void* scratch, float feedback) {
    launch_tvdenoise(s, width, height, iterations, sigma_luminance, sigma_normal, sigma_alpha, color, alpha, normal, g_object, history, history, moments,
                     out_color, out_variance, scratch, feedback);
}

} // namespace rayn
