// denoise_variance.hip — the variance-guided a-trous filter of the film's Color channel (rayn_hip_denoise_variance_device): the spatial
// half of SVGF (Schied et al., HPG 2017) driven by what a progressive render measured.  An extension: rayn has neither a denoiser nor
// a progressive render.  It runs downstream of the film: it reads the mean film's Color / Alpha / WorldNormal planes and the
// progressive state (the per-pixel Welford m2 of the luminance and the per-tile epoch counts) and writes a new Color plane and,
// optionally, the filtered variance; the film and the state are not touched.
//
// The definition (include/rayn_hip.h; tests/denoise_variance_np.py restates it in numpy and the tests compare bit
// for bit).  Pixel p of tile k (the reference's x-major grid; under-covered pixels are in no tile) with n = the tile's epochs starts
// with v_p = m2_p / (float)((uint64)n (n - 1)), the variance of the mean of its luminance.  p is GUIDED when it lies in a tile, n >= 2,
// v_p is finite and >= 0 and c_p has three finite components; a pixel that is not guided passes through every pass unchanged and is
// skipped as a tap.  Pass i = 0 .. L-1 with step s = 2^i, on the previous pass's (c, v), for every guided p:
//     l_x = (0.2126f c_x.r + 0.7152f c_x.g) + 0.0722f c_x.b
//     g_p = (sum k_j v_j) / (sum k_j)    3x3 at unit spacing around p, k = 1/4 centre, 1/8 edges, 1/16 corners, centre first, then raster
//                                        order; taps outside the image or not guided are left out of both sums
//     inv = 1.0f / (sigma_luminance sqrtf(g_p) + 1e-8f)
//     W = 9/64, S = W c_p, V = (W W) v_p, then the 24 other taps of the 5x5 B3 stencil in raster order, q = p + (kx, ky) s, skipped
//     outside the image or where q is not guided:
//         e = (fabsf(l_p - l_q) inv + d_n kn) + d_a ka      (d_n, d_a, kn, ka as in denoise.hip; a term whose sigma is 0 is left out)
//         w = (h[ky+2] h[kx+2]) expf(-e);  a NaN w skips the tap;  W += w, S += w c_q, V += (w w) v_q
//     c'_p = S / W, v'_p = V / (W W)
// and p stays guided for the next pass when c'_p has three finite components and v'_p is finite (it is >= 0 by construction); else
// it keeps c'_p and is not guided from then on (only an overflow gets there).  f32 throughout, built with -ffp-contract=off, IEEE
// division and square root; expf is the pinned dm_expf of rayn_detmath.h, evaluated through dmf_expf.
//
// Layout, as denoise.hip's: 16-byte records in the caller's scratch, one thread per pixel in 16x16 blocks, every tap a plain global
// load served by L2 / the Infinity Cache.  The pack kernel writes A = (r, g, b, v) - ping-ponged by the passes - and B = (nx, ny, nz,
// alpha) - written once; "not guided" is v = NaN, so a tap needs no third load: 48 B of scratch per pixel and two 128-bit loads per
// tap, as the fixed-sigma filter.  Per pixel a pass adds eight dword loads (the neighbours' v, lines the 5x5 taps of step 1 touch
// anyway), one sqrtf and two divisions; per tap a luminance, fabsf, a multiply, w w and one more accumulate.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "denoise_variance.h"
#include "post_checks.h"
#include "post_device.h"
#include "progressive.h"

namespace rayn {
namespace {

constexpr uint32_t TERM_LUMINANCE = VATROUS_LUMINANCE, TERM_NORMAL = VATROUS_NORMAL, TERM_ALPHA = VATROUS_ALPHA;

struct VarGeom { uint32_t width, height, tile_w, tile_h, tiles_x, tiles_y; };

// One thread per pixel: planar colour, alpha and normal, the state's m2 (plane s2, .w) and the tile records -> a[p] = (r, g, b, v or
// NaN), b[p] = (nx, ny, nz, alpha).  A guide that is switched off is not read (its pointer may be null) and reads as 0; b is null
// when both are off.  n < 2^31; the tile index of a pixel inside the grid is < tiles_x * tiles_y = the number of records.
__global__ void __launch_bounds__(256) k_vdenoise_pack(VarGeom g, const float* __restrict__ color, const float* __restrict__ alpha,
                                                       const float* __restrict__ normal, const float4* __restrict__ s2,
                                                       const uint4* __restrict__ rec, float4* __restrict__ a, float4* __restrict__ b) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= g.width * g.height) return;
    const uint32_t y = p / g.width, x = p - y * g.width;
    const size_t f = (size_t)p * 3u;
    const float cr = color[f], cg = color[f + 1], cb = color[f + 2];
    // the reference's tile order is x-major (src/film.rs:399-427): tile k = column k / tiles_y, row k % tiles_y
    const uint32_t tx = x / g.tile_w, ty = y / g.tile_h;
    float v = quiet_nan();
    if (tx < g.tiles_x && ty < g.tiles_y) {
        const uint32_t n = rec[tx * g.tiles_y + ty].x;
        if (n >= 2u) {
            const float vp = s2[p].w / (float)((uint64_t)n * (uint64_t)(n - 1u));
            if (__builtin_isfinite(vp) && vp >= 0.0f && finite3(cr, cg, cb)) v = vp;
        }
    }
    a[p] = make_float4(cr, cg, cb, v);
    write_guide_record(b, p, f, normal, alpha);
}

// What pass 0 of rayn_hip_denoise_temporal_variance_feedback_device gets on top of a pass's arguments: plane A of the temporal history and
// the strength.  The plain pass carries nothing, so its arguments and its code are what they were before there was a feedback.
template <bool FEEDBACK> struct VatrousFeedback {};
template <> struct VatrousFeedback<true> { float4* hist; float beta; };

// One pass with step `step` (a power of two <= 128).  Blocks of 16x16 threads, one per 16x16 block of the image, in a 1-D grid
// (row-major, blocks_x per row).  TERMS: which of the luminance / normal / alpha terms are on.  LAST: write the planar colour (and the
// variance plane, when there is one) instead of the next record plane.  FEEDBACK (launched for pass 0, step 1, only): also blend the
// pass's colour into the history, fb = c + beta * (c' - c) per component, where v' is not NaN and fb is finite; n' in .w keeps its bits:
// three dword stores, which compile to one global_store_dwordx3, and no read of the history.  The taps come from `a`, never from the
// history, so the write races with no neighbour's read.
template <uint32_t TERMS, bool LAST, bool FEEDBACK = false>
__global__ void __launch_bounds__(256) k_vatrous(uint32_t width, uint32_t height, uint32_t blocks_x, uint32_t step, float sigma_luminance,
                                                 float sigma_normal, float sigma_alpha, const float4* __restrict__ a,
                                                 const float4* __restrict__ b, float4* __restrict__ a_out, float* __restrict__ out_color,
                                                 float* __restrict__ out_variance, VatrousFeedback<FEEDBACK> fb = {}) {
    const uint32_t by = blockIdx.x / blocks_x, bx = blockIdx.x - by * blocks_x;
    const uint32_t x = bx * 16u + threadIdx.x, y = by * 16u + threadIdx.y;
    if (x >= width || y >= height) return;
    const uint32_t p = x + y * width; // < 2^31
    const float4 ap = a[p];
    float r = ap.x, g = ap.y, bl = ap.z, v = ap.w;
    if (v == v) { // guided
        float inv = 0.0f;
        if (TERMS & TERM_LUMINANCE) {
            // the 3x3 pre-filter of the variance at unit spacing: centre, then raster order
            float num = 0.25f * v, den = 0.25f;
#pragma unroll
            for (int dy = -1; dy <= 1; dy++) {
                const uint32_t qy = y + (uint32_t)dy; // unsigned wrap: -1 past the edge becomes >= height
                if (qy >= height) continue;
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) {
                    if (dx == 0 && dy == 0) continue;
                    const uint32_t qx = x + (uint32_t)dx;
                    if (qx >= width) continue;
                    const float vq = a[qx + qy * width].w;
                    if (vq != vq) continue;
                    const float k = (dx == 0 || dy == 0) ? 0.125f : 0.0625f;
                    num += k * vq;
                    den += k;
                }
            }
            inv = 1.0f / (sigma_luminance * sqrtf(num / den) + 1e-8f);
        }
        const float kn = (TERMS & TERM_NORMAL) ? 1.0f / (sigma_normal * sigma_normal) : 0.0f;
        const float ka = (TERMS & TERM_ALPHA) ? 1.0f / (sigma_alpha * sigma_alpha) : 0.0f;
        const float4 bp = (TERMS & (TERM_NORMAL | TERM_ALPHA)) ? b[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const float lp = luminance(r, g, bl);
        const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
        float W = 9.0f / 64.0f, Sr = W * r, Sg = W * g, Sb = W * bl, V = (W * W) * v;
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
                const float4 aq = a[q];
                if (aq.w != aq.w) continue; // not guided
                float e = 0.0f; // 0 + t == t for every term t (t >= +0, inf or NaN): the same bits as the definition's sum
                if (TERMS & TERM_LUMINANCE) e = e + fabsf(lp - luminance(aq.x, aq.y, aq.z)) * inv;
                if (TERMS & (TERM_NORMAL | TERM_ALPHA)) {
                    const float4 bq = b[q];
                    if (TERMS & TERM_NORMAL) {
                        const float dx = bp.x - bq.x, dy = bp.y - bq.y, dz = bp.z - bq.z;
                        e = e + (dx * dx + dy * dy + dz * dz) * kn;
                    }
                    if (TERMS & TERM_ALPHA) {
                        const float da = bp.w - bq.w;
                        e = e + (da * da) * ka;
                    }
                }
                const float w = (h[ky + 2] * h[kx + 2]) * dmf_expf(-e);
                if (w != w) continue;
                W += w;
                Sr += w * aq.x;
                Sg += w * aq.y;
                Sb += w * aq.z;
                V += (w * w) * aq.w;
            }
        }
        r = Sr / W; // W >= 9/64
        g = Sg / W;
        bl = Sb / W;
        v = V / (W * W);
        if (!(finite3(r, g, bl) && __builtin_isfinite(v))) v = quiet_nan(); // an overflow: not guided from here on
    }
    if constexpr (FEEDBACK) {
        if (v == v) { // not guided on entry, or dropped by the overflow rule: the history keeps its colour
            const float dr = r - ap.x, dg = g - ap.y, db = bl - ap.z;
            const float mr = fb.beta * dr, mg = fb.beta * dg, mb = fb.beta * db;
            const float fr = ap.x + mr, fg = ap.y + mg, fbl = ap.z + mb;
            if (finite3(fr, fg, fbl)) {
                float* hp = (float*)(fb.hist + p); // 16-byte aligned; .w = n' is not written
                hp[0] = fr;
                hp[1] = fg;
                hp[2] = fbl;
            }
        }
    }
    if (LAST) {
        const size_t f = (size_t)p * 3u;
        out_color[f] = r;
        out_color[f + 1] = g;
        out_color[f + 2] = bl;
        if (out_variance) out_variance[p] = v;
    } else {
        a_out[p] = make_float4(r, g, bl, v);
    }
}

// hist != nullptr: the feedback variant (the caller passes it for pass 0 only)
template <uint32_t TERMS>
void launch_pass(hipStream_t s, bool last, dim3 grid, uint32_t width, uint32_t height, uint32_t blocks_x, uint32_t step, float sl, float sn,
                 float sa, const float4* a, const float4* b, float4* a_out, float* out_color, float* out_variance, float4* hist, float beta) {
    const dim3 block(16, 16);
    if (hist) {
        const VatrousFeedback<true> fb{hist, beta};
        if (last)
            hipLaunchKernelGGL((k_vatrous<TERMS, true, true>), grid, block, 0, s, width, height, blocks_x, step, sl, sn, sa, a, b, a_out, out_color, out_variance, fb);
        else
            hipLaunchKernelGGL((k_vatrous<TERMS, false, true>), grid, block, 0, s, width, height, blocks_x, step, sl, sn, sa, a, b, a_out, out_color, out_variance, fb);
    } else if (last)
        hipLaunchKernelGGL((k_vatrous<TERMS, true>), grid, block, 0, s, width, height, blocks_x, step, sl, sn, sa, a, b, a_out, out_color, out_variance, VatrousFeedback<false>{});
    else
        hipLaunchKernelGGL((k_vatrous<TERMS, false>), grid, block, 0, s, width, height, blocks_x, step, sl, sn, sa, a, b, a_out, out_color, out_variance, VatrousFeedback<false>{});
}

} // namespace

size_t denoise_variance_scratch_bytes(uint32_t width, uint32_t height) {
    return atrous_scratch_bytes(width, height);
}

const char* denoise_variance_check_args(const rayn_frame_params* p, uint32_t iterations, float sigma_luminance, float sigma_normal,
                                        float sigma_alpha, const float* color, const float* alpha, const float* normal, const void* state,
                                        size_t state_bytes, const float* out_color, const float* out_variance, const void* scratch,
                                        size_t scratch_bytes) {
    if (const char* why = progressive_check_geometry(p, state, state_bytes)) return why;
    if (const char* why = check_atrous_params(iterations, sigma_luminance, "sigma_luminance must be 0 (off) or in [2^-30, 2^30]", sigma_normal, sigma_alpha,
                                              color && out_color && scratch, normal, alpha))
        return why;
    if (scratch_bytes < denoise_variance_scratch_bytes(p->width, p->height)) return "scratch smaller than rayn_denoise_variance_scratch_bytes(width, height)";
    if ((uintptr_t)scratch % 16u) return "scratch not 16-byte aligned";
    if (out_color == color) return "d_out_color must not be d_color";
    if (out_variance && (out_variance == color || out_variance == alpha || out_variance == normal || (const void*)out_variance == state ||
                         out_variance == out_color))
        return "d_out_variance must not be an input or d_out_color";
    return nullptr;
}

// The passes of k_vatrous on packed records: plane 0 of the scratch holds A = (r, g, b, v or NaN), plane 2 B = (nx, ny, nz, alpha) when a
// guide is on; plane 1 is the other half of the ping-pong.  Shared by every entry that packs a variance (this file, denoise_temporal.hip).
// With a history and feedback != 0, pass 0 is the feedback variant; every other pass, and every pass without them, is the plain kernel.
void launch_vatrous_passes(hipStream_t s, uint32_t width, uint32_t height, uint32_t iterations, float sigma_luminance, float sigma_normal,
                           float sigma_alpha, float* out_color, float* out_variance, void* scratch, void* history, float feedback) {
    const uint32_t n = width * height;
    const uint32_t terms = vatrous_terms(sigma_luminance, sigma_normal, sigma_alpha);
    float4* plane[2] = {(float4*)scratch, (float4*)scratch + n};
    float4* guides = vatrous_guides(terms, width, height, scratch);
    const uint32_t blocks_x = (width + 15u) / 16u, blocks_y = (height + 15u) / 16u;
    const dim3 grid(blocks_x * blocks_y); // < 2^27 blocks
    for (uint32_t i = 0; i < iterations; i++) {
        const bool last = i + 1 == iterations;
        const float4* in = plane[i & 1u];
        float4* out = plane[(i + 1u) & 1u];
        const uint32_t step = 1u << i;
        float4* hist = (i == 0 && feedback != 0.0f) ? (float4*)history : nullptr;
        with_terms<3>(terms, [&](auto T) {
            launch_pass<decltype(T)::value>(s, last, grid, width, height, blocks_x, step, sigma_luminance, sigma_normal, sigma_alpha, in, guides, out, out_color,
                                            out_variance, hist, feedback);
        });
    }
}

void launch_denoise_variance(hipStream_t s, const rayn_frame_params& p, uint32_t iterations, float sigma_luminance, float sigma_normal,
                             float sigma_alpha, const float* color, const float* alpha, const float* normal, const void* state, float* out_color,
                             float* out_variance, void* scratch) {
    const ProgLayout L = progressive_layout(p.width, p.height, p.tile_w, p.tile_h);
    const uint32_t width = p.width, height = p.height, n = width * height;
    const uint32_t terms = vatrous_terms(sigma_luminance, sigma_normal, sigma_alpha);
    const char* base = (const char*)state;
    const VarGeom g{width, height, p.tile_w, p.tile_h, L.n_tiles / L.tiles_y, L.tiles_y};
    hipLaunchKernelGGL(k_vdenoise_pack, dim3((n + 255u) / 256u), dim3(256), 0, s, g, color, (terms & VATROUS_ALPHA) ? alpha : nullptr,
                       (terms & VATROUS_NORMAL) ? normal : nullptr, (const float4*)(base + L.off_s2), (const uint4*)(base + L.off_records),
                       (float4*)scratch, vatrous_guides(terms, width, height, scratch));
    launch_vatrous_passes(s, width, height, iterations, sigma_luminance, sigma_normal, sigma_alpha, out_color, out_variance, scratch);
}

} // namespace rayn

extern "C" size_t rayn_denoise_variance_scratch_bytes(uint32_t width, uint32_t height) { return rayn::denoise_variance_scratch_bytes(width, height); }
