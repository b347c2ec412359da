// display.hip — the HDR display transform of the film's Color channel: auto exposure (log-average metering with adaptation over the
// frames of a sequence), bloom (a pyramid of 2x2 box downsamples and bilinear 2x upsamples of the bright pass) and a tone operator
// (linear, extended Reinhard on luminance, Narkowicz's ACES fit), in front of save_to's own gamma 2.2 and 8-bit quantisation
// (rayn_hip_display_pixels_device, rayn_hip_display_color_device).  An extension: rayn's save_to clamps the film to [0, 1].  It runs
// downstream of the film: it reads the finished Color / Alpha / Background planes; the film itself is not touched.
//
// The definition is in include/rayn_hip.h and DESIGN.md section 8; tests/display_np.py restates it in numpy and the tests compare bit
// for bit.  f32 throughout, built with -ffp-contract=off and IEEE division; logf / expf / powf are the pinned dm_logf / dm_expf /
// dm_powf of rayn_detmath.h.  With exposure scale 1, the linear operator and no bloom the image is save_to's, byte for byte.
//
// Metering: k_display_meter sums dm_logf of the luminance over blocks of 256 consecutive film pixels in a FIXED order - the halving tree
// a[j] += a[j + s], s = 128 .. 1, whose s = 128 and 64 steps go through LDS and whose s <= 32 steps are wave shuffles - and
// k_display_expose (one block) adds the block partials, thread t the partials t, t + 256, ... in ascending order, runs the same tree,
// applies the adaptation to the two-word state and leaves the exposure scale e in the scratch header.  Every later kernel reads e from
// there: the host never sees it, so nothing synchronises.
//
// Bloom layout: levels 1 .. L are planes of 16-byte records (r, g, b, 0), as denoise.hip's are: a tap is one 128-bit load, lane i at
// base + 16 i in the upsample (the widest coalesced access) and two adjacent records per lane in the downsample; planar floats would
// move 12 bytes per pixel instead of 16 but cost three loads per tap, the downsample's at stride 2.  Level 0 is never stored: the first
// downsample and the final kernel recompute the bright pass from the film.  The upsample adds into its level in place (U_k = D_k + up
// (U_k+1) reads D_k only at its own pixel), and the last one is fused with tone, gamma and quantisation.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rayn_detmath.h"
#include "display.h"
#include "post_checks.h"
#include "post_device.h"
#include "save_to.h"

namespace rayn {
namespace {

constexpr uint32_t MAX_LEVELS = 8u, HEADER_BYTES = 256u;
enum Tone : uint32_t { TONE_LINEAR = 0u, TONE_REINHARD = 1u, TONE_ACES = 2u }; // rayn_display_params.tone

// save_to.hip's rust_min / rust_max / quant8 / saturate1 / gamma22, written the same way (a NaN operand yields the OTHER operand)
__device__ inline float rmin(float a, float b) { return a != a ? b : (b != b ? a : (a < b ? a : b)); }
__device__ inline float rmax(float a, float b) { return a != a ? b : (b != b ? a : (a > b ? a : b)); }
__device__ inline uint8_t quant8(float v) { return (uint8_t)rmax(rmin(v * 255.0f, 255.0f), 0.0f); }
__device__ inline float saturate1(float x) { return rmin(rmax(x, 0.0f), 1.0f); }
__device__ inline float gamma22(float x) { return dm_powf(x, 1.0f / 2.2f); }

__device__ inline float fin0(float v) { return __builtin_isfinite(v) ? v : 0.0f; }
__device__ inline float bright(float e, float c, float threshold) { return rmax(e * fin0(c) - threshold, 0.0f); }

// the input colour of film pixel f: color, or color + background in the Color + Background arm
template <int ARM>
__device__ inline void load_c(const float* __restrict__ color, const float* __restrict__ background, size_t f, float c[3]) {
    for (int k = 0; k < 3; k++) {
        c[k] = color[3 * f + k];
        if (ARM == SAVE_COLOR_BG) c[k] = c[k] + background[3 * f + k];
    }
}

// The halving tree over the 256 values of a block (thread t holds a[t]): a[j] += a[j + s] for s = 128, 64 through LDS - after both,
// a[j] = (a[j] + a[j + 128]) + (a[j + 64] + a[j + 192]) for j < 64 - then s = 32 .. 1 inside wave 0 by shuffle.  The result is thread
// 0's; the counts go the same way in u32.
__device__ inline void block_tree(float& v, uint32_t& k) {
    __shared__ float sv[256];
    __shared__ uint32_t sk[256];
    const uint32_t t = threadIdx.x;
    sv[t] = v;
    sk[t] = k;
    __syncthreads();
    if (t < 64u) {
        v = (sv[t] + sv[t + 128u]) + (sv[t + 64u] + sv[t + 192u]);
        k = (sk[t] + sk[t + 128u]) + (sk[t + 64u] + sk[t + 192u]);
        for (int s = 32; s >= 1; s >>= 1) {
            v = v + __shfl_down(v, s, 64);
            k = k + __shfl_down(k, s, 64);
        }
    }
    __syncthreads(); // the LDS arrays may be written again by a second call
}

// Stage 1: one thread per film pixel, one logarithm each; block b writes partial[b] and count[b].  n < 2^31.
template <int ARM>
__global__ void __launch_bounds__(256) k_display_meter(uint32_t n, const float* __restrict__ color, const float* __restrict__ background,
                                                       float* __restrict__ partial, uint32_t* __restrict__ count) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    float v = 0.0f;
    uint32_t k = 0u;
    if (i < n) {
        float c[3];
        load_c<ARM>(color, background, i, c);
        const float l = luminance(c[0], c[1], c[2]);
        if (__builtin_isfinite(c[0]) && __builtin_isfinite(c[1]) && __builtin_isfinite(c[2]) && l > 0.0f) {
            v = dm_logf(rmax(l, 1e-4f));
            k = 1u;
        }
    }
    block_tree(v, k);
    if (threadIdx.x == 0u) {
        partial[blockIdx.x] = v;
        count[blockIdx.x] = k;
    }
}

// Stage 2: one block.  state = {m (f32), valid (u32)}; header[0] = e, header[1] = m; out_meter (null-able) = {m, e}.
__global__ void __launch_bounds__(256) k_display_expose(uint32_t nb, const float* __restrict__ partial, const uint32_t* __restrict__ count, float key,
                                                        float adapt, uint32_t* __restrict__ state, float* __restrict__ header,
                                                        float* __restrict__ out_meter) {
    float v = 0.0f;
    uint32_t k = 0u;
    for (uint32_t i = threadIdx.x; i < nb; i += 256u) {
        v = v + partial[i];
        k = k + count[i];
    }
    block_tree(v, k);
    if (threadIdx.x != 0u) return;
    float m = __uint_as_float(state[0]), e = 1.0f;
    if (k != 0u) {
        const float m_now = v / (float)k;
        m = (state[1] == 0u || adapt == 1.0f) ? m_now : m + (m_now - m) * adapt;
        e = key / dm_expf(m);
        state[0] = __float_as_uint(m);
        state[1] = 1u;
    }
    header[0] = e;
    header[1] = m;
    if (out_meter) {
        out_meter[0] = m;
        out_meter[1] = e;
    }
}

// manual exposure with the {m, e} output requested
__global__ void k_display_put2(float* __restrict__ out, float a, float b) {
    out[0] = a;
    out[1] = b;
}

// First downsample, fused with the bright pass: one thread per level-1 pixel, the four taps computed from the film.  w1 * h1 < 2^31.
template <int ARM>
__global__ void __launch_bounds__(256) k_display_down0(uint32_t w0, uint32_t h0, uint32_t w1, uint32_t h1, const float* __restrict__ color,
                                                       const float* __restrict__ background, const float* __restrict__ e_ptr, float e_manual,
                                                       float threshold, float4* __restrict__ out) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= w1 * h1) return;
    const float e = e_ptr ? *e_ptr : e_manual;
    const uint32_t y = p / w1, x = p - y * w1;
    const uint32_t x0 = 2u * x, y0 = 2u * y; // <= w0 - 1, h0 - 1: w1 = (w0 + 1) / 2
    const uint32_t x1 = x0 + 1u < w0 ? x0 + 1u : w0 - 1u, y1 = y0 + 1u < h0 ? y0 + 1u : h0 - 1u;
    float a[3], b[3], c[3], d[3], r[3];
    load_c<ARM>(color, background, (size_t)x0 + (size_t)y0 * w0, a);
    load_c<ARM>(color, background, (size_t)x1 + (size_t)y0 * w0, b);
    load_c<ARM>(color, background, (size_t)x0 + (size_t)y1 * w0, c);
    load_c<ARM>(color, background, (size_t)x1 + (size_t)y1 * w0, d);
    for (int k = 0; k < 3; k++)
        r[k] = ((bright(e, a[k], threshold) + bright(e, b[k], threshold)) + (bright(e, c[k], threshold) + bright(e, d[k], threshold))) * 0.25f;
    out[p] = make_float4(r[0], r[1], r[2], 0.0f);
}

// Downsample of level k - 1 (wp x hp) into level k (w x h): one thread per pixel of level k.
__global__ void __launch_bounds__(256) k_display_down(uint32_t wp, uint32_t hp, uint32_t w, uint32_t h, const float4* __restrict__ in,
                                                      float4* __restrict__ out) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= w * h) return;
    const uint32_t y = p / w, x = p - y * w;
    const uint32_t x0 = 2u * x, y0 = 2u * y;
    const uint32_t x1 = x0 + 1u < wp ? x0 + 1u : wp - 1u, y1 = y0 + 1u < hp ? y0 + 1u : hp - 1u;
    const float4 a = in[x0 + y0 * wp], b = in[x1 + y0 * wp], c = in[x0 + y1 * wp], d = in[x1 + y1 * wp];
    out[p] = make_float4(((a.x + b.x) + (c.x + d.x)) * 0.25f, ((a.y + b.y) + (c.y + d.y)) * 0.25f, ((a.z + b.z) + (c.z + d.z)) * 0.25f, 0.0f);
}

// The two taps and weights of the bilinear 2x filter along one axis: destination coordinate x, source extent ws (>= 1).
__device__ inline void up_axis(uint32_t x, uint32_t ws, uint32_t& t0, uint32_t& t1, float& w0, float& w1) {
    const uint32_t h = x >> 1;
    if (x & 1u) {
        t0 = h;
        t1 = h + 1u;
        w0 = 0.75f;
        w1 = 0.25f;
    } else {
        t0 = h ? h - 1u : 0u;
        t1 = h;
        w0 = 0.25f;
        w1 = 0.75f;
    }
    t0 = t0 < ws ? t0 : ws - 1u;
    t1 = t1 < ws ? t1 : ws - 1u;
}

// up(src)(x, y) for a destination pixel (x, y); src is ws x hs
__device__ inline void upsample(const float4* __restrict__ src, uint32_t ws, uint32_t hs, uint32_t x, uint32_t y, float r[3]) {
    uint32_t x0, x1, y0, y1;
    float wx0, wx1, wy0, wy1;
    up_axis(x, ws, x0, x1, wx0, wx1);
    up_axis(y, hs, y0, y1, wy0, wy1);
    const float4 a = src[x0 + y0 * ws], b = src[x1 + y0 * ws], c = src[x0 + y1 * ws], d = src[x1 + y1 * ws];
    r[0] = wy0 * (wx0 * a.x + wx1 * b.x) + wy1 * (wx0 * c.x + wx1 * d.x);
    r[1] = wy0 * (wx0 * a.y + wx1 * b.y) + wy1 * (wx0 * c.y + wx1 * d.y);
    r[2] = wy0 * (wx0 * a.z + wx1 * b.z) + wy1 * (wx0 * c.z + wx1 * d.z);
}

// U_k = D_k + up(U_k+1), in place in level k (w x h); src = level k + 1 (ws x hs).
__global__ void __launch_bounds__(256) k_display_up(uint32_t w, uint32_t h, uint32_t ws, uint32_t hs, const float4* __restrict__ src,
                                                    float4* __restrict__ dst) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= w * h) return;
    const uint32_t y = p / w, x = p - y * w;
    float u[3];
    upsample(src, ws, hs, x, y, u);
    const float4 dk = dst[p];
    dst[p] = make_float4(dk.x + u[0], dk.y + u[1], dk.z + u[2], 0.0f);
}

// The final kernel: exposure, the last upsample of the bloom (level 0 = the bright pass, recomputed), tone, then the arm's own chain of
// save_to.  OUT8: one thread per OUTPUT pixel i (rows top-down, reading film pixel x + (height - 1 - y) * width, as k_save_to), writing
// the 8-bit image; otherwise one thread per film pixel writing the float plane d.  n = width * height < 2^31.
template <int ARM, bool OUT8>
__global__ void __launch_bounds__(256) k_display_final(uint32_t width, uint32_t height, const float* __restrict__ color,
                                                       const float* __restrict__ alpha, const float* __restrict__ background,
                                                       const float* __restrict__ e_ptr, float e_manual, uint32_t tone, float iw2, float threshold,
                                                       float bscale, const float4* __restrict__ u1, uint32_t w1, uint32_t h1,
                                                       uint8_t* __restrict__ out8, float* __restrict__ out_color, float* __restrict__ out_bloom) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= width * height) return;
    const uint32_t y = i / width, x = i - y * width;
    const uint32_t fy = OUT8 ? height - 1u - y : y; // the film row
    const size_t o = i, f = (size_t)x + (size_t)fy * width;
    const float e = e_ptr ? *e_ptr : e_manual;
    float c[3], v[3], d[3];
    load_c<ARM>(color, background, f, c);
    for (int k = 0; k < 3; k++) v[k] = e * c[k];
    if (u1) {
        float u[3];
        upsample(u1, w1, h1, x, fy, u);
        for (int k = 0; k < 3; k++) {
            const float b = (bright(e, c[k], threshold) + u[k]) * bscale;
            v[k] = v[k] + b;
            if (out_bloom) out_bloom[3 * f + k] = b;
        }
    }
    if (tone == TONE_REINHARD) {
        const float lx = luminance(v[0], v[1], v[2]);
        float s = 1.0f;
        const bool on = __builtin_isfinite(lx) && lx > 0.0f;
        if (on) s = (1.0f + lx * iw2) / (1.0f + lx);
        for (int k = 0; k < 3; k++) d[k] = on ? v[k] * s : v[k];
    } else if (tone == TONE_ACES) {
        for (int k = 0; k < 3; k++) {
            const float t = rmax(v[k], 0.0f);
            d[k] = (t * (2.51f * t + 0.03f)) / (t * (2.43f * t + 0.59f) + 0.14f);
        }
    } else {
        for (int k = 0; k < 3; k++) d[k] = v[k];
    }
    if (!OUT8) {
        for (int k = 0; k < 3; k++) out_color[3 * f + k] = d[k];
    } else if (ARM == SAVE_COLOR_RGBA) {
        for (int k = 0; k < 3; k++) out8[4 * o + k] = quant8(gamma22(saturate1(d[k])));
        out8[4 * o + 3] = quant8(alpha[f]);
    } else if (ARM == SAVE_COLOR_BG) {
        for (int k = 0; k < 3; k++) out8[3 * o + k] = quant8(gamma22(saturate1(d[k])));
    } else {
        for (int k = 0; k < 3; k++) out8[3 * o + k] = quant8(gamma22(d[k]));
    }
}

struct Pyramid {
    uint32_t w[MAX_LEVELS + 1], h[MAX_LEVELS + 1];
    size_t offset[MAX_LEVELS + 1]; // bytes from the start of the scratch; level 0 has no plane
    size_t partial, total;
};

// n = width * height in (0, 2^31), levels <= 8
Pyramid plan(uint32_t width, uint32_t height, uint32_t levels) {
    Pyramid p = {};
    const size_t nb = ((size_t)width * height + 255u) / 256u;
    p.w[0] = width;
    p.h[0] = height;
    p.partial = HEADER_BYTES;
    size_t at = HEADER_BYTES + (nb * 8u + 255u) / 256u * 256u;
    for (uint32_t k = 1; k <= levels; k++) {
        p.w[k] = (p.w[k - 1] + 1u) / 2u;
        p.h[k] = (p.h[k - 1] + 1u) / 2u;
        p.offset[k] = at;
        at += (size_t)p.w[k] * p.h[k] * sizeof(float4);
    }
    p.total = at;
    return p;
}

bool finite_f(float v) { return v - v == 0.0f; }

template <int ARM>
void launch_arm(hipStream_t s, const rayn_display_params& dp, uint32_t width, uint32_t height, const float* color, const float* alpha,
                const float* background, void* state, void* scratch, uint8_t* out8, float* out_color, float* out_meter, float* out_bloom) {
    const uint32_t n = width * height, nb = (n + 255u) / 256u, L = dp.levels;
    const dim3 block(256);
    const Pyramid pyr = plan(width, height, L);
    char* base = (char*)scratch;
    const float* e_ptr = nullptr;
    if (dp.auto_exposure) {
        float* partial = (float*)(base + pyr.partial);
        uint32_t* count = (uint32_t*)(partial + nb);
        hipLaunchKernelGGL(k_display_meter<ARM>, dim3(nb), block, 0, s, n, color, background, partial, count);
        hipLaunchKernelGGL(k_display_expose, dim3(1), block, 0, s, nb, partial, count, dp.key, dp.adapt, (uint32_t*)state, (float*)base, out_meter);
        e_ptr = (const float*)base;
    } else if (out_meter) {
        hipLaunchKernelGGL(k_display_put2, dim3(1), dim3(1), 0, s, out_meter, 0.0f, dp.exposure_scale);
    }
    const float4* u1 = nullptr;
    if (L) {
        auto level = [&](uint32_t k) { return (float4*)(base + pyr.offset[k]); };
        auto blocks = [&](uint32_t k) { return dim3((pyr.w[k] * pyr.h[k] + 255u) / 256u); };
        hipLaunchKernelGGL(k_display_down0<ARM>, blocks(1), block, 0, s, width, height, pyr.w[1], pyr.h[1], color, background, e_ptr,
                           dp.exposure_scale, dp.threshold, level(1));
        for (uint32_t k = 2; k <= L; k++)
            hipLaunchKernelGGL(k_display_down, blocks(k), block, 0, s, pyr.w[k - 1], pyr.h[k - 1], pyr.w[k], pyr.h[k], (const float4*)level(k - 1), level(k));
        for (uint32_t k = L - 1u; k >= 1u; k--)
            hipLaunchKernelGGL(k_display_up, blocks(k), block, 0, s, pyr.w[k], pyr.h[k], pyr.w[k + 1], pyr.h[k + 1], (const float4*)level(k + 1), level(k));
        u1 = level(1);
    }
    const float bscale = L ? dp.strength / (float)(L + 1u) : 0.0f;
    if (out8)
        hipLaunchKernelGGL((k_display_final<ARM, true>), dim3(nb), block, 0, s, width, height, color, alpha, background, e_ptr, dp.exposure_scale, dp.tone,
                           dp.iw2, dp.threshold, bscale, u1, pyr.w[1], pyr.h[1], out8, out_color, out_bloom);
    else
        hipLaunchKernelGGL((k_display_final<ARM, false>), dim3(nb), block, 0, s, width, height, color, alpha, background, e_ptr, dp.exposure_scale, dp.tone,
                           dp.iw2, dp.threshold, bscale, u1, pyr.w[1], pyr.h[1], out8, out_color, out_bloom);
}

} // namespace

size_t display_scratch_bytes(uint32_t width, uint32_t height, uint32_t levels) {
    if (check_size(width, height) || levels > MAX_LEVELS) return 0;
    return plan(width, height, levels).total;
}

const char* display_check_args(const rayn_display_params* dp, uint32_t have_mask, int transparent_background, uint32_t width, uint32_t height,
                               const float* color, const float* alpha, const float* background, const void* state, const void* scratch,
                               size_t scratch_bytes, int* arm) {
    if (!dp) return "null display params";
    const char* why = nullptr;
    *arm = save_to_arm(0, have_mask, transparent_background, &why); // the Color kind; < 0: why = the reference's Err text
    if (*arm < 0) return why;
    if (const char* size = check_size(width, height)) return size;
    if (dp->tone > TONE_ACES) return "unknown tone operator (0 linear, 1 reinhard, 2 aces)";
    if (dp->levels > MAX_LEVELS) return "bloom levels must be in 0..8 (0 = off)";
    if (dp->auto_exposure > 1u) return "auto_exposure must be 0 (manual) or 1 (auto)";
    if (dp->auto_exposure) {
        if (!state) return "null state with auto exposure";
        if ((uintptr_t)state % 4u) return "state not 4-byte aligned";
        if (!(finite_f(dp->key) && dp->key > 0.0f)) return "key must be finite and > 0";
        if (!(dp->adapt >= 0.0f && dp->adapt <= 1.0f)) return "adapt must be in [0, 1]";
    } else if (!(finite_f(dp->exposure_scale) && dp->exposure_scale >= 0.0f)) {
        return "exposure_scale must be finite and >= 0";
    }
    if (dp->tone == TONE_REINHARD && !(finite_f(dp->iw2) && dp->iw2 >= 0.0f)) return "iw2 must be finite and >= 0";
    if (dp->levels && !(finite_f(dp->threshold) && finite_f(dp->strength) && dp->strength >= 0.0f))
        return "bloom threshold must be finite and strength finite and >= 0";
    const uint32_t reads = save_to_arm_reads(*arm);
    if (!color || ((reads & 2u) && !alpha) || ((reads & 4u) && !background)) return "null buffer";
    if (dp->auto_exposure || dp->levels) {
        if (!scratch) return "null scratch with auto exposure or bloom";
        if (scratch_bytes < display_scratch_bytes(width, height, dp->levels)) return "scratch smaller than rayn_display_scratch_bytes(width, height, levels)";
        if ((uintptr_t)scratch % 16u) return "scratch not 16-byte aligned";
    }
    return nullptr;
}

void launch_display(hipStream_t s, int arm, const rayn_display_params& dp, uint32_t width, uint32_t height, const float* color, const float* alpha,
                    const float* background, void* state, void* scratch, uint8_t* out8, float* out_color, float* out_meter, float* out_bloom) {
    switch (arm) {
    case SAVE_COLOR_RGBA: launch_arm<SAVE_COLOR_RGBA>(s, dp, width, height, color, alpha, background, state, scratch, out8, out_color, out_meter, out_bloom); break;
    case SAVE_COLOR_BG: launch_arm<SAVE_COLOR_BG>(s, dp, width, height, color, alpha, background, state, scratch, out8, out_color, out_meter, out_bloom); break;
    default: launch_arm<SAVE_COLOR_ONLY>(s, dp, width, height, color, alpha, background, state, scratch, out8, out_color, out_meter, out_bloom); break;
    }
}

} // namespace rayn

extern "C" size_t rayn_display_scratch_bytes(uint32_t width, uint32_t height, uint32_t levels) {
    return rayn::display_scratch_bytes(width, height, levels);
}
