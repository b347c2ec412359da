// progressive.hip — progressive rendering downstream of the film: the finished films of successive epochs (ordinary renders of the same
// frame under the sample tables of rayn_progressive_seed) are accumulated into running sums, a per-pixel Welford estimate of the
// luminance's standard error decides which tiles still need samples, and the tiles that do are handed back as an ascending list for
// rayn_hip_set_tile_subset.  An extension: rayn only carries an unused progressive_epoch counter (src/film.rs:178-179).
//
// The definition (include/rayn_hip.h; tests/progressive_np.py restates it in numpy and the tests compare bit for
// bit).  For every pixel of a listed tile, n = the tile's epoch count after this epoch, F = the epoch's film:
//     sum[k] = sum[k] + F[k]   (k = the ten film floats; a fresh state holds -0.0f, the identity of IEEE addition: one epoch's sum is F's bits)
//     c = F.color + F.background;  y = (0.2126f c.r + 0.7152f c.g) + 0.0722f c.b
//     d = y - mean_y;  mean_y = mean_y + d / (float)n;  m2 = m2 + d * (y - mean_y)
//     mean film[k] = sum[k] / (float)n
//     n >= 2:  se = sqrtf(m2 / (float)(n (n - 1)));  e_p = se / (fabsf(mean_y) + noise_floor)
// outliers = pixels of the tile with e_p > target_error, max_e = the largest e_p > 0 (0 if there is none): a NaN e_p is in neither.
// The tile retires (adaptive only) when n >= min_epochs and outliers * 1000 <= outlier_permille * tile pixels; it stays retired.
// f32 throughout, built with -ffp-contract=off, IEEE division and square root.
//
// k_prog_accumulate: one workgroup of 256 threads per listed tile, a thread per pixel (row-major inside the tile, so a wave reads whole
// row segments), everything fused: 40 B of epoch film and 48 B of state read, 48 B of state and 40 B of mean film written per pixel.  The
// state is three float4 planes in film pixel order, so its accesses are 128-bit; the film's planes are 3 + 1 + 3 + 3 floats per pixel and
// are read and written as such.  The tile's outlier count is ballot + popcount per wave, its max_e the maximum of the bit patterns of the
// positive e_p (ordered like the floats): both exact and independent of the order of the pixels.  The kernel is HBM-bound.
// k_prog_compact: ONE workgroup of 1024 threads walks the tile records in ascending chunks of 1024 and appends the active tiles of each
// chunk behind those of the chunks before (ballot, popcount of the lanes below, per-wave counts through LDS): a stable compaction
// without atomics, 16 B read per tile.  It also sums the outliers and takes the maximum of max_e over all tiles.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/rayn_hip.h"
#include "progressive.h"
#include "tiles.h"

namespace rayn {
namespace {

struct ProgGeom { uint32_t width, height, tile_w, tile_h, tiles_y, n_tiles; };

__device__ inline uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const uint32_t u = (uint32_t)__shfl_xor((int)v, o);
        v = u > v ? u : v;
    }
    return v;
}

// A fresh state: sums -0.0f, mean_y = m2 = +0, no epochs, nothing retired, every tile active.
__global__ void __launch_bounds__(256) k_prog_reset(uint32_t pixels, uint32_t n_tiles, float4* __restrict__ s0, float4* __restrict__ s1,
                                                    float4* __restrict__ s2, uint4* __restrict__ rec, uint32_t* __restrict__ totals,
                                                    uint32_t* __restrict__ active) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < pixels) {
        s0[i] = make_float4(-0.0f, -0.0f, -0.0f, -0.0f);
        s1[i] = make_float4(-0.0f, -0.0f, -0.0f, 0.0f);
        s2[i] = make_float4(-0.0f, -0.0f, -0.0f, 0.0f);
    }
    if (i < n_tiles) {
        rec[i] = make_uint4(0u, 0u, 0u, 0u);
        active[i] = i;
    }
    if (i == 0) {
        totals[0] = n_tiles;
        totals[1] = totals[2] = totals[3] = 0u;
    }
}

__global__ void __launch_bounds__(256) k_prog_accumulate(ProgGeom g, float target_error, float noise_floor, uint32_t min_epochs,
                                                         uint32_t outlier_permille, uint32_t adaptive, const uint32_t* __restrict__ list,
                                                         const float* __restrict__ f_color, const float* __restrict__ f_alpha,
                                                         const float* __restrict__ f_background, const float* __restrict__ f_normal,
                                                         float4* __restrict__ s0, float4* __restrict__ s1, float4* __restrict__ s2,
                                                         uint4* __restrict__ rec, float* __restrict__ o_color, float* __restrict__ o_alpha,
                                                         float* __restrict__ o_background, float* __restrict__ o_normal) {
    __shared__ uint32_t sh_out[4], sh_max[4];
    const uint32_t k = list ? list[blockIdx.x] : blockIdx.x; // < n_tiles (checked by the host)
    // the reference's tile order is x-major (src/film.rs:399-427): tile k = column k / tiles_y, row k % tiles_y
    const uint32_t tx = k / g.tiles_y, ty = k - tx * g.tiles_y;
    const uint32_t x0 = tx * g.tile_w, y0 = ty * g.tile_h; // < width, < height for every tile of the list
    const uint32_t tw = g.width - x0 < g.tile_w ? g.width - x0 : g.tile_w;
    const uint32_t th = g.height - y0 < g.tile_h ? g.height - y0 : g.tile_h;
    const uint32_t npix = tw * th;
    const uint4 old = rec[k];
    const uint32_t n = old.x + 1u;
    const float fn = (float)n;
    const float fnn = (float)((uint64_t)n * (uint64_t)(n - 1u));
    uint32_t wave_outliers = 0u, my_max = 0u;
    for (uint32_t base = 0; base < npix; base += 256u) {
        const uint32_t i = base + threadIdx.x;
        bool outlier = false;
        if (i < npix) {
            const uint32_t row = i / tw, col = i - row * tw;
            const uint32_t p = (x0 + col) + (y0 + row) * g.width; // < 2^31
            const size_t f = (size_t)p * 3u;
            const float cr = f_color[f], cg = f_color[f + 1], cb = f_color[f + 2], al = f_alpha[p];
            const float br = f_background[f], bg = f_background[f + 1], bb = f_background[f + 2];
            const float nx = f_normal[f], ny = f_normal[f + 1], nz = f_normal[f + 2];
            float4 a = s0[p], b = s1[p], c = s2[p];
            a.x = a.x + cr; a.y = a.y + cg; a.z = a.z + cb; a.w = a.w + al;
            b.x = b.x + br; b.y = b.y + bg; b.z = b.z + bb;
            c.x = c.x + nx; c.y = c.y + ny; c.z = c.z + nz;
            const float lr = cr + br, lg = cg + bg, lb = cb + bb;
            const float y = (0.2126f * lr + 0.7152f * lg) + 0.0722f * lb;
            const float d = y - b.w;
            const float mean = b.w + d / fn;
            const float m2 = c.w + d * (y - mean);
            b.w = mean;
            c.w = m2;
            s0[p] = a;
            s1[p] = b;
            s2[p] = c;
            o_color[f] = a.x / fn; o_color[f + 1] = a.y / fn; o_color[f + 2] = a.z / fn;
            o_alpha[p] = a.w / fn;
            o_background[f] = b.x / fn; o_background[f + 1] = b.y / fn; o_background[f + 2] = b.z / fn;
            o_normal[f] = c.x / fn; o_normal[f + 1] = c.y / fn; o_normal[f + 2] = c.z / fn;
            if (n >= 2u) {
                const float se = sqrtf(m2 / fnn);
                const float e = se / (fabsf(mean) + noise_floor);
                outlier = e > target_error; // false for a NaN e
                if (e > 0.0f) { // positive floats are ordered like their bit patterns; NaN and 0 contribute nothing
                    const uint32_t bits = __float_as_uint(e);
                    my_max = bits > my_max ? bits : my_max;
                }
            }
        }
        wave_outliers += (uint32_t)__popcll(__ballot(outlier)); // the loop's trip count is uniform over the block
    }
    my_max = wave_max_u32(my_max);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) {
        sh_out[wave] = wave_outliers;
        sh_max[wave] = my_max;
    }
    __syncthreads(); // also orders every thread's read of rec[k] before the write below
    if (threadIdx.x == 0) {
        uint32_t outliers = 0u, mx = 0u;
        for (int w = 0; w < 4; w++) {
            outliers += sh_out[w];
            mx = sh_max[w] > mx ? sh_max[w] : mx;
        }
        uint32_t retired = old.y;
        if (adaptive && n >= min_epochs && (uint64_t)outliers * 1000u <= (uint64_t)outlier_permille * (uint64_t)npix) retired = 1u;
        rec[k] = make_uint4(n, retired, outliers, mx);
    }
}

__global__ void __launch_bounds__(1024) k_prog_compact(uint32_t n_tiles, const uint4* __restrict__ rec, uint32_t* __restrict__ totals,
                                                       uint32_t* __restrict__ active) {
    __shared__ uint32_t sh_count[16], sh_max[16];
    __shared__ unsigned long long sh_out[16];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t run = 0u, my_max = 0u; // run: active tiles of the chunks before this one (the same in every thread)
    unsigned long long my_out = 0ull;
    for (uint32_t base = 0; base < n_tiles; base += 1024u) {
        const uint32_t k = base + threadIdx.x;
        bool act = false;
        if (k < n_tiles) {
            const uint4 r = rec[k];
            act = r.y == 0u;
            my_out += r.z;
            my_max = r.w > my_max ? r.w : my_max;
        }
        const unsigned long long b = __ballot(act);
        const uint32_t below = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) sh_count[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t before = 0u, total = 0u;
        for (uint32_t w = 0; w < 16u; w++) {
            const uint32_t c = sh_count[w];
            before += w < wave ? c : 0u;
            total += c;
        }
        if (act) active[run + before + below] = k; // run + before + below < n_tiles
        run += total;
        __syncthreads(); // sh_count is rewritten by the next chunk
    }
    my_max = wave_max_u32(my_max);
#pragma unroll
    for (int o = 32; o; o >>= 1) my_out += (unsigned long long)__shfl_xor((long long)my_out, o);
    if (lane == 0) {
        sh_max[wave] = my_max;
        sh_out[wave] = my_out;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t mx = 0u;
        unsigned long long out = 0ull;
        for (int w = 0; w < 16; w++) {
            mx = sh_max[w] > mx ? sh_max[w] : mx;
            out += sh_out[w];
        }
        totals[0] = run;
        totals[1] = mx;
        totals[2] = (uint32_t)out;
        totals[3] = (uint32_t)(out >> 32);
    }
}

size_t round16(size_t v) { return (v + 15u) & ~(size_t)15u; }

} // namespace

ProgLayout progressive_layout(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h) {
    ProgLayout L;
    memset(&L, 0, sizeof L);
    const uint64_t n = (uint64_t)width * height;
    if (!n || n >= ((uint64_t)1 << 31) || !tile_w || !tile_h) return L;
    const TileGrid grid(width, height, tile_w, tile_h);
    if (!grid.count()) return L;
    L.width = width; L.height = height; L.tile_w = tile_w; L.tile_h = tile_h;
    L.tiles_y = grid.ny;
    L.n_tiles = grid.count();
    L.pixels = n;
    const size_t plane = (size_t)n * 16u, t = L.n_tiles;
    L.off_s0 = 0;
    L.off_s1 = plane;
    L.off_s2 = 2u * plane;
    L.off_records = 3u * plane;
    L.off_totals = L.off_records + 16u * t;
    L.off_active = L.off_totals + 16u;
    L.off_listed = L.off_active + 4u * t;
    L.bytes = round16(L.off_listed + 4u * t);
    return L;
}

const char* progressive_check_geometry(const rayn_frame_params* p, const void* state, size_t state_bytes) {
    if (!p) return "null frame parameters";
    if (!p->width || !p->height) return "zero-sized film";
    if ((uint64_t)p->width * p->height >= ((uint64_t)1 << 31)) return "film larger than 2^31 pixels unsupported (32-bit pixel indices)";
    if (!p->tile_w || !p->tile_h) return "zero-sized tile";
    const ProgLayout L = progressive_layout(p->width, p->height, p->tile_w, p->tile_h);
    if (!L.n_tiles) return "the tile size leaves the film without tiles";
    if (!state) return "null buffer";
    if (state_bytes < L.bytes) return "state smaller than rayn_progressive_state_bytes(width, height, tile_w, tile_h)";
    if ((uintptr_t)state % 16u) return "state not 16-byte aligned";
    return nullptr;
}

const char* progressive_check_params(const rayn_progressive_params* pp) {
    if (!pp) return "null progressive parameters";
    if (!(pp->target_error >= 0.0f) || !(pp->target_error <= 3.402823466e38f)) return "target_error must be finite and >= 0";
    if (!(pp->noise_floor >= 0.0f) || !(pp->noise_floor <= 3.402823466e38f)) return "noise_floor must be finite and >= 0";
    if (pp->min_epochs < 2u) return "min_epochs must be >= 2";
    if (pp->max_epochs < pp->min_epochs) return "max_epochs must be >= min_epochs";
    if (pp->max_epochs > 65536u) return "max_epochs must be <= 65536 (the epoch seeds of a frame)";
    if (pp->outlier_permille > 1000u) return "outlier_permille must be <= 1000";
    return nullptr;
}

const char* progressive_check_tiles(const ProgLayout& L, const uint32_t* tiles, uint32_t n_tiles) {
    if (!tiles) return n_tiles ? "null tile list with n_tiles != 0" : nullptr;
    if (!n_tiles) return "empty tile list (pass NULL for every tile)";
    for (uint32_t i = 0; i < n_tiles; i++) {
        if (tiles[i] >= L.n_tiles) return "tile index beyond the film's tile count";
        if (i && tiles[i] <= tiles[i - 1]) return "tile list not strictly ascending";
    }
    return nullptr;
}

void launch_progressive_reset(hipStream_t s, const ProgLayout& L, void* state) {
    char* base = (char*)state;
    const uint32_t n = (uint32_t)L.pixels > L.n_tiles ? (uint32_t)L.pixels : L.n_tiles;
    hipLaunchKernelGGL(k_prog_reset, dim3((n + 255u) / 256u), dim3(256), 0, s, (uint32_t)L.pixels, L.n_tiles, (float4*)(base + L.off_s0),
                       (float4*)(base + L.off_s1), (float4*)(base + L.off_s2), (uint4*)(base + L.off_records), (uint32_t*)(base + L.off_totals),
                       (uint32_t*)(base + L.off_active));
}

void launch_progressive_accumulate(hipStream_t s, const ProgLayout& L, const rayn_progressive_params& pp, const uint32_t* d_list, uint32_t n_listed,
                                   const float* color, const float* alpha, const float* background, const float* normal, void* state,
                                   float* out_color, float* out_alpha, float* out_background, float* out_normal) {
    char* base = (char*)state;
    const ProgGeom g{L.width, L.height, L.tile_w, L.tile_h, L.tiles_y, L.n_tiles};
    hipLaunchKernelGGL(k_prog_accumulate, dim3(d_list ? n_listed : L.n_tiles), dim3(256), 0, s, g, pp.target_error, pp.noise_floor, pp.min_epochs,
                       pp.outlier_permille, pp.adaptive, d_list, color, alpha, background, normal, (float4*)(base + L.off_s0),
                       (float4*)(base + L.off_s1), (float4*)(base + L.off_s2), (uint4*)(base + L.off_records), out_color, out_alpha,
                       out_background, out_normal);
}

void launch_progressive_compact(hipStream_t s, const ProgLayout& L, void* state) {
    char* base = (char*)state;
    hipLaunchKernelGGL(k_prog_compact, dim3(1), dim3(1024), 0, s, L.n_tiles, (const uint4*)(base + L.off_records), (uint32_t*)(base + L.off_totals),
                       (uint32_t*)(base + L.off_active));
}

} // namespace rayn

extern "C" size_t rayn_progressive_state_bytes(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h) {
    return rayn::progressive_layout(width, height, tile_w, tile_h).bytes;
}

extern "C" int rayn_progressive_seed(uint32_t frame, uint32_t epoch, uint32_t max_bounces, uint32_t volume_marches, uint32_t* out_seed) {
    if (!out_seed) return RAYN_ERR_INVALID_ARG;
    // rayn_sets_1d + rayn_sets_2d = 3 + (max_bounces + 1) (15 + 9 volume_marches), in 64 bits
    const uint64_t sets = 3u + ((uint64_t)max_bounces + 1u) * (15u + 9u * (uint64_t)volume_marches);
    if (sets > 65536u) return RAYN_ERR_INVALID_ARG; // the sets of one epoch would reach into the next epoch's
    const uint64_t seed = (uint64_t)frame + (uint64_t)epoch * 65536u;
    if (seed >= ((uint64_t)1 << 32)) return RAYN_ERR_INVALID_ARG; // an error, not a wrap
    *out_seed = (uint32_t)seed;
    return RAYN_OK;
}
