// interpolate.hip — a frame T of a sequence generated from two rendered key frames A and B and T's own primary-hit G-buffer
// (rayn_hip_interpolate_device): motion-compensated frame interpolation whose motion is traced, not estimated.  An extension: rayn renders
// every frame.  It runs downstream of the film: it reads the keys' planes and writes new planes; nothing it reads is touched.
//
// The definition (include/rayn_hip.h; tests/interpolate_np.py restates it in numpy and the tests compare bit for bit):
// per pixel of T the primary hit is moved by its hitable's linear motion to each key's time and projected through that key's camera (steps
// 2 and 3 of the temporal accumulate); the four bilinear taps there count when they show the same object at the projected depth and hold
// a finite colour; a key with taps contributes their weighted mean, and the two keys are blended by time - or, where only one of them sees
// the point, that one is taken alone.  Where neither does, the keys' own pixels are cross-faded.  One weight set serves every plane.  f32
// throughout, built with -ffp-contract=off and IEEE division.  Nothing here depends on the mul_add policy: the file is built once.
//
// Layout: one thread per pixel, blocks of 256 threads over the linear pixel index (rows are contiguous, so a wave reads and writes whole
// runs of a row).  A pixel reads 20 bytes of its own guide and writes up to 44; its taps - per key and tap the object (4 B), the depth
// dword of the record (the other 12 B of the record are never used) and the planes (40 B) - are shared with the pixels around it and
// come from L2.  The tests are ordered cheapest first, object, depth, colour, so that a rejected tap reads nothing further.  Both keys go
// through one inlined function.  project, closure3, the vectors and Sums / add_tap are post_device.h's.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "interpolate.h"
#include "post_checks.h"
#include "post_device.h"

namespace rayn {
namespace {

constexpr uint32_t BLOCK = 256u;

// the ten floats of one film pixel; planes the film lacks are not looked at
struct Pixel {
    float c[3], a, b[3], n[3];
};

__device__ inline UpscalePlanes key_planes(const InterpolateKey& K) {
    return UpscalePlanes{K.color, K.alpha, K.background, K.normal, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
}

// Steps 1 and 2 for one key: the taps of the pixel (X, Y) with object o and record G in key K, into S.  vel: the hitable's center_vel
// (w != 0: animated).  Every index is bounded by its plane: a tap is used only with 0 <= qx < width and 0 <= qy < height.
__device__ inline void gather_key(Sums& S, const InterpolateKey& K, uint32_t X, uint32_t Y, uint32_t o, float4 G, float4 vel, float ts,
                                  float depth_tolerance, uint32_t width, uint32_t height) {
    const bool hit = o != MISS_OBJECT;
    float fx = (float)X, fy = (float)Y, te = 0.0f;
    if (hit) {
        v3 Pp = v3{G.x, G.y, G.z};
        const float dt = ts - K.time;
        if (vel.w != 0.0f) Pp = v3{G.x - vel.x * dt, G.y - vel.y * dt, G.z - vel.z * dt};
        if (!project(K.cam, K.time, Pp, width, height, &fx, &fy, &te)) return;
    }
    const float x0f = __builtin_floorf(fx), y0f = __builtin_floorf(fy);
    const float wx1 = fx - x0f, wx0 = 1.0f - wx1, wy1 = fy - y0f, wy0 = 1.0f - wy1;
    const long long x0 = (long long)__builtin_fminf(__builtin_fmaxf(x0f, -2.0f), 2147483648.0f);
    const long long y0 = (long long)__builtin_fminf(__builtin_fmaxf(y0f, -2.0f), 2147483648.0f);
    const float tol = depth_tolerance * te;
    const UpscalePlanes pl = key_planes(K);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const long long qx = x0 + (k & 1), qy = y0 + (k >> 1);
        if (qx < 0 || qx >= (long long)width || qy < 0 || qy >= (long long)height) continue;
        const float b = ((k & 1) ? wx1 : wx0) * ((k >> 1) ? wy1 : wy0);
        if (!(b > 0.0f)) continue;
        const size_t q = (size_t)qx + (size_t)qy * width; // < 2^31
        if (K.object[q] != o) continue;
        if (hit && !(__builtin_fabsf(((const float*)K.records)[4u * q + 3u] - te) <= tol)) continue;
        const float cr = K.color[3u * q], cg = K.color[3u * q + 1], cb = K.color[3u * q + 2];
        if (!finite3(cr, cg, cb)) continue;
        add_tap<false>(S, b, q, cr, cg, cb, pl);
    }
}

__device__ inline Pixel mean_pixel(const Sums& S, const InterpolateKey& K) {
    Pixel v;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        v.c[i] = S.c[i] / S.W;
        v.b[i] = K.background ? S.b[i] / S.W : 0.0f;
        v.n[i] = K.normal ? S.n[i] / S.W : 0.0f;
    }
    v.a = K.alpha ? S.a / S.W : 0.0f;
    return v;
}

// the key's own pixel P; c: its colour, which the caller has read
__device__ inline Pixel own_pixel(const InterpolateKey& K, size_t P, const float c[3]) {
    Pixel v;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        v.c[i] = c[i];
        v.b[i] = K.background ? K.background[3u * P + i] : 0.0f;
        v.n[i] = K.normal ? K.normal[3u * P + i] : 0.0f;
    }
    v.a = K.alpha ? K.alpha[P] : 0.0f;
    return v;
}

__device__ inline float blend(float a, float b, float wA, float wB) {
    const float pa = a * wA, pb = b * wB;
    return pa + pb;
}

struct InterpolateArgs {
    InterpolateCall c;
    uint32_t n; // width * height
    float wA, wB;
};

__global__ void __launch_bounds__(BLOCK) k_interpolate(const InterpolateArgs A) {
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= A.n) return;
    const InterpolateCall& c = A.c;
    const uint32_t Y = p / c.width, X = p - Y * c.width;
    const size_t P = p;
    const uint32_t o = c.object[P];
    float4 G = make_float4(0.0f, 0.0f, 0.0f, 0.0f), vel = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (o != MISS_OBJECT) {
        G = ((const float4*)c.records)[P];
        // a select per hitable, not an index: a lane-varying index into the by-value argument would go through scratch
#pragma unroll
        for (uint32_t k = 0; k < RAYN_MAX_HITABLES; k++)
            if (k < c.n_hitables && o == k) vel = c.hvel[k];
    }
    Sums SA, SB;
    gather_key(SA, c.a, X, Y, o, G, vel, c.time, c.depth_tolerance, c.width, c.height);
    gather_key(SB, c.b, X, Y, o, G, vel, c.time, c.depth_tolerance, c.width, c.height);
    bool useA = SA.W > 0.0f, useB = SB.W > 0.0f;
    Pixel vA, vB;
    uint32_t source;
    if (useA || useB) {
        // tier 1
        source = useA ? (useB ? 0u : 1u) : 2u;
        if (useA) vA = mean_pixel(SA, c.a);
        if (useB) vB = mean_pixel(SB, c.b);
    } else {
        // tier 2: the keys' own pixels
        float ca[3], cb[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            ca[i] = c.a.color[3u * P + i];
            cb[i] = c.b.color[3u * P + i];
        }
        useA = finite3(ca[0], ca[1], ca[2]);
        useB = finite3(cb[0], cb[1], cb[2]);
        source = (useA && useB) ? 3u : 4u;
        if (!useA && !useB) {
            useA = A.wA >= A.wB;
            useB = !useA;
        }
        if (useA) vA = own_pixel(c.a, P, ca);
        if (useB) vB = own_pixel(c.b, P, cb);
    }
    Pixel out;
    if (useA && useB) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            out.c[i] = blend(vA.c[i], vB.c[i], A.wA, A.wB);
            out.b[i] = blend(vA.b[i], vB.b[i], A.wA, A.wB);
            out.n[i] = blend(vA.n[i], vB.n[i], A.wA, A.wB);
        }
        out.a = blend(vA.a, vB.a, A.wA, A.wB);
    } else {
        out = useA ? vA : vB;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) c.out_color[3u * P + i] = out.c[i];
    if (c.out_alpha) c.out_alpha[P] = out.a;
    if (c.out_background) {
#pragma unroll
        for (int i = 0; i < 3; i++) c.out_background[3u * P + i] = out.b[i];
    }
    if (c.out_normal) {
#pragma unroll
        for (int i = 0; i < 3; i++) c.out_normal[3u * P + i] = out.n[i];
    }
    if (c.out_source) c.out_source[P] = source;
}

inline bool finite_f(float v) { return v - v == 0.0f; }

} // namespace

const char* interpolate_check_args(const rayn_frame_params* p, const rayn_interpolate_params* ip, const rayn_interpolate_key* key_a,
                                   const rayn_interpolate_key* key_b, const void* g_records, const uint32_t* g_object, const float* out_color,
                                   const float* out_alpha, const float* out_background, const float* out_normal, const uint32_t* out_source) {
    if (!p) return "null frame params";
    if (!ip) return "null interpolate params";
    if (!key_a || !key_b) return "null key";
    if (const char* why = check_size(p->width, p->height)) return why;
    if (!(ip->depth_tolerance >= 0.0f) || !(ip->depth_tolerance <= 3.40282347e+38f)) return "depth_tolerance must be finite and >= 0";
    if (!key_a->camera || !key_b->camera) return "null camera";
    if (key_a->camera->kind > RAYN_CAM_ORTHOGRAPHIC || key_b->camera->kind > RAYN_CAM_ORTHOGRAPHIC) return "unknown camera kind";
    const float ta = key_a->time_start, tb = key_b->time_start, ts = p->time_start;
    if (!finite_f(ta) || !finite_f(tb) || !finite_f(ts)) return "the time_starts must be finite";
    if (!(ta < tb)) return "key A must lie before key B";
    if (!(ta <= ts && ts <= tb)) return "time_start must lie between the keys";
    if (!key_a->d_color || !key_b->d_color || !out_color) return "null Color buffer";
    if (!key_a->d_records || !key_a->d_object || !key_b->d_records || !key_b->d_object || !g_records || !g_object) return "null G-buffer";
    if (!key_a->d_alpha != !key_b->d_alpha || !key_a->d_alpha != !out_alpha || !key_a->d_background != !key_b->d_background ||
        !key_a->d_background != !out_background || !key_a->d_normal != !key_b->d_normal || !key_a->d_normal != !out_normal)
        return "a plane must be present in both keys and the output, or in none";
    if ((uintptr_t)key_a->d_records % 16u || (uintptr_t)key_b->d_records % 16u || (uintptr_t)g_records % 16u) return "G-buffer records not 16-byte aligned";
    if ((uintptr_t)key_a->d_object % 4u || (uintptr_t)key_b->d_object % 4u || (uintptr_t)g_object % 4u) return "G-buffer objects not 4-byte aligned";
    if ((uintptr_t)out_source % 4u) return "d_out_source not 4-byte aligned";
    const size_t n = (size_t)p->width * p->height;
    Span in[14];
    int k = 0;
    for (const rayn_interpolate_key* key : {key_a, key_b}) {
        in[k++] = Span{key->d_color, 12u * n};
        in[k++] = Span{key->d_alpha, 4u * n};
        in[k++] = Span{key->d_background, 12u * n};
        in[k++] = Span{key->d_normal, 12u * n};
        in[k++] = Span{key->d_records, 16u * n};
        in[k++] = Span{key->d_object, 4u * n};
    }
    in[k++] = Span{g_records, 16u * n};
    in[k++] = Span{g_object, 4u * n};
    const Span out[5] = {{out_color, 12u * n}, {out_alpha, 4u * n}, {out_background, 12u * n}, {out_normal, 12u * n}, {out_source, 4u * n}};
    for (int i = 0; i < 5; i++) {
        if (first_overlap(out + i, 1, in, 14)) return "an output must not alias an input";
        if (first_overlap(out + i, 1, out + i + 1, 4 - i)) return "the outputs must not alias each other";
    }
    return nullptr;
}

void launch_interpolate(hipStream_t s, const InterpolateCall& c) {
    InterpolateArgs A;
    A.c = c;
    A.n = c.width * c.height;
    const float ta = c.a.time, tb = c.b.time;
    const float num = c.time - ta, den = tb - ta;
    A.wB = num / den;
    A.wA = 1.0f - A.wB;
    hipLaunchKernelGGL(k_interpolate, dim3((A.n + BLOCK - 1u) / BLOCK), dim3(BLOCK), 0, s, A);
}

} // namespace rayn
