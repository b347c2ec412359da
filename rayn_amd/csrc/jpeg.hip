// jpeg.hip — the entropy-coded scan of a baseline JPEG, encoded on the device (rayn_hip_jpeg_encode_device; the definition is in
// include/rayn_hip.h, restated in tests/jpeg_np.py).  Four kernels, no memset:
//   k_jpeg_transform  a wave per 8x8 block: replicate-pad, colour conversion, 4:2:0 box, the two integer DCT passes through LDS, the
//                     quantiser; int16 coefficients in zigzag order, 128 bytes per block, blocks in the order of the scan
//   k_jpeg_segment    a workgroup per restart segment: the bits of every block (its DC predictor is the neighbour's coefficient, so there
//                     is no serial chain), their exclusive sum, the codes at their bit offsets into the segment's words of the scratch,
//                     the padding with 1 bits, the count of FF bytes, its exclusive sum, the stuffed bytes into the segment's slot
//   k_jpeg_layout     one workgroup: the exclusive sum of the segment sizes and their markers, the 16-byte header
//   k_jpeg_compact    a thread per output word: the segments from their slots and the RST markers between them, contiguously
// The segment kernel works through global scratch whatever the restart interval: one path, correct for every Ri (see DESIGN.md section 8
// for what an LDS path would save).  Integer arithmetic only; policy-free, built once.  Every store is a vector store; shared words are
// combined with integer atomicOr on words the kernel zeroed itself.
#include "jpeg.h"

#include "png_device.h"
#include "post_checks.h"

namespace rayn {

namespace {

constexpr uint32_t BT = PNG_BT;

// ---- the tables: ITU T.81 Annex K.1, K.2 (quantisation, row-major) and K.3 - K.6 (Huffman: BITS, HUFFVAL).  The one place they stand. ----
struct JpegHuffSpec {
    uint8_t bits[16];
    uint8_t vals[162];
    uint32_t n;
};
constexpr uint8_t BASE_QUANT[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61,
     12, 12, 14, 19, 26, 58, 60, 55,
     14, 13, 16, 24, 40, 57, 69, 56,
     14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77,
     24, 35, 55, 64, 81, 104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101,
     72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99,
     18, 21, 26, 66, 99, 99, 99, 99,
     24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99}};
// which = 2 * table id + class: 0 DC luminance, 1 AC luminance, 2 DC chrominance, 3 AC chrominance
constexpr JpegHuffSpec HUFF[4] = {
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12u},
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
     {1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113,
      20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98, 114,
      130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55,
      56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89,
      90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131,
      132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163,
      164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195,
      196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226,
      227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
     162u},
    {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12u},
    {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119},
     {0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34,
      50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114, 209,
      10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54,
      55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88,
      89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122,
      130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
      162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186,
      194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218,
      226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250},
     162u}};

constexpr uint32_t longest_code(const JpegHuffSpec& h) {
    uint32_t l = 0;
    for (uint32_t k = 0; k < 16u; k++)
        if (h.bits[k]) l = k + 1u;
    return l;
}
static_assert(longest_code(HUFF[0]) + 11u + 63u * (longest_code(HUFF[1]) + 10u) == JPEG_LUMA_BLOCK_BITS, "jpeg.h: the luminance block bound");
static_assert(longest_code(HUFF[2]) + 11u + 63u * (longest_code(HUFF[3]) + 10u) == JPEG_CHROMA_BLOCK_BITS, "jpeg.h: the chrominance block bound");

// What the kernels read: the transform matrix, the zigzag position of every row-major index, the base quantisation tables and the codes
// (code | length << 16; 0 for a symbol the table does not have) by symbol
struct JpegTables {
    int32_t T[64];
    uint8_t zpos[64];
    uint8_t base[2][64];
    uint32_t dc[2][12];
    uint32_t ac[2][256];
};

constexpr JpegTables make_tables() {
    JpegTables t = {};
    constexpr int32_t K[8] = {4096, 4017, 3784, 3406, 2896, 2276, 1567, 799}; // round(4096 cos(k pi / 16))
    for (uint32_t u = 0; u < 8u; u++)
        for (uint32_t x = 0; x < 8u; x++) {
            if (u == 0u) {
                t.T[x] = K[4];
                continue;
            }
            uint32_t m = ((2u * x + 1u) * u) & 31u; // cos((2x+1) u pi / 16) = cos(m pi / 16)
            if (m > 16u) m = 32u - m;
            t.T[u * 8u + x] = m > 8u ? -K[16u - m] : K[m]; // m is never 0, 8 or 16 for u in 1..7
        }
    uint32_t k = 0;
    for (uint32_t s = 0; s < 15u; s++) { // the diagonals v + u = s, upwards on the even ones
        const uint32_t lo = s > 7u ? s - 7u : 0u, hi = s < 7u ? s : 7u;
        for (uint32_t i = lo; i <= hi; i++) {
            const uint32_t v = (s & 1u) ? i : hi - (i - lo);
            t.zpos[v * 8u + (s - v)] = (uint8_t)k++;
        }
    }
    for (uint32_t c = 0; c < 2u; c++)
        for (uint32_t i = 0; i < 64u; i++) t.base[c][i] = BASE_QUANT[c][i];
    for (uint32_t w = 0; w < 4u; w++) {
        uint32_t code = 0, at = 0;
        for (uint32_t len = 1; len <= 16u; len++) {
            for (uint32_t i = 0; i < HUFF[w].bits[len - 1u]; i++) {
                const uint32_t e = code++ | (len << 16), sym = HUFF[w].vals[at++];
                if (w & 1u) t.ac[w >> 1][sym] = e;
                else t.dc[w >> 1][sym] = e;
            }
            code <<= 1;
        }
    }
    return t;
}
constexpr JpegTables HOST_TABLES = make_tables();
__constant__ JpegTables d_tables = make_tables();

// IJG's quality scaling of a base table entry
constexpr uint32_t quality_scale(uint32_t q) { return q < 50u ? 5000u / q : 200u - 2u * q; }
__host__ __device__ constexpr uint32_t scaled_quant(uint32_t base, uint32_t scale) {
    const uint32_t v = (base * scale + 50u) / 100u;
    return v < 1u ? 1u : (v > 255u ? 255u : v);
}

struct JpegShape {
    uint32_t w, h, bpp, sub, bpm, mcus_x, mcus, blocks, ri;
};

// component c (0 Y, 1 Cb, 2 Cr) of the pixel (x, y) of the image padded by replication
__device__ inline int component(const uint8_t* __restrict__ img, const JpegShape& g, uint32_t c, uint32_t x, uint32_t y) {
    const uint8_t* p = img + ((size_t)min(y, g.h - 1u) * g.w + min(x, g.w - 1u)) * g.bpp;
    if (g.bpp == 1u) return p[0];
    const int R = p[0], G = p[1], B = p[2];
    if (c == 0u) return (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
    if (c == 1u) return (-11059 * R - 21709 * G + 32768 * B + 8388608 + 32767) >> 16;
    return (32768 * R - 27439 * G - 5329 * B + 8388608 + 32767) >> 16;
}

__global__ __launch_bounds__(256) void k_jpeg_transform(const uint8_t* __restrict__ img, JpegShape g, uint32_t scale, int16_t* __restrict__ coef) {
    __shared__ int s[4][64], a[4][64];
    const uint32_t t = threadIdx.x, wv = t >> 6, l = t & 63u, x = l & 7u, y = l >> 3;
    const uint32_t b = blockIdx.x * 4u + wv;
    const bool live = b < g.blocks;
    int sample = 128;
    uint32_t chroma = 0;
    if (live) {
        const uint32_t mcu = b / g.bpm, j = b - mcu * g.bpm, my = mcu / g.mcus_x, mx = mcu - my * g.mcus_x;
        if (g.sub == 0u) {
            chroma = j ? 1u : 0u;
            sample = component(img, g, j, mx * 8u + x, my * 8u + y);
        } else if (j < 4u) {
            sample = component(img, g, 0u, mx * 16u + (j & 1u) * 8u + x, my * 16u + (j >> 1) * 8u + y);
        } else {
            const uint32_t c = j - 3u, px = mx * 16u + 2u * x, py = my * 16u + 2u * y;
            chroma = 1u;
            sample = (component(img, g, c, px, py) + component(img, g, c, px + 1u, py) + component(img, g, c, px, py + 1u)
                      + component(img, g, c, px + 1u, py + 1u) + 2) >> 2;
        }
    }
    s[wv][l] = sample - 128;
    __syncthreads();
    int acc = 0; // rows: this thread is (y, u = x)
    for (uint32_t k = 0; k < 8u; k++) acc += d_tables.T[x * 8u + k] * s[wv][y * 8u + k];
    a[wv][l] = (acc + 1024) >> 11;
    __syncthreads();
    int F = 0; // columns: this thread is (v = y, u = x)
    for (uint32_t k = 0; k < 8u; k++) F += d_tables.T[y * 8u + k] * a[wv][k * 8u + x];
    const uint32_t Q = scaled_quant(d_tables.base[chroma][l], scale);
    const int m = (int)(((uint32_t)abs(F) + Q * 16384u) / (Q * 32768u));
    if (live) coef[(size_t)b * 64u + d_tables.zpos[l]] = (int16_t)(F < 0 ? -m : m);
}

__device__ inline uint32_t bit_length(uint32_t v) { return 32u - (uint32_t)__clz((int)v); } // v != 0

// The codes of one block in order: f(bits, count), count <= 26 (a 16-bit AC code and 10 value bits), the Huffman code in front of the value bits.  pred: the DC predictor.
template <class F>
__device__ inline void walk_block(const int16_t* __restrict__ c, int pred, uint32_t chroma, F&& f) {
    const uint32_t* dc = d_tables.dc[chroma];
    const uint32_t* ac = d_tables.ac[chroma];
    {
        const int d = (int)c[0] - pred;
        const uint32_t size = d ? bit_length((uint32_t)abs(d)) : 0u, e = dc[size];
        const uint32_t v = (uint32_t)(d < 0 ? d + (1 << size) - 1 : d);
        f(((e & 0xFFFFu) << size) | v, (e >> 16) + size);
    }
    uint32_t run = 0;
    for (uint32_t k = 1; k < 64u; k++) {
        const int v = c[k];
        if (!v) {
            run++;
            continue;
        }
        for (; run >= 16u; run -= 16u) f(ac[0xF0] & 0xFFFFu, ac[0xF0] >> 16);
        const uint32_t size = bit_length((uint32_t)abs(v)), e = ac[(run << 4) | size];
        f(((e & 0xFFFFu) << size) | (uint32_t)(v < 0 ? v + (1 << size) - 1 : v), (e >> 16) + size);
        run = 0;
    }
    if (run) f(ac[0] & 0xFFFFu, ac[0] >> 16);
}

// Bits from bit `at` of the words on, most significant first: bit p of the stream is bit 31 - (p & 31) of word p >> 5.  A word this thread
// fills alone is stored; the first and last words, which a neighbour may share, are or-ed into the zeroed words.
struct MsbWriter {
    uint32_t* w;
    uint64_t acc;
    uint32_t filled;
    bool shared;
    __device__ MsbWriter(uint32_t* words, uint32_t at) : w(words + (at >> 5)), acc(0), filled(at & 31u), shared((at & 31u) != 0u) {}
    __device__ void put(uint32_t v, uint32_t n) { // 1 <= n <= 32
        acc |= (uint64_t)v << (64u - filled - n);
        filled += n;
        if (filled >= 32u) {
            if (shared) {
                if ((uint32_t)(acc >> 32)) atomicOr(w, (uint32_t)(acc >> 32));
                shared = false;
            } else {
                *w = (uint32_t)(acc >> 32);
            }
            w++, acc <<= 32, filled -= 32u;
        }
    }
    __device__ void finish() {
        if ((uint32_t)(acc >> 32)) atomicOr(w, (uint32_t)(acc >> 32));
    }
};

// the block whose DC coefficient predicts block b's, or b itself when the predictor is 0 (the segment's first block of that component)
__device__ inline uint32_t predictor_block(const JpegShape& g, uint32_t b, uint32_t first_mcu) {
    const uint32_t mcu = b / g.bpm, j = b - mcu * g.bpm;
    if (g.sub == 1u && j < 4u) {
        if (j) return b - 1u;
        return mcu == first_mcu ? b : b - g.bpm + 3u;
    }
    return mcu == first_mcu ? b : b - g.bpm;
}
__device__ inline uint32_t block_chroma(const JpegShape& g, uint32_t b) {
    const uint32_t j = b % g.bpm;
    return g.sub == 1u ? (j >= 4u ? 1u : 0u) : (j ? 1u : 0u);
}

// a word other threads of the workgroup wrote or or-ed: read past the first-level cache
__device__ inline uint32_t load_shared_word(uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(BT) void k_jpeg_segment(const int16_t* __restrict__ coef, JpegShape g, uint32_t* __restrict__ bits, uint32_t* __restrict__ raw,
                                                     uint32_t raw_words, uint8_t* __restrict__ slots, uint32_t slot_bytes, uint32_t* __restrict__ meta) {
    __shared__ uint32_t sums[BT];
    const uint32_t t = threadIdx.x, seg = blockIdx.x;
    const uint32_t mcu0 = seg * g.ri, mcu1 = min(mcu0 + g.ri, g.mcus), b0 = mcu0 * g.bpm, b1 = mcu1 * g.bpm;
    uint32_t* words = raw + (size_t)seg * raw_words;
    uint8_t* slot = slots + (size_t)seg * slot_bytes;

    // the bits of the own blocks: b0 + t, b0 + t + BT, ...
    uint32_t mine = 0;
    for (uint32_t b = b0 + t; b < b1; b += BT) {
        const uint32_t pb = predictor_block(g, b, mcu0);
        uint32_t n = 0;
        walk_block(coef + (size_t)b * 64u, pb == b ? 0 : (int)coef[(size_t)pb * 64u], block_chroma(g, b), [&](uint32_t, uint32_t count) { n += count; });
        bits[b] = n;
        mine += n;
    }
    uint32_t total;
    block_exclusive_sum(sums, mine, &total);
    const uint32_t nbytes = (total + 7u) >> 3, nwords = (nbytes + 3u) >> 2;
    for (uint32_t k = t; k < nwords; k += BT) words[k] = 0u;
    __threadfence();
    __syncthreads();

    // the codes, a tile of BT consecutive blocks at a time
    uint32_t base = 0;
    for (uint32_t tile = b0; tile < b1; tile += BT) {
        const uint32_t b = tile + t, n = b < b1 ? bits[b] : 0u; // written by this thread above
        uint32_t tile_bits;
        const uint32_t at = base + block_exclusive_sum(sums, n, &tile_bits);
        if (b < b1) {
            const uint32_t pb = predictor_block(g, b, mcu0);
            MsbWriter bw(words, at);
            walk_block(coef + (size_t)b * 64u, pb == b ? 0 : (int)coef[(size_t)pb * 64u], block_chroma(g, b), [&](uint32_t v, uint32_t count) { bw.put(v, count); });
            bw.finish();
        }
        base += tile_bits;
    }
    if (t == 0u && (total & 7u)) { // 1 bits up to the byte
        const uint32_t pad = 8u - (total & 7u);
        atomicOr(words + (total >> 5), ((1u << pad) - 1u) << (32u - (total & 31u) - pad));
    }
    __threadfence();
    __syncthreads();

    // the stuffing: a run of consecutive words per thread
    const uint32_t chunk = (nwords + BT - 1u) / BT, w0 = min(t * chunk, nwords), w1 = min(w0 + chunk, nwords);
    uint32_t ff = 0;
    for (uint32_t k = w0; k < w1; k++) {
        const uint32_t v = load_shared_word(words + k);
        for (uint32_t j = 0; j < 4u; j++)
            if (4u * k + j < nbytes && ((v >> (24u - 8u * j)) & 255u) == 255u) ff++;
    }
    uint32_t ffs;
    uint32_t at = 4u * w0 + block_exclusive_sum(sums, ff, &ffs);
    for (uint32_t k = w0; k < w1; k++) {
        const uint32_t v = load_shared_word(words + k);
        for (uint32_t j = 0; j < 4u; j++) {
            if (4u * k + j >= nbytes) break;
            const uint32_t byte = (v >> (24u - 8u * j)) & 255u;
            slot[at++] = (uint8_t)byte;
            if (byte == 255u) slot[at++] = 0u;
        }
    }
    if (t == 0u) meta[seg] = nbytes + ffs;
}

// offsets[k]: where segment k starts in the scan; offsets[segments]: the scan's bytes + 2, so that segment k has
// offsets[k + 1] - offsets[k] - 2 bytes, the marker behind it aside
__global__ __launch_bounds__(BT) void k_jpeg_layout(const uint32_t* __restrict__ meta, JpegShape g, uint32_t segments, uint32_t* __restrict__ offsets,
                                                    uint32_t* __restrict__ totals, uint32_t* __restrict__ out_header) {
    __shared__ uint32_t sums[BT];
    const uint32_t t = threadIdx.x, chunk = (segments + BT - 1u) / BT, k0 = min(t * chunk, segments), k1 = min(k0 + chunk, segments);
    uint32_t bytes = 0;
    for (uint32_t k = k0; k < k1; k++) bytes += meta[k] + 2u;
    uint32_t total;
    uint32_t at = block_exclusive_sum(sums, bytes, &total);
    for (uint32_t k = k0; k < k1; k++) {
        offsets[k] = at;
        at += meta[k] + 2u;
    }
    if (t == 0u) {
        offsets[segments] = total;
        totals[0] = total - 2u;
        out_header[0] = total - 2u, out_header[1] = segments, out_header[2] = g.ri, out_header[3] = g.blocks;
    }
}

__global__ __launch_bounds__(256) void k_jpeg_compact(const uint8_t* __restrict__ slots, uint32_t slot_bytes, const uint32_t* __restrict__ offsets,
                                                      const uint32_t* __restrict__ totals, uint32_t segments, uint32_t max_words, uint32_t* __restrict__ out) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x, scan = totals[0], p0 = 4u * k;
    if (k >= max_words || p0 >= scan) return;
    uint32_t lo = 0, hi = segments; // the segment holding p0: the last one with offsets[.] <= p0
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (offsets[mid] <= p0) lo = mid;
        else hi = mid;
    }
    uint32_t sg = lo, word = 0;
    for (uint32_t j = 0; j < 4u; j++) {
        const uint32_t p = p0 + j;
        if (p >= scan) break; // the word holding the last byte is zero-padded
        while (p >= offsets[sg + 1u]) sg++;
        const uint32_t rel = p - offsets[sg], len = offsets[sg + 1u] - offsets[sg] - 2u;
        const uint32_t v = rel < len ? slots[(size_t)sg * slot_bytes + rel] : (rel == len ? 0xFFu : 0xD0u + (sg & 7u));
        word |= v << (8u * j);
    }
    out[JPEG_HEADER_BYTES / 4u + k] = word;
}

inline size_t align16(size_t x) { return (x + 15u) & ~(size_t)15u; }

} // namespace

JpegGeometry jpeg_geometry(uint32_t w, uint32_t h, uint32_t bpp, uint32_t subsampling, uint32_t ri) {
    JpegGeometry g = {};
    if (!w || !h) return g.why = "zero-sized image", g;
    if (w > 65535u || h > 65535u) return g.why = "a JPEG has at most 65535 columns and rows", g;
    if (bpp != 1u && bpp != 3u) return g.why = "bpp must be 1 or 3 (JPEG has no alpha)", g;
    if (subsampling > 1u) return g.why = "subsampling must be 0 (4:4:4) or 1 (4:2:0)", g;
    if (subsampling == 1u && bpp != 3u) return g.why = "4:2:0 needs three components", g;
    if (ri < 1u || ri > 65535u) return g.why = "restart_interval must be in 1..65535", g;
    const uint32_t side = subsampling ? 16u : 8u;
    g.width = w, g.height = h, g.bpp = bpp, g.subsampling = subsampling, g.ri = ri;
    g.bpm = bpp == 1u ? 1u : (subsampling ? 6u : 3u);
    g.mcus_x = (w + side - 1u) / side;
    const uint64_t mcus = (uint64_t)g.mcus_x * ((h + side - 1u) / side);
    const uint64_t mcu_bits = bpp == 1u ? JPEG_LUMA_BLOCK_BITS : (subsampling ? 4u : 1u) * JPEG_LUMA_BLOCK_BITS + 2u * JPEG_CHROMA_BLOCK_BITS;
    const uint64_t segments = (mcus + ri - 1u) / ri, full = segments - 1u, last = mcus - full * ri;
    const uint64_t seg_raw = ((ri < mcus ? ri : mcus) * mcu_bits + 7u) / 8u; // unstuffed bytes of the longest segment
    const uint64_t scan = full * (2u * ((ri * mcu_bits + 7u) / 8u) + 2u) + 2u * ((last * mcu_bits + 7u) / 8u);
    if (JPEG_HEADER_BYTES + scan + 16u >= ((uint64_t)1 << 31)) return g.why = "scan bound of 2^31 bytes or more unsupported (32-bit offsets)", g;
    g.ok = true;
    g.mcus = (uint32_t)mcus;
    g.blocks = g.mcus * g.bpm;
    g.segments = (uint32_t)segments;
    g.raw_words = (uint32_t)(align16(seg_raw) / 4u);
    g.slot_bytes = (uint32_t)align16(2u * seg_raw);
    g.bound = align16(JPEG_HEADER_BYTES + scan);
    g.off_bits = (size_t)g.blocks * 128u;
    g.off_meta = g.off_bits + align16(4u * (size_t)g.blocks);
    g.off_offsets = g.off_meta + align16(4u * (size_t)g.segments);
    g.off_totals = g.off_offsets + align16(4u * ((size_t)g.segments + 1u));
    g.off_raw = g.off_totals + 16u;
    g.off_slots = g.off_raw + (size_t)g.segments * g.raw_words * 4u;
    g.scratch_bytes = g.off_slots + (size_t)g.segments * g.slot_bytes;
    return g;
}

const char* jpeg_check_args(uint32_t w, uint32_t h, uint32_t bpp, uint32_t quality, uint32_t subsampling, uint32_t restart_interval, const uint8_t* d_img,
                            const void* d_out, size_t out_bytes, const void* d_scratch, size_t scratch_bytes) {
    const JpegGeometry g = jpeg_geometry(w, h, bpp, subsampling, restart_interval);
    if (!g.ok) return g.why;
    if (quality < 1u || quality > 100u) return "quality must be in 1..100";
    if (!d_img || !d_out || !d_scratch) return "null buffer";
    if (((uintptr_t)d_out & 15u) || ((uintptr_t)d_scratch & 15u)) return "misaligned buffer (d_out and d_scratch: 16 bytes)";
    if (out_bytes < g.bound) return "d_out smaller than rayn_jpeg_scan_bound";
    if (scratch_bytes < g.scratch_bytes) return "d_scratch smaller than rayn_jpeg_scratch_bytes";
    const size_t img_bytes = (size_t)w * h * bpp;
    if (d_out == (const void*)d_img || overlap(d_out, out_bytes, d_img, img_bytes)) return "d_out must not overlap d_img";
    if (overlap(d_scratch, scratch_bytes, d_img, img_bytes) || overlap(d_scratch, scratch_bytes, d_out, out_bytes)) return "d_scratch overlaps d_img or d_out";
    return nullptr;
}

static JpegShape shape_of(const JpegGeometry& g) { return {g.width, g.height, g.bpp, g.subsampling, g.bpm, g.mcus_x, g.mcus, g.blocks, g.ri}; }

void launch_jpeg_transform(hipStream_t s, const JpegGeometry& g, uint32_t quality, const uint8_t* d_img, void* d_scratch) {
    k_jpeg_transform<<<(g.blocks + 3u) / 4u, 256, 0, s>>>(d_img, shape_of(g), quality_scale(quality), (int16_t*)d_scratch);
}

void launch_jpeg_entropy(hipStream_t s, const JpegGeometry& g, void* d_out, void* d_scratch) {
    uint8_t* sc = (uint8_t*)d_scratch;
    const int16_t* coef = (const int16_t*)sc;
    uint32_t* bits = (uint32_t*)(sc + g.off_bits);
    uint32_t* meta = (uint32_t*)(sc + g.off_meta);
    uint32_t* offsets = (uint32_t*)(sc + g.off_offsets);
    uint32_t* totals = (uint32_t*)(sc + g.off_totals);
    const JpegShape sh = shape_of(g);
    k_jpeg_segment<<<g.segments, BT, 0, s>>>(coef, sh, bits, (uint32_t*)(sc + g.off_raw), g.raw_words, sc + g.off_slots, g.slot_bytes, meta);
    k_jpeg_layout<<<1, BT, 0, s>>>(meta, sh, g.segments, offsets, totals, (uint32_t*)d_out);
    const uint32_t max_words = (uint32_t)((g.bound - JPEG_HEADER_BYTES) / 4u);
    k_jpeg_compact<<<(max_words + 255u) / 256u, 256, 0, s>>>(sc + g.off_slots, g.slot_bytes, offsets, totals, g.segments, max_words, (uint32_t*)d_out);
}

void launch_jpeg_encode(hipStream_t s, const JpegGeometry& g, uint32_t quality, const uint8_t* d_img, void* d_out, void* d_scratch) {
    launch_jpeg_transform(s, g, quality, d_img, d_scratch);
    launch_jpeg_entropy(s, g, d_out, d_scratch);
}

} // namespace rayn

size_t rayn_jpeg_scan_bound(uint32_t w, uint32_t h, uint32_t bpp, uint32_t subsampling, uint32_t restart_interval) {
    const rayn::JpegGeometry g = rayn::jpeg_geometry(w, h, bpp, subsampling, restart_interval);
    return g.ok ? g.bound : 0;
}

size_t rayn_jpeg_scratch_bytes(uint32_t w, uint32_t h, uint32_t bpp, uint32_t subsampling, uint32_t restart_interval) {
    const rayn::JpegGeometry g = rayn::jpeg_geometry(w, h, bpp, subsampling, restart_interval);
    return g.ok ? g.scratch_bytes : 0;
}

int rayn_jpeg_quant_table(uint32_t quality, uint32_t which, uint8_t* out) {
    if (quality < 1u || quality > 100u || which > 1u || !out) return RAYN_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < 64u; i++) out[rayn::HOST_TABLES.zpos[i]] = (uint8_t)rayn::scaled_quant(rayn::BASE_QUANT[which][i], rayn::quality_scale(quality));
    return RAYN_OK;
}

int rayn_jpeg_huffman_table(uint32_t which, uint8_t* bits, uint8_t* vals, uint32_t n) {
    if (which > 3u || !bits || (!vals && n)) return -1;
    const rayn::JpegHuffSpec& h = rayn::HUFF[which];
    for (uint32_t k = 0; k < 16u; k++) bits[k] = h.bits[k];
    for (uint32_t k = 0; k < h.n && k < n; k++) vals[k] = h.vals[k];
    return (int)h.n;
}
