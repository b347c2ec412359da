// png_device.h — device side the two PNG block kernels share (k_png_block of png.hip, k_png_lz_block of png_lz.hip): the block's bytes
// in padded LDS, the length and distance codes of RFC 1951 3.2.5, the bit writer, the workgroup's exclusive sum and the Huffman
// construction of include/rayn_hip.h, generic in the symbol count.  Integer arithmetic only; every store is a vector store; shared words
// are combined with integer atomicOr / atomicAdd on zero-initialised words.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "png.h"

namespace rayn {

constexpr uint32_t PNG_BT = 256u;                                           // threads of a block kernel
constexpr uint32_t PNG_SPAN = PNG_BLOCK / PNG_BT;                           // consecutive bytes of the block a thread tokenises
constexpr uint32_t PNG_LDS_WORDS = PNG_BLOCK / 4u + PNG_BLOCK / 128u + 2u;  // one pad word per 32: a thread's 32 words start on bank (33 * t) % 32;
                                                                            // two more, so that the word behind the last one can be read
constexpr uint32_t PNG_NSYM = 286u, PNG_NDIST = 30u, PNG_END_OF_BLOCK = 256u, PNG_ADLER = 65521u;
constexpr uint32_t PNG_NO_START = 0xFFFFFFFFu;

// Where block blk lies in R.  SEG = false: R is one stream of n bytes, cut every PNG_BLOCK.  SEG = true: R is segments of seg.bytes
// bytes (the last one may be shorter), every segment cut on its own into seg.blocks blocks - a stream of its own, with its own final block.
struct PngBlockSpan {
    uint32_t base, len;
    bool final_block;
};
template <bool SEG>
__device__ inline PngBlockSpan block_span(uint32_t blk, uint32_t n, uint32_t nblocks, PngSegments seg) {
    if constexpr (SEG) {
        const uint32_t first = blk / seg.blocks * seg.bytes, at = blk % seg.blocks * PNG_BLOCK, left = min(seg.bytes, n - first) - at;
        return {first + at, min(PNG_BLOCK, left), left <= PNG_BLOCK};
    } else {
        const uint32_t base = blk * PNG_BLOCK;
        return {base, min(PNG_BLOCK, n - base), blk + 1u == nblocks};
    }
}

__device__ inline uint32_t byte_at(const uint32_t* sw, uint32_t i) {
    const uint32_t wi = i >> 2;
    return (sw[wi + (wi >> 5)] >> ((i & 3u) * 8u)) & 255u;
}

// (symbol, extra bits, extra value) of a match length 3..258, RFC 1951 3.2.5
__device__ inline void length_code(uint32_t n, uint32_t* sym, uint32_t* xbits, uint32_t* xval) {
    const uint32_t l = n - 3u;
    if (n == 258u) {
        *sym = 285u, *xbits = 0u, *xval = 0u;
    } else if (l < 8u) {
        *sym = 257u + l, *xbits = 0u, *xval = 0u;
    } else {
        const uint32_t x = 29u - (uint32_t)__clz((int)l); // floor(log2 l) - 2
        *sym = 261u + 4u * x + ((l >> x) & 3u), *xbits = x, *xval = l & ((1u << x) - 1u);
    }
}
__device__ inline uint32_t symbol_extra_bits(uint32_t s) { return s < 265u || s == 285u ? 0u : (s - 261u) >> 2; }

// (symbol, extra bits, extra value) of a match distance 1..32768, RFC 1951 3.2.5
__device__ inline void distance_code(uint32_t d, uint32_t* sym, uint32_t* xbits, uint32_t* xval) {
    const uint32_t l = d - 1u;
    if (l < 4u) {
        *sym = l, *xbits = 0u, *xval = 0u;
    } else {
        const uint32_t x = 30u - (uint32_t)__clz((int)l); // floor(log2 l) - 1
        *sym = 2u * x + 2u + ((l >> x) & 1u), *xbits = x, *xval = l & ((1u << x) - 1u);
    }
}
__device__ inline uint32_t distance_extra_bits(uint32_t s) { return s < 4u ? 0u : (s - 2u) >> 1; }

// the bits of v (<= 32) at bit `at` of zero-initialised words others write too, in LDS or in global memory
__device__ inline void or_bits(uint32_t* words, uint32_t at, uint32_t v) {
    const uint64_t x = (uint64_t)v << (at & 31u);
    uint32_t* w = words + (at >> 5);
    if ((uint32_t)x) atomicOr(w, (uint32_t)x);
    if ((uint32_t)(x >> 32)) atomicOr(w + 1, (uint32_t)(x >> 32));
}

// Bits from bit `at` of the slot on, least-significant first.  A word this thread fills alone is stored; the first and last words, which
// a neighbour may share, are or-ed into the zero-initialised slot.
struct BitWriter {
    uint32_t* w;
    uint64_t acc;
    uint32_t filled;
    bool shared;
    __device__ BitWriter(uint32_t* words, uint32_t at) : w(words + (at >> 5)), acc(0), filled(at & 31u), shared((at & 31u) != 0u) {}
    __device__ void put(uint32_t v, uint32_t n) { // n <= 32
        acc |= (uint64_t)v << filled;
        filled += n;
        if (filled >= 32u) {
            if (shared) {
                if ((uint32_t)acc) atomicOr(w, (uint32_t)acc);
                shared = false;
            } else {
                *w = (uint32_t)acc;
            }
            w++, acc >>= 32, filled -= 32u;
        }
    }
    __device__ void finish() {
        if ((uint32_t)acc) atomicOr(w, (uint32_t)acc);
    }
};

// blockDim.x = PNG_BT: the exclusive sum of v over the threads; *total the sum.  buf: PNG_BT words of LDS.
__device__ inline uint32_t block_exclusive_sum(uint32_t* buf, uint32_t v, uint32_t* total) {
    const uint32_t t = threadIdx.x;
    __syncthreads();
    buf[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < PNG_BT; d <<= 1) {
        const uint32_t add = t >= d ? buf[t - d] : 0u;
        __syncthreads();
        buf[t] += add;
        __syncthreads();
    }
    const uint32_t incl = buf[t];
    *total = buf[PNG_BT - 1u];
    __syncthreads();
    return incl - v;
}

// The LDS of one Huffman code over N symbols
template <uint32_t N>
struct HuffmanLds {
    uint32_t work[N], tab[N], clen[N]; // halved frequencies, (reversed code | length << 16), lengths
    uint32_t wt[N];                    // weights of the internal nodes, in creation order
    uint16_t sorted[N], parent[2u * N];
    uint32_t count[16], next_code[16];
    uint32_t leaves, depth;
};

// The whole workgroup (PNG_BT threads): the code of the frequencies hist[0..N) into h.clen and h.tab.  Code lengths are the depths of the
// Huffman tree, frequencies halved while a depth exceeds 15; the codes are the canonical ones of RFC 1951 3.2.2, bit-reversed: deflate
// packs a Huffman code from its most significant bit.  With fewer than two symbols in use the used one - symbol 0 when there is none -
// gets length 1.  hist is published by the first barrier in here; h.clen and h.tab by the last.
template <uint32_t N>
__device__ inline void huffman_code(const uint32_t* hist, HuffmanLds<N>& h) {
    const uint32_t t = threadIdx.x;
    __syncthreads();
    for (uint32_t s = t; s < N; s += PNG_BT) h.work[s] = hist[s];
    for (;;) {
        if (t == 0u) h.leaves = h.depth = 0u;
        __syncthreads();
        for (uint32_t s = t; s < N; s += PNG_BT) { // rank of (weight, symbol) among the symbols in use
            const uint32_t f = h.work[s];
            if (f) {
                uint32_t rank = 0;
                for (uint32_t u = 0; u < N; u++) {
                    const uint32_t g = h.work[u];
                    rank += (g != 0u && (g < f || (g == f && u < s))) ? 1u : 0u;
                }
                h.sorted[rank] = (uint16_t)s;
                atomicAdd(&h.leaves, 1u);
            }
        }
        __syncthreads();
        const uint32_t leaves = h.leaves;
        if (leaves < 2u) {
            for (uint32_t s = t; s < N; s += PNG_BT) h.clen[s] = (leaves ? h.work[s] != 0u : s == 0u) ? 1u : 0u;
            __syncthreads();
            break;
        }
        const uint32_t root = N + leaves - 2u;
        if (t == 0u) { // two queues: the sorted leaves, and the internal nodes in creation order; a leaf goes first on equal weight
            uint32_t li = 0, ii = 0;
            for (uint32_t k = 0; k + 1u < leaves; k++) {
                uint32_t sum = 0;
                for (int j = 0; j < 2; j++) {
                    const uint32_t lw = li < leaves ? h.work[h.sorted[li]] : 0xFFFFFFFFu, iw = ii < k ? h.wt[ii] : 0xFFFFFFFFu;
                    if (lw <= iw) {
                        h.parent[h.sorted[li++]] = (uint16_t)(N + k);
                        sum += lw;
                    } else {
                        h.parent[N + ii++] = (uint16_t)(N + k);
                        sum += iw;
                    }
                }
                h.wt[k] = sum;
            }
        }
        __syncthreads();
        for (uint32_t s = t; s < N; s += PNG_BT) {
            uint32_t d = 0;
            if (h.work[s])
                for (uint32_t k = s; k != root; k = h.parent[k]) d++;
            h.clen[s] = d;
            if (d) atomicMax(&h.depth, d);
        }
        __syncthreads();
        if (h.depth <= 15u) break;
        __syncthreads(); // everyone has read the depth before it is reset
        for (uint32_t s = t; s < N; s += PNG_BT)
            if (h.work[s]) h.work[s] = (h.work[s] + 1u) >> 1;
    }
    if (t < 16u) h.count[t] = 0u;
    __syncthreads();
    for (uint32_t s = t; s < N; s += PNG_BT)
        if (h.clen[s]) atomicAdd(&h.count[h.clen[s]], 1u);
    __syncthreads();
    if (t == 0u) {
        uint32_t code = 0;
        h.next_code[0] = 0u;
        for (uint32_t bits = 1; bits < 16u; bits++) {
            code = (code + (bits > 1u ? h.count[bits - 1u] : 0u)) << 1;
            h.next_code[bits] = code;
        }
    }
    __syncthreads();
    for (uint32_t s = t; s < N; s += PNG_BT) {
        const uint32_t l = h.clen[s];
        uint32_t e = 0;
        if (l) {
            uint32_t code = h.next_code[l];
            for (uint32_t u = 0; u < s; u++) code += h.clen[u] == l ? 1u : 0u;
            e = (__brev(code) >> (32u - l)) | (l << 16);
        }
        h.tab[s] = e;
    }
    __syncthreads();
}

// The stored form of the block (BTYPE 0) into its slot: BFINAL, LEN, NLEN, the bytes
__device__ inline void store_block(uint8_t* out, const uint32_t* sw, uint32_t len, bool final_block) {
    const uint32_t t = threadIdx.x;
    if (t == 0u) {
        out[0] = final_block ? 1u : 0u;
        out[1] = (uint8_t)len, out[2] = (uint8_t)(len >> 8);
        out[3] = (uint8_t)~len, out[4] = (uint8_t)(~len >> 8);
    }
    for (uint32_t i = t; i < len; i += PNG_BT) out[5u + i] = (uint8_t)byte_at(sw, i);
}

} // namespace rayn
