// png_lz.hip — the device PNG encoder with LZ77 matches (rayn_hip_png_encode_lz77_device) and its deflate stage alone
// (rayn_hip_deflate_lz77_device); the definition is in include/rayn_hip.h, restated in tests/png_lz_np.py.  k_png_filter, k_png_layout and
// k_png_compact are those of png.hip; k_png_lz_block takes k_png_block's place: a workgroup per 32 KiB block of R, its bytes in LDS.
//   sort      prev(i), the last position with the same three bytes: the positions sorted by their 24-bit trigram, a stable LSD radix
//             sort of six 4-bit digits between a 64 KiB array in LDS and one in the block's global scratch; equal keys then sit in
//             position order and prev is the sorted predecessor with an equal key.  No hash: the result is a function of the bytes alone.
//   matches   every thread goes backwards over its own 128 bytes: m(i, 1) from the end of the run, m(i, S) and m(i, i - prev(i)) from
//             the value at i + 1 when the distance is the same (m(i, d) = m(i + 1, d) + 1 when the first byte matches), else compared a
//             word at a time.  Long runs and short periods therefore cost one step per byte.  D(i) (0: a literal) replaces prev(i) in
//             place, and with it the exit of i: the first token start at or behind the span's end on the greedy path from i.
//   parse     one lane chains the 256 spans' exits from 0: where the greedy parse enters each span.
//   code      every thread walks its own tokens three times - histograms, sizes, bits - as k_png_block does; two Huffman codes.
// Integer arithmetic only; policy-free, built once.  Every store is a vector store; shared words are combined with integer atomicOr /
// atomicAdd on zero-initialised words.
#include "png.h"

#include "png_device.h"
#include "post_checks.h"

namespace rayn {

namespace {

constexpr uint32_t BT = PNG_BT, SPAN = PNG_SPAN, NSYM = PNG_NSYM, NDIST = PNG_NDIST, END_OF_BLOCK = PNG_END_OF_BLOCK, ADLER = PNG_ADLER;
constexpr uint32_t HEADER_BITS = 1338u, CODES_AT = 74u, DIST_AT = CODES_AT + 4u * NSYM, HDR_WORDS = (HEADER_BITS + 31u) / 32u;
constexpr uint32_t NONE = 0xFFFFu, MAX_MATCH = 258u, FAR = 4096u, DIGITS = 16u, PASSES = 6u;
static_assert(SPAN == 128u && PNG_BLOCK == 32768u, "a position takes 15 bits, an exit behind its span's end 9");

// the four bytes from byte i on (the word behind the block's last is there to be read, see PNG_LDS_WORDS)
__device__ inline uint32_t word_at(const uint32_t* sw, uint32_t i) {
    const uint32_t w0 = i >> 2, w1 = w0 + 1u;
    const uint64_t x = ((uint64_t)sw[w1 + (w1 >> 5)] << 32) | sw[w0 + (w0 >> 5)];
    return (uint32_t)(x >> ((i & 3u) * 8u));
}
__device__ inline uint32_t trigram(const uint32_t* sw, uint32_t i) { return word_at(sw, i) & 0xFFFFFFu; }

// m: the largest L <= cap with byte a + k == byte b + k for all k < L (a < b, b + cap <= len; the ranges may overlap)
__device__ inline uint32_t match_len(const uint32_t* sw, uint32_t a, uint32_t b, uint32_t cap) {
    uint32_t L = 0;
    while (L < cap) {
        const uint32_t x = word_at(sw, a + L) ^ word_at(sw, b + L);
        if (x) {
            L += ((uint32_t)__ffs((int)x) - 1u) >> 3;
            break;
        }
        L += 4u;
    }
    return min(L, cap);
}

// One pass of the sort: the elements src[k0..k1) of this thread (k itself when src is null), in order, to where their digit puts them.
// cnt: DIGITS * BT counters, cnt[d * BT + t] thread t's alone.  Stable: the counters are summed digit-major, thread-minor.
template <class Src, class Dst>
__device__ __forceinline__ void sort_pass(const uint32_t* sw, Src src, Dst dst, uint32_t* cnt, uint32_t* sums, uint32_t pass, uint32_t k0, uint32_t k1) {
    const uint32_t t = threadIdx.x, at = pass >> 1, shift = (pass & 1u) * 4u;
    for (uint32_t d = 0; d < DIGITS; d++) cnt[d * BT + t] = 0u;
    for (uint32_t k = k0; k < k1; k++) {
        const uint32_t e = src ? (uint32_t)src[k] : k;
        cnt[((byte_at(sw, e + at) >> shift) & 15u) * BT + t]++;
    }
    __syncthreads();
    uint32_t sum = 0;
    for (uint32_t j = 0; j < DIGITS; j++) sum += cnt[DIGITS * t + j];
    uint32_t total;
    uint32_t run = block_exclusive_sum(sums, sum, &total);
    for (uint32_t j = 0; j < DIGITS; j++) {
        const uint32_t v = cnt[DIGITS * t + j];
        cnt[DIGITS * t + j] = run;
        run += v;
    }
    __syncthreads();
    for (uint32_t k = k0; k < k1; k++) {
        const uint32_t e = src ? (uint32_t)src[k] : k;
        dst[cnt[((byte_at(sw, e + at) >> shift) & 15u) * BT + t]++] = (uint16_t)e;
    }
    __syncthreads();
}

// The tokens that start in this thread's span, in order, from where the parse enters it: f(first byte, M, D), M = 0 for a literal
template <class F>
__device__ inline void walk_tokens(const uint32_t* sw, const uint16_t* pos, uint32_t enter, uint32_t hi, uint32_t len, F&& f) {
    if (enter == PNG_NO_START) return;
    for (uint32_t p = enter; p < hi;) {
        const uint32_t D = pos[p] & 0x7FFFu;
        if (D) {
            const uint32_t M = match_len(sw, p - D, p, min(MAX_MATCH, len - p));
            f(0u, M, D);
            p += max(M, 1u); // M >= 3: D(p) reaches M(p)
        } else {
            f(byte_at(sw, p), 0u, 0u);
            p++;
        }
    }
}

template <bool SEG>
__global__ __launch_bounds__(BT) void k_png_lz_block(const uint8_t* __restrict__ R, uint32_t n, uint32_t stride, uint32_t nblocks, PngSegments seg,
                                                     PngMeta* __restrict__ meta, uint8_t* __restrict__ slots, uint16_t* positions) {
    __shared__ uint32_t sw[PNG_LDS_WORDS];
    __shared__ uint16_t pos[PNG_BLOCK];      // the sort's array in LDS; prev(i); then D(i) | bit 8 of the exit << 15
    __shared__ uint32_t ex[PNG_BLOCK / 4u];  // the sort's counters; then a byte per position: bits 0..7 of the exit, relative to the span's end
    __shared__ uint32_t hist[NSYM], dhist[NDIST];
    __shared__ HuffmanLds<NSYM> hl;
    __shared__ HuffmanLds<NDIST> hd;
    __shared__ uint32_t first_start[BT], sums[BT], enter[BT];
    __shared__ uint32_t hdr[HDR_WORDS];
    __shared__ uint32_t sh_a, sh_b, sh_bits;

    const uint32_t t = threadIdx.x, blk = blockIdx.x;
    const PngBlockSpan span = block_span<SEG>(blk, n, nblocks, seg);
    const uint32_t base = span.base, len = span.len;
    const bool final_block = span.final_block;
    uint32_t* slot = (uint32_t*)(slots + (size_t)blk * PNG_SLOT);
    uint16_t* far = positions + (size_t)blk * PNG_BLOCK; // the sort's second array
    uint8_t* ex8 = (uint8_t*)ex;

    // the block's bytes, a word at a time (R is 16-byte aligned and padded to 16: the word holding the last byte can be read whole)
    const uint32_t* Rw = (const uint32_t*)(R + base);
    for (uint32_t k = t; k < (len + 3u) >> 2; k += BT) sw[k + (k >> 5)] = Rw[k];
    for (uint32_t s = t; s < NSYM; s += BT) hist[s] = 0u;
    if (t < NDIST) dhist[t] = 0u;
    if (t < HDR_WORDS) hdr[t] = 0u;
    enter[t] = PNG_NO_START;
    if (t == 0u) sh_a = sh_b = sh_bits = 0u;
    __syncthreads();

    // run starts of the own span, Adler-32 partial sums
    const uint32_t lo = min(t * SPAN, len), hi = min(lo + SPAN, len);
    {
        uint32_t first = PNG_NO_START, a = 0, b = 0, before = lo ? byte_at(sw, lo - 1u) : 256u;
        for (uint32_t i = lo; i < hi; i++) {
            const uint32_t v = byte_at(sw, i);
            if (v != before && first == PNG_NO_START) first = i;
            before = v;
            a += v;
            b += (len - i) * v; // <= 128 * 32768 * 255 < 2^32
        }
        first_start[t] = first;
        atomicAdd(&sh_a, a % ADLER);
        atomicAdd(&sh_b, b % ADLER);
    }

    // prev(i) into pos[i]: the positions with three bytes in front of them, sorted by those bytes
    const uint32_t npos = len >= 3u ? len - 2u : 0u, k0 = min(t * SPAN, npos), k1 = min(k0 + SPAN, npos);
    sort_pass(sw, (const uint16_t*)nullptr, pos, ex, sums, 0u, k0, k1);
    sort_pass(sw, (const uint16_t*)pos, far, ex, sums, 1u, k0, k1);
    sort_pass(sw, (const uint16_t*)far, pos, ex, sums, 2u, k0, k1);
    sort_pass(sw, (const uint16_t*)pos, far, ex, sums, 3u, k0, k1);
    sort_pass(sw, (const uint16_t*)far, pos, ex, sums, 4u, k0, k1);
    sort_pass(sw, (const uint16_t*)pos, far, ex, sums, 5u, k0, k1);
    static_assert(PASSES == 6u, "six digits of four bits: the 24-bit key");
    for (uint32_t k = k0; k < k1; k++) {
        const uint32_t e = far[k];
        uint32_t p = NONE;
        if (k) {
            const uint32_t e0 = far[k - 1u];
            if (trigram(sw, e0) == trigram(sw, e)) p = e0;
        }
        pos[e] = (uint16_t)p;
    }
    if (t == 0u)
        for (uint32_t i = npos; i < len; i++) pos[i] = (uint16_t)NONE;
    __syncthreads();

    // M(i), D(i) and the exits of the own span, backwards
    if (lo < hi) {
        uint32_t re = len; // where the run holding byte hi - 1 ends: the first run start at or behind hi
        for (uint32_t u = t + 1u; u < BT; u++)
            if (first_start[u] != PNG_NO_START) {
                re = first_start[u];
                break;
            }
        uint32_t rS = (stride && hi < len && hi >= stride) ? match_len(sw, hi - stride, hi, min(MAX_MATCH, len - hi)) : 0u;
        uint32_t rP = 0, d_behind = 0, behind = 256u; // the match at prev's distance and that distance at i + 1; byte i + 1
        for (uint32_t i = hi; i-- > lo;) {
            const uint32_t v = byte_at(sw, i);
            if (behind != 256u && behind != v) re = i + 1u;
            behind = v;
            const uint32_t cap = min(MAX_MATCH, len - i);
            const uint32_t m1 = (i && byte_at(sw, i - 1u) == v) ? min(MAX_MATCH, re - i) : 0u;
            rS = (stride && i >= stride && byte_at(sw, i - stride) == v) ? min(rS + 1u, MAX_MATCH) : 0u;
            const uint32_t p = pos[i];
            uint32_t dP = 0;
            if (p != NONE) {
                dP = i - p;
                rP = dP == d_behind ? min(rP + 1u, MAX_MATCH) : match_len(sw, p, i, cap);
            } else {
                rP = 0u;
            }
            d_behind = dP;
            uint32_t M = m1, D = 1u; // the longest, at the smallest distance that reaches it
            if (rP > M || (rP == M && dP < D)) M = rP, D = dP;
            if (rS > M || (rS == M && stride < D)) M = rS, D = stride;
            const bool take = M >= 3u && !(M == 3u && D > FAR);
            const uint32_t next = i + (take ? M : 1u);
            const uint32_t x = next >= hi ? next - hi : (uint32_t)ex8[next] | ((uint32_t)(pos[next] >> 15) << 8);
            ex8[i] = (uint8_t)x;
            pos[i] = (uint16_t)((take ? D : 0u) | ((x >> 8) << 15));
        }
    }
    __syncthreads();
    if (t == 0u) // the greedy parse from 0, a span at a time
        for (uint32_t cur = 0; cur < len;) {
            const uint32_t u = cur / SPAN;
            enter[u] = cur;
            cur = min((u + 1u) * SPAN, len) + ((uint32_t)ex8[cur] | ((uint32_t)(pos[cur] >> 15) << 8));
        }
    __syncthreads();
    const uint32_t mine_from = enter[t];

    // histograms over the 286 literal/length and the 30 distance symbols; end-of-block counts 1
    walk_tokens(sw, pos, mine_from, hi, len, [&](uint32_t v, uint32_t M, uint32_t D) {
        uint32_t sym = v, dsym, xb, xv;
        if (M) {
            length_code(M, &sym, &xb, &xv);
            distance_code(D, &dsym, &xb, &xv);
            atomicAdd(&dhist[dsym], 1u);
        }
        atomicAdd(&hist[sym], 1u);
    });
    if (t == 0u) atomicAdd(&hist[END_OF_BLOCK], 1u);
    huffman_code(hist, hl);
    huffman_code(dhist, hd);
    for (uint32_t s = t; s < NSYM; s += BT) {
        const uint32_t l = hl.clen[s];
        if (l) atomicAdd(&sh_bits, hist[s] * (l + symbol_extra_bits(s)));
        or_bits(hdr, CODES_AT + 4u * s, __brev(l) >> 28); // the code-length code: symbol l has the 4-bit code l
    }
    if (t < NDIST) {
        const uint32_t l = hd.clen[t];
        if (dhist[t]) atomicAdd(&sh_bits, dhist[t] * (l + distance_extra_bits(t)));
        or_bits(hdr, DIST_AT + 4u * t, __brev(l) >> 28);
    }
    __syncthreads();
    const uint32_t bits = HEADER_BITS + sh_bits, huffman_bytes = (bits + 7u) >> 3;
    const bool stored = huffman_bytes >= len + 5u;

    uint32_t bytes;
    if (stored) {
        store_block((uint8_t*)slot, sw, len, final_block);
        bytes = len + 5u;
    } else {
        if (t == 0u) {
            or_bits(hdr, 0u, (final_block ? 1u : 0u) | (2u << 1) | (29u << 3) | (29u << 8) | (15u << 13)); // BFINAL BTYPE HLIT HDIST HCLEN
            for (uint32_t j = 0; j < 16u; j++) or_bits(hdr, 26u + 3u * j, 4u); // lengths of the code-length code: 0 for 16, 17, 18, then 4
        }
        const uint32_t* tab = hl.tab;
        const uint32_t* dtab = hd.tab;
        // where the own tokens go
        uint32_t mine = 0;
        walk_tokens(sw, pos, mine_from, hi, len, [&](uint32_t v, uint32_t M, uint32_t D) {
            uint32_t sym = v, dsym, xb = 0, dxb, xv;
            if (M) {
                length_code(M, &sym, &xb, &xv);
                distance_code(D, &dsym, &dxb, &xv);
                mine += (dtab[dsym] >> 16) + dxb;
            }
            mine += (tab[sym] >> 16) + xb;
        });
        if (t == BT - 1u) mine += tab[END_OF_BLOCK] >> 16;
        uint32_t total;
        const uint32_t at = HEADER_BITS + block_exclusive_sum(sums, mine, &total); // its barriers also publish hdr
        if (t < HDR_WORDS - 1u) slot[t] = hdr[t];
        else if (t == HDR_WORDS - 1u) atomicOr(&slot[t], hdr[t]);
        BitWriter bw(slot, at);
        walk_tokens(sw, pos, mine_from, hi, len, [&](uint32_t v, uint32_t M, uint32_t D) {
            uint32_t sym = v, dsym, xb = 0, xv = 0, dxb, dxv;
            if (M) length_code(M, &sym, &xb, &xv);
            const uint32_t e = tab[sym], l = e >> 16;
            bw.put((e & 0xFFFFu) | (xv << l), l + xb);
            if (M) {
                distance_code(D, &dsym, &dxb, &dxv);
                const uint32_t de = dtab[dsym], dl = de >> 16;
                bw.put((de & 0xFFFFu) | (dxv << dl), dl + dxb);
            }
        });
        if (t == BT - 1u) bw.put(tab[END_OF_BLOCK] & 0xFFFFu, tab[END_OF_BLOCK] >> 16);
        bw.finish();
        if (final_block) {
            bytes = huffman_bytes;
        } else { // an empty stored block: 000, zero padding to the byte, 00 00 FF FF
            const uint32_t p = (bits + 3u + 7u) >> 3;
            if (t == 0u) or_bits(slot, 8u * (p + 2u), 0xFFFFu);
            bytes = p + 4u;
        }
    }
    if (t == 0u) meta[blk] = PngMeta{bytes, sh_a % ADLER, sh_b % ADLER, stored ? 1u : 0u};
}

// What both entries ask of their buffers, png_check_args' rules: src is d_img or d_data
const char* check_buffers(const PngGeometry& g, const void* src, size_t src_bytes, const void* d_out, size_t out_bytes, const void* d_scratch,
                          size_t scratch_bytes, const char* small_out, const char* small_scratch, const char* out_on_src, const char* scratch_on) {
    if (!src || !d_out || !d_scratch) return "null buffer";
    if (((uintptr_t)d_out & 15u) || ((uintptr_t)d_scratch & 15u)) return "misaligned buffer (d_out and d_scratch: 16 bytes)";
    if (out_bytes < g.bound) return small_out;
    if (scratch_bytes < png_lz_scratch_bytes(g)) return small_scratch;
    if (d_out == src || overlap(d_out, out_bytes, src, src_bytes)) return out_on_src;
    if (overlap(d_scratch, scratch_bytes, src, src_bytes) || overlap(d_scratch, scratch_bytes, d_out, out_bytes)) return scratch_on;
    return nullptr;
}

hipError_t launch_blocks(hipStream_t s, const PngGeometry& g, uint32_t stride, void* d_out, void* d_scratch) {
    uint8_t* sc = (uint8_t*)d_scratch;
    k_png_lz_block<false><<<g.blocks, BT, 0, s>>>(sc, g.n, stride, g.blocks, PngSegments{}, (PngMeta*)(sc + g.off_meta), sc + g.off_slots, (uint16_t*)(sc + g.scratch_bytes));
    launch_png_finish(s, g, d_out, d_scratch);
    return hipSuccess;
}

} // namespace

size_t png_lz_scratch_bytes(const PngGeometry& g) { return g.scratch_bytes + (size_t)g.blocks * PNG_LZ_POSITIONS; }

const char* png_lz_check_args(uint32_t w, uint32_t h, uint32_t bpp, const uint8_t* d_img, const void* d_out, size_t out_bytes, const void* d_scratch,
                              size_t scratch_bytes) {
    const PngGeometry g = png_geometry(w, h, bpp);
    if (!g.ok) return g.why;
    return check_buffers(g, d_img, (size_t)w * h * bpp, d_out, out_bytes, d_scratch, scratch_bytes, "d_out smaller than rayn_png_stream_bound",
                         "d_scratch smaller than rayn_png_scratch_bytes_lz77", "d_out must not overlap d_img", "d_scratch overlaps d_img or d_out");
}

const char* deflate_check_args(const void* d_data, size_t n, const void* d_out, size_t out_bytes, const void* d_scratch, size_t scratch_bytes) {
    const PngGeometry g = stream_geometry(n);
    if (!g.ok) return g.why;
    return check_buffers(g, d_data, n, d_out, out_bytes, d_scratch, scratch_bytes, "d_out smaller than rayn_deflate_stream_bound",
                         "d_scratch smaller than rayn_deflate_scratch_bytes", "d_out must not overlap d_data", "d_scratch overlaps d_data or d_out");
}

void launch_png_lz_block_segmented(hipStream_t s, const uint8_t* R, uint32_t n, uint32_t nblocks, PngSegments seg, uint32_t stride, PngMeta* meta,
                                   uint8_t* slots, uint16_t* positions) {
    k_png_lz_block<true><<<nblocks, BT, 0, s>>>(R, n, stride, nblocks, seg, meta, slots, positions);
}

hipError_t launch_png_encode_lz77(hipStream_t s, uint32_t w, uint32_t h, uint32_t bpp, const uint8_t* d_img, void* d_out, void* d_scratch) {
    const PngGeometry g = png_geometry(w, h, bpp);
    uint8_t* sc = (uint8_t*)d_scratch;
    if (hipError_t e = hipMemsetAsync(sc + g.off_slots, 0, (size_t)g.blocks * PNG_SLOT, s)) return e; // the emit ors into zeroed words
    launch_png_filter(s, w, h, bpp, d_img, sc);
    return launch_blocks(s, g, g.stride, d_out, d_scratch);
}

hipError_t launch_deflate_lz77(hipStream_t s, const void* d_data, uint32_t n, uint32_t stride, void* d_out, void* d_scratch) {
    const PngGeometry g = stream_geometry(n);
    uint8_t* sc = (uint8_t*)d_scratch;
    if (hipError_t e = hipMemsetAsync(sc + g.off_slots, 0, (size_t)g.blocks * PNG_SLOT, s)) return e;
    if (hipError_t e = hipMemcpyAsync(sc, d_data, n, hipMemcpyDeviceToDevice, s)) return e; // R: aligned, and padded to the word the kernel reads
    return launch_blocks(s, g, stride, d_out, d_scratch);
}

} // namespace rayn

size_t rayn_png_scratch_bytes_lz77(uint32_t w, uint32_t h, uint32_t bpp) {
    const rayn::PngGeometry g = rayn::png_geometry(w, h, bpp);
    return g.ok ? rayn::png_lz_scratch_bytes(g) : 0;
}

size_t rayn_deflate_stream_bound(size_t n) {
    const rayn::PngGeometry g = rayn::stream_geometry(n);
    return g.ok ? g.bound : 0;
}

size_t rayn_deflate_scratch_bytes(size_t n) {
    const rayn::PngGeometry g = rayn::stream_geometry(n);
    return g.ok ? rayn::png_lz_scratch_bytes(g) : 0;
}
