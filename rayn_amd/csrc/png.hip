// png.hip — the zlib stream of a PNG's IDAT chunk, encoded on the device (rayn_hip_png_encode_device; the definition is in
// include/rayn_hip.h, restated in tests/png_np.py).  Four kernels behind one memset:
//   k_png_filter   a workgroup per row: the five PNG filters and their costs, the row of the filtered stream R
//   k_png_block    a workgroup per 32 KiB block of R, the block's bytes in LDS: run tokens, histogram, Huffman code, the choice between the
//                  Huffman and the stored form, the block's bytes into its own slot of the scratch, its Adler-32 partial sums
//   k_png_layout   one workgroup: the exclusive sum of the block sizes, the Adler-32, the 16-byte header
//   k_png_compact  a thread per output word: 78 01, the blocks from their slots, the Adler-32, contiguously into the output
// k_png_block<true> is the same kernel on segments of R that are streams of their own (the chunks of exr.hip): only where a block lies
// and which one is final differ (block_span, png_device.h).
// Integer arithmetic only; policy-free, built once.  Every store is a vector store; shared words are combined with integer atomicOr on
// zero-initialised words.
#include "png.h"

#include "png_device.h"
#include "post_checks.h"

namespace rayn {

namespace {

constexpr uint32_t BT = PNG_BT, SPAN = PNG_SPAN, LDS_WORDS = PNG_LDS_WORDS;
constexpr uint32_t NSYM = PNG_NSYM, END_OF_BLOCK = PNG_END_OF_BLOCK, ADLER = PNG_ADLER, HEADER_BITS = 1222u, CODES_AT = 74u, DIST_AT = 1218u;
constexpr uint32_t NO_START = PNG_NO_START;

// The tokens whose first byte lies in [lo, hi), in order: f(symbol, extra bits, extra value).  run_start: where the run holding byte lo
// begins (<= lo); next_start: the first run start at or behind hi, the block's length when there is none.
template <class F>
__device__ inline void walk_tokens(const uint32_t* sw, uint32_t lo, uint32_t hi, uint32_t run_start, uint32_t next_start, F&& f) {
    uint32_t i = lo, s = run_start;
    while (i < hi) {
        const uint32_t v = byte_at(sw, i);
        uint32_t seg_end = i + 1u;
        while (seg_end < hi && byte_at(sw, seg_end) == v) seg_end++;
        const uint32_t e = seg_end == hi ? next_start : seg_end; // the run is [s, e); [i, seg_end) of it is ours
        if (s == i) f(v, 0u, 0u);
        const uint32_t r = e - s - 1u, full = r / 258u, tail = r - full * 258u, base = s + 1u, ts = base + full * 258u;
        if (full) {
            uint32_t q = i <= base ? 0u : (i - base + 257u) / 258u;
            for (; q < full && base + q * 258u < seg_end; q++) f(285u, 0u, 0u);
        }
        if (tail >= 3u) {
            if (ts >= i && ts < seg_end) {
                uint32_t sym, xb, xv;
                length_code(tail, &sym, &xb, &xv);
                f(sym, xb, xv);
            }
        } else {
            for (uint32_t k = 0; k < tail; k++)
                if (ts + k >= i && ts + k < seg_end) f(v, 0u, 0u);
        }
        i = s = seg_end;
    }
}

__device__ inline uint32_t abs_i8(uint32_t f) {
    f &= 255u;
    return f < 128u ? f : 256u - f;
}

// The byte x of row y under filter `type`; a, b, c: the bytes to the left, above and above-left (0 outside the image)
__device__ inline uint32_t filtered(uint32_t type, uint32_t X, uint32_t a, uint32_t b, uint32_t c) {
    switch (type) {
    case 0: return X;
    case 1: return (X - a) & 255u;
    case 2: return (X - b) & 255u;
    case 3: return (X - ((a + b) >> 1)) & 255u;
    default: {
        const int p = (int)a + (int)b - (int)c;
        const int pa = abs(p - (int)a), pb = abs(p - (int)b), pc = abs(p - (int)c);
        const uint32_t pr = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
        return (X - pr) & 255u;
    }
    }
}

__global__ __launch_bounds__(256) void k_png_filter(const uint8_t* __restrict__ img, uint32_t rowbytes, uint32_t bpp, uint8_t* __restrict__ R) {
    __shared__ uint32_t cost[5];
    const uint32_t y = blockIdx.x, t = threadIdx.x;
    const uint8_t* cur = img + (size_t)y * rowbytes;
    const uint8_t* prev = cur - rowbytes; // read for y > 0 only
    if (t < 5u) cost[t] = 0u;
    __syncthreads();
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
    for (uint32_t x = t; x < rowbytes; x += 256u) {
        const uint32_t X = cur[x], a = x >= bpp ? cur[x - bpp] : 0u, b = y ? prev[x] : 0u, c = (y && x >= bpp) ? prev[x - bpp] : 0u;
        c0 += abs_i8(filtered(0, X, a, b, c));
        c1 += abs_i8(filtered(1, X, a, b, c));
        c2 += abs_i8(filtered(2, X, a, b, c));
        c3 += abs_i8(filtered(3, X, a, b, c));
        c4 += abs_i8(filtered(4, X, a, b, c));
    }
    atomicAdd(&cost[0], c0);
    atomicAdd(&cost[1], c1);
    atomicAdd(&cost[2], c2);
    atomicAdd(&cost[3], c3);
    atomicAdd(&cost[4], c4);
    __syncthreads();
    uint32_t type = 0, best = cost[0];
    for (uint32_t k = 1; k < 5u; k++)
        if (cost[k] < best) best = cost[k], type = k; // the lowest type wins a tie
    uint8_t* out = R + (size_t)y * (rowbytes + 1u);
    if (t == 0u) out[0] = (uint8_t)type;
    for (uint32_t x = t; x < rowbytes; x += 256u) {
        const uint32_t X = cur[x], a = x >= bpp ? cur[x - bpp] : 0u, b = y ? prev[x] : 0u, c = (y && x >= bpp) ? prev[x - bpp] : 0u;
        out[1u + x] = (uint8_t)filtered(type, X, a, b, c);
    }
}

template <bool SEG>
__global__ __launch_bounds__(BT) void k_png_block(const uint8_t* __restrict__ R, uint32_t n, uint32_t nblocks, PngSegments seg, PngMeta* __restrict__ meta,
                                                  uint8_t* __restrict__ slots) {
    __shared__ uint32_t sw[LDS_WORDS];
    __shared__ uint32_t hist[NSYM];
    __shared__ HuffmanLds<NSYM> hl;
    __shared__ uint32_t first_start[BT], last_start[BT], sums[BT];
    __shared__ uint32_t hdr[40];
    __shared__ uint32_t sh_a, sh_b, sh_bits, sh_matches;

    const uint32_t t = threadIdx.x, blk = blockIdx.x;
    const PngBlockSpan span = block_span<SEG>(blk, n, nblocks, seg);
    const uint32_t base = span.base, len = span.len;
    const bool final_block = span.final_block;
    uint32_t* slot = (uint32_t*)(slots + (size_t)blk * PNG_SLOT);

    // the block's bytes, a word at a time (R is 16-byte aligned and padded to 16: the word holding the last byte can be read whole)
    const uint32_t* Rw = (const uint32_t*)(R + base);
    for (uint32_t k = t; k < (len + 3u) >> 2; k += BT) sw[k + (k >> 5)] = Rw[k];
    for (uint32_t s = t; s < NSYM; s += BT) hist[s] = 0u;
    if (t < 40u) hdr[t] = 0u;
    if (t == 0u) sh_a = sh_b = sh_bits = sh_matches = 0u;
    __syncthreads();

    // run starts of the own span, Adler-32 partial sums
    const uint32_t lo = min(t * SPAN, len), hi = min(lo + SPAN, len);
    {
        uint32_t first = NO_START, last = NO_START, a = 0, b = 0, prev = lo ? byte_at(sw, lo - 1u) : 256u;
        for (uint32_t i = lo; i < hi; i++) {
            const uint32_t v = byte_at(sw, i);
            if (v != prev) {
                if (first == NO_START) first = i;
                last = i;
            }
            prev = v;
            a += v;
            b += (len - i) * v; // <= 128 * 32768 * 255 < 2^32
        }
        first_start[t] = first;
        last_start[t] = last;
        atomicAdd(&sh_a, a % ADLER);
        atomicAdd(&sh_b, b % ADLER);
    }
    __syncthreads();
    uint32_t run_start = lo, next_start = len;
    if (lo < hi) {
        if (first_start[t] != lo) // byte lo continues a run: byte 0 starts one, so an earlier thread has a start
            for (uint32_t u = t; u-- > 0u;)
                if (last_start[u] != NO_START) {
                    run_start = last_start[u];
                    break;
                }
        for (uint32_t u = t + 1u; u < BT; u++)
            if (first_start[u] != NO_START) {
                next_start = first_start[u];
                break;
            }
    }

    // histogram over the 286 literal/length symbols; end-of-block counts 1
    walk_tokens(sw, lo, hi, run_start, next_start, [&](uint32_t sym, uint32_t, uint32_t) { atomicAdd(&hist[sym], 1u); });
    if (t == 0u) atomicAdd(&hist[END_OF_BLOCK], 1u);
    huffman_code(hist, hl);
    const uint32_t* tab = hl.tab;
    for (uint32_t s = t; s < NSYM; s += BT) {
        const uint32_t l = hl.clen[s];
        if (l) {
            atomicAdd(&sh_bits, hist[s] * (l + symbol_extra_bits(s) + (s > END_OF_BLOCK ? 1u : 0u)));
            if (s > END_OF_BLOCK) atomicAdd(&sh_matches, hist[s]);
        }
        or_bits(hdr, CODES_AT + 4u * s, __brev(l) >> 28); // the code-length code: symbol l has the 4-bit code l
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
            or_bits(hdr, 0u, (final_block ? 1u : 0u) | (2u << 1) | (29u << 3) | (0u << 8) | (15u << 13)); // BFINAL BTYPE HLIT HDIST HCLEN
            for (uint32_t j = 0; j < 16u; j++) or_bits(hdr, 26u + 3u * j, 4u); // lengths of the code-length code: 0 for 16, 17, 18, then 4
            if (sh_matches) or_bits(hdr, DIST_AT, 8u);                         // the one distance code: length 1
        }
        // where the own tokens go
        uint32_t mine = 0;
        walk_tokens(sw, lo, hi, run_start, next_start,
                    [&](uint32_t sym, uint32_t xb, uint32_t) { mine += (tab[sym] >> 16) + xb + (sym > END_OF_BLOCK ? 1u : 0u); });
        if (t == BT - 1u) mine += tab[END_OF_BLOCK] >> 16;
        uint32_t total;
        const uint32_t at = HEADER_BITS + block_exclusive_sum(sums, mine, &total); // its barriers also publish hdr
        if (t < 38u) slot[t] = hdr[t];
        else if (t == 38u) atomicOr(&slot[38], hdr[38]);
        BitWriter bw(slot, at);
        walk_tokens(sw, lo, hi, run_start, next_start, [&](uint32_t sym, uint32_t xb, uint32_t xv) {
            const uint32_t e = tab[sym], l = e >> 16;
            bw.put((e & 0xFFFFu) | (xv << l), l + xb + (sym > END_OF_BLOCK ? 1u : 0u)); // a match ends in the distance code 0
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

// offsets[b]: where block b starts in the zlib stream, offsets[nblocks]: where the Adler-32 does; totals: (stream bytes, Adler-32)
__global__ __launch_bounds__(BT) void k_png_layout(const PngMeta* __restrict__ meta, uint32_t nblocks, uint32_t n, uint32_t* __restrict__ offsets,
                                                   uint32_t* __restrict__ totals, uint32_t* __restrict__ out_header) {
    __shared__ uint32_t sums[BT];
    __shared__ uint32_t sh_a, sh_b, sh_stored;
    const uint32_t t = threadIdx.x, chunk = (nblocks + BT - 1u) / BT, b0 = min(t * chunk, nblocks), b1 = min(b0 + chunk, nblocks);
    if (t == 0u) sh_a = sh_b = sh_stored = 0u;
    uint32_t bytes = 0, a = 0, b = 0, st = 0;
    for (uint32_t k = b0; k < b1; k++) {
        const PngMeta m = meta[k];
        const uint32_t behind = n - min((k + 1u) * PNG_BLOCK, n); // bytes of R behind block k
        bytes += m.bytes;
        a = (a + m.a) % ADLER;
        b = (uint32_t)((b + m.b + (uint64_t)(behind % ADLER) * m.a) % ADLER);
        st += m.stored;
    }
    uint32_t total;
    uint32_t at = 2u + block_exclusive_sum(sums, bytes, &total); // its first barrier publishes the zeroed sums
    atomicAdd(&sh_a, a);
    atomicAdd(&sh_b, b);
    atomicAdd(&sh_stored, st);
    for (uint32_t k = b0; k < b1; k++) {
        offsets[k] = at;
        at += meta[k].bytes;
    }
    __syncthreads();
    if (t == 0u) {
        const uint32_t stream = 2u + total + 4u;
        offsets[nblocks] = stream - 4u;
        totals[0] = stream;
        totals[1] = (((n % ADLER + sh_b % ADLER) % ADLER) << 16) | ((1u + sh_a % ADLER) % ADLER);
        out_header[0] = stream, out_header[1] = n, out_header[2] = nblocks, out_header[3] = sh_stored;
    }
}

__global__ __launch_bounds__(256) void k_png_compact(const uint8_t* __restrict__ slots, const uint32_t* __restrict__ offsets,
                                                     const uint32_t* __restrict__ totals, uint32_t nblocks, uint32_t max_words,
                                                     uint32_t* __restrict__ out) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x, stream = totals[0], p0 = 4u * k;
    if (k >= max_words || p0 >= stream) return;
    const uint32_t adler = totals[1], adler_at = stream - 4u;
    uint32_t word = 0, b = NO_START;
    for (uint32_t j = 0; j < 4u; j++) {
        const uint32_t p = p0 + j;
        uint32_t v;
        if (p >= stream) v = 0u; // the word holding the last byte is zero-padded
        else if (p < 2u) v = p ? 0x01u : 0x78u;
        else if (p >= adler_at) v = (adler >> (8u * (3u - (p - adler_at)))) & 255u;
        else {
            if (b == NO_START) { // the block holding p: the last b with offsets[b] <= p
                uint32_t lo = 0, hi = nblocks;
                while (hi - lo > 1u) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (offsets[mid] <= p) lo = mid;
                    else hi = mid;
                }
                b = lo;
            }
            while (p >= offsets[b + 1u]) b++;
            v = slots[(size_t)b * PNG_SLOT + (p - offsets[b])];
        }
        word |= v << (8u * j);
    }
    out[PNG_HEADER_BYTES / 4u + k] = word;
}

inline size_t align16(size_t x) { return (x + 15u) & ~(size_t)15u; }

} // namespace

PngGeometry png_geometry(uint32_t w, uint32_t h, uint32_t bpp) {
    PngGeometry g = {};
    if (!w || !h) return g.why = "zero-sized image", g;
    if (bpp != 1u && bpp != 3u && bpp != 4u) return g.why = "bpp must be 1, 3 or 4", g;
    const uint64_t stride = 1u + (uint64_t)w * bpp;
    if (stride > ((uint64_t)1 << 24)) return g.why = "row longer than 2^24 bytes unsupported (32-bit filter costs)", g;
    const uint64_t n = stride * h;
    if (n >= ((uint64_t)1 << 31)) return g.why = "image larger than 2^31 filtered bytes unsupported (32-bit offsets)", g;
    g = stream_geometry(n);
    g.stride = (uint32_t)stride;
    return g;
}

PngGeometry stream_geometry(uint64_t n) {
    PngGeometry g = {};
    if (!n) return g.why = "empty buffer", g;
    if (n >= ((uint64_t)1 << 31)) return g.why = "buffer of 2^31 bytes or more unsupported (32-bit offsets)", g;
    g.ok = true;
    g.n = (uint32_t)n;
    g.blocks = (uint32_t)((n + PNG_BLOCK - 1u) / PNG_BLOCK);
    g.off_meta = align16(n);
    g.off_offsets = g.off_meta + sizeof(PngMeta) * g.blocks;
    g.off_totals = g.off_offsets + align16(4u * ((size_t)g.blocks + 1u));
    g.off_slots = g.off_totals + 16u;
    g.scratch_bytes = g.off_slots + (size_t)g.blocks * PNG_SLOT;
    g.bound = align16(PNG_HEADER_BYTES + 2u + n + 10u * (size_t)g.blocks + 4u);
    return g;
}

const char* png_check_args(uint32_t w, uint32_t h, uint32_t bpp, const uint8_t* d_img, const void* d_out, size_t out_bytes, const void* d_scratch,
                           size_t scratch_bytes) {
    const PngGeometry g = png_geometry(w, h, bpp);
    if (!g.ok) return g.why;
    if (!d_img || !d_out || !d_scratch) return "null buffer";
    if (((uintptr_t)d_out & 15u) || ((uintptr_t)d_scratch & 15u)) return "misaligned buffer (d_out and d_scratch: 16 bytes)";
    if (out_bytes < g.bound) return "d_out smaller than rayn_png_stream_bound";
    if (scratch_bytes < g.scratch_bytes) return "d_scratch smaller than rayn_png_scratch_bytes";
    const size_t img_bytes = (size_t)w * h * bpp;
    if (d_out == (const void*)d_img || overlap(d_out, out_bytes, d_img, img_bytes)) return "d_out must not overlap d_img";
    if (overlap(d_scratch, scratch_bytes, d_img, img_bytes) || overlap(d_scratch, scratch_bytes, d_out, out_bytes)) return "d_scratch overlaps d_img or d_out";
    return nullptr;
}

void launch_png_filter(hipStream_t s, uint32_t w, uint32_t h, uint32_t bpp, const uint8_t* d_img, uint8_t* R) {
    k_png_filter<<<h, 256, 0, s>>>(d_img, w * bpp, bpp, R);
}

void launch_png_finish(hipStream_t s, const PngGeometry& g, void* d_out, void* d_scratch) {
    uint8_t* sc = (uint8_t*)d_scratch;
    const PngMeta* meta = (const PngMeta*)(sc + g.off_meta);
    uint32_t* offsets = (uint32_t*)(sc + g.off_offsets);
    uint32_t* totals = (uint32_t*)(sc + g.off_totals);
    k_png_layout<<<1, BT, 0, s>>>(meta, g.blocks, g.n, offsets, totals, (uint32_t*)d_out);
    const uint32_t max_words = (uint32_t)((g.bound - PNG_HEADER_BYTES) / 4u);
    k_png_compact<<<(max_words + 255u) / 256u, 256, 0, s>>>(sc + g.off_slots, offsets, totals, g.blocks, max_words, (uint32_t*)d_out);
}

void launch_png_block_segmented(hipStream_t s, const uint8_t* R, uint32_t n, uint32_t nblocks, PngSegments seg, PngMeta* meta, uint8_t* slots) {
    k_png_block<true><<<nblocks, BT, 0, s>>>(R, n, nblocks, seg, meta, slots);
}

hipError_t launch_png_encode(hipStream_t s, uint32_t w, uint32_t h, uint32_t bpp, const uint8_t* d_img, void* d_out, void* d_scratch) {
    const PngGeometry g = png_geometry(w, h, bpp);
    uint8_t* sc = (uint8_t*)d_scratch;
    if (hipError_t e = hipMemsetAsync(sc + g.off_slots, 0, (size_t)g.blocks * PNG_SLOT, s)) return e; // the emit ors into zeroed words
    launch_png_filter(s, w, h, bpp, d_img, sc);
    k_png_block<false><<<g.blocks, BT, 0, s>>>(sc, g.n, g.blocks, PngSegments{}, (PngMeta*)(sc + g.off_meta), sc + g.off_slots);
    launch_png_finish(s, g, d_out, d_scratch);
    return hipSuccess;
}

} // namespace rayn

size_t rayn_png_stream_bound(uint32_t w, uint32_t h, uint32_t bpp) {
    const rayn::PngGeometry g = rayn::png_geometry(w, h, bpp);
    return g.ok ? g.bound : 0;
}

size_t rayn_png_scratch_bytes(uint32_t w, uint32_t h, uint32_t bpp) {
    const rayn::PngGeometry g = rayn::png_geometry(w, h, bpp);
    return g.ok ? g.scratch_bytes : 0;
}
