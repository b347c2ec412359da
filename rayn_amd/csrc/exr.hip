// exr.hip — the ZIP-compressed scanline chunks of an OpenEXR file, encoded on the device (rayn_hip_exr_encode_device; the definition is in
// include/rayn_hip.h, restated in tests/exr_np.py).  One memset and four launches, whatever the height:
//   k_exr_pack     a workgroup per 4096 16-bit units of a chunk: the planes' words, converted, rows flipped, into LDS; from there the
//                  chunk's RAW bytes and its pre-processed bytes P - the units' low bytes, then their high bytes, each minus its predecessor
//   k_png_block /  the block kernels of png.hip / png_lz.hip in their segmented instantiation: every chunk's P is a stream of its own
//   k_png_lz_block
//   k_exr_layout   one workgroup: per chunk the stream's size, its Adler-32 and the raw-or-compressed decision; the exclusive sum of the
//                  chunks; the header words and the chunk table
//   k_exr_compact  a thread per word of the body: y, size and the payload, from the blocks' slots or from RAW
// Integer arithmetic only; policy-free, built once.  Every store is a vector store.
#include "exr.h"

#include "png_device.h"
#include "post_checks.h"

namespace rayn {

namespace {

constexpr uint32_t BT = PNG_BT, ADLER = PNG_ADLER;
constexpr uint32_t PACK_T = 256u, PACK_PER = 16u, TILE = PACK_T * PACK_PER; // 16-bit units of RAW per workgroup of k_exr_pack
static_assert(TILE % 4u == 0u, "a tile starts on a word of RAW and of P's low half");

struct ExrChannel {
    const uint32_t* plane;
    uint32_t stride, offset, type;
    uint32_t first; // the channel's first unit in a row: width * (the sizes in front of it) / 2
};
struct ExrPack { // k_exr_pack's argument: the channel table travels with the launch
    ExrChannel ch[EXR_MAX_CHANNELS];
    uint32_t n_channels, w, h, row_units, tiles, chunk_bytes; // tiles: per chunk; chunk_bytes: of a full chunk
};

// f32 bits -> binary16 bits, include/rayn_hip.h "f32 to half": in integers, so that the build's denormal mode has no say
__device__ inline uint32_t half_bits(uint32_t x) {
    const uint32_t sign = (x >> 16) & 0x8000u, a = x & 0x7FFFFFFFu;
    if (a > 0x7F800000u) { // NaN: the payload's top ten bits, never the infinity
        const uint32_t m = (a & 0x7FFFFFu) >> 13;
        return sign | 0x7C00u | m | (m == 0u ? 1u : 0u);
    }
    if (a >= 0x477FF000u) return sign | 0x7C00u; // >= 65520, the infinity included
    if (a >= 0x38800000u) {                      // a normal half: >= 2^-14
        const uint32_t r = a - 0x38000000u;
        return sign | ((r + 0xFFFu + ((r >> 13) & 1u)) >> 13);
    }
    if (a <= 0x33000000u) return sign; // <= 2^-25: the tie goes to the even 0
    const uint32_t shift = 126u - (a >> 23), m = (a & 0x7FFFFFu) | 0x800000u; // 14..24: m * 2^-shift half denormal units
    const uint32_t q = m >> shift, rem = m & ((1u << shift) - 1u), tie = 1u << (shift - 1u);
    return sign | (q + ((rem > tie || (rem == tie && (q & 1u))) ? 1u : 0u));
}

// The 16-bit unit u of chunk `chunk`'s RAW bytes: a HALF value, or one half of a 32-bit one
__device__ inline uint32_t raw_unit(const ExrPack& a, uint32_t chunk, uint32_t u) {
    const uint32_t r = u / a.row_units, q = u - r * a.row_units;
    const uint32_t* plane = a.ch[0].plane;
    uint32_t stride = a.ch[0].stride, offset = a.ch[0].offset, type = a.ch[0].type, first = 0u;
    for (uint32_t k = 1; k < a.n_channels; k++) // k is uniform: the table is read through scalar loads
        if (q >= a.ch[k].first) plane = a.ch[k].plane, stride = a.ch[k].stride, offset = a.ch[k].offset, type = a.ch[k].type, first = a.ch[k].first;
    const uint32_t v = q - first, x = type == 1u ? v : v >> 1;
    const uint32_t film_row = a.h - 1u - (chunk * EXR_ROWS + r); // the file's rows run top-down
    const uint32_t word = plane[((size_t)film_row * a.w + x) * stride + offset];
    return type == 1u ? half_bits(word) : ((v & 1u) ? word >> 16 : word & 0xFFFFu);
}

// The bytes [lo, hi) of base (4-byte aligned), byte lo + i being g(i): whole words where the range holds them, bytes at its two ends
template <class G>
__device__ inline void store_range(uint8_t* base, uint32_t lo, uint32_t hi, G&& g) {
    for (uint32_t wi = (lo >> 2) + threadIdx.x; wi < (hi + 3u) >> 2; wi += PACK_T) {
        const uint32_t p = 4u * wi;
        if (p >= lo && p + 4u <= hi) {
            ((uint32_t*)base)[wi] = g(p - lo) | (g(p + 1u - lo) << 8) | (g(p + 2u - lo) << 16) | (g(p + 3u - lo) << 24);
        } else {
            for (uint32_t j = 0; j < 4u; j++)
                if (p + j >= lo && p + j < hi) base[p + j] = (uint8_t)g(p + j - lo);
        }
    }
}

__global__ __launch_bounds__(PACK_T) void k_exr_pack(const ExrPack a, uint8_t* __restrict__ P, uint32_t* __restrict__ RAW) {
    __shared__ uint32_t un[TILE + 1u]; // un[0]: the unit in front of the tile; un[1 + i]: the tile's unit i
    __shared__ uint32_t sh_last;       // the chunk's last unit, whose low byte precedes the first high byte
    const uint32_t t = threadIdx.x, chunk = blockIdx.x / a.tiles, tile0 = blockIdx.x % a.tiles * TILE;
    const uint32_t units = min(EXR_ROWS, a.h - chunk * EXR_ROWS) * a.row_units; // n_k / 2
    if (tile0 >= units) return; // the last chunk may be shorter
    const uint32_t cnt = min(TILE, units - tile0);
    for (uint32_t k = t; k < cnt; k += PACK_T) un[1u + k] = raw_unit(a, chunk, tile0 + k);
    if (t == 0u) un[0] = tile0 ? raw_unit(a, chunk, tile0 - 1u) : 0u;
    if (t == 64u && tile0 == 0u) sh_last = raw_unit(a, chunk, units - 1u);
    __syncthreads();

    const size_t chunk_at = (size_t)chunk * a.chunk_bytes; // a multiple of 32
    uint32_t* raw = RAW + chunk_at / 4u + tile0 / 2u;
    for (uint32_t k = t; 2u * k < cnt; k += PACK_T) raw[k] = un[1u + 2u * k] | ((2u * k + 1u < cnt ? un[2u + 2u * k] : 0u) << 16);

    uint8_t* Pc = P + chunk_at;
    const uint32_t before_low = tile0 ? un[0] & 255u : 128u;             // P[0] = T[0]
    const uint32_t before_high = tile0 ? un[0] >> 8 : sh_last & 255u;    // T[n / 2 - 1] is the last low byte
    store_range(Pc, tile0, tile0 + cnt, [&](uint32_t i) { return ((un[1u + i] & 255u) - (i ? un[i] & 255u : before_low) + 128u) & 255u; });
    store_range(Pc, units + tile0, units + tile0 + cnt, [&](uint32_t i) { return ((un[1u + i] >> 8) - (i ? un[i] >> 8 : before_high) + 128u) & 255u; });
}

struct ExrLayout {
    uint32_t n, chunks, blocks, body_words_at; // body_words_at: the body's first word in d_out
    PngSegments seg;
};

__device__ inline uint32_t chunk_bytes(const ExrLayout& g, uint32_t c) { return min(g.seg.bytes, g.n - c * g.seg.bytes); }

// block_at[b]: where block b starts in its chunk's zlib stream; starts[c]: where chunk c starts in the body, starts[chunks]: the body's
// bytes; sizes[c]: the payload's bytes, n_c for a raw chunk; adlers[c]
__global__ __launch_bounds__(BT) void k_exr_layout(const PngMeta* __restrict__ meta, const ExrLayout g, uint32_t* __restrict__ block_at,
                                                   uint32_t* __restrict__ starts, uint32_t* __restrict__ sizes, uint32_t* __restrict__ adlers,
                                                   uint32_t* __restrict__ out) {
    __shared__ uint32_t sums[BT];
    __shared__ uint32_t sh_raw;
    const uint32_t t = threadIdx.x, per = (g.chunks + BT - 1u) / BT, c0 = min(t * per, g.chunks), c1 = min(c0 + per, g.chunks);
    if (t == 0u) sh_raw = 0u;
    uint32_t mine = 0, raws = 0;
    for (uint32_t c = c0; c < c1; c++) {
        const uint32_t nc = chunk_bytes(g, c), nb = (nc + PNG_BLOCK - 1u) / PNG_BLOCK;
        uint32_t bytes = 0, a = 0, b = 0;
        for (uint32_t j = 0; j < nb; j++) {
            const uint32_t blk = c * g.seg.blocks + j;
            const PngMeta m = meta[blk];
            const uint32_t behind = nc - min((j + 1u) * PNG_BLOCK, nc); // bytes of the chunk behind block j
            block_at[blk] = 2u + bytes;
            bytes += m.bytes;
            a = (a + m.a) % ADLER;
            b = (uint32_t)((b + m.b + (uint64_t)(behind % ADLER) * m.a) % ADLER);
        }
        const uint32_t stream = 2u + bytes + 4u, raw = stream >= nc ? 1u : 0u;
        sizes[c] = raw ? nc : stream;
        adlers[c] = (((nc % ADLER + b) % ADLER) << 16) | ((1u + a) % ADLER);
        mine += 8u + (raw ? nc : stream);
        raws += raw;
    }
    uint32_t total;
    uint32_t at = block_exclusive_sum(sums, mine, &total); // its first barrier publishes the zeroed sh_raw
    atomicAdd(&sh_raw, raws);
    for (uint32_t c = c0; c < c1; c++) {
        starts[c] = at;
        out[EXR_HEADER_BYTES / 4u + c] = at;
        at += 8u + sizes[c];
    }
    for (uint32_t k = EXR_HEADER_BYTES / 4u + g.chunks + t; k < g.body_words_at; k += BT) out[k] = 0u;
    __syncthreads();
    if (t == 0u) {
        starts[g.chunks] = total;
        out[0] = total, out[1] = g.chunks, out[2] = sh_raw, out[3] = g.blocks;
    }
}

__global__ __launch_bounds__(256) void k_exr_compact(const uint8_t* __restrict__ slots, const uint8_t* __restrict__ RAW,
                                                     const uint32_t* __restrict__ block_at, const uint32_t* __restrict__ starts,
                                                     const uint32_t* __restrict__ sizes, const uint32_t* __restrict__ adlers, const ExrLayout g,
                                                     uint32_t max_words, uint32_t* __restrict__ out) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x, body = starts[g.chunks], p0 = 4u * k;
    if (k >= max_words || p0 >= body) return;
    uint32_t c; // the chunk holding p0: the last c with starts[c] <= p0
    {
        uint32_t lo = 0, hi = g.chunks;
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (starts[mid] <= p0) lo = mid;
            else hi = mid;
        }
        c = lo;
    }
    uint32_t word = 0, b = PNG_NO_START;
    for (uint32_t j = 0; j < 4u; j++) {
        const uint32_t p = p0 + j;
        if (p >= body) break; // the word holding the last byte is zero-padded
        while (p >= starts[c + 1u]) c++, b = PNG_NO_START;
        const uint32_t q = p - starts[c], size = sizes[c];
        uint32_t v;
        if (q < 4u) v = (c * EXR_ROWS) >> (8u * q);
        else if (q < 8u) v = size >> (8u * (q - 4u));
        else {
            const uint32_t r = q - 8u, nc = chunk_bytes(g, c);
            if (size == nc) v = RAW[(size_t)c * g.seg.bytes + r];
            else if (r < 2u) v = r ? 0x01u : 0x78u;
            else if (r >= size - 4u) v = adlers[c] >> (8u * (3u - (r - (size - 4u))));
            else {
                const uint32_t* at = block_at + (size_t)c * g.seg.blocks;
                const uint32_t nb = (nc + PNG_BLOCK - 1u) / PNG_BLOCK;
                if (b == PNG_NO_START) { // the block holding r: the last b with at[b] <= r
                    uint32_t lo = 0, hi = nb;
                    while (hi - lo > 1u) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if (at[mid] <= r) lo = mid;
                        else hi = mid;
                    }
                    b = lo;
                }
                while (b + 1u < nb && r >= at[b + 1u]) b++;
                v = slots[((size_t)c * g.seg.blocks + b) * PNG_SLOT + (r - at[b])];
            }
        }
        word |= (v & 255u) << (8u * j);
    }
    out[g.body_words_at + k] = word;
}

inline size_t align16(size_t x) { return (x + 15u) & ~(size_t)15u; }
inline uint32_t channel_size(uint32_t type) { return type == 1u ? 2u : 4u; }

ExrLayout layout_of(const ExrGeometry& g) { return ExrLayout{g.n, g.chunks, g.blocks, (uint32_t)(g.body_at / 4u), g.seg}; }

} // namespace

ExrGeometry exr_geometry(uint32_t w, uint32_t h, uint32_t n_channels, const uint32_t* layout, uint32_t matches) {
    ExrGeometry g = {};
    if (!w || !h) return g.why = "zero-sized image", g;
    if (!n_channels || n_channels > EXR_MAX_CHANNELS) return g.why = "n_channels must be 1..16", g;
    if (!layout) return g.why = "null layout", g;
    uint64_t pixel_bytes = 0;
    for (uint32_t c = 0; c < n_channels; c++) {
        const uint32_t stride = layout[3u * c], offset = layout[3u * c + 1u], type = layout[3u * c + 2u];
        if (type > 2u) return g.why = "channel type must be 0 (UINT), 1 (HALF) or 2 (FLOAT)", g;
        if (!stride || offset >= stride) return g.why = "channel stride must not be 0 and its offset must be below it", g;
        pixel_bytes += channel_size(type);
    }
    if (matches > 1u) return g.why = "matches must be 0 or 1", g;
    const uint64_t S = (uint64_t)w * pixel_bytes, limit = (uint64_t)1 << 31;
    if (EXR_ROWS * S >= limit) return g.why = "16 rows of 2^31 bytes or more unsupported (32-bit offsets)", g;
    const uint64_t n = S * h, chunks = ((uint64_t)h + EXR_ROWS - 1u) / EXR_ROWS;
    const uint64_t body_at = (EXR_HEADER_BYTES + 4u * chunks + 15u) & ~(uint64_t)15u, bound = body_at + ((n + 8u * chunks + 15u) & ~(uint64_t)15u);
    if (bound >= limit) return g.why = "output of 2^31 bytes or more unsupported (32-bit offsets): write fewer channels or HALF", g;
    g.ok = true;
    g.row_bytes = (uint32_t)S;
    g.n = (uint32_t)n;
    g.chunks = (uint32_t)chunks;
    g.seg.bytes = EXR_ROWS * g.row_bytes;
    g.seg.blocks = (g.seg.bytes + PNG_BLOCK - 1u) / PNG_BLOCK;
    const uint32_t last = g.n - (g.chunks - 1u) * g.seg.bytes;
    g.blocks = (g.chunks - 1u) * g.seg.blocks + (last + PNG_BLOCK - 1u) / PNG_BLOCK;
    g.body_at = (size_t)body_at;
    g.bound = (size_t)bound;
    g.off_raw = align16(g.n);
    g.off_meta = g.off_raw + align16(g.n);
    g.off_block_at = g.off_meta + sizeof(PngMeta) * g.blocks;
    g.off_starts = g.off_block_at + align16(4u * (size_t)g.blocks);
    g.off_sizes = g.off_starts + align16(4u * ((size_t)g.chunks + 1u));
    g.off_adler = g.off_sizes + align16(4u * (size_t)g.chunks);
    g.off_slots = g.off_adler + align16(4u * (size_t)g.chunks);
    g.scratch_bytes = g.off_slots + (size_t)g.blocks * PNG_SLOT + (matches ? (size_t)g.blocks * PNG_LZ_POSITIONS : 0u);
    return g;
}

const char* exr_check_args(uint32_t w, uint32_t h, uint32_t n_channels, const void* const* d_planes, const uint32_t* layout, uint32_t matches,
                           const void* d_out, size_t out_bytes, const void* d_scratch, size_t scratch_bytes) {
    const ExrGeometry g = exr_geometry(w, h, n_channels, layout, matches);
    if (!g.ok) return g.why;
    if (!d_planes || !d_out || !d_scratch) return "null buffer";
    for (uint32_t c = 0; c < n_channels; c++) {
        if (!d_planes[c]) return "null buffer (a plane)";
        if ((uintptr_t)d_planes[c] & 3u) return "misaligned plane (4 bytes)";
    }
    if (((uintptr_t)d_out & 15u) || ((uintptr_t)d_scratch & 15u)) return "misaligned buffer (d_out and d_scratch: 16 bytes)";
    if (out_bytes < g.bound) return "d_out smaller than rayn_exr_stream_bound";
    if (scratch_bytes < g.scratch_bytes) return "d_scratch smaller than rayn_exr_scratch_bytes";
    if (overlap(d_scratch, scratch_bytes, d_out, out_bytes)) return "d_scratch overlaps d_out";
    for (uint32_t c = 0; c < n_channels; c++) {
        const size_t bytes = 4u * (((size_t)w * h - 1u) * layout[3u * c] + layout[3u * c + 1u] + 1u);
        if (overlap(d_out, out_bytes, d_planes[c], bytes)) return "d_out must not overlap a plane";
        if (overlap(d_scratch, scratch_bytes, d_planes[c], bytes)) return "d_scratch overlaps a plane";
    }
    return nullptr;
}

hipError_t launch_exr_encode(hipStream_t s, uint32_t w, uint32_t h, uint32_t n_channels, const void* const* d_planes, const uint32_t* layout,
                             uint32_t matches, void* d_out, void* d_scratch) {
    const ExrGeometry g = exr_geometry(w, h, n_channels, layout, matches);
    uint8_t* sc = (uint8_t*)d_scratch;
    if (hipError_t e = hipMemsetAsync(sc + g.off_slots, 0, (size_t)g.blocks * PNG_SLOT, s)) return e; // the emit ors into zeroed words
    ExrPack a = {};
    uint32_t units = 0; // of a pixel, in front of the channel
    for (uint32_t c = 0; c < n_channels; c++) {
        a.ch[c] = ExrChannel{(const uint32_t*)d_planes[c], layout[3u * c], layout[3u * c + 1u], layout[3u * c + 2u], w * units};
        units += channel_size(layout[3u * c + 2u]) / 2u;
    }
    a.n_channels = n_channels, a.w = w, a.h = h, a.row_units = g.row_bytes / 2u, a.chunk_bytes = g.seg.bytes;
    a.tiles = (g.seg.bytes / 2u + TILE - 1u) / TILE;
    k_exr_pack<<<g.chunks * a.tiles, PACK_T, 0, s>>>(a, sc, (uint32_t*)(sc + g.off_raw));
    PngMeta* meta = (PngMeta*)(sc + g.off_meta);
    if (matches)
        launch_png_lz_block_segmented(s, sc, g.n, g.blocks, g.seg, g.row_bytes / 2u, meta, sc + g.off_slots, (uint16_t*)(sc + g.off_slots + (size_t)g.blocks * PNG_SLOT));
    else
        launch_png_block_segmented(s, sc, g.n, g.blocks, g.seg, meta, sc + g.off_slots);
    uint32_t* block_at = (uint32_t*)(sc + g.off_block_at);
    uint32_t* starts = (uint32_t*)(sc + g.off_starts);
    uint32_t* sizes = (uint32_t*)(sc + g.off_sizes);
    uint32_t* adlers = (uint32_t*)(sc + g.off_adler);
    const ExrLayout lay = layout_of(g);
    k_exr_layout<<<1, BT, 0, s>>>(meta, lay, block_at, starts, sizes, adlers, (uint32_t*)d_out);
    const uint32_t max_words = (uint32_t)((g.bound - g.body_at) / 4u);
    k_exr_compact<<<(max_words + 255u) / 256u, 256, 0, s>>>(sc + g.off_slots, sc + g.off_raw, block_at, starts, sizes, adlers, lay, max_words,
                                                            (uint32_t*)d_out);
    return hipSuccess;
}

} // namespace rayn

size_t rayn_exr_stream_bound(uint32_t w, uint32_t h, uint32_t n_channels, const uint32_t* layout) {
    const rayn::ExrGeometry g = rayn::exr_geometry(w, h, n_channels, layout, 0u);
    return g.ok ? g.bound : 0;
}

size_t rayn_exr_scratch_bytes(uint32_t w, uint32_t h, uint32_t n_channels, const uint32_t* layout, uint32_t matches) {
    const rayn::ExrGeometry g = rayn::exr_geometry(w, h, n_channels, layout, matches);
    return g.ok ? g.scratch_bytes : 0;
}
