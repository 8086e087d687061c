// png_indexed.hip — the kernels of the indexed-colour form of the device PNG encoder (product code; include/maray_hip.h,
// "Indexed colour").
//
//   maray_png_colors        a capped grid strides over the raster, four pixels a lane: three aligned dwords of its own and the
//                           next lane's first one by __shfl_down (the wavefront's last lane loads it), shifted into place by
//                           v_alignbyte_b32, so that every byte is read once at any source alignment.  A pixel that differs
//                           from the one before it goes, as R << 16 | G << 8 | B | 1 << 24, into an open-addressed set in LDS
//                           (a plain read first, then ds_cmpst on an empty slot); the tag keeps black from looking like an
//                           empty slot.  A block whose set holds more than 256 colours stops.  Every block STORES its count and
//                           its colours to a slab of its own, and
//   maray_png_colors_merge  one block of 16 wavefronts forms the union of the slabs -- and of the palette of the bands before, one
//                           more list -- in the same set (the lists' counts first, then their entries, four loads a lane in flight), saturates the count at 257, ranks every colour by counting the smaller ones (the
//                           ascending order) and stores count and palette (maray_frame_delta's two launches: no device-wide
//                           counter).
//   maray_png_index         the palette into a lookup table in LDS once per block (a set like the above, the colour's index
//                           beside its key); a lane per packed byte: its 8 / depth pixels looked up, packed from the high bits
//                           down, pad bits zero, one byte stored.
//   maray_png_compress_idx  maray_png_compress's frame on packed bytes: a wavefront per segment of 768 bytes, four per block, a
//                           lane per byte of a 64-byte step; __shfl_up and __ballot give the mask of bytes equal to the byte
//                           before them; the lane that starts a run of L emits one match of distance 1 (L >= 3) or L literals;
//                           the six-step scan of the bit lengths, the whole slot staged in LDS by ds_or_b32, the Adler shares.
// No device-wide counter, no inline assembly, no scratch memory.  LDS: 8,200 bytes per block of maray_png_colors, 11,284 of
// maray_png_colors_merge, 8,196 of maray_png_index, 4 x 896 of maray_png_compress_idx.
#include <hip/hip_runtime.h>

#include <string>

#include "png_indexed.hpp"

namespace maray {

namespace {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            throw Error{MARAY_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)};           \
    } while (0)

constexpr uint32_t TAG = 1u << 24;
constexpr uint32_t MORE = PNG_PALETTE_MAX + 1u;
constexpr int MERGE_BLOCK = 1024, MERGE_BATCH = 4;
static_assert(PNG_COLORS_SET >= PNG_PALETTE_MAX + MERGE_BLOCK, "the set never fills up");
constexpr int PC_WAVES = 4, PC_BLOCK = 64 * PC_WAVES;
constexpr int STAGE_DW = PNG_SLOT_MAX / 4;

// where a key starts its probes: the high bits of a multiplicative hash, so that colours that differ in any one byte, or only
// in their high bits, spread over the slots
template <uint32_t SLOTS>
__device__ __forceinline__ uint32_t slot_of(uint32_t key)
{
    static_assert((SLOTS & (SLOTS - 1u)) == 0u, "a power of two");
    return (key * 0x9E3779B1u) >> (32 - __builtin_ctz(SLOTS));
}

// key (tagged: never 0) into the set; *count counts the keys in it.  Returns the key's slot, or SLOTS for a set that is full
// (never: png_indexed.hpp's static_assert).
template <uint32_t SLOTS>
__device__ __forceinline__ uint32_t set_insert(uint32_t *set, uint32_t *count, uint32_t key)
{
    uint32_t h = slot_of<SLOTS>(key);
    for (uint32_t i = 0u; i < SLOTS; i++, h = (h + 1u) & (SLOTS - 1u)) {
        uint32_t old = set[h];
        if (old == 0u) {
            old = atomicCAS(&set[h], 0u, key);
            if (old == 0u) { atomicAdd(count, 1u); return h; }
        }
        if (old == key) return h;
    }
    return SLOTS;
}

// the packed pixel R | G << 8 | B << 16 as the palette's key: R << 16 | G << 8 | B, tagged
__device__ __forceinline__ uint32_t key_of(uint32_t pix) { return (__builtin_bswap32(pix) >> 8) | TAG; }

// the pixel at p (any alignment) from the aligned dwords that hold its three bytes (png_device.hip's load_pixel)
__device__ __forceinline__ uint32_t load_pixel(const unsigned char *p)
{
    const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t *q = (const uint32_t *)(p - mis);
    const uint32_t d0 = q[0], d1 = mis >= 2u ? q[1] : 0u;
    return __builtin_amdgcn_alignbyte(d1, d0, mis) & 0xFFFFFFu;
}

// the set's keys to out[1 ..] in any order, at most PNG_PALETTE_MAX of them; *fill counts them
__device__ __forceinline__ void set_compact(const uint32_t *set, uint32_t *fill, uint32_t *out, uint32_t block)
{
    for (uint32_t i = threadIdx.x; i < PNG_COLORS_SET; i += block) {
        const uint32_t key = set[i];
        if (key) {
            const uint32_t at = atomicAdd(fill, 1u);
            if (at < PNG_PALETTE_MAX) out[1u + at] = key;
        }
    }
}

}   // namespace

__global__ __launch_bounds__(PNG_COLORS_BLOCK) void maray_png_colors(const unsigned char *src, uint64_t npix, uint32_t *slabs)
{
    __shared__ uint32_t set[PNG_COLORS_SET];
    __shared__ uint32_t count, fill;
    for (uint32_t i = threadIdx.x; i < PNG_COLORS_SET; i += PNG_COLORS_BLOCK) set[i] = 0u;
    if (threadIdx.x == 0u) { count = 0u; fill = 0u; }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t mis = (uint32_t)((uintptr_t)src & 3u);
    const uint32_t *base = (const uint32_t *)(src - mis);                 // dword j holds the bytes 4 j - mis .. 4 j - mis + 3 of the raster
    const uint64_t n_dw = (3u * npix + mis + 3u) / 4u;                    // the dwords that hold a byte of the raster
    const uint64_t n_groups = (npix + 3u) / 4u;                           // groups of four pixels: twelve bytes, three dwords
    // (block-uniform trip counts: the shuffles below see whole wavefronts; no barrier inside)
    for (uint64_t g0 = (uint64_t)blockIdx.x * PNG_COLORS_BLOCK; g0 < n_groups; g0 += (uint64_t)gridDim.x * PNG_COLORS_BLOCK) {
        if (__any(*(volatile uint32_t *)&count > PNG_PALETTE_MAX)) break;      // (wave-uniform)
        const uint64_t g = g0 + threadIdx.x, j = 3u * g;
        const uint32_t d0 = j < n_dw ? base[j] : 0u, d1 = j + 1u < n_dw ? base[j + 1u] : 0u, d2 = j + 2u < n_dw ? base[j + 2u] : 0u;
        uint32_t d3 = (uint32_t)__shfl_down((int)d0, 1);
        if (lane == 63u) d3 = mis && j + 3u < n_dw ? base[j + 3u] : 0u;   // (with mis = 0 the group ends with d2)
        const uint32_t e0 = __builtin_amdgcn_alignbyte(d1, d0, mis), e1 = __builtin_amdgcn_alignbyte(d2, d1, mis),
                       e2 = __builtin_amdgcn_alignbyte(d3, d2, mis);
        const uint32_t p[4] = {e0 & 0xFFFFFFu, (e0 >> 24) | ((e1 & 0xFFFFu) << 8), (e1 >> 16) | ((e2 & 0xFFu) << 16), e2 >> 8};
        uint32_t prev = (uint32_t)__shfl_up((int)p[3], 1);
        if (lane == 0u) prev = ~0u;                                       // (no pixel: the wavefront's first one is always looked at)
#pragma unroll
        for (uint32_t k = 0u; k < 4u; k++) {
            if (4u * g + k < npix && p[k] != prev) set_insert<PNG_COLORS_SET>(set, &count, key_of(p[k]));
            prev = p[k];
        }
    }
    __syncthreads();
    uint32_t *out = slabs + (size_t)blockIdx.x * PNG_COLORS_STRIDE;
    set_compact(set, &fill, out, PNG_COLORS_BLOCK);
    if (threadIdx.x == 0u) out[0] = count > PNG_PALETTE_MAX ? MORE : count;
}

// `palette` in: with `add`, the palette so far; out: the union's.  n_slabs <= PNG_COLORS_MAX_BLOCKS.
__global__ __launch_bounds__(MERGE_BLOCK) void maray_png_colors_merge(const uint32_t *slabs, uint32_t n_slabs, uint32_t *palette, uint32_t add)
{
    __shared__ uint32_t set[PNG_COLORS_SET];
    __shared__ uint32_t list[1 + PNG_PALETTE_MAX];
    __shared__ uint32_t counts[PNG_COLORS_MAX_BLOCKS + 1];
    __shared__ uint32_t count, fill, more;
    for (uint32_t i = threadIdx.x; i < PNG_COLORS_SET; i += MERGE_BLOCK) set[i] = 0u;
    if (threadIdx.x == 0u) { count = 0u; fill = 0u; more = 0u; }
    __syncthreads();
    // the lists: the slabs, then the palette so far.  Their counts first, one load each, all in flight together
    const uint32_t n_lists = n_slabs + add;
    for (uint32_t b = threadIdx.x; b < n_lists; b += MERGE_BLOCK) {
        const uint32_t n = b < n_slabs ? slabs[(size_t)b * PNG_COLORS_STRIDE] : palette[0];
        counts[b] = n;
        if (n > PNG_PALETTE_MAX) more = 1u;
    }
    __syncthreads();
    // then entry i of list b for every b and i < 256 that the list holds, MERGE_BATCH loads at a time.  A lane inserts while it
    // sees at most 256 colours in the set: with all lanes of the block behind such a look the set holds at most 256 + 1024.
    const uint32_t total = n_lists * PNG_PALETTE_MAX;
    for (uint32_t e0 = threadIdx.x; e0 < total; e0 += MERGE_BLOCK * MERGE_BATCH) {
        uint32_t key[MERGE_BATCH];
#pragma unroll
        for (uint32_t u = 0u; u < MERGE_BATCH; u++) {
            const uint32_t e = e0 + u * MERGE_BLOCK, b = e / PNG_PALETTE_MAX, i = e % PNG_PALETTE_MAX;
            const bool in = e < total && counts[b] <= PNG_PALETTE_MAX && i < counts[b];
            key[u] = !in ? 0u : b < n_slabs ? slabs[(size_t)b * PNG_COLORS_STRIDE + 1u + i] : palette[1u + i] | TAG;
        }
#pragma unroll
        for (uint32_t u = 0u; u < MERGE_BATCH; u++)
            if (key[u] && *(volatile uint32_t *)&count <= PNG_PALETTE_MAX) set_insert<PNG_COLORS_SET>(set, &count, key[u]);
    }
    __syncthreads();                                        // (every read of the palette so far is behind us)
    set_compact(set, &fill, list, MERGE_BLOCK);
    __syncthreads();
    const uint32_t n = more || count > PNG_PALETTE_MAX ? MORE : count;
    if (threadIdx.x == 0u) palette[0] = n;
    if (n > PNG_PALETTE_MAX) return;
    if (threadIdx.x < n) {
        const uint32_t mine = list[1u + threadIdx.x];
        uint32_t rank = 0u;
        for (uint32_t i = 0u; i < n; i++) rank += list[1u + i] < mine ? 1u : 0u;
        palette[1u + rank] = mine & 0xFFFFFFu;
    } else if (threadIdx.x < PNG_PALETTE_MAX)
        palette[1u + threadIdx.x] = 0u;
}

__global__ __launch_bounds__(PNG_INDEX_BLOCK) void maray_png_index(const unsigned char *src, uint32_t w, uint32_t rows, const uint32_t *palette,
                                                                   uint32_t n, uint32_t depth, unsigned char *dst)
{
    __shared__ uint32_t keys[PNG_INDEX_TABLE], index_of[PNG_INDEX_TABLE];
    __shared__ uint32_t count;
    for (uint32_t i = threadIdx.x; i < PNG_INDEX_TABLE; i += PNG_INDEX_BLOCK) keys[i] = 0u;
    if (threadIdx.x == 0u) count = 0u;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n && i < PNG_PALETTE_MAX; i += PNG_INDEX_BLOCK) {
        const uint32_t h = set_insert<PNG_INDEX_TABLE>(keys, &count, palette[1u + i] | TAG);
        if (h < PNG_INDEX_TABLE) index_of[h] = i;
    }
    __syncthreads();
    const uint32_t rb = (uint32_t)(((uint64_t)w * depth + 7u) / 8u), per = 8u / depth;
    const uint32_t n_bytes = rows * rb;                     // (a band's: below 2^30; the launcher checks)
    for (uint32_t at = blockIdx.x * PNG_INDEX_BLOCK + threadIdx.x; at < n_bytes; at += gridDim.x * PNG_INDEX_BLOCK) {
        const uint32_t row = at / rb, col = at - row * rb;
        const uint32_t x0 = col * per, x1 = min(w, x0 + per);
        const unsigned char *p = src + ((size_t)row * w + x0) * 3;
        uint32_t byte = 0u;
        for (uint32_t x = x0; x < x1; x++, p += 3) {
            const uint32_t key = key_of(load_pixel(p));
            uint32_t h = slot_of<PNG_INDEX_TABLE>(key), found = 0u;
            for (uint32_t i = 0u; i < PNG_INDEX_TABLE; i++, h = (h + 1u) & (PNG_INDEX_TABLE - 1u)) {      // (a colour of the raster is in the table)
                const uint32_t k = keys[h];
                if (k == key) { found = index_of[h]; break; }
                if (k == 0u) break;
            }
            byte |= found << (8u - depth * (x - x0 + 1u));
        }
        dst[at] = (unsigned char)byte;
    }
}

namespace {

// the fixed-Huffman code of literal v, bit-reversed for the LSB-first stream; *nb = its length (png_device.hip's)
__device__ __forceinline__ uint32_t literal(uint32_t v, uint32_t *nb)
{
    const bool lo = v < 144u;
    *nb = lo ? 8u : 9u;
    return lo ? __brev(0x30u + v) >> 24 : __brev(0x190u + (v - 144u)) >> 23;
}

// a match of `len` bytes (3 .. 258) at distance 1: reversed length code, extra bits as they are, distance code 0: five zero bits
__device__ __forceinline__ uint32_t match1(uint32_t len, uint32_t *nb)
{
    const uint32_t l = len - 3u;
    uint32_t code, eb, extra;
    if (len == 258u) { code = 285u; eb = 0u; extra = 0u; }
    else if (l < 8u) { code = 257u + l; eb = 0u; extra = 0u; }
    else {
        eb = 29u - (uint32_t)__clz((int)l);                 // floor(log2 l) - 2: 1 .. 5
        code = 261u + 4u * eb + ((l >> eb) & 3u);
        extra = l & ((1u << eb) - 1u);
    }
    uint32_t hb, hc;
    if (code < 280u) { hb = 7u; hc = __brev(code - 256u) >> 25; }
    else { hb = 8u; hc = __brev(0xC0u + (code - 280u)) >> 24; }
    *nb = hb + eb + 5u;
    return hc | (extra << hb);
}

__device__ __forceinline__ void or_bits(uint32_t *stage, uint32_t bit, uint32_t value)
{
    const uint32_t d = bit >> 5, sh = bit & 31u;
    const uint64_t v = (uint64_t)value << sh;
    if (d < (uint32_t)STAGE_DW) atomicOr(&stage[d], (uint32_t)v);
    if ((uint32_t)(v >> 32) && d + 1u < (uint32_t)STAGE_DW) atomicOr(&stage[d + 1u], (uint32_t)(v >> 32));
}

}   // namespace

__global__ __launch_bounds__(PC_BLOCK) void maray_png_compress_idx(const PngBandArgs a)
{
    __shared__ uint32_t stage_all[PC_WAVES * STAGE_DW];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t *stage = stage_all + wave * STAGE_DW;
    for (uint32_t i = lane; i < (uint32_t)STAGE_DW; i += 64u) stage[i] = 0u;
    __syncthreads();
    const uint32_t seg = blockIdx.x * PC_WAVES + wave;
    const bool active = seg < a.n_segs;                     // (wave-uniform; nobody leaves before the second barrier)
    uint32_t seg_len = 0u;
    if (active) {
        const uint32_t rb = a.row_bytes - 1u;
        const uint32_t row = seg / a.nseg, s = seg - row * a.nseg;
        const uint32_t nby = min(PNG_IDX_SEG, rb - s * PNG_IDX_SEG), first = s == 0u ? 1u : 0u;
        const uint32_t n = nby + first;                     // the segment's filtered bytes
        const unsigned char *src = a.src + (size_t)row * rb + (size_t)s * PNG_IDX_SEG;
        // block header BFINAL = 0, BTYPE = 01 (the bits 0, 1, 0), then in a row's first segment the filter byte 0 as a literal
        uint32_t bitpos = 3u;
        if (lane == 0u) {
            or_bits(stage, 0u, 2u);
            if (first) { uint32_t nb; const uint32_t c = literal(0u, &nb); or_bits(stage, 3u, c); }
        }
        if (first) bitpos += 8u;
        uint32_t sum_a = 0u, sum_b = 0u, last = 0u;
        for (uint32_t p0 = 0u; p0 < nby; p0 += 64u) {
            const uint32_t px = p0 + lane;
            const bool valid = px < nby;
            const uint32_t byte = valid ? src[px] : 0u;
            uint32_t prev = (uint32_t)__shfl_up((int)byte, 1);
            if (lane == 0u) prev = last;
            const bool eq = valid && px != 0u && byte == prev;
            const uint64_t m = __ballot(eq);
            last = (uint32_t)__shfl((int)byte, 63);         // (only a full step is followed by another)
            uint32_t tok = 0u, nb = 0u;
            if (valid && !eq) tok = literal(byte, &nb);
            else if (eq && (lane == 0u || !((m >> (lane - 1u)) & 1ull))) {
                const uint64_t rest = ~(m >> lane);         // (the shift fills with zeros: a one ends the run at 64 - lane at the latest)
                const uint32_t run = rest ? (uint32_t)__ffsll((long long)rest) - 1u : 64u;
                if (run >= 3u) tok = match1(run, &nb);
                else {                                      // one or two literals
                    uint32_t n0;
                    const uint32_t c = literal(byte, &n0);
                    tok = run == 2u ? c | (c << n0) : c;
                    nb = run * n0;
                }
            }
            if (valid) {                                    // Adler terms: byte i of the segment weighs n - i
                sum_a += byte;
                sum_b += (n - (first + px)) * byte;
            }
            uint32_t inc = nb;                              // exclusive scan of the bit lengths
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t t = (uint32_t)__shfl_up((int)inc, d);
                if (lane >= (uint32_t)d) inc += t;
            }
            if (nb) or_bits(stage, bitpos + inc - nb, tok);
            bitpos += (uint32_t)__shfl((int)inc, 63);
        }
        // end-of-block (seven zero bits), the empty stored block (three zero bits, zeros to the byte), 00 00 FF FF
        const uint32_t at = (bitpos + 7u + 3u + 7u) >> 3;
        if (lane == 0u) or_bits(stage, 8u * (at + 2u), 0xFFFFu);
        seg_len = at + 4u;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            sum_a += (uint32_t)__shfl_xor((int)sum_a, d);
            sum_b += (uint32_t)__shfl_xor((int)sum_b, d);
        }
        if (lane == 0u) {                                   // the Adler shares: maray_png_compress's, on rows of row_bytes
            const uint32_t after = (a.rows - 1u - row) * a.row_bytes + (a.row_bytes - (1u + s * PNG_IDX_SEG + nby));
            const uint32_t ra = sum_a % PNG_ADLER_MOD;
            a.lens[seg] = seg_len;
            a.adler[2 * (size_t)seg] = ra;
            a.adler[2 * (size_t)seg + 1] = (sum_b % PNG_ADLER_MOD + ra * (after % PNG_ADLER_MOD)) % PNG_ADLER_MOD;
        }
    }
    __syncthreads();
    if (active) {
        uint32_t *slot = (uint32_t *)(a.slots + (size_t)seg * a.slot_bytes);
        const uint32_t ndw = min((seg_len + 3u) >> 2, min(a.slot_bytes >> 2, (uint32_t)STAGE_DW));
        for (uint32_t i = lane; i < ndw; i += 64u) slot[i] = stage[i];
    }
}

void png_colors(const unsigned char *src, uint64_t npix, uint32_t *slabs, uint32_t *palette, bool add, hipStream_t st)
{
    if (!src || !npix || !slabs || !palette) throw Error{MARAY_E_INTERNAL, "device PNG encoder: bad colour arguments"};
    (void)hipGetLastError();
    const uint32_t blocks = png_colors_blocks(npix);
    hipLaunchKernelGGL(maray_png_colors, dim3(blocks), dim3(PNG_COLORS_BLOCK), 0, st, src, npix, slabs);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(maray_png_colors_merge, dim3(1), dim3(MERGE_BLOCK), 0, st, (const uint32_t *)slabs, blocks, palette, add ? 1u : 0u);
    HIP_TRY(hipGetLastError());
}

void png_index(const unsigned char *src, uint32_t w, uint32_t rows, const uint32_t *palette, uint32_t n, uint32_t depth, unsigned char *dst,
               hipStream_t st)
{
    if (!src || !w || !rows || !palette || !dst || !n || n > PNG_PALETTE_MAX || depth != png_idx_depth(n) ||
        (uint64_t)rows * png_idx_row_bytes(w, depth) > 1ull << 30)
        throw Error{MARAY_E_INTERNAL, "device PNG encoder: bad index arguments"};
    (void)hipGetLastError();
    const uint64_t n_bytes = (uint64_t)rows * png_idx_row_bytes(w, depth);
    const uint64_t blocks = (n_bytes + PNG_INDEX_BLOCK - 1) / PNG_INDEX_BLOCK;
    hipLaunchKernelGGL(maray_png_index, dim3((uint32_t)(blocks < PNG_INDEX_MAX_BLOCKS ? blocks : PNG_INDEX_MAX_BLOCKS)), dim3(PNG_INDEX_BLOCK), 0, st,
                       src, w, rows, palette, n, depth, dst);
    HIP_TRY(hipGetLastError());
}

void png_band_compress_idx(const PngBandArgs &a, hipStream_t st)
{
    if (!a.row_bytes || a.codes != MARAY_PNG_CODES_FIXED || a.filter) throw Error{MARAY_E_INTERNAL, "device PNG encoder: not an indexed band"};
    if (!a.src || !a.slots || !a.lens || !a.adler || !a.rows || a.nseg != png_idx_row_segments(a.row_bytes - 1u) ||
        a.slot_bytes != png_idx_slot_bytes(a.row_bytes - 1u) || a.slot_bytes > PNG_SLOT_MAX || (uint64_t)a.rows * a.nseg != a.n_segs ||
        ((uintptr_t)a.slots & 15) || (uint64_t)a.rows * a.row_bytes > 1ull << 30)
        throw Error{MARAY_E_INTERNAL, "device PNG encoder: bad indexed band arguments"};
    (void)hipGetLastError();
    hipLaunchKernelGGL(maray_png_compress_idx, dim3((a.n_segs + PC_WAVES - 1) / PC_WAVES), dim3(PC_BLOCK), 0, st, a);
    HIP_TRY(hipGetLastError());
}

}   // namespace maray
