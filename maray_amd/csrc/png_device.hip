// png_device.hip — the kernels of the device PNG encoder (product code; include/maray_hip.h, "device PNG encoder").
//
//   maray_png_compress  one wavefront per segment (PNG_SEG pixels of one row), four segments per block.  In steps of 64
//                       pixels: a lane loads its pixel (the aligned dwords that hold its three bytes, shifted into place),
//                       compares all three channels with the pixel before it (lane 0: the last pixel of the step before;
//                       a segment's first pixel is always a literal), __ballot gives the run mask, and every literal pixel
//                       and the first lane of every run makes one token: three fixed-Huffman literals (24 .. 27 bits) or a
//                       match of distance 3 over the run (length code, extra bits, distance code 2: 12 .. 18 bits).  A
//                       run ends with its step, so a match is at most 192 bytes.  An exclusive scan of the tokens' bit
//                       lengths gives every lane its place; lanes OR their bits into the wavefront's staging buffer in LDS
//                       (ds_or_b32, one or two dwords each), which holds the whole segment and goes to the segment's slot
//                       with coalesced dword stores at the end.  The same lanes sum the segment's Adler terms.
//   maray_png_scan      one block: the segments' byte lengths summed in groups of 64, the groups' places in the stream (an
//                       exclusive scan), and the sum of the segments' Adler shares, which is the band's Adler part.
//   maray_png_gather    one wavefront per segment: its place (the group's plus the lengths before it in the group), and
//                       its bytes from the slot to that place in the contiguous stream, in
//                       dwords aligned to the destination (v_alignbyte_b32 on the source), bytes at the two ends.
// No device-wide counter, no inline assembly, no scratch memory.  LDS: 4 x 896 bytes per block of maray_png_compress.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "png_device.hpp"
#include "png_indexed.hpp"

namespace maray {

namespace {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            throw Error{MARAY_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)};           \
    } while (0)

constexpr int PC_WAVES = 4, PC_BLOCK = 64 * PC_WAVES;
constexpr int STAGE_DW = PNG_SLOT_MAX / 4;            // dwords of a wavefront's staging buffer: a whole slot
constexpr int SCAN_BLOCK = 1024;
constexpr uint32_t SCAN_BATCH = 16;                   // groups whose loads the scan kernel keeps in flight together

// bytes of segment s of a row of w pixels: its pixels and, in the row's first segment, the filter byte
__device__ __forceinline__ uint32_t seg_pixels(uint32_t w, uint32_t s) { return min(PNG_SEG, w - s * PNG_SEG); }

// the fixed-Huffman code of literal v, bit-reversed for the LSB-first stream; *nb = its length
__device__ __forceinline__ uint32_t literal(uint32_t v, uint32_t *nb)
{
    const bool lo = v < 144u;
    *nb = lo ? 8u : 9u;
    return lo ? __brev(0x30u + v) >> 24 : __brev(0x190u + (v - 144u)) >> 23;
}

// a match of `len` bytes (3 .. 258) at distance 3: reversed length code, extra bits as they are, reversed distance code 2
__device__ __forceinline__ uint32_t match3(uint32_t len, uint32_t *nb)
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
    return hc | (extra << hb) | (8u << (hb + eb));          // 00010 reversed = 01000
}

__device__ __forceinline__ void or_bits(uint32_t *stage, uint32_t bit, uint32_t value)
{
    const uint32_t d = bit >> 5, sh = bit & 31u;
    const uint64_t v = (uint64_t)value << sh;
    if (d < (uint32_t)STAGE_DW) atomicOr(&stage[d], (uint32_t)v);
    if ((uint32_t)(v >> 32) && d + 1u < (uint32_t)STAGE_DW) atomicOr(&stage[d + 1u], (uint32_t)(v >> 32));
}

// the pixel at p (any alignment) from the aligned dwords that hold its three bytes
__device__ __forceinline__ uint32_t load_pixel(const unsigned char *p)
{
    const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t *q = (const uint32_t *)(p - mis);
    const uint32_t d0 = q[0], d1 = mis >= 2u ? q[1] : 0u;
    return __builtin_amdgcn_alignbyte(d1, d0, mis) & 0xFFFFFFu;
}

// ---- row filters (include/maray_hip.h, "Row filters") ------------------------------------------------------------------------
// PNG's filter type t (0 .. 4, bpp = 3) on one pixel, byte by byte on the packed 24 bits: x the pixel, a the pixel on its left,
// b the pixel above, c the pixel above a.  Average is the floor of the 9-bit sum's half, Paeth's ties go a, b, c.
__device__ __forceinline__ uint32_t filter_pixel(uint32_t t, uint32_t x, uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t out = 0u;
#pragma unroll
    for (uint32_t sh = 0u; sh < 24u; sh += 8u) {
        const int ba = (int)((a >> sh) & 255u), bb = (int)((b >> sh) & 255u), bc = (int)((c >> sh) & 255u);
        int pred = 0;
        if (t == 1u) pred = ba;
        else if (t == 2u) pred = bb;
        else if (t == 3u) pred = (ba + bb) >> 1;
        else if (t == 4u) {
            const int p = ba + bb - bc, pa = abs(p - ba), pb = abs(p - bb), pc = abs(p - bc);
            pred = pa <= pb && pa <= pc ? ba : pb <= pc ? bb : bc;
        }
        out |= (((x >> sh) - (uint32_t)pred) & 255u) << sh;
    }
    return out;
}

// Where a segment's pixels and the pixels above them lie.  Segments cut the compression, not the filter: a segment that is
// not its row's first has the previous segment's last pixels on its left.
struct FilterSeg {
    const unsigned char *src;       // the segment's first pixel
    const unsigned char *up;        // the pixel above it; null: the row above is all zeros (row 0 of the image)
    bool has_left;
};
// the raw pixel and the pixel above it of lane 63 of the step before
struct FilterCarry { uint32_t x, b; };

__device__ __forceinline__ FilterSeg filter_seg(const PngBandArgs &a, uint32_t row, uint32_t s, const unsigned char *src)
{
    FilterSeg f;
    f.src = src;
    // rows are 3 w bytes apart: the row above is aligned differently from the row itself
    f.up = row ? src - (size_t)a.w * 3 : a.above ? a.above + (size_t)s * PNG_SEG * 3 : nullptr;
    f.has_left = s != 0u;
    return f;
}

// One step of 64 pixels: lane's pixel x (0 past the segment's end) and its neighbours a, b, c.  Left neighbours come by
// __shfl_up; lane 0 takes them from the step before (fc), and at the segment's start from the previous segment (two loads
// more) or, at x = 0 of the row, as zeros.
__device__ __forceinline__ void filter_neighbours(const FilterSeg &f, uint32_t p0, uint32_t npix, uint32_t lane, FilterCarry *fc, uint32_t *x,
                                                  uint32_t *a, uint32_t *b, uint32_t *c)
{
    const uint32_t px = p0 + lane;
    const bool valid = px < npix;
    const uint32_t vx = valid ? load_pixel(f.src + (size_t)px * 3) : 0u;
    const uint32_t vb = valid && f.up ? load_pixel(f.up + (size_t)px * 3) : 0u;
    uint32_t va = (uint32_t)__shfl_up((int)vx, 1), vc = (uint32_t)__shfl_up((int)vb, 1);
    if (lane == 0u) {
        if (p0) { va = fc->x; vc = fc->b; }
        else if (f.has_left) { va = load_pixel(f.src - 3); vc = f.up ? load_pixel(f.up - 3) : 0u; }
        else { va = 0u; vc = 0u; }
    }
    fc->x = (uint32_t)__shfl((int)vx, 63);                  // (only a full step is followed by another)
    fc->b = (uint32_t)__shfl((int)vb, 63);
    *x = vx; *a = va; *b = vb; *c = vc;
}

// the lane's filtered pixel under type t (wave-uniform); 0 past the segment's end
__device__ __forceinline__ uint32_t filter_step(const FilterSeg &f, uint32_t t, uint32_t p0, uint32_t npix, uint32_t lane, FilterCarry *fc)
{
    uint32_t x, a, b, c;
    filter_neighbours(f, p0, npix, lane, fc, &x, &a, &b, &c);
    return p0 + lane < npix ? filter_pixel(t, x, a, b, c) : 0u;
}

// One step of the tokeniser on the lane's (filtered) pixel `pix`, exactly as maray_png_compress cuts a step into tokens.
// Returns 0: this lane starts no token; 1: its pixel is three literals; 2: it starts a match of *run pixels.  `last` carries
// the step's last pixel on.
__device__ __forceinline__ uint32_t token_of(uint32_t pix, uint32_t px, uint32_t npix, uint32_t lane, uint32_t *last, uint32_t *run)
{
    const bool valid = px < npix;
    uint32_t prev = (uint32_t)__shfl_up((int)pix, 1);
    if (lane == 0u) prev = *last;
    const bool eq = valid && px != 0u && pix == prev;
    const uint64_t m = __ballot(eq);
    *last = (uint32_t)__shfl((int)pix, 63);
    *run = 0u;
    if (valid && !eq) return 1u;
    if (eq && (lane == 0u || !((m >> (lane - 1u)) & 1ull))) {
        const uint64_t rest = ~(m >> lane);
        *run = rest ? (uint32_t)__ffsll((long long)rest) - 1u : 64u;
        return 2u;
    }
    return 0u;
}

// F: the filtered form (the row's type from a.row_filter, the pixels through filter_step); else today's kernel
template <bool F>
__device__ __forceinline__ void compress_body(const PngBandArgs &a, uint32_t *stage_all)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t *stage = stage_all + wave * STAGE_DW;
    for (uint32_t i = lane; i < (uint32_t)STAGE_DW; i += 64u) stage[i] = 0u;
    __syncthreads();
    const uint32_t seg = blockIdx.x * PC_WAVES + wave;
    const bool active = seg < a.n_segs;                     // (wave-uniform; nobody leaves before the second barrier)
    uint32_t seg_len = 0u;
    if (active) {
        const uint32_t row = seg / a.nseg, s = seg - row * a.nseg;
        const uint32_t npix = seg_pixels(a.w, s), first = s == 0u ? 1u : 0u;
        const uint32_t n = 3u * npix + first;               // the segment's filtered bytes
        const unsigned char *src = a.src + ((size_t)row * a.w + (size_t)s * PNG_SEG) * 3;
        // block header BFINAL = 0, BTYPE = 01 (the bits 0, 1, 0), then in a row's first segment the filter byte as a literal
        const uint32_t ft = F ? a.row_filter[row] : 0u;
        const FilterSeg fs = F ? filter_seg(a, row, s, src) : FilterSeg{};
        uint32_t bitpos = 3u;
        if (lane == 0u) {
            or_bits(stage, 0u, 2u);
            if (first) { uint32_t nb; const uint32_t c = literal(ft, &nb); or_bits(stage, 3u, c); }
        }
        if (first) bitpos += 8u;
        uint32_t sum_a = 0u, sum_b = 0u, last = 0u;
        FilterCarry fc{0u, 0u};
        if (F && first && lane == 0u) { sum_a = ft; sum_b = n * ft; }     // the filter byte is byte 0 of its segment
        for (uint32_t p0 = 0u; p0 < npix; p0 += 64u) {
            const uint32_t px = p0 + lane;
            const bool valid = px < npix;
            uint32_t pix = 0u;
            if (F) pix = filter_step(fs, ft, p0, npix, lane, &fc);
            else if (valid) {
                // the three bytes at src + 3 px from the aligned dwords that hold them (every dword read holds one of them)
                const unsigned char *p = src + (size_t)px * 3;
                const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
                const uint32_t *q = (const uint32_t *)(p - mis);
                const uint32_t d0 = q[0], d1 = mis >= 2u ? q[1] : 0u;
                pix = __builtin_amdgcn_alignbyte(d1, d0, mis) & 0xFFFFFFu;
            }
            uint32_t prev = (uint32_t)__shfl_up((int)pix, 1);
            if (lane == 0u) prev = last;
            const bool eq = valid && px != 0u && pix == prev;
            const uint64_t m = __ballot(eq);
            last = (uint32_t)__shfl((int)pix, 63);          // (only a full step is followed by another)
            uint32_t tok = 0u, nb = 0u;
            if (valid && !eq) {
                uint32_t n0, n1, n2;
                const uint32_t c0 = literal(pix & 255u, &n0), c1 = literal((pix >> 8) & 255u, &n1), c2 = literal(pix >> 16, &n2);
                tok = c0 | (c1 << n0) | (c2 << (n0 + n1));
                nb = n0 + n1 + n2;
            } else if (eq && (lane == 0u || !((m >> (lane - 1u)) & 1ull))) {
                const uint64_t rest = ~(m >> lane);         // (the shift fills with zeros: a one ends the run at 64 - lane at the latest)
                const uint32_t run = rest ? (uint32_t)__ffsll((long long)rest) - 1u : 64u;
                tok = match3(3u * run, &nb);
            }
            if (valid) {
                // Adler terms: byte i of the segment weighs n - i
                const uint32_t wgt = n - (first + 3u * px);
                const uint32_t r = pix & 255u, g = (pix >> 8) & 255u, b = pix >> 16;
                sum_a += r + g + b;
                sum_b += wgt * r + (wgt - 1u) * g + (wgt - 2u) * b;
            }
            // exclusive scan of the bit lengths
            uint32_t inc = nb;
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
        if (lane == 0u) {
            // The segment's share of the band's Adler part: A, and B + A x (the band's bytes after this segment) -- a byte that
            // weighs n - i in its segment weighs that many more in the band -- both modulo 65521 (a band has at most 2^30
            // filtered bytes; residues' products stay below 2^32).  Shares add up in any order.
            const uint32_t row_bytes = 3u * a.w + 1u;
            const uint32_t after = (a.rows - 1u - row) * row_bytes + (row_bytes - (1u + 3u * (s * PNG_SEG + npix)));
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

__global__ __launch_bounds__(PC_BLOCK) void maray_png_compress(const PngBandArgs a)
{
    __shared__ uint32_t stage_all[PC_WAVES * STAGE_DW];
    compress_body<false>(a, stage_all);
}

__global__ __launch_bounds__(PC_BLOCK) void maray_png_compress_filtered(const PngBandArgs a)
{
    __shared__ uint32_t stage_all[PC_WAVES * STAGE_DW];
    compress_body<true>(a, stage_all);
}

// segments per group of the scan: a multiple of 64 that makes at most SCAN_BLOCK groups
__host__ __device__ inline uint32_t scan_group(uint32_t n_segs) { return 64u * ((n_segs + 64u * SCAN_BLOCK - 1u) / (64u * SCAN_BLOCK)); }

// x modulo 65521 without a 64-bit division (a bit-serial loop on this target): 2^32 = 225 modulo 65521
__device__ __forceinline__ uint32_t mod_adler(uint64_t x)
{
    const uint32_t hi = (uint32_t)(x >> 32), lo = (uint32_t)x;
    return ((hi % PNG_ADLER_MOD) * 225u + lo % PNG_ADLER_MOD) % PNG_ADLER_MOD;
}

// One block of 16 wavefronts.  The segments are taken in groups of G (64 for up to 65,536 segments): wavefront v sums the
// lengths of the groups 64 v .. 64 v + 63, one coalesced load and one wavefront reduction per 64 segments, independent from
// group to group, and lane i keeps group 64 v + i's sum.  An exclusive scan of the at most 1024 sums (wavefront scans, the 16
// totals through LDS) gives every group its place in the stream (offsets[g]); the gather kernel adds the lengths in front
// of a segment inside its group itself.  All lanes also add up the segments' Adler shares (plain sums: the compress kernel
// has put every segment's place in the band into its share).
__global__ __launch_bounds__(SCAN_BLOCK) void maray_png_scan(const PngBandArgs a)
{
    constexpr uint32_t WAVES = SCAN_BLOCK / 64;
    __shared__ uint64_t w_len[WAVES], w_a[WAVES], w_b[WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t G = scan_group(a.n_segs), n_groups = (a.n_segs + G - 1u) / G;
    uint64_t mine = 0, sa = 0, sb = 0;                 // (shares are below 65521: 2^31 of them fit)
    for (uint32_t i0 = 0; i0 < 64u; i0 += SCAN_BATCH) { // SCAN_BATCH groups at a time, their loads in flight together
        uint64_t x[SCAN_BATCH];
        uint32_t ya[SCAN_BATCH], yb[SCAN_BATCH];
#pragma unroll
        for (uint32_t u = 0; u < SCAN_BATCH; u++) {     // unconditional loads at a clamped index: no branch, no wait between them
            const uint64_t j = (uint64_t)(wave * 64u + i0 + u) * G + lane;
            const uint64_t jj = j < a.n_segs ? j : a.n_segs - 1u;
            x[u] = a.lens[jj]; ya[u] = a.adler[2 * jj]; yb[u] = a.adler[2 * jj + 1];
        }
#pragma unroll
        for (uint32_t u = 0; u < SCAN_BATCH; u++) {     // the first 64 segments of each group
            const bool in = (uint64_t)(wave * 64u + i0 + u) * G + lane < a.n_segs;
            x[u] = in ? x[u] : 0u;
            sa += in ? ya[u] : 0u;
            sb += in ? yb[u] : 0u;
        }
        if (G > 64u) {                                  // bands of more than 65,536 segments: the rest of each group
            for (uint32_t u = 0; u < SCAN_BATCH; u++) {
                const uint64_t j0 = (uint64_t)(wave * 64u + i0 + u) * G, j1 = j0 + G < a.n_segs ? j0 + G : a.n_segs;
                for (uint64_t j = j0 + 64u + lane; j < j1; j += 64) {
                    x[u] += a.lens[j];
                    sa += a.adler[2 * j];
                    sb += a.adler[2 * j + 1];
                }
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < SCAN_BATCH; u++) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) x[u] += __shfl_xor(x[u], d);
            if (lane == i0 + u) mine = x[u];
        }
    }
    uint64_t inc = mine;                                // inclusive scan of the wavefront's 64 group sums
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t t = __shfl_up(inc, d);
        if (lane >= (uint32_t)d) inc += t;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        sa += __shfl_xor(sa, d);
        sb += __shfl_xor(sb, d);
    }
    if (lane == 63u) w_len[wave] = inc;
    if (lane == 0u) { w_a[wave] = sa; w_b[wave] = sb; }
    __syncthreads();
    uint64_t base = 0;
    for (uint32_t v = 0; v < wave; v++) base += w_len[v];
    const uint32_t g = wave * 64u + lane;
    if (g < n_groups) a.offsets[g] = base + inc - mine;
    if (threadIdx.x == 0) {
        uint64_t tl = 0;
        uint32_t ta = 0, tb = 0;
        for (uint32_t v = 0; v < WAVES; v++) { tl += w_len[v]; ta += mod_adler(w_a[v]); tb += mod_adler(w_b[v]); }
        const uint32_t row_bytes = a.row_bytes ? a.row_bytes : 3u * a.w + 1u;
        const uint32_t n = (a.rows * row_bytes) % PNG_ADLER_MOD;             // (a band has at most 2^30 filtered bytes)
        a.totals[0] = tl;
        a.totals[1] = (uint64_t)n | ((uint64_t)(ta % PNG_ADLER_MOD) << 32);
        a.totals[2] = tb % PNG_ADLER_MOD;
    }
}

__global__ __launch_bounds__(PC_BLOCK) void maray_png_gather(const PngBandArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t seg = blockIdx.x * PC_WAVES + (threadIdx.x >> 6);
    if (seg >= a.n_segs) return;
    // where the segment starts: its group's place plus the lengths in front of it inside the group
    const uint32_t G = scan_group(a.n_segs), g = seg / G;
    uint32_t before = 0;
    for (uint64_t j = (uint64_t)g * G + lane; j < seg; j += 64) before += a.lens[j];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) before += (uint32_t)__shfl_xor((int)before, d);
    const uint32_t len = min(a.lens[seg], a.slot_bytes);
    const unsigned char *src = a.slots + (size_t)seg * a.slot_bytes;
    unsigned char *dst = a.stream + (a.offsets[g] + before);
    const uint32_t head = min(len, (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u);
    if (lane < head) dst[lane] = src[lane];
    const uint32_t nd = (len - head) >> 2, r = head & 3u;
    const uint32_t *s32 = (const uint32_t *)src;
    uint32_t *d32 = (uint32_t *)(dst + head);
    for (uint32_t k = lane; k < nd; k += 64u) {
        const uint32_t q = (head + 4u * k) >> 2;            // (with r > 0 dword q + 1 holds byte head + 4 k + 3 < len: inside the slot)
        const uint32_t lo = s32[q], hi = r ? s32[q + 1u] : 0u;
        d32[k] = __builtin_amdgcn_alignbyte(hi, lo, r);
    }
    const uint32_t t0 = head + 4u * nd;
    if (lane < len - t0) dst[t0 + lane] = src[t0 + lane];
}

// ---- dynamic-Huffman codes: the same tokens, counted, then written with the band's own code ----------------------------------
//   maray_png_histogram      maray_png_compress's tokeniser (load, __shfl_up, __ballot, run length) feeding the 286 counts of
//                            the literal/length alphabet in LDS (ds_add_u32); a capped grid whose wavefronts stride over the
//                            segments; every block STORES its counts, and
//   maray_png_histogram_sum  one block adds the blocks' counts up (maray_frame_delta's two launches: no device-wide counter).
//                            A band's distance count is the sum of its length symbols' counts: every match is at distance 3.
//   maray_png_compress_dyn   maray_png_compress with the band's code from a table in LDS (reversed code | length << 16, filled
//                            once per block): a literal pixel is up to 45 bits, a match its length code, the extra bits and
//                            one zero bit (the only distance code, of length 1); no header, no end-of-block, no sync; the
//                            segment's length is kept in BITS, so that maray_png_scan yields bit offsets.
//   maray_png_zero           zeroes the span of the stream the band's bits will take (the total is on the device by then), and
//   maray_png_gather_bits    one wavefront per segment shifts its slot's bits to their bit offset behind the header's bits (a
//                            64-bit funnel shift per destination dword): dwords wholly inside the segment are plain stores,
//                            the first and the last are atomicOr -- short segments share a dword with their neighbours, and
//                            OR does not care for the order.
// LDS: 1,152 bytes per block of maray_png_histogram; 1,144 + 4 x 1,456 bytes per block of maray_png_compress_dyn.
constexpr int STAGE_DW_DYN = PNG_SLOT_MAX_DYN / 4;
constexpr int HIST_BLOCK = 64 * PNG_HIST_WAVES, HIST_SUM_BLOCK = 320, ZERO_BLOCK = 256, ZERO_MAX_BLOCKS = 2048;
static_assert(HIST_SUM_BLOCK >= (int)PNG_HIST_STRIDE && PNG_HIST_STRIDE >= PNG_LIT_SYMS, "one lane per count");

// One step of 64 pixels of a segment exactly as maray_png_compress cuts it into tokens.  Returns 0: this lane starts no
// token; 1: its pixel is three literals; 2: it starts a match of *run pixels.  `last` carries the step's last pixel on.
__device__ __forceinline__ uint32_t step_token(const unsigned char *src, uint32_t p0, uint32_t npix, uint32_t lane, uint32_t *last,
                                               uint32_t *pix_out, uint32_t *run)
{
    const uint32_t px = p0 + lane;
    const bool valid = px < npix;
    const uint32_t pix = valid ? load_pixel(src + (size_t)px * 3) : 0u;
    uint32_t prev = (uint32_t)__shfl_up((int)pix, 1);
    if (lane == 0u) prev = *last;
    const bool eq = valid && px != 0u && pix == prev;
    const uint64_t m = __ballot(eq);
    *last = (uint32_t)__shfl((int)pix, 63);
    *pix_out = pix;
    *run = 0u;
    if (valid && !eq) return 1u;
    if (eq && (lane == 0u || !((m >> (lane - 1u)) & 1ull))) {
        const uint64_t rest = ~(m >> lane);
        *run = rest ? (uint32_t)__ffsll((long long)rest) - 1u : 64u;
        return 2u;
    }
    return 0u;
}

// the length symbol of a match of len bytes (3 .. 258), its number of extra bits and their value (match3's first half)
__device__ __forceinline__ uint32_t length_symbol(uint32_t len, uint32_t *eb, uint32_t *extra)
{
    const uint32_t l = len - 3u;
    *eb = 0u; *extra = 0u;
    if (len == 258u) return 285u;
    if (l < 8u) return 257u + l;
    const uint32_t e = 29u - (uint32_t)__clz((int)l);
    *eb = e;
    *extra = l & ((1u << e) - 1u);
    return 261u + 4u * e + ((l >> e) & 3u);
}

template <bool F>
__device__ __forceinline__ void histogram_body(const PngBandArgs &a, uint32_t *hist)
{
    for (uint32_t i = threadIdx.x; i < PNG_HIST_STRIDE; i += HIST_BLOCK) hist[i] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // (wave-uniform trip counts, no barrier inside; seg + the stride stays below 2^32: n_segs < 2^31)
    for (uint32_t seg = blockIdx.x * PNG_HIST_WAVES + wave; seg < a.n_segs; seg += gridDim.x * PNG_HIST_WAVES) {
        const uint32_t row = seg / a.nseg, s = seg - row * a.nseg;
        const uint32_t npix = seg_pixels(a.w, s);
        const unsigned char *src = a.src + ((size_t)row * a.w + (size_t)s * PNG_SEG) * 3;
        const uint32_t ft = F ? a.row_filter[row] : 0u;
        const FilterSeg fs = F ? filter_seg(a, row, s, src) : FilterSeg{};
        FilterCarry fc{0u, 0u};
        if (s == 0u && lane == 0u) atomicAdd(&hist[ft], 1u);        // the row's filter byte
        uint32_t last = 0u;
        for (uint32_t p0 = 0u; p0 < npix; p0 += 64u) {
            uint32_t pix, run, kind;
            if (F) {
                pix = filter_step(fs, ft, p0, npix, lane, &fc);
                kind = token_of(pix, p0 + lane, npix, lane, &last, &run);
            } else
                kind = step_token(src, p0, npix, lane, &last, &pix, &run);
            if (kind == 1u) {
                atomicAdd(&hist[pix & 255u], 1u);
                atomicAdd(&hist[(pix >> 8) & 255u], 1u);
                atomicAdd(&hist[pix >> 16], 1u);
            } else if (kind == 2u) {
                uint32_t eb, extra;
                atomicAdd(&hist[length_symbol(3u * run, &eb, &extra)], 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < PNG_HIST_STRIDE; i += HIST_BLOCK) a.hist[(size_t)blockIdx.x * PNG_HIST_STRIDE + i] = hist[i];
}

__global__ __launch_bounds__(HIST_BLOCK) void maray_png_histogram(const PngBandArgs a)
{
    __shared__ uint32_t hist[PNG_HIST_STRIDE];
    histogram_body<false>(a, hist);
}

__global__ __launch_bounds__(HIST_BLOCK) void maray_png_histogram_filtered(const PngBandArgs a)
{
    __shared__ uint32_t hist[PNG_HIST_STRIDE];
    histogram_body<true>(a, hist);
}

// count i of the band = the sum of the blocks' counts i (a band has at most 2^28 bytes: no count overflows)
__global__ __launch_bounds__(HIST_SUM_BLOCK) void maray_png_histogram_sum(uint32_t *hist, uint32_t n_blocks)
{
    const uint32_t i = threadIdx.x;
    if (i >= PNG_HIST_STRIDE) return;
    uint32_t sum = 0u;
    for (uint32_t b = 0; b < n_blocks; b++) sum += hist[(size_t)b * PNG_HIST_STRIDE + i];
    hist[(size_t)n_blocks * PNG_HIST_STRIDE + i] = sum;
}

// value (up to 45 bits) at bit `bit` of the staging buffer: up to three dwords
__device__ __forceinline__ void or_bits64(uint32_t *stage, uint32_t bit, uint64_t value)
{
    const uint32_t d = bit >> 5, sh = bit & 31u;
    const uint64_t v = value << sh;
    const uint32_t w0 = (uint32_t)v, w1 = (uint32_t)(v >> 32), w2 = sh ? (uint32_t)(value >> (64u - sh)) : 0u;
    if (w0 && d < (uint32_t)STAGE_DW_DYN) atomicOr(&stage[d], w0);
    if (w1 && d + 1u < (uint32_t)STAGE_DW_DYN) atomicOr(&stage[d + 1u], w1);
    if (w2 && d + 2u < (uint32_t)STAGE_DW_DYN) atomicOr(&stage[d + 2u], w2);
}

template <bool F>
__device__ __forceinline__ void compress_dyn_body(const PngBandArgs &a, uint32_t *table, uint32_t *stage_all)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t *stage = stage_all + wave * STAGE_DW_DYN;
    for (uint32_t i = threadIdx.x; i < PNG_LIT_SYMS; i += PC_BLOCK) table[i] = a.table[i];
    for (uint32_t i = lane; i < (uint32_t)STAGE_DW_DYN; i += 64u) stage[i] = 0u;
    __syncthreads();
    const uint32_t seg = blockIdx.x * PC_WAVES + wave;
    const bool active = seg < a.n_segs;                     // (wave-uniform; nobody leaves before the second barrier)
    uint32_t seg_bits = 0u;
    if (active) {
        const uint32_t row = seg / a.nseg, s = seg - row * a.nseg;
        const uint32_t npix = seg_pixels(a.w, s), first = s == 0u ? 1u : 0u;
        const uint32_t n = 3u * npix + first;
        const unsigned char *src = a.src + ((size_t)row * a.w + (size_t)s * PNG_SEG) * 3;
        uint32_t bitpos = 0u;
        const uint32_t ft = F ? a.row_filter[row] : 0u;
        const FilterSeg fs = F ? filter_seg(a, row, s, src) : FilterSeg{};
        FilterCarry fc{0u, 0u};
        if (first) {                                        // the filter byte as a literal
            const uint32_t e = table[ft];
            if (lane == 0u) or_bits64(stage, 0u, e & 0xFFFFu);
            bitpos = e >> 16;
        }
        uint32_t sum_a = 0u, sum_b = 0u, last = 0u;
        if (F && first && lane == 0u) { sum_a = ft; sum_b = n * ft; }     // the filter byte is byte 0 of its segment
        for (uint32_t p0 = 0u; p0 < npix; p0 += 64u) {
            uint32_t pix, run, kind;
            if (F) {
                pix = filter_step(fs, ft, p0, npix, lane, &fc);
                kind = token_of(pix, p0 + lane, npix, lane, &last, &run);
            } else
                kind = step_token(src, p0, npix, lane, &last, &pix, &run);
            const uint32_t px = p0 + lane;
            uint64_t tok = 0u;
            uint32_t nb = 0u;
            if (kind == 1u) {
                const uint32_t e0 = table[pix & 255u], e1 = table[(pix >> 8) & 255u], e2 = table[pix >> 16];
                const uint32_t n0 = e0 >> 16, n1 = e1 >> 16, n2 = e2 >> 16;
                tok = (uint64_t)(e0 & 0xFFFFu) | ((uint64_t)(e1 & 0xFFFFu) << n0) | ((uint64_t)(e2 & 0xFFFFu) << (n0 + n1));
                nb = n0 + n1 + n2;
            } else if (kind == 2u) {
                uint32_t eb, extra;
                const uint32_t e = table[length_symbol(3u * run, &eb, &extra)];
                const uint32_t n0 = e >> 16;
                tok = (uint64_t)(e & 0xFFFFu) | ((uint64_t)extra << n0);
                nb = n0 + eb + 1u;                          // and the distance code: one zero bit
            }
            if (px < npix) {
                const uint32_t wgt = n - (first + 3u * px);
                const uint32_t r = pix & 255u, g = (pix >> 8) & 255u, b = pix >> 16;
                sum_a += r + g + b;
                sum_b += wgt * r + (wgt - 1u) * g + (wgt - 2u) * b;
            }
            uint32_t inc = nb;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t t = (uint32_t)__shfl_up((int)inc, d);
                if (lane >= (uint32_t)d) inc += t;
            }
            if (nb) or_bits64(stage, bitpos + inc - nb, tok);
            bitpos += (uint32_t)__shfl((int)inc, 63);
        }
        seg_bits = bitpos;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            sum_a += (uint32_t)__shfl_xor((int)sum_a, d);
            sum_b += (uint32_t)__shfl_xor((int)sum_b, d);
        }
        if (lane == 0u) {                                   // the Adler shares: exactly maray_png_compress's
            const uint32_t row_bytes = 3u * a.w + 1u;
            const uint32_t after = (a.rows - 1u - row) * row_bytes + (row_bytes - (1u + 3u * (s * PNG_SEG + npix)));
            const uint32_t ra = sum_a % PNG_ADLER_MOD;
            a.lens[seg] = seg_bits;
            a.adler[2 * (size_t)seg] = ra;
            a.adler[2 * (size_t)seg + 1] = (sum_b % PNG_ADLER_MOD + ra * (after % PNG_ADLER_MOD)) % PNG_ADLER_MOD;
        }
    }
    __syncthreads();
    if (active) {
        uint32_t *slot = (uint32_t *)(a.slots + (size_t)seg * a.slot_bytes);
        const uint32_t ndw = min((seg_bits + 31u) >> 5, min(a.slot_bytes >> 2, (uint32_t)STAGE_DW_DYN));
        for (uint32_t i = lane; i < ndw; i += 64u) slot[i] = stage[i];
    }
}

__global__ __launch_bounds__(PC_BLOCK) void maray_png_compress_dyn(const PngBandArgs a)
{
    __shared__ uint32_t table[PNG_LIT_SYMS];
    __shared__ uint32_t stage_all[PC_WAVES * STAGE_DW_DYN];
    compress_dyn_body<false>(a, table, stage_all);
}

__global__ __launch_bounds__(PC_BLOCK) void maray_png_compress_dyn_filtered(const PngBandArgs a)
{
    __shared__ uint32_t table[PNG_LIT_SYMS];
    __shared__ uint32_t stage_all[PC_WAVES * STAGE_DW_DYN];
    compress_dyn_body<true>(a, table, stage_all);
}

// bytes of the stream a dynamic band may take: the slots' bytes, the header's and a dword's slack, in whole 16 bytes
__host__ __device__ inline uint64_t dyn_stream_cap(uint32_t n_segs, uint32_t slot_bytes) { return (uint64_t)n_segs * slot_bytes + 512u; }

__global__ __launch_bounds__(ZERO_BLOCK) void maray_png_zero(const PngBandArgs a)
{
    const uint64_t bits = (uint64_t)a.header_bits + a.totals[0];
    const uint64_t cap16 = dyn_stream_cap(a.n_segs, a.slot_bytes) / 16u;
    const uint64_t n16 = min(((bits + 7u) / 8u + 15u) / 16u + 1u, cap16);
    uint4 *dst = (uint4 *)a.stream;
    for (uint64_t i = (uint64_t)blockIdx.x * ZERO_BLOCK + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * ZERO_BLOCK)
        dst[i] = make_uint4(0u, 0u, 0u, 0u);
}

__global__ __launch_bounds__(PC_BLOCK) void maray_png_gather_bits(const PngBandArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t seg = blockIdx.x * PC_WAVES + (threadIdx.x >> 6);
    if (seg >= a.n_segs) return;
    const uint32_t G = scan_group(a.n_segs), g = seg / G;
    uint32_t before = 0;                                    // (a band's bits fit 32 bits)
    for (uint64_t j = (uint64_t)g * G + lane; j < seg; j += 64) before += a.lens[j];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) before += (uint32_t)__shfl_xor((int)before, d);
    const uint32_t nbits = min(a.lens[seg], 8u * a.slot_bytes);
    const uint64_t at = (uint64_t)a.header_bits + a.offsets[g] + before;      // the segment's first bit in the stream
    if (!nbits || at + nbits > 8u * (dyn_stream_cap(a.n_segs, a.slot_bytes) - 16u)) return;      // (never: the scan's sums are the slots' bits)
    const uint32_t sh = (uint32_t)at & 31u;
    const uint32_t *src = (const uint32_t *)(a.slots + (size_t)seg * a.slot_bytes);
    uint32_t *dst = (uint32_t *)a.stream + (at >> 5);
    const uint32_t nsrc = (nbits + 31u) >> 5, nd = (sh + nbits + 31u) >> 5;
    for (uint32_t k = lane; k < nd; k += 64u) {
        // destination dword k holds the source's bits 32 k - sh .. 32 k - sh + 31: the top of dword k - 1, the bottom of dword k
        const uint32_t lo = k >= 1u && k - 1u < nsrc ? src[k - 1u] : 0u, hi = k < nsrc ? src[k] : 0u;
        const uint32_t v = (uint32_t)((((uint64_t)hi << 32) | lo) >> (32u - sh));
        if (k == 0u || k == nd - 1u) { if (v) atomicOr(&dst[k], v); }
        else dst[k] = v;
    }
}

// ---- row filters: which type a row takes (MARAY_PNG_FILTER_ADAPTIVE) -------------------------------------------------------------
//   maray_png_filter_cost   one wavefront per segment, four per block, like maray_png_compress: the tokeniser's counting for
//                           all five types at once, nothing emitted.  Per step the lane's pixel and its three neighbours are
//                           loaded once, then five filtered pixels, five __ballot run masks and the bits of the lane's
//                           literals or match; per-lane sums over the segment's steps, one packed wavefront reduction at the
//                           end, and five (bytes, bits) pairs per segment: what the segment would occupy as a fixed-Huffman
//                           segment (maray_png_compress's seg_len) and its token bits.
//   maray_png_filter_pick   one wavefront per row: the sums of the row's segments' pairs, and the smallest (bytes, bits, type).
// No LDS, no barrier, no scratch memory.
constexpr int FC_WAVES = 4, FC_BLOCK = 64 * FC_WAVES;

// the bits of a pixel's three fixed-Huffman literals (literal's lengths)
__device__ __forceinline__ uint32_t literal_bits(uint32_t pix)
{
    return 24u + ((pix & 255u) >= 144u) + (((pix >> 8) & 255u) >= 144u) + ((pix >> 16) >= 144u);
}

// the bits of match3(len)
__device__ __forceinline__ uint32_t match3_bits(uint32_t len)
{
    const uint32_t l = len - 3u;
    if (len == 258u) return 8u + 5u;
    if (l < 8u) return 7u + 5u;
    const uint32_t eb = 29u - (uint32_t)__clz((int)l), code = 261u + 4u * eb + ((l >> eb) & 3u);
    return (code < 280u ? 7u : 8u) + eb + 5u;
}

__global__ __launch_bounds__(FC_BLOCK) void maray_png_filter_cost(const PngBandArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t seg = blockIdx.x * FC_WAVES + (threadIdx.x >> 6);
    if (seg >= a.n_segs) return;                            // (wave-uniform; the kernel has no barrier)
    const uint32_t row = seg / a.nseg, s = seg - row * a.nseg;
    const uint32_t npix = seg_pixels(a.w, s), first = s == 0u ? 1u : 0u;
    const unsigned char *src = a.src + ((size_t)row * a.w + (size_t)s * PNG_SEG) * 3;
    const FilterSeg fs = filter_seg(a, row, s, src);
    FilterCarry fc{0u, 0u};
    uint32_t last[5] = {0u, 0u, 0u, 0u, 0u}, acc[5] = {0u, 0u, 0u, 0u, 0u};     // (fully unrolled below: registers)
    for (uint32_t p0 = 0u; p0 < npix; p0 += 64u) {
        const uint32_t px = p0 + lane;
        uint32_t x, pa, pb, pc;
        filter_neighbours(fs, p0, npix, lane, &fc, &x, &pa, &pb, &pc);
#pragma unroll
        for (uint32_t t = 0u; t < 5u; t++) {
            const uint32_t pix = px < npix ? filter_pixel(t, x, pa, pb, pc) : 0u;
            uint32_t run;
            const uint32_t kind = token_of(pix, px, npix, lane, &last[t], &run);
            acc[t] += kind == 1u ? literal_bits(pix) : kind == 2u ? match3_bits(3u * run) : 0u;
        }
    }
    // a lane's sum is at most 4 x 27 bits, the wavefront's 256 x 27 < 2^16: four of them in one 64-bit word
    uint64_t lo = (uint64_t)acc[0] | ((uint64_t)acc[1] << 16) | ((uint64_t)acc[2] << 32) | ((uint64_t)acc[3] << 48);
    uint32_t hi = acc[4];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo += __shfl_xor(lo, d);
        hi += (uint32_t)__shfl_xor((int)hi, d);
    }
    if (lane < 5u) {
        // maray_png_compress's arithmetic: the block header's 3 bits, the filter byte's 8 (every type is a literal below 144),
        // the tokens; then end-of-block, the stored block's 3 bits, zeros to the byte, 00 00 FF FF
        const uint32_t tokens = lane < 4u ? (uint32_t)(lo >> (16u * lane)) & 0xFFFFu : hi;
        const uint32_t bits = 3u + 8u * first + tokens;
        uint32_t *out = a.cost + (size_t)seg * 10u + 2u * lane;
        out[0] = ((bits + 7u + 3u + 7u) >> 3) + 4u;
        out[1] = bits;
    }
}

__global__ __launch_bounds__(FC_BLOCK) void maray_png_filter_pick(const PngBandArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t row = blockIdx.x * FC_WAVES + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    uint32_t sum[10] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};     // (a row's bits fit 32 bits: 27 per pixel at most)
    for (uint32_t s = lane; s < a.nseg; s += 64u) {
        const uint32_t *c = a.cost + ((size_t)row * a.nseg + s) * 10u;
#pragma unroll
        for (int i = 0; i < 10; i++) sum[i] += c[i];
    }
#pragma unroll
    for (int i = 0; i < 10; i++) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) sum[i] += (uint32_t)__shfl_xor((int)sum[i], d);
    }
    if (lane == 0u) {
        uint32_t best = 0u, best_bytes = sum[0], best_bits = sum[1];
#pragma unroll
        for (uint32_t t = 1u; t < 5u; t++) {                // the smallest (bytes, bits, t): a later type must be strictly better
            const uint32_t by = sum[2 * t], bi = sum[2 * t + 1];
            if (by < best_bytes || (by == best_bytes && bi < best_bits)) { best = t; best_bytes = by; best_bits = bi; }
        }
        a.row_filter[row] = (uint8_t)best;
    }
}

void check_band(const PngBandArgs &a)
{
    const bool dyn = a.codes == MARAY_PNG_CODES_DYNAMIC;
    if (a.row_bytes) {                                      // an indexed band: fixed codes, filter 0, its own segments
        const uint32_t rb = a.row_bytes - 1u;
        if (!rb || dyn || a.filter || a.nseg != png_idx_row_segments(rb) || a.slot_bytes != png_idx_slot_bytes(rb) ||
            (uint64_t)a.rows * a.row_bytes > 1ull << 30)
            throw Error{MARAY_E_INTERNAL, "device PNG encoder: bad indexed band arguments"};
    }
    if (a.filter > MARAY_PNG_FILTER_PAETH || (a.filter && !a.row_filter) || (a.filter == MARAY_PNG_FILTER_ADAPTIVE && (!a.cost || ((uintptr_t)a.cost & 3))))
        throw Error{MARAY_E_INTERNAL, "device PNG encoder: bad filter arguments"};
    if (!a.src || !a.slots || !a.lens || !a.adler || !a.offsets || !a.stream || !a.totals || !a.w || !a.rows ||
        (a.codes != MARAY_PNG_CODES_FIXED && !dyn) || (dyn && (!a.hist || a.header_bits > PNG_DYN_HEADER_MAX_BITS || ((uintptr_t)a.stream & 15))) ||
        (!a.row_bytes && (a.nseg != png_row_segments(a.w) || a.slot_bytes != (dyn ? png_slot_bytes_dyn(a.w) : png_slot_bytes(a.w)))) ||
        a.slot_bytes > (dyn ? PNG_SLOT_MAX_DYN : PNG_SLOT_MAX) ||
        (uint64_t)a.rows * a.nseg != a.n_segs || ((uintptr_t)a.slots & 15) ||
        (!a.row_bytes && (uint64_t)a.rows * (3ull * a.w + 1ull) > (dyn ? PNG_DYN_BAND_MAX_BYTES : 1ull << 30)))
        throw Error{MARAY_E_INTERNAL, "device PNG encoder: bad band arguments"};
}

}   // namespace

namespace {
// the rows' types into a.row_filter, in front of the band's first pass over its pixels
void band_filter(const PngBandArgs &a, hipStream_t st)
{
    if (a.filter != MARAY_PNG_FILTER_ADAPTIVE) {            // a forced type: PNG type filter - 1 in every row
        HIP_TRY(hipMemsetAsync(a.row_filter, (int)(a.filter - 1u), a.rows, st));
        return;
    }
    hipLaunchKernelGGL(maray_png_filter_cost, dim3((a.n_segs + FC_WAVES - 1) / FC_WAVES), dim3(FC_BLOCK), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(maray_png_filter_pick, dim3((a.rows + FC_WAVES - 1) / FC_WAVES), dim3(FC_BLOCK), 0, st, a);
    HIP_TRY(hipGetLastError());
}
}   // namespace

void png_band_compress(const PngBandArgs &a, hipStream_t st)
{
    check_band(a);
    (void)hipGetLastError();
    const bool f = a.filter != MARAY_PNG_FILTER_NONE;
    if (f && (a.codes != MARAY_PNG_CODES_DYNAMIC || !a.table)) band_filter(a, st);      // (a dynamic band's second pass finds them set)
    const dim3 segs((a.n_segs + PC_WAVES - 1) / PC_WAVES);
    if (a.codes == MARAY_PNG_CODES_DYNAMIC && !a.table) {
        const uint32_t blocks = png_hist_blocks(a.n_segs);
        if (f) hipLaunchKernelGGL(maray_png_histogram_filtered, dim3(blocks), dim3(HIST_BLOCK), 0, st, a);
        else hipLaunchKernelGGL(maray_png_histogram, dim3(blocks), dim3(HIST_BLOCK), 0, st, a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(maray_png_histogram_sum, dim3(1), dim3(HIST_SUM_BLOCK), 0, st, a.hist, blocks);
    } else if (a.codes == MARAY_PNG_CODES_DYNAMIC) {
        if (f) hipLaunchKernelGGL(maray_png_compress_dyn_filtered, segs, dim3(PC_BLOCK), 0, st, a);
        else hipLaunchKernelGGL(maray_png_compress_dyn, segs, dim3(PC_BLOCK), 0, st, a);
    } else if (f)
        hipLaunchKernelGGL(maray_png_compress_filtered, segs, dim3(PC_BLOCK), 0, st, a);
    else
        hipLaunchKernelGGL(maray_png_compress, segs, dim3(PC_BLOCK), 0, st, a);
    HIP_TRY(hipGetLastError());
}

void png_band_scan(const PngBandArgs &a, hipStream_t st)
{
    check_band(a);
    (void)hipGetLastError();
    hipLaunchKernelGGL(maray_png_scan, dim3(1), dim3(SCAN_BLOCK), 0, st, a);
    HIP_TRY(hipGetLastError());
}

void png_band_gather(const PngBandArgs &a, hipStream_t st)
{
    check_band(a);
    (void)hipGetLastError();
    if (a.codes == MARAY_PNG_CODES_DYNAMIC) {
        if (!a.table) throw Error{MARAY_E_INTERNAL, "device PNG encoder: a dynamic band is gathered after its code is set"};
        const uint64_t n16 = dyn_stream_cap(a.n_segs, a.slot_bytes) / 16;
        const uint32_t zb = (uint32_t)std::min<uint64_t>((n16 + ZERO_BLOCK - 1) / ZERO_BLOCK, ZERO_MAX_BLOCKS);
        hipLaunchKernelGGL(maray_png_zero, dim3(zb), dim3(ZERO_BLOCK), 0, st, a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(maray_png_gather_bits, dim3((a.n_segs + PC_WAVES - 1) / PC_WAVES), dim3(PC_BLOCK), 0, st, a);
    } else
        hipLaunchKernelGGL(maray_png_gather, dim3((a.n_segs + PC_WAVES - 1) / PC_WAVES), dim3(PC_BLOCK), 0, st, a);
    HIP_TRY(hipGetLastError());
}

}   // namespace maray
