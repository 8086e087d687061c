// png_device.hpp — the device PNG encoder (include/maray_hip.h, "device PNG encoder"): the kernels that turn RGB8 rows in HBM
// into the segments of a zlib stream (png_device.hip) and the object that owns their scratch, brings the compressed bytes
// to the host and wraps them in the container (png_device.cpp).  Builds no program's kernels: not part of a code key.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

#include "expr.hpp"
#include "maray_hip.h"

namespace maray {

constexpr uint32_t PNG_SEG = 256;             // pixels per segment (SEG of the stream contract)
constexpr uint32_t PNG_ADLER_MOD = 65521;

// A segment of n filtered bytes occupies at most ceil(9 n / 8) + 16 bytes; a slot is that for the image's longest segment,
// rounded up to 16 (the kernels store and load whole dwords).
inline uint32_t png_slot_bytes(uint32_t w)
{
    const uint32_t n = 3 * (w < PNG_SEG ? w : PNG_SEG) + 1;
    return ((9 * n + 7) / 8 + 16 + 15) / 16 * 16;
}
constexpr uint32_t PNG_SLOT_MAX = ((9 * (3 * PNG_SEG + 1) + 7) / 8 + 16 + 15) / 16 * 16;
inline uint32_t png_row_segments(uint32_t w) { return (w + PNG_SEG - 1) / PNG_SEG; }

// ---- dynamic-Huffman codes (MARAY_PNG_CODES_DYNAMIC): the same tokens, one dynamic block per band --------------------------
// A segment of n filtered bytes is at most 15 n bits: ceil(15 n / 8) bytes, rounded up to 16 like the fixed coder's slot.
inline uint32_t png_slot_bytes_dyn(uint32_t w)
{
    const uint32_t n = 3 * (w < PNG_SEG ? w : PNG_SEG) + 1;
    return ((15 * n + 7) / 8 + 15) / 16 * 16;
}
constexpr uint32_t PNG_SLOT_MAX_DYN = ((15 * (3 * PNG_SEG + 1) + 7) / 8 + 15) / 16 * 16;
constexpr uint64_t PNG_DYN_BAND_MAX_BYTES = (uint64_t)1 << 28;    // filtered bytes of a dynamic band: every bit offset fits 32 bits
constexpr uint32_t PNG_LIT_SYMS = 286, PNG_DIST_SYMS = 30;
constexpr uint32_t PNG_DYN_HEADER_MAX_BITS = 17 + 19 * 3 + (PNG_LIT_SYMS + PNG_DIST_SYMS) * 7;    // no run symbols: 2286
// maray_png_histogram: blocks of PNG_HIST_WAVES wavefronts, one segment per wavefront and pass; the grid is capped at
// PNG_HIST_MAX_BLOCKS and strides over the band's segments.  Every block stores PNG_HIST_STRIDE words of partial counts.
constexpr uint32_t PNG_HIST_WAVES = 4, PNG_HIST_MAX_BLOCKS = 512, PNG_HIST_STRIDE = 288;
inline uint32_t png_hist_blocks(uint32_t n_segs)
{
    const uint32_t b = (n_segs + PNG_HIST_WAVES - 1) / PNG_HIST_WAVES;
    return b < 1 ? 1 : b > PNG_HIST_MAX_BLOCKS ? PNG_HIST_MAX_BLOCKS : b;
}

// What a run of segments contributes to the Adler-32, as an element of a monoid: n bytes with A = sum b_i and
// B = sum (n - i) b_i, all three modulo 65521.  (s1, s2) after the run = (s1 + A, s2 + n s1 + B).
struct AdlerPart {
    uint32_t n = 0, a = 0, b = 0;
    void append(const AdlerPart &r) {        // this run followed by r
        b = (uint32_t)(((uint64_t)b + (uint64_t)r.n * a + r.b) % PNG_ADLER_MOD);
        a = (a + r.a) % PNG_ADLER_MOD;
        n = (n + r.n) % PNG_ADLER_MOD;
    }
};

// One band: `rows` rows of w pixels at src (packed RGB8, any alignment), segment j = row j / nseg, pixels
// (j % nseg) * PNG_SEG ...  All pointers are the encoder's scratch.
struct PngBandArgs {
    const unsigned char *src;
    unsigned char *slots;           // n_segs slots of slot_bytes each, 16-byte aligned
    uint32_t *lens;                 // per segment: bytes of its slot in use
    uint32_t *adler;                // per segment: its shares of the band's Adler part, modulo 65521: A, and B + A x (the band's
                                    // bytes after the segment); the band's part is their sums
    uint64_t *offsets;              // per group of segments (png_device.hip: 64 or more, at most 1024 groups): where its first
                                    // segment starts in the gathered stream
    unsigned char *stream;          // the gathered stream
    uint64_t *totals;               // [0] = bytes of the stream, [1] = n | a << 32, [2] = b: the band's AdlerPart
    uint32_t w, rows, nseg, slot_bytes;
    uint32_t n_segs;                // rows * nseg
    // MARAY_PNG_CODES_DYNAMIC (else all zero): lens and offsets count BITS, totals[0] is the band's bits, slots are
    // png_slot_bytes_dyn wide and the stream starts with header_bits zero bits for the host's block header
    uint32_t codes;                 // MARAY_PNG_CODES_*
    uint32_t header_bits;           // bits of the block header in front of the first token; 0 while the band is being counted
    uint32_t *hist;                 // png_hist_blocks(n_segs) x PNG_HIST_STRIDE partial counts, then PNG_HIST_STRIDE words: their sums
    const uint32_t *table;          // PNG_LIT_SYMS words: reversed code | length << 16; null while the band is being counted
    // Row filters (MARAY_PNG_FILTER_*; with MARAY_PNG_FILTER_NONE all zero, and the kernels launched are the ones above)
    uint32_t filter;                // MARAY_PNG_FILTER_*: the option, not a PNG filter type
    uint8_t *row_filter;            // per row of the band: its PNG filter type 0 .. 4
    const unsigned char *above;     // the 3 w bytes of the row above the band's first row; null: the band starts at row 0
    uint32_t *cost;                 // MARAY_PNG_FILTER_ADAPTIVE: per segment and type t, [10 seg + 2 t] = the bytes and
                                    // [10 seg + 2 t + 1] = the token bits of the segment as a fixed-Huffman segment under t
    // Indexed colour (png_indexed.hpp; else 0): src holds rows of row_bytes - 1 packed index bytes, nseg and slot_bytes are
    // png_idx_row_segments and png_idx_slot_bytes of that, and a row has row_bytes filtered bytes instead of 3 w + 1
    uint32_t row_bytes;
};
// The launchers dispatch on a.codes.  FIXED: maray_png_compress, maray_png_scan, maray_png_gather.  DYNAMIC: compress is
// maray_png_histogram + maray_png_histogram_sum while a.table is null and maray_png_compress_dyn once it is set; scan is
// maray_png_scan; gather is maray_png_zero + maray_png_gather_bits.
// With a.filter set, png_band_compress first fills a.row_filter in the band's first pass (FIXED: the only one; DYNAMIC: the
// counting pass) -- ADAPTIVE: maray_png_filter_cost (per segment, the five types' costs) and maray_png_filter_pick (per row,
// the smallest (bytes, bits, type)); a forced type: the constant -- and launches the filtered forms
// maray_png_compress_filtered, maray_png_histogram_filtered and maray_png_compress_dyn_filtered.  Scan and gather are the
// same kernels.
void png_band_compress(const PngBandArgs &a, hipStream_t st);
void png_band_scan(const PngBandArgs &a, hipStream_t st);
void png_band_gather(const PngBandArgs &a, hipStream_t st);

// The host's part of a dynamic band (png_device.cpp; maray_png_dynamic_codes is the public form of the first).
// table[s] = the canonical code of literal/length symbol s, bit-reversed for the LSB-first stream, | length << 16
void png_dynamic_table(const uint8_t lit_lens[PNG_LIT_SYMS], uint32_t table[PNG_LIT_SYMS]);
// z holds, from byte `base` on, `bits` bits of a band (header and tokens) and nothing behind them: appends symbol 256
// (table[256]) and the empty stored block that ends on a byte boundary (three zero bits, zeros to the byte, 00 00 FF FF)
void png_dynamic_close(std::vector<uint8_t> &z, uint64_t bits, uint32_t code256, size_t base = 0);

// The compressed segments of rows [y0, y1) of an image, on the host, with their Adler part
struct PngPiece {
    uint32_t y0 = 0, y1 = 0;
    std::vector<uint8_t> z;
    AdlerPart adler;
};

// Scratch, staging and a stream of one device.  One call at a time; every call waits for its own work before it returns, so
// the scratch is idle between calls whatever streams they ran on.
struct PngEncoder {
    int device = 0;
    uint32_t band_rows_env = 0;               // MARAY_PNG_BAND_ROWS when the encoder was created (0: the byte budget)
    size_t band_bytes = (size_t)64 << 20;     // raster bytes of one band
    hipStream_t own_stream = nullptr;         // for callers that bring none (maray_hip_render_png, gen)
    unsigned char *slots = nullptr; size_t slots_cap = 0;
    unsigned char *stream = nullptr; size_t stream_cap = 0;
    unsigned char *meta = nullptr; size_t meta_cap = 0;         // lens, adler, offsets, totals
    unsigned char *raster = nullptr; size_t raster_cap = 0;     // a band's rows, for the rendering entry points
    unsigned char *filt = nullptr; size_t filt_cap = 0;         // row filters: the rows' types, then the segments' costs
    unsigned char *carry = nullptr; size_t carry_cap = 0;       // row filters: the row above the band being rendered
    unsigned char *staging = nullptr; size_t staging_cap = 0;   // pinned host
    uint64_t *h_totals = nullptr;                                // pinned host, 3 words

    explicit PngEncoder(int dev);
    ~PngEncoder();
    PngEncoder(const PngEncoder &) = delete;
    uint32_t *h_counts = nullptr;                                // pinned host: PNG_HIST_STRIDE counts down, PNG_LIT_SYMS table words up
    uint32_t band_rows(uint32_t w, uint32_t codes = MARAY_PNG_CODES_FIXED) const;
    unsigned char *band_buffer(size_t bytes);                    // `raster`, grown to hold `bytes` (the animation writer's crops)
    // rows x w pixels at d_rgb8 (device memory, any alignment), enqueued on st and waited for; appends to `out`
    // filter: MARAY_PNG_FILTER_*; above: the 3 w bytes of the row above the first one in device memory (null: that is row 0 of
    // the image); later bands of the call read the row above them in d_rgb8 itself
    void encode_rows(const unsigned char *d_rgb8, uint32_t w, uint32_t rows, hipStream_t st, PngPiece &out, uint32_t codes = MARAY_PNG_CODES_FIXED,
                     uint32_t filter = MARAY_PNG_FILTER_NONE, const unsigned char *above = nullptr);
    // rows [y0, y1) band by band: render(b0, b1, d8, st) enqueues the rows' RGB8 into d8 on st.  With a filter (y0 = 0 only)
    // the last row of a band is kept in `carry` for the next one.
    void encode_rendered(uint32_t w, uint32_t y0, uint32_t y1, hipStream_t st,
                         const std::function<void(uint32_t, uint32_t, unsigned char *, hipStream_t)> &render, PngPiece &out,
                         uint32_t codes = MARAY_PNG_CODES_FIXED, uint32_t filter = MARAY_PNG_FILTER_NONE);
    void want_staging(size_t bytes);                             // `staging`, grown to hold `bytes`

    // ---- indexed colour (png_indexed.hpp; the methods are png_indexed.cpp's) ----
    unsigned char *index = nullptr; size_t index_cap = 0;       // a band's packed index rows
    unsigned char *colors = nullptr; size_t colors_cap = 0;     // the palette (1 + 256 words), then the collecting blocks' slabs
    uint32_t *h_palette = nullptr;                               // pinned host: 1 + 256 words
    // the distinct colours of npix pixels at d_rgb8 into the encoder's palette, enqueued on st; add: to the ones it holds
    void collect_colors(const unsigned char *d_rgb8, uint64_t npix, hipStream_t st, bool add);
    // waits for st and brings the palette to the host (1,028 bytes): the number of colours, 257 for more than 256, and for up
    // to 256 their R, G, B in ascending order
    uint32_t fetch_palette(hipStream_t st, uint8_t rgb[768]);
    // encode_rows for an indexed file: the rows' indices into the palette the encoder holds (n_colors of them), packed and
    // compressed band by band
    void encode_rows_indexed(const unsigned char *d_rgb8, uint32_t w, uint32_t rows, uint32_t n_colors, hipStream_t st, PngPiece &out);
};
// p, grown to `want` bytes of device memory (what it held is gone)
void png_grow(unsigned char *&p, size_t &cap, size_t want);

// An encoder of `device`: one an earlier call left, or a new one (MARAY_PNG_BAND_ROWS is read here: a kept encoder made
// under another value is not handed out).  release() keeps up to two per device for the next call.
PngEncoder *png_encoder_acquire(int device);
void png_encoder_release(PngEncoder *e);
struct PngEncoderLease {
    PngEncoder *e;
    explicit PngEncoderLease(int device) : e(png_encoder_acquire(device)) {}
    ~PngEncoderLease() { png_encoder_release(e); }
    PngEncoderLease(const PngEncoderLease &) = delete;
    PngEncoder *operator->() const { return e; }
};

// bytes the process' encoders have copied to the host so far: payloads and totals (measurements)
uint64_t png_bytes_to_host();
// w, h within what the writers take (else Error MARAY_E_LIMIT), before anything is launched
void png_check_size(uint32_t w, uint32_t h);
// payload bytes another writer on an encoder's device has copied to the host (the animation writer's boxes)
void png_count_bytes_to_host(uint64_t n);
// The zlib stream of rows [pieces.front()->y0, h_end) : 78 01, the pieces' segments in row order (each starts where the one
// before it ended, the last ends at h_end), the final empty stored block, the Adler-32 combined from the pieces' parts.
std::vector<uint8_t> png_close_stream(uint32_t h_end, const std::vector<const PngPiece *> &pieces);
// The file: png_close_stream of pieces that cover [0, h), in the container (png_container.hpp).
std::vector<uint8_t> png_assemble(uint32_t w, uint32_t h, const std::vector<const PngPiece *> &pieces);
// The indexed file (png_indexed.cpp): the same stream around pieces of packed index rows, the palette's n colours in PLTE
std::vector<uint8_t> png_assemble_indexed(uint32_t w, uint32_t h, const uint8_t *palette, uint32_t n, const std::vector<const PngPiece *> &pieces);
// png_time_kernels with a colour mode other than MARAY_PNG_COLOR_RGB (png_indexed.cpp): the colour kernels, then the indexed
// band's or, for MARAY_PNG_COLOR_AUTO on more than 256 colours, the truecolour band's; the palette is fetched once, untimed
float png_time_kernels_color(int device, const unsigned char *d_rgb8, uint32_t w, uint32_t rows, uint32_t color, int reps, uint64_t *stream_bytes);
// Average ms of compress + scan + gather over the caller's w x rows raster in device memory, as one band (measurements);
// *stream_bytes = the bytes of the gathered stream.
// With DYNAMIC codes the six kernels of a band whose code is fitted once, before the timed loop (the host's round trip is
// not a kernel); *stream_bytes = the bytes of the band's piece.
// With a filter the kernels that set the rows' types are timed with the rest.
float png_time_kernels(int device, const unsigned char *d_rgb8, uint32_t w, uint32_t rows, int reps, uint64_t *stream_bytes,
                       uint32_t codes = MARAY_PNG_CODES_FIXED, uint32_t filter = MARAY_PNG_FILTER_NONE);
inline bool png_filter_known(uint32_t f) { return f <= MARAY_PNG_FILTER_PAETH; }

}   // namespace maray
