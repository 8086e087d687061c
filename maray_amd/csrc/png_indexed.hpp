// png_indexed.hpp — the indexed-colour form of the device PNG encoder (include/maray_hip.h, "Indexed colour"): the kernels that
// collect a raster's distinct colours, turn RGB8 rows into packed palette indices and tokenise the packed bytes
// (png_indexed.hip).  The scan and the gather are png_device.hip's; the encoder object is png_device.cpp's.  Builds no
// program's kernels: not part of a code key.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "png_device.hpp"

namespace maray {

constexpr uint32_t PNG_IDX_SEG = 768;          // packed bytes per segment: with the filter byte 769, the truecolour maximum
constexpr uint32_t PNG_PALETTE_MAX = 256;      // colours of a palette; a count of PNG_PALETTE_MAX + 1 says "more"

inline uint32_t png_idx_depth(uint32_t n) { return n <= 2 ? 1 : n <= 4 ? 2 : n <= 16 ? 4 : 8; }
inline uint32_t png_idx_row_bytes(uint32_t w, uint32_t depth) { return (uint32_t)(((uint64_t)w * depth + 7) / 8); }      // rb
inline uint32_t png_idx_row_segments(uint32_t rb) { return (rb + PNG_IDX_SEG - 1) / PNG_IDX_SEG; }
// the slot of a row's longest segment: png_slot_bytes' bound on min(rb, PNG_IDX_SEG) + 1 filtered bytes
inline uint32_t png_idx_slot_bytes(uint32_t rb)
{
    const uint32_t n = (rb < PNG_IDX_SEG ? rb : PNG_IDX_SEG) + 1;
    return ((9 * n + 7) / 8 + 16 + 15) / 16 * 16;
}
static_assert(((9 * (PNG_IDX_SEG + 1) + 7) / 8 + 16 + 15) / 16 * 16 == PNG_SLOT_MAX, "an indexed segment fits the truecolour slot");

// maray_png_colors: blocks of PNG_COLORS_BLOCK lanes, PNG_COLORS_LANE_PIXELS pixels a lane and pass; the grid is capped at
// PNG_COLORS_MAX_BLOCKS and strides over the raster.  Every block stores PNG_COLORS_STRIDE words: its count, then its colours.
constexpr uint32_t PNG_COLORS_BLOCK = 256, PNG_COLORS_LANE_PIXELS = 4, PNG_COLORS_MAX_BLOCKS = 512;
constexpr uint32_t PNG_COLORS_STRIDE = 1 + PNG_PALETTE_MAX;
constexpr uint32_t PNG_COLORS_SET = 2048;      // slots of the colour set in LDS (maray_png_colors, maray_png_colors_merge)
constexpr uint32_t PNG_INDEX_TABLE = 1024;     // slots of the palette's lookup table in LDS (maray_png_index)
constexpr uint32_t PNG_INDEX_BLOCK = 256, PNG_INDEX_MAX_BLOCKS = 1024;
// every lane of a block may insert its pixels after the count was last seen at PNG_PALETTE_MAX: the set holds them all
static_assert(PNG_COLORS_SET >= PNG_PALETTE_MAX + PNG_COLORS_BLOCK * PNG_COLORS_LANE_PIXELS, "the set never fills up");
inline uint32_t png_colors_blocks(uint64_t npix)
{
    const uint64_t per = (uint64_t)PNG_COLORS_BLOCK * PNG_COLORS_LANE_PIXELS, b = (npix + per - 1) / per;
    return b < 1 ? 1u : b > PNG_COLORS_MAX_BLOCKS ? PNG_COLORS_MAX_BLOCKS : (uint32_t)b;
}
// A palette in device memory is 1 + PNG_PALETTE_MAX words: the count (PNG_PALETTE_MAX + 1: more; the rest is then unspecified)
// and the colours as R << 16 | G << 8 | B, ascending.
constexpr size_t PNG_PALETTE_BYTES = 4 * (1 + PNG_PALETTE_MAX);

// The distinct colours of npix packed RGB8 pixels at src (any alignment) into `palette`: maray_png_colors into `slabs`
// (png_colors_blocks(npix) x PNG_COLORS_STRIDE words), then maray_png_colors_merge, which also takes the colours `palette`
// already holds when `add` is set (the bands of one image).
void png_colors(const unsigned char *src, uint64_t npix, uint32_t *slabs, uint32_t *palette, bool add, hipStream_t st);
// rows x w pixels at src -> rows of png_idx_row_bytes(w, depth) packed bytes at dst (no gap between rows): maray_png_index
// with the n colours of `palette`
void png_index(const unsigned char *src, uint32_t w, uint32_t rows, const uint32_t *palette, uint32_t n, uint32_t depth, unsigned char *dst,
               hipStream_t st);
// maray_png_compress_idx on a band whose a.src holds packed index rows and whose a.row_bytes = rb + 1; then png_band_scan and
// png_band_gather as for a truecolour band
void png_band_compress_idx(const PngBandArgs &a, hipStream_t st);

}   // namespace maray
