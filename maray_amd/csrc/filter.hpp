// filter.hpp — the tent reconstruction filter of a supersampled render (include/maray_hip.h, "reconstruction filter"):
// a plain back-end of the supersampled program renders bands of the sample raster into scratch in HBM, and
// maray_filter_tent<K> (filter.hip) turns each band into output rows.  Builds no program's kernels: not part of a code key.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "backend.hpp"
#include "expr.hpp"
#include "maray_hip.h"

namespace maray {

constexpr uint32_t FILTER_TILE_W = 64, FILTER_TILE_H = 8;      // output pixels a block computes
constexpr size_t FILTER_PAD = 16;       // bytes in front of and behind a band that the kernel's dword loads may touch (never use)

inline bool filter_samples_ok(uint32_t k) { return k == 2 || k == 4 || k == 8; }

// One pass: output rows [oy0, oy0 + n_out) of a w-pixel-wide image from a band of its sample raster.  `src` is the first
// byte of sample row band_row0 (image coordinates); the band holds band_rows rows of sw * 3 bytes, which must cover
// [k oy0 - k/2, k (oy0 + n_out) + k/2) clipped to [0, sh); FILTER_PAD bytes in front of src and behind the band's last row
// are readable.  dst: n_out packed rows of w * 3 bytes, any alignment.
struct TentArgs {
    const unsigned char *src;
    unsigned char *dst;
    uint32_t w;                     // output width
    uint32_t sw, sh;                // the image's sample raster: k w x k h
    uint32_t band_row0, band_rows;
    uint32_t oy0, n_out;
};

void filter_tent(uint32_t k, const TentArgs &a, hipStream_t st);      // enqueues one pass; throws Error
float filter_time_tent(int device, uint32_t w, uint32_t rows, uint32_t k, int reps);     // maray_hip_time_filter

// Sample rows a filter's footprint reaches beyond [k y0, k y1) on either side: the box none, the tent k/2, Catmull-Rom 3k/2.
constexpr uint32_t filter_halo(uint32_t filter, uint32_t k)
{
    return filter == MARAY_FILTER_CATROM ? 3 * k / 2 : filter == MARAY_FILTER_TENT ? k / 2 : 0;
}

// MARAY_FILTER_CATROM (catrom.hip): maray_filter_catrom<K>, one pass with TentArgs as above but for the halo, which is 3k/2
// rows: the band must cover [k oy0 - 3k/2, k (oy0 + n_out) + 3k/2) clipped to [0, sh).  Its footprint is 12k bytes of a row
// from an aligned dword on: FILTER_PAD covers it as it covers the tent's.  A block's tile depends on k (32-bit sums in LDS);
// never lower than FILTER_TILE_H, so a band the tent's kernel takes in one pass this one takes too.
constexpr uint32_t catrom_tile_w(uint32_t k) { return k == 8 ? 32 : 64; }
constexpr uint32_t catrom_tile_h(uint32_t k) { return k == 2 ? 16 : 8; }
void filter_catrom(uint32_t k, const TentArgs &a, hipStream_t st);    // enqueues one pass; throws Error
float filter_time_catrom(int device, uint32_t w, uint32_t rows, uint32_t k, int reps);   // maray_hip_time_filter_ex

// The reduces in linear light (include/maray_hip.h, "transfer"; linear.hip): maray_filter_box_lin<K> and
// maray_filter_tent_lin<K>, one pass each with TentArgs as above.  The box has no halo: its band covers [k oy0, k (oy0 + n_out)).
// Blocks loop over tiles of rows, so a pass takes any number of rows.
void filter_lin(uint32_t filter, uint32_t k, const TentArgs &a, hipStream_t st);      // enqueues one pass; throws Error
float filter_time_lin(int device, uint32_t w, uint32_t rows, uint32_t k, uint32_t filter, int reps);     // maray_hip_time_filter_ex

// The context behind MARAY_FILTER_TENT and behind MARAY_TRANSFER_SRGB: takes over `inner`, a plain (samples = 1) back-end of
// the (supersampled) program on `device`.  k = 1 (SRGB only): nothing to filter, launches pass through; the wrapper is there
// for the shutter's linear reduce.  Also the context behind MARAY_FILTER_CATROM (transfer NONE only, k = 2, 4, 8).  Throws
// Error (then `inner` is still the caller's).
Backend *make_filter_backend(int device, Backend *inner, uint32_t k, uint32_t n_params, uint32_t filter = MARAY_FILTER_TENT,
                             uint32_t transfer = MARAY_TRANSFER_NONE);

}   // namespace maray
