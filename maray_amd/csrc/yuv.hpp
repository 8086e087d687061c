// yuv.hpp — RGB8 -> limited-range Y'CbCr planes on the device (include/maray_hip.h, "raw video"): the conversion kernel's
// launch constants and host entry points (yuv.hip).  Builds no program's kernels: not part of a code key.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "expr.hpp"
#include "maray_hip.h"

namespace maray {

// maray_rgb_to_ycc: a lane takes YCC_LANE_PIXELS adjacent pixels of two rows, a wavefront YCC_WAVE_PIXELS of them, a block of
// YCC_BLOCK lanes a tile of YCC_BLOCK_PIXELS x YCC_BLOCK_ROWS pixels (its wavefronts lie under each other); the grid is capped
// at YCC_MAX_BLOCKS and blocks stride over the tiles
constexpr uint32_t YCC_BLOCK = 256, YCC_LANE_PIXELS = 8, YCC_MAX_BLOCKS = 2048;
constexpr uint32_t YCC_WAVE_PIXELS = 64 * YCC_LANE_PIXELS;
constexpr uint32_t YCC_BLOCK_PIXELS = YCC_WAVE_PIXELS, YCC_BLOCK_ROWS = 2 * (YCC_BLOCK / 64);
constexpr uint64_t YCC_FRAME_MAX_BYTES = (uint64_t)1 << 30;        // 3 w h of one frame: every byte index fits 32 bits

inline uint32_t ycc_tiles_x(uint32_t w) { return (w + YCC_BLOCK_PIXELS - 1) / YCC_BLOCK_PIXELS; }
inline uint32_t ycc_tiles_y(uint32_t h) { return (h + YCC_BLOCK_ROWS - 1) / YCC_BLOCK_ROWS; }
inline uint32_t ycc_blocks(uint32_t w, uint32_t h)
{
    const uint64_t tiles = (uint64_t)ycc_tiles_x(w) * ycc_tiles_y(h);
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(tiles, 1), YCC_MAX_BLOCKS);
}

// the option words of a maray_ycc_opts (null: the defaults); an unknown word or a reserved one that is not 0: Error MARAY_E_ARG
void ycc_opts_words(const maray_ycc_opts *opts, uint32_t *sampling, uint32_t *matrix);
// w, h > 0 (else MARAY_E_ARG), within MARAY_DOMAIN_MAX and 3 w h <= YCC_FRAME_MAX_BYTES (else MARAY_E_LIMIT)
void ycc_check_frame(uint32_t w, uint32_t h);
// bytes of the three planes of one frame: w h + 2 cw ch
inline size_t ycc_frame_bytes(uint32_t w, uint32_t h, uint32_t sampling)
{
    const size_t cw = sampling == MARAY_YCC_444 ? w : ((size_t)w + 1) / 2, ch = sampling == MARAY_YCC_444 ? h : ((size_t)h + 1) / 2;
    return (size_t)w * h + 2 * cw * ch;
}

// One packed w x h RGB8 raster (pitch 3 w, any alignment) -> Y', Cb, Cr packed one after the other at d_planes (any
// alignment): one kernel enqueued on st of the current device, nothing waited for.  Only dwords that hold a byte of the
// raster are read: the buffers need no pad.  Throws Error.
void rgb_to_ycc(const unsigned char *d_rgb, uint32_t w, uint32_t h, uint32_t sampling, uint32_t matrix, unsigned char *d_planes, hipStream_t st);
// maray_hip_time_rgb_to_ycc: average ms of the kernel over a raster of the call's own; *copy_ms (may be null): a
// device-to-device hipMemcpyAsync that moves as many bytes (it copies half of 3 w h + the planes' bytes), in the same call
float rgb_to_ycc_time(int device, uint32_t w, uint32_t h, uint32_t sampling, uint32_t matrix, int reps, float *copy_ms);

}   // namespace maray
