// apng_device.hpp — the animation writer (include/maray_hip.h, "animation"): the kernels that find the bounding box of the
// pixels in which two RGB8 rasters in HBM differ (apng_device.hip), and the object that keeps two whole frames on a device,
// encodes of every frame after the first only that box through the device PNG encoder (png_device.hpp) and puts the streams
// into one APNG (apng_device.cpp; the container is png_container.hpp's).  Builds no program's kernels: not part of a code key.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

#include "expr.hpp"
#include "maray_hip.h"
#include "png_device.hpp"

namespace maray {

// maray_frame_delta: blocks of DELTA_BLOCK lanes, a lane takes 16 bytes per step, the grid is capped and strides
constexpr uint32_t DELTA_BLOCK = 256, DELTA_MAX_BLOCKS = 2048;
constexpr uint64_t APNG_FRAME_MAX_BYTES = (uint64_t)1 << 30;       // 3 w h of one frame: every byte index fits 32 bits

inline uint32_t frame_delta_blocks(size_t bytes)
{
    const size_t blocks = (bytes / 16 + DELTA_BLOCK - 1) / DELTA_BLOCK;
    return (uint32_t)std::min<size_t>(std::max<size_t>(blocks, 1), DELTA_MAX_BLOCKS);
}

// Two packed w x h RGB8 rasters (pitch 3 w, any byte alignment, independently; 3 w h <= APNG_FRAME_MAX_BYTES):
// d_box[0 .. 3] = x0, y0, x1, y1, the half-open bounding box of the pixels in which a byte differs, 0 0 0 0 when none does.
// d_partials: DELTA_MAX_BLOCKS x 4 words of scratch, 16-byte aligned.  Enqueues two kernels on st; throws Error.
void frame_delta(const unsigned char *d_prev, const unsigned char *d_cur, uint32_t w, uint32_t h, uint32_t *d_partials, uint32_t *d_box,
                 hipStream_t st);
// w, h within what frame_delta and the writer take (else Error MARAY_E_LIMIT), before anything is launched
void apng_check_frame(uint32_t w, uint32_t h);
// maray_hip_frame_delta: scratch of the call's own, enqueued on st and waited for
void frame_delta_once(int device, const unsigned char *d_prev, const unsigned char *d_cur, uint32_t w, uint32_t h, hipStream_t st, uint32_t box[4]);
// maray_hip_time_frame_delta: average ms of frame_delta over two w x h rasters of the call's own that differ in their two far
// corners; *copy_ms (may be null): a device-to-device hipMemcpyAsync of one raster's bytes, timed the same way in the same call
float frame_delta_time(int device, uint32_t w, uint32_t h, int reps, float *copy_ms);

// The rectangle a frame after the first is written with: the box, or 1 x 1 at (0, 0) for the empty one (APNG has no empty
// frame, and a SOURCE blend of an unchanged pixel changes nothing).  A box outside the canvas: Error MARAY_E_INTERNAL.
struct ApngRect { uint32_t x, y, w, h; };
inline ApngRect apng_rect(const uint32_t box[4], uint32_t w, uint32_t h)
{
    if (!box[0] && !box[1] && !box[2] && !box[3]) return ApngRect{0, 0, 1, 1};
    if (box[0] >= box[2] || box[1] >= box[3] || box[2] > w || box[3] > h) throw Error{MARAY_E_INTERNAL, "animation writer: the frames' box is outside the canvas"};
    return ApngRect{box[0], box[1], box[2] - box[0], box[3] - box[1]};
}

// delay_num, delay_den as the file holds them (u16; a denominator of 0 means 100), n_frames >= 1: else Error MARAY_E_ARG
void apng_check_timing(uint32_t n_frames, uint32_t delay_num, uint32_t delay_den);

// One animation on the encoder's device.  add_frame renders the next frame into the writer's `cur` raster in the encoder's
// band steps -- render(b0, b1, d8, st) enqueues rows [b0, b1) as packed RGB8 into d8 on st, encode_rendered's callback --
// and appends the frame's chunks: all rows for frame 0, else the rows and columns of the box of (cur != prev), cropped
// into the encoder's band buffer.  Every call waits for its own work.  finish() returns the file once n_frames were added.
struct ApngWriter {
    using Render = std::function<void(uint32_t, uint32_t, unsigned char *, hipStream_t)>;
    PngEncoder &E;
    const uint32_t w, h, n_frames, delay_num, delay_den;
    const uint32_t codes;                                // MARAY_PNG_CODES_*: how every frame's rows are coded (encode_rows)
    unsigned char *raster[2] = {nullptr, nullptr};      // prev and cur, swapped between frames
    uint32_t *d_partials = nullptr, *d_box = nullptr;    // one allocation
    uint32_t *h_box = nullptr;                           // pinned host
    uint32_t added = 0, seq = 0;
    std::vector<uint8_t> file;
    std::vector<ApngRect> rects;                         // per frame (measurements)

    ApngWriter(PngEncoder &enc, uint32_t w, uint32_t h, uint32_t n_frames, uint32_t delay_num, uint32_t delay_den, uint32_t n_plays,
               uint32_t codes = MARAY_PNG_CODES_FIXED);
    ~ApngWriter();
    ApngWriter(const ApngWriter &) = delete;
    void add_frame(const Render &render, hipStream_t st);
    std::vector<uint8_t> finish();
    void release();                                      // the device and pinned memory (the destructor's work)
};

// maray_hip_render_apng with the codes of every frame (api.cpp); with MARAY_PNG_CODES_FIXED exactly that call
int render_apng_codes(maray_ctx *c, uint32_t w, uint32_t h, const double *values, uint32_t n_images, uint32_t n_sub, uint32_t delay_num,
                      uint32_t delay_den, uint32_t n_plays, uint32_t codes, uint8_t **out, size_t *n_out);

}   // namespace maray
