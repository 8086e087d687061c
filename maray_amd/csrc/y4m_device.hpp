// y4m_device.hpp — the raw-video writer (include/maray_hip.h, "raw video"): the object that turns the frames of an
// animation into one YUV4MPEG2 stream -- every frame converted to Y'CbCr planes on the device (yuv.hpp), copied to pinned
// host memory on a copy stream and handed to a sink while the next frame renders (y4m_device.cpp).  The animation twin of
// apng_device.hpp without an encoder: it creates no PNG encoder.  Builds no program's kernels: not part of a code key.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>

#include "expr.hpp"
#include "maray_hip.h"
#include "yuv.hpp"

namespace maray {

// n_frames >= 1, delay_num in 1 .. 65535, delay_den in 0 .. 65535: else Error MARAY_E_ARG
void y4m_check_timing(uint32_t n_frames, uint32_t delay_num, uint32_t delay_den);
// the header line: fn:fd = delay_den:delay_num, delay_den = 0 meaning 100, not reduced
std::string y4m_header(uint32_t w, uint32_t h, uint32_t delay_num, uint32_t delay_den, uint32_t sampling);

// One animation on one device.  add_frame enqueues the conversion of a packed RGB8 raster in device memory on st, then the
// planes' copy to pinned host memory on the writer's copy stream behind an event, and hands the frame BEFORE it -- whose copy
// ran meanwhile -- to the sink; finish() hands over the last one.  The sink gets the header line with the first frame, so a
// failure before any frame is ready writes nothing.  raster() is a w x h RGB8 raster of the writer's to render into: the
// conversion that reads it and the next render that overwrites it are ordered by st, which must be the same for every frame.
struct Y4mWriter {
    using Sink = std::function<void(const void *, size_t)>;
    const int device;
    const uint32_t w, h, n_frames, sampling, matrix;
    const size_t frame_bytes;
    Sink sink;
    std::string header;
    unsigned char *d_rgb = nullptr;                     // raster(), allocated on demand
    unsigned char *d_planes[2] = {nullptr, nullptr};
    unsigned char *h_planes[2] = {nullptr, nullptr};    // pinned host
    hipStream_t copy_st = nullptr;
    hipEvent_t converted[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr};
    uint32_t added = 0, written = 0;

    Y4mWriter(int device, uint32_t w, uint32_t h, uint32_t n_frames, uint32_t delay_num, uint32_t delay_den, uint32_t sampling, uint32_t matrix, Sink sink);
    ~Y4mWriter();
    Y4mWriter(const Y4mWriter &) = delete;
    unsigned char *raster();
    void add_frame(const unsigned char *d_rgb8, hipStream_t st);
    void finish();
    void release();                                      // waits for the copy stream; the device and pinned memory (the destructor's work)

private:
    void write_one();                                    // frame `written`: waits for its copy
};

// The stream a context's frames are rendered and converted on: one per device, created at the first call and kept for the
// life of the process.  (A back-end remembers the stream of its last launch and records an event on it when the next launch
// comes on another one, so a stream handed to render_device* must outlive the context: never one of a single call's.)
hipStream_t y4m_render_stream(int device);

// maray_hip_render_y4m into a sink (api.cpp): maray_gen_animation_ex's way in
int render_y4m_to(maray_ctx *c, uint32_t w, uint32_t h, const double *values, uint32_t n_images, uint32_t n_sub, uint32_t delay_num,
                  uint32_t delay_den, const maray_ycc_opts *opts, const Y4mWriter::Sink &sink);

}   // namespace maray
