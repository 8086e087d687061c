// apng_device.cpp — the object behind the animation entry points (product code; include/maray_hip.h, "animation"): over an
// encoder of the device PNG encoder it keeps two whole frames in HBM, has every frame rendered into one of them, finds the
// box in which it differs from the frame before (apng_device.hip), brings the box's 16 bytes to the host, crops the box's
// rows into the encoder's band buffer and has them encoded there; every frame's segments are closed into a zlib stream of
// their own (png_close_stream) and go into the container as IDAT (frame 0) or fdAT chunks (png_container.hpp).
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "apng_device.hpp"
#include "png_container.hpp"

namespace maray {

namespace {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            throw Error{MARAY_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)};           \
    } while (0)

}   // namespace

void apng_check_frame(uint32_t w, uint32_t h)
{
    png_check_size(w, h);
    if ((uint64_t)w * 3 * h > APNG_FRAME_MAX_BYTES) throw Error{MARAY_E_LIMIT, "frame too large for the animation writer: more than 2^30 bytes"};
}

void apng_check_timing(uint32_t n_frames, uint32_t delay_num, uint32_t delay_den)
{
    if (!n_frames) throw Error{MARAY_E_ARG, "an animation needs at least one image"};
    if (delay_num > 65535 || delay_den > 65535) throw Error{MARAY_E_ARG, "delay_num and delay_den must fit 16 bits"};
}

ApngWriter::ApngWriter(PngEncoder &enc, uint32_t w_, uint32_t h_, uint32_t n_frames_, uint32_t delay_num_, uint32_t delay_den_, uint32_t n_plays,
                       uint32_t codes_)
    : E(enc), w(w_), h(h_), n_frames(n_frames_), delay_num(delay_num_), delay_den(delay_den_), codes(codes_)
{
    if (codes != MARAY_PNG_CODES_FIXED && codes != MARAY_PNG_CODES_DYNAMIC) throw Error{MARAY_E_ARG, "unknown PNG codes"};
    apng_check_timing(n_frames, delay_num, delay_den);
    if (!w || !h) throw Error{MARAY_E_ARG, "empty image"};
    apng_check_frame(w, h);
    HIP_TRY(hipSetDevice(E.device));
    const size_t bytes = (size_t)w * 3 * h;
    try {
        HIP_TRY(hipMalloc((void **)&raster[0], bytes));
        if (n_frames > 1) {
            HIP_TRY(hipMalloc((void **)&raster[1], bytes));
            HIP_TRY(hipMalloc((void **)&d_partials, (size_t)DELTA_MAX_BLOCKS * 16 + 16));
            d_box = d_partials + 4 * (size_t)DELTA_MAX_BLOCKS;
            HIP_TRY(hipHostMalloc((void **)&h_box, 16, hipHostMallocDefault));
        }
    } catch (...) {
        release();
        throw;
    }
    apng_begin(file, w, h, n_frames, n_plays);
}

ApngWriter::~ApngWriter() { release(); }

void ApngWriter::release()
{
    (void)hipSetDevice(E.device);
    (void)hipFree(raster[0]); (void)hipFree(raster[1]); (void)hipFree(d_partials);
    if (h_box) (void)hipHostFree(h_box);
    raster[0] = raster[1] = nullptr; d_partials = nullptr; h_box = nullptr;
}

void ApngWriter::add_frame(const Render &render, hipStream_t st)
{
    if (added >= n_frames) throw Error{MARAY_E_INTERNAL, "animation writer: more frames than announced"};
    HIP_TRY(hipSetDevice(E.device));
    unsigned char *cur = raster[added & 1u], *prev = raster[(added & 1u) ^ 1u];
    const uint32_t step = E.band_rows(w);
    for (uint32_t b0 = 0; b0 < h; b0 += std::min(step, h - b0)) {
        const uint32_t b1 = b0 + std::min(step, h - b0);
        render(b0, b1, cur + (size_t)b0 * w * 3, st);
        HIP_TRY(hipSetDevice(E.device));
    }
    PngPiece piece;
    ApngRect r{0, 0, w, h};
    if (added) {
        frame_delta(prev, cur, w, h, d_partials, d_box, st);
        HIP_TRY(hipMemcpyAsync(h_box, d_box, 16, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        png_count_bytes_to_host(16);
        r = apng_rect(h_box, w, h);
    }
    piece.y0 = 0; piece.y1 = r.h;
    if (r.w == w)
        E.encode_rows(cur + (size_t)r.y * w * 3, w, r.h, st, piece, codes);      // whole rows are packed already
    else {
        // the box's rows, cropped band by band: encode_rows wants packed rows of the box's width
        const uint32_t bstep = E.band_rows(r.w, codes);
        unsigned char *band = E.band_buffer((size_t)std::min(bstep, r.h) * r.w * 3);
        for (uint32_t y = 0; y < r.h; y += std::min(bstep, r.h - y)) {
            const uint32_t rows = std::min(bstep, r.h - y);
            HIP_TRY(hipMemcpy2DAsync(band, (size_t)r.w * 3, cur + ((size_t)(r.y + y) * w + r.x) * 3, (size_t)w * 3, (size_t)r.w * 3, rows,
                                     hipMemcpyDeviceToDevice, st));
            E.encode_rows(band, r.w, rows, st, piece, codes);
        }
    }
    const std::vector<uint8_t> z = png_close_stream(r.h, {&piece});
    apng_fctl(file, seq, r.w, r.h, r.x, r.y, delay_num, delay_den);
    if (added) apng_fdat(file, seq, z.data(), z.size());
    else apng_idat(file, z.data(), z.size());
    rects.push_back(r);
    added++;
}

std::vector<uint8_t> ApngWriter::finish()
{
    if (added != n_frames) throw Error{MARAY_E_INTERNAL, "animation writer: fewer frames than announced"};
    apng_end(file);
    return std::move(file);
}

}   // namespace maray
