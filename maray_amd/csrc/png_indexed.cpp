// png_indexed.cpp — the host's part of the indexed-colour form of the device PNG encoder (product code; include/maray_hip.h,
// "Indexed colour"): the encoder's colour scratch and index buffer, the palette's way to the host, the bands of an indexed
// file and its assembly.  A file of its own, so that the programs built from png_device.cpp alone need none of the kernels'
// launchers declared in png_indexed.hpp.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "backend.hpp"
#include "png_container.hpp"
#include "png_indexed.hpp"

namespace maray {

namespace {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            throw Error{MARAY_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)};           \
    } while (0)

size_t up16(size_t n) { return (n + 15) / 16 * 16; }

uint32_t *palette_of(PngEncoder &E) { return (uint32_t *)E.colors; }

// the scratch of an indexed band of `rows` rows of rb packed bytes at E.index (png_device.cpp's band_args)
PngBandArgs band_args_idx(PngEncoder &E, uint32_t w, uint32_t rb, uint32_t rows)
{
    PngBandArgs a{};
    a.src = E.index; a.w = w; a.rows = rows;
    a.row_bytes = rb + 1;
    a.nseg = png_idx_row_segments(rb);
    a.slot_bytes = png_idx_slot_bytes(rb);
    a.codes = MARAY_PNG_CODES_FIXED;
    const uint64_t n = (uint64_t)rows * a.nseg;
    if (n > 0x7FFFFFFFull) throw Error{MARAY_E_INTERNAL, "device PNG encoder: band too large"};
    a.n_segs = (uint32_t)n;
    const size_t payload = (size_t)n * a.slot_bytes;
    png_grow(E.slots, E.slots_cap, payload);
    png_grow(E.stream, E.stream_cap, payload);
    const size_t o_adler = up16((size_t)n * 4), o_off = o_adler + up16((size_t)n * 8), o_tot = o_off + up16((size_t)n * 8);
    png_grow(E.meta, E.meta_cap, o_tot + 32);
    a.slots = E.slots; a.stream = E.stream;
    a.lens = (uint32_t *)E.meta;
    a.adler = (uint32_t *)(E.meta + o_adler);
    a.offsets = (uint64_t *)(E.meta + o_off);
    a.totals = (uint64_t *)(E.meta + o_tot);
    return a;
}

void band_kernels(PngEncoder &E, const unsigned char *d_rgb8, uint32_t w, uint32_t n_colors, const PngBandArgs &a, hipStream_t st)
{
    png_index(d_rgb8, w, a.rows, palette_of(E), n_colors, png_idx_depth(n_colors), E.index, st);
    png_band_compress_idx(a, st);
    png_band_scan(a, st);
    png_band_gather(a, st);
}

// two events around a timed loop
struct Events {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    Events() { HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1)); }
    ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    Events(const Events &) = delete;
};

}   // namespace

void PngEncoder::collect_colors(const unsigned char *d_rgb8, uint64_t npix, hipStream_t st, bool add)
{
    if (!d_rgb8 || !npix) throw Error{MARAY_E_ARG, "null argument"};
    HIP_TRY(hipSetDevice(device));
    // (one size for every raster: growing would lose the palette of the bands before)
    png_grow(colors, colors_cap, up16(PNG_PALETTE_BYTES) + (size_t)PNG_COLORS_MAX_BLOCKS * PNG_COLORS_STRIDE * 4);
    png_colors(d_rgb8, npix, (uint32_t *)(colors + up16(PNG_PALETTE_BYTES)), palette_of(*this), add, st);
}

uint32_t PngEncoder::fetch_palette(hipStream_t st, uint8_t rgb[768])
{
    if (!colors) throw Error{MARAY_E_INTERNAL, "device PNG encoder: no colours were collected"};
    HIP_TRY(hipSetDevice(device));
    if (!h_palette) HIP_TRY(hipHostMalloc((void **)&h_palette, PNG_PALETTE_BYTES, hipHostMallocDefault));
    HIP_TRY(hipMemcpyAsync(h_palette, colors, PNG_PALETTE_BYTES, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    png_count_bytes_to_host(PNG_PALETTE_BYTES);
    const uint32_t n = h_palette[0];
    if (!n || n > PNG_PALETTE_MAX + 1) throw Error{MARAY_E_INTERNAL, "device PNG encoder: bad colour count"};
    for (uint32_t i = 0; i < n && i < PNG_PALETTE_MAX; i++) {
        const uint32_t c = h_palette[1 + i];
        rgb[3 * i] = (uint8_t)(c >> 16); rgb[3 * i + 1] = (uint8_t)(c >> 8); rgb[3 * i + 2] = (uint8_t)c;
    }
    return n;
}

void PngEncoder::encode_rows_indexed(const unsigned char *d_rgb8, uint32_t w, uint32_t rows, uint32_t n_colors, hipStream_t st, PngPiece &out)
{
    if (!rows || !w) return;
    if (!d_rgb8) throw Error{MARAY_E_ARG, "null argument"};
    if (!n_colors || n_colors > PNG_PALETTE_MAX || !colors) throw Error{MARAY_E_INTERNAL, "device PNG encoder: no palette"};
    HIP_TRY(hipSetDevice(device));
    const uint32_t rb = png_idx_row_bytes(w, png_idx_depth(n_colors));
    const uint32_t step = band_rows(w);
    for (uint32_t r0 = 0; r0 < rows; r0 += std::min(step, rows - r0)) {
        const uint32_t n = std::min(step, rows - r0);
        png_grow(index, index_cap, (size_t)n * rb);
        const PngBandArgs a = band_args_idx(*this, w, rb, n);
        band_kernels(*this, d_rgb8 + (size_t)r0 * w * 3, w, n_colors, a, st);
        HIP_TRY(hipMemcpyAsync(h_totals, a.totals, 24, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const uint64_t total = h_totals[0];
        if (total > (uint64_t)a.n_segs * a.slot_bytes) throw Error{MARAY_E_INTERNAL, "device PNG encoder: a band's stream exceeds its bound"};
        want_staging((size_t)total);
        HIP_TRY(hipMemcpyAsync(staging, a.stream, (size_t)total, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        out.z.insert(out.z.end(), staging, staging + (size_t)total);
        AdlerPart p;
        p.n = (uint32_t)(h_totals[1] & 0xFFFFFFFFu); p.a = (uint32_t)(h_totals[1] >> 32); p.b = (uint32_t)h_totals[2];
        out.adler.append(p);
        png_count_bytes_to_host(total + 24);
    }
}

std::vector<uint8_t> png_assemble_indexed(uint32_t w, uint32_t h, const uint8_t *palette, uint32_t n, const std::vector<const PngPiece *> &pieces)
{
    if (!palette || !n || n > PNG_PALETTE_MAX) throw Error{MARAY_E_INTERNAL, "device PNG encoder: a palette holds 1 to 256 colours"};
    if (!pieces.empty() && pieces.front()->y0 != 0) throw Error{MARAY_E_INTERNAL, "device PNG encoder: the pieces do not cover the image in row order"};
    const std::vector<uint8_t> z = png_close_stream(h, pieces);
    return png_file_indexed(w, h, png_idx_depth(n), palette, n, z.data(), z.size());
}

float png_time_kernels_color(int device, const unsigned char *d_rgb8, uint32_t w, uint32_t rows, uint32_t color, int reps, uint64_t *stream_bytes)
{
    if (color != MARAY_PNG_COLOR_INDEXED && color != MARAY_PNG_COLOR_AUTO) throw Error{MARAY_E_ARG, "unknown PNG color mode"};
    if (!d_rgb8 || !w || !rows || reps <= 0) throw Error{MARAY_E_ARG, "png_time_kernels: a raster, w, rows and reps > 0"};
    png_check_size(w, rows);
    if (((uint64_t)w * 3 + 1) * rows > (uint64_t)1 << 30) throw Error{MARAY_E_LIMIT, "png_time_kernels: more than one band's bytes"};
    uint8_t rgb[768];
    uint32_t n_colors;
    {
        PngEncoderLease E(device);
        E->collect_colors(d_rgb8, (uint64_t)w * rows, E->own_stream, false);
        n_colors = E->fetch_palette(E->own_stream, rgb);
    }
    if (n_colors > PNG_PALETTE_MAX) {
        if (color == MARAY_PNG_COLOR_INDEXED) throw Error{MARAY_E_LIMIT, "the raster holds more than 256 colours"};
        // the truecolour band, and the collection that led to it, timed apart and added (two runs of `reps`)
        const float tc = png_time_kernels(device, d_rgb8, w, rows, reps, stream_bytes);
        PngEncoderLease E(device);
        HIP_TRY(hipSetDevice(device));
        const hipStream_t st = E->own_stream;
        Events ev;
        E->collect_colors(d_rgb8, (uint64_t)w * rows, st, false);
        HIP_TRY(hipEventRecord(ev.e0, st));
        for (int i = 0; i < reps; i++) E->collect_colors(d_rgb8, (uint64_t)w * rows, st, false);
        HIP_TRY(hipEventRecord(ev.e1, st));
        HIP_TRY(hipStreamSynchronize(st));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
        return tc + ms / (float)reps;
    }
    PngEncoderLease E(device);
    HIP_TRY(hipSetDevice(device));
    const hipStream_t st = E->own_stream;
    const uint32_t rb = png_idx_row_bytes(w, png_idx_depth(n_colors));
    png_grow(E->index, E->index_cap, (size_t)rows * rb);
    const PngBandArgs a = band_args_idx(*E.e, w, rb, rows);
    Events ev;
    auto once = [&] { E->collect_colors(d_rgb8, (uint64_t)w * rows, st, false); band_kernels(*E.e, d_rgb8, w, n_colors, a, st); };
    once();
    HIP_TRY(hipEventRecord(ev.e0, st));
    for (int i = 0; i < reps; i++) once();
    HIP_TRY(hipEventRecord(ev.e1, st));
    HIP_TRY(hipMemcpyAsync(E->h_totals, a.totals, 24, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (stream_bytes) *stream_bytes = E->h_totals[0];
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    return ms / (float)reps;
}

}   // namespace maray
