// apng_asan.cpp — host-only sanitizer harness for the animation writer's host code (test infrastructure).
// Built with -fsanitize=address,undefined together with maray_amd/csrc/apng_device.cpp, png_device.cpp and png.cpp; needs no device and
// launches nothing (the kernel launchers are stubs that fail).  It plays the device's part on the host -- a rectangle's
// filtered bytes as stored deflate blocks ended by the sync flush, the Adler part from per-row shares as the kernels form
// them -- and drives the stream-closing helper (png_close_stream), the APNG container writer of png_container.hpp, with the
// chunk limit lowered so that streams split into several IDAT / fdAT chunks, and the box-to-rectangle logic (apng_rect),
// the empty box included.  Every file is taken apart again here: CRCs, sequence numbers, rectangles, and every frame's
// stream through the library's PNG reader (wrapped as a still of the rectangle's size), composed and compared.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "apng_device.hpp"
#include "backend.hpp"
#include "maray_hip.h"
#include "png_container.hpp"
#include "png_device.hpp"

namespace maray {
static std::string g_last;
void set_last_error(const std::string &m) { g_last = m; }
void png_band_compress(const PngBandArgs &, hipStream_t) { throw Error{MARAY_E_INTERNAL, "no device in this harness"}; }
void png_band_scan(const PngBandArgs &, hipStream_t) { throw Error{MARAY_E_INTERNAL, "no device in this harness"}; }
void png_band_gather(const PngBandArgs &, hipStream_t) { throw Error{MARAY_E_INTERNAL, "no device in this harness"}; }
void frame_delta(const unsigned char *, const unsigned char *, uint32_t, uint32_t, uint32_t *, uint32_t *, hipStream_t) { throw Error{MARAY_E_INTERNAL, "no device in this harness"}; }
}   // namespace maray
extern "C" void maray_free(void *p) { free(p); }

using namespace maray;

typedef std::vector<uint8_t> Bytes;

// rows [0, bh) of the bw-wide rectangle at (x, y) of a w-wide raster, in bands of `band` rows
static void host_piece(const Bytes &img, uint32_t w, const ApngRect &r, uint32_t band, PngPiece &p)
{
    p.y0 = 0; p.y1 = r.h;
    const uint32_t row_bytes = 3 * r.w + 1;
    for (uint32_t b0 = 0; b0 < r.h; b0 += band) {
        const uint32_t b1 = std::min(r.h, b0 + band), rows = b1 - b0;
        uint64_t sa = 0, sb = 0;
        for (uint32_t y = b0; y < b1; y++) {
            Bytes line(1, 0);
            const size_t at = ((size_t)(r.y + y) * w + r.x) * 3;
            line.insert(line.end(), img.begin() + at, img.begin() + at + (size_t)r.w * 3);
            for (size_t o = 0; o < line.size(); o += 65535) {
                const size_t n = std::min<size_t>(65535, line.size() - o);
                const uint8_t head[5] = {0, (uint8_t)n, (uint8_t)(n >> 8), (uint8_t)~n, (uint8_t)(~n >> 8)};
                p.z.insert(p.z.end(), head, head + 5);
                p.z.insert(p.z.end(), line.begin() + o, line.begin() + o + n);
            }
            const uint8_t sync[5] = {0, 0, 0, 0xFF, 0xFF};
            p.z.insert(p.z.end(), sync, sync + 5);
            uint64_t a = 0, bb = 0;
            for (size_t i = 0; i < line.size(); i++) { a += line[i]; bb += (uint64_t)(line.size() - i) * line[i]; }
            const uint64_t after = (uint64_t)(rows - 1 - (y - b0)) * row_bytes;
            sa += a % PNG_ADLER_MOD;
            sb += (bb % PNG_ADLER_MOD + (a % PNG_ADLER_MOD) * (after % PNG_ADLER_MOD)) % PNG_ADLER_MOD;
        }
        AdlerPart part;
        part.n = (uint32_t)(((uint64_t)rows * row_bytes) % PNG_ADLER_MOD);
        part.a = (uint32_t)(sa % PNG_ADLER_MOD); part.b = (uint32_t)(sb % PNG_ADLER_MOD);
        p.adler.append(part);
    }
}

static void host_box(const Bytes &a, const Bytes &b, uint32_t w, uint32_t h, uint32_t box[4])
{
    uint32_t x0 = w, y0 = h, x1 = 0, y1 = 0;
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++)
            if (memcmp(&a[((size_t)y * w + x) * 3], &b[((size_t)y * w + x) * 3], 3)) {
                x0 = std::min(x0, x); y0 = std::min(y0, y); x1 = std::max(x1, x + 1); y1 = std::max(y1, y + 1);
            }
    if (!x1) x0 = y0 = 0;
    box[0] = x0; box[1] = y0; box[2] = x1; box[3] = y1;
}

// what ApngWriter::add_frame does with its pieces, with the chunk limit as a parameter
static Bytes host_apng(const std::vector<Bytes> &frames, uint32_t w, uint32_t h, uint32_t band, size_t limit, std::vector<ApngRect> &rects)
{
    Bytes file;
    uint32_t seq = 0;
    apng_begin(file, w, h, (uint32_t)frames.size(), 3);
    for (size_t i = 0; i < frames.size(); i++) {
        ApngRect r{0, 0, w, h};
        if (i) {
            uint32_t box[4];
            host_box(frames[i - 1], frames[i], w, h, box);
            r = apng_rect(box, w, h);
        }
        PngPiece p;
        host_piece(frames[i], w, r, band, p);
        const Bytes z = png_close_stream(r.h, {&p});
        apng_fctl(file, seq, r.w, r.h, r.x, r.y, 2, 50);
        if (i) apng_fdat(file, seq, z.data(), z.size(), limit);
        else apng_idat(file, z.data(), z.size(), limit);
        rects.push_back(r);
    }
    apng_end(file);
    return file;
}

static uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

// the file taken apart: returns the number of faults found
static int check_apng(const Bytes &file, const std::vector<Bytes> &frames, uint32_t w, uint32_t h, const std::vector<ApngRect> &rects, size_t limit)
{
    int bad = 0;
    size_t at = 8;
    uint32_t seq = 0;
    std::vector<Bytes> streams;
    std::vector<ApngRect> seen;
    bool actl = false, idat = false;
    while (at + 12 <= file.size()) {
        const uint32_t n = be32(&file[at]);
        if (at + 12 + n > file.size()) return bad + 1;
        const std::string kind((const char *)&file[at + 4], 4);
        const uint8_t *d = &file[at + 8];
        if (be32(d + n) != (uint32_t)crc32(0L, &file[at + 4], n + 4)) bad++;
        if (n > limit && (kind == "IDAT" || kind == "fdAT")) bad++;
        if (kind == "acTL") { actl = true; if (idat || n != 8 || be32(d) != frames.size() || be32(d + 4) != 3) bad++; }
        else if (kind == "fcTL") {
            if (n != 26 || be32(d) != seq++ || d[20] != 0 || d[21] != 2 || d[22] != 0 || d[23] != 50 || d[24] || d[25]) bad++;
            seen.push_back(ApngRect{be32(d + 12), be32(d + 16), be32(d + 4), be32(d + 8)});
            streams.emplace_back();
        }
        else if (kind == "IDAT") { idat = true; if (streams.size() != 1) bad++; else streams[0].insert(streams[0].end(), d, d + n); }
        else if (kind == "fdAT") {
            if (streams.size() < 2 || n < 4 || be32(d) != seq++) bad++;
            else streams.back().insert(streams.back().end(), d + 4, d + n);
        }
        at += 12 + n;
    }
    if (at != file.size() || !actl || seen.size() != frames.size() || seen.size() != rects.size()) return bad + 1;
    Bytes canvas((size_t)w * h * 3, 0);
    for (size_t i = 0; i < seen.size(); i++) {
        const ApngRect &r = seen[i];
        if (r.x != rects[i].x || r.y != rects[i].y || r.w != rects[i].w || r.h != rects[i].h || !r.w || !r.h || r.x + r.w > w || r.y + r.h > h) { bad++; continue; }
        const Bytes still = png_file(r.w, r.h, streams[i].data(), streams[i].size());       // the frame's stream as a still: the library's reader
        uint8_t *rgb = nullptr;
        uint32_t w2 = 0, h2 = 0;
        if (png_decode(still, &rgb, &w2, &h2) || w2 != r.w || h2 != r.h) { printf("frame %zu: %s\n", i, g_last.c_str()); free(rgb); bad++; continue; }
        for (uint32_t y = 0; y < r.h; y++) memcpy(&canvas[((size_t)(r.y + y) * w + r.x) * 3], rgb + (size_t)y * r.w * 3, (size_t)r.w * 3);
        free(rgb);
        if (canvas != frames[i]) { printf("frame %zu does not compose to its raster\n", i); bad++; }
    }
    return bad;
}

int main()
{
    int bad = 0;
    // the box-to-rectangle logic
    {
        const uint32_t empty[4] = {0, 0, 0, 0}, one[4] = {0, 0, 1, 1}, corner[4] = {6, 4, 7, 5}, full[4] = {0, 0, 7, 5};
        ApngRect r = apng_rect(empty, 7, 5);
        if (r.x || r.y || r.w != 1 || r.h != 1) bad++;
        r = apng_rect(one, 7, 5);
        if (r.x || r.y || r.w != 1 || r.h != 1) bad++;
        r = apng_rect(corner, 7, 5);
        if (r.x != 6 || r.y != 4 || r.w != 1 || r.h != 1) bad++;
        r = apng_rect(full, 7, 5);
        if (r.x || r.y || r.w != 7 || r.h != 5) bad++;
        const uint32_t outside[][4] = {{0, 0, 8, 5}, {0, 0, 7, 6}, {3, 0, 3, 5}, {0, 4, 7, 4}, {5, 0, 2, 5}, {0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0}};
        for (auto &b : outside) {
            try { apng_rect(b, 7, 5); bad++; } catch (const Error &e) { if (e.code != MARAY_E_INTERNAL) bad++; }
        }
        printf("rectangles ok\n");
    }
    // the timing checks
    try { apng_check_timing(1, 65535, 0); } catch (const Error &) { bad++; }
    for (auto &t : std::vector<std::vector<uint32_t>>{{0, 1, 25}, {1, 65536, 25}, {1, 1, 65536}}) {
        try { apng_check_timing(t[0], t[1], t[2]); bad++; } catch (const Error &e) { if (e.code != MARAY_E_ARG) bad++; }
    }
    // the stream-closing helper refuses pieces that do not cover the rectangle's rows
    {
        PngPiece p;
        Bytes img(5 * 3 * 3, 9);
        host_piece(img, 5, ApngRect{1, 0, 3, 3}, 2, p);
        try { png_close_stream(4, {&p}); bad++; } catch (const Error &) {}
        try { png_close_stream(3, {}); bad++; } catch (const Error &) {}
        if (png_close_stream(3, {&p}).size() != 2 + p.z.size() + 5 + 4) bad++;
    }
    // whole animations
    const uint32_t sizes[][2] = {{1, 1}, {5, 3}, {67, 41}, {300, 77}};
    for (auto &wh : sizes) {
        const uint32_t w = wh[0], h = wh[1];
        std::vector<Bytes> frames(6, Bytes((size_t)w * h * 3));
        uint32_t x = 99u * w + h;
        for (auto &v : frames[0]) { x = x * 1664525u + 1013904223u; v = (uint8_t)(x >> 24); }
        for (size_t i = 1; i < frames.size(); i++) {
            frames[i] = frames[i - 1];
            if (i == 3) continue;                                   // an unchanged frame: the empty box
            x = x * 1664525u + 1013904223u;
            const uint32_t x0 = (x >> 8) % w, y0 = (x >> 20) % h;
            const uint32_t x1 = i == 4 ? x0 + 1 : w - (i == 5 ? 0 : (x >> 3) % (w - x0)), y1 = i == 5 ? y0 + 1 : h;      // one column; one row of full width
            for (uint32_t yy = y0; yy < y1; yy++)
                for (uint32_t xx = x0; xx < x1; xx++) frames[i][((size_t)yy * w + xx) * 3 + i % 3] ^= 0x5A;
        }
        Bytes first;
        for (uint32_t band : {1u, 3u, 1000u})
            for (size_t limit : {(size_t)PNG_CHUNK_MAX, (size_t)4096, (size_t)9, (size_t)5}) {
                std::vector<ApngRect> rects;
                const Bytes file = host_apng(frames, w, h, band, limit, rects);
                if (limit == PNG_CHUNK_MAX) {
                    if (first.empty()) first = file;
                    if (file != first) { printf("%ux%u band %u: the file depends on the cut\n", w, h, band); bad++; }
                }
                if (rects[3].w != 1 || rects[3].h != 1 || rects[3].x || rects[3].y) bad++;
                const int b = check_apng(file, frames, w, h, rects, limit);
                if (b) { printf("%ux%u band %u limit %zu: %d faults\n", w, h, band, limit, b); bad += b; }
            }
        printf("%ux%u ok\n", w, h);
    }
    // frames too large for the writer
    try { apng_check_frame(1u << 15, (1u << 15) / 3 + 1); bad++; } catch (const Error &e) { if (e.code != MARAY_E_LIMIT) bad++; }
    try { apng_check_frame((1u << 20) + 1, 1); bad++; } catch (const Error &e) { if (e.code != MARAY_E_LIMIT) bad++; }
    apng_check_frame(1u << 15, (1u << 15) / 3);
    printf("%s\n", bad ? "FAILED" : "all ok");
    return bad ? 1 : 0;
}
