// png_device_asan.cpp — host-only sanitizer harness for the device PNG encoder's host code (test infrastructure).
// Built with -fsanitize=address,undefined together with maray_amd/csrc/png_device.cpp and png.cpp; needs no device and
// launches nothing (the three kernel launchers are stubs that fail).  It plays the device's part on the host -- per band
// of rows the filtered bytes as stored deflate blocks ended by the sync flush, and the band's Adler part from per-row
// shares exactly as the kernels form them -- and checks that png_assemble's file, for several cuts of the image into pieces
// and bands, is accepted by the library's reader and decodes to the raster: the stream's frame, the Adler-32 combined
// across pieces, the container, the size checks.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "backend.hpp"
#include "maray_hip.h"
#include "png_device.hpp"

namespace maray {
static std::string g_last;
void set_last_error(const std::string &m) { g_last = m; }
void png_band_compress(const PngBandArgs &, hipStream_t) { throw Error{MARAY_E_INTERNAL, "no device in this harness"}; }
void png_band_scan(const PngBandArgs &, hipStream_t) { throw Error{MARAY_E_INTERNAL, "no device in this harness"}; }
void png_band_gather(const PngBandArgs &, hipStream_t) { throw Error{MARAY_E_INTERNAL, "no device in this harness"}; }
}   // namespace maray
extern "C" void maray_free(void *p) { free(p); }

using namespace maray;

// rows [y0, y1) in bands of `band` rows: stored blocks, and the Adler part the way a band's shares add up
static void host_piece(const std::vector<uint8_t> &img, uint32_t w, uint32_t y0, uint32_t y1, uint32_t band, PngPiece &p)
{
    p.y0 = y0; p.y1 = y1;
    const uint32_t row_bytes = 3 * w + 1;
    for (uint32_t b0 = y0; b0 < y1; b0 += band) {
        const uint32_t b1 = std::min(y1, b0 + band), rows = b1 - b0;
        AdlerPart part;
        uint64_t sa = 0, sb = 0;
        for (uint32_t y = b0; y < b1; y++) {
            std::vector<uint8_t> line(1, 0);
            line.insert(line.end(), img.begin() + (size_t)y * w * 3, img.begin() + (size_t)(y + 1) * w * 3);
            for (size_t at = 0; at < line.size(); at += 65535) {          // stored blocks of the row, not final
                const size_t n = std::min<size_t>(65535, line.size() - at);
                const uint8_t head[5] = {0, (uint8_t)n, (uint8_t)(n >> 8), (uint8_t)~n, (uint8_t)(~n >> 8)};
                p.z.insert(p.z.end(), head, head + 5);
                p.z.insert(p.z.end(), line.begin() + at, line.begin() + at + n);
            }
            const uint8_t sync[5] = {0, 0, 0, 0xFF, 0xFF};
            p.z.insert(p.z.end(), sync, sync + 5);
            // the row as one segment: A, and B + A x (the band's bytes after it), modulo 65521
            uint64_t a = 0, bb = 0;
            for (size_t i = 0; i < line.size(); i++) { a += line[i]; bb += (uint64_t)(line.size() - i) * line[i]; }
            const uint64_t after = (uint64_t)(rows - 1 - (y - b0)) * row_bytes;
            sa += a % PNG_ADLER_MOD;
            sb += (bb % PNG_ADLER_MOD + (a % PNG_ADLER_MOD) * (after % PNG_ADLER_MOD)) % PNG_ADLER_MOD;
        }
        part.n = (uint32_t)(((uint64_t)rows * row_bytes) % PNG_ADLER_MOD);
        part.a = (uint32_t)(sa % PNG_ADLER_MOD); part.b = (uint32_t)(sb % PNG_ADLER_MOD);
        p.adler.append(part);
    }
}

int main()
{
    int bad = 0;
    const uint32_t sizes[][2] = {{1, 1}, {5, 3}, {67, 41}, {300, 77}, {30000, 3}};
    for (auto &wh : sizes) {
        const uint32_t w = wh[0], h = wh[1];
        std::vector<uint8_t> img((size_t)w * h * 3);
        uint32_t x = 12345u * w + h;
        for (auto &v : img) { x = x * 1664525u + 1013904223u; v = (uint8_t)(x >> 24) | (uint8_t)((x >> 13) & 0x80); }      // (many bytes of 128 and more)
        std::vector<uint8_t> first;
        for (uint32_t tile : {h, 1u, 2u, 7u})
            for (uint32_t band : {1u, 3u, 1000u}) {
                std::vector<PngPiece> pieces;
                for (uint32_t y = 0; y < h; y += tile) { pieces.emplace_back(); host_piece(img, w, y, std::min(h, y + tile), band, pieces.back()); }
                std::vector<const PngPiece *> order;
                for (auto &p : pieces) order.push_back(&p);
                const std::vector<uint8_t> file = png_assemble(w, h, order);
                if (first.empty()) first = file;
                if (file != first) { printf("%ux%u tile %u band %u: the file depends on the cut\n", w, h, tile, band); bad++; }
                uint8_t *rgb = nullptr;
                uint32_t w2 = 0, h2 = 0;
                const int rc = png_decode(file, &rgb, &w2, &h2);
                if (rc || w2 != w || h2 != h || memcmp(rgb, img.data(), img.size())) { printf("%ux%u tile %u band %u: rc %d %s\n", w, h, tile, band, rc, g_last.c_str()); bad++; }
                free(rgb);
            }
        // pieces out of order or short of the image are refused
        PngPiece p;
        host_piece(img, w, 0, h, 1000, p);
        p.y1 = h + 1;
        try { png_assemble(w, h, {&p}); bad++; } catch (const Error &) {}
        printf("%ux%u ok\n", w, h);
    }
    const uint32_t too_big[][2] = {{(1u << 20) + 1, 1}, {1, (1u << 20) + 1}, {1u << 20, 1u << 20}};
    for (auto &wh : too_big) {
        try { png_check_size(wh[0], wh[1]); bad++; } catch (const Error &e) { if (e.code != MARAY_E_LIMIT) bad++; }
    }
    png_check_size(1u << 20, 5000);
    printf("%s\n", bad ? "FAILED" : "all ok");
    return bad ? 1 : 0;
}
