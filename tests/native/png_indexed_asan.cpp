// png_indexed_asan.cpp — host-only sanitizer harness for the host code of the indexed-colour files (test infrastructure).
// Built with -fsanitize=address,undefined together with maray_amd/csrc/png_indexed.cpp, png_device.cpp and png.cpp; needs no
// device and launches nothing (the kernel launchers are stubs that fail).  It plays the device's part on the host -- the
// sorted palette, the packed index rows as stored deflate blocks ended by the sync flush, and a band's Adler part from
// per-row shares over rows of rb + 1 bytes -- and checks that png_assemble_indexed's file (the container with PLTE, the depth
// rule, the stream's frame) is the same for every cut, has the chunks and the depth the contract names, and is read back to
// the raster by the library's reader.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "backend.hpp"
#include "maray_hip.h"
#include "png_container.hpp"
#include "png_indexed.hpp"

namespace maray {
static std::string g_last;
void set_last_error(const std::string &m) { g_last = m; }
static Error none() { return Error{MARAY_E_INTERNAL, "no device in this harness"}; }
void png_band_compress(const PngBandArgs &, hipStream_t) { throw none(); }
void png_band_scan(const PngBandArgs &, hipStream_t) { throw none(); }
void png_band_gather(const PngBandArgs &, hipStream_t) { throw none(); }
void png_colors(const unsigned char *, uint64_t, uint32_t *, uint32_t *, bool, hipStream_t) { throw none(); }
void png_index(const unsigned char *, uint32_t, uint32_t, const uint32_t *, uint32_t, uint32_t, unsigned char *, hipStream_t) { throw none(); }
void png_band_compress_idx(const PngBandArgs &, hipStream_t) { throw none(); }
}   // namespace maray
extern "C" void maray_free(void *p) { free(p); }

using namespace maray;

// rows [y0, y1) of packed index rows (rb bytes each) in bands of `band` rows: stored blocks, and the Adler part the way a
// band's shares add up
static void host_piece(const std::vector<uint8_t> &packed, uint32_t rb, uint32_t y0, uint32_t y1, uint32_t band, PngPiece &p)
{
    p.y0 = y0; p.y1 = y1;
    const uint32_t row_bytes = rb + 1;
    for (uint32_t b0 = y0; b0 < y1; b0 += band) {
        const uint32_t b1 = std::min(y1, b0 + band), rows = b1 - b0;
        uint64_t sa = 0, sb = 0;
        for (uint32_t y = b0; y < b1; y++) {
            std::vector<uint8_t> line(1, 0);
            line.insert(line.end(), packed.begin() + (size_t)y * rb, packed.begin() + (size_t)(y + 1) * rb);
            const size_t n = line.size();                                      // (rb <= 65534 here: one stored block)
            const uint8_t head[5] = {0, (uint8_t)n, (uint8_t)(n >> 8), (uint8_t)~n, (uint8_t)(~n >> 8)};
            p.z.insert(p.z.end(), head, head + 5);
            p.z.insert(p.z.end(), line.begin(), line.end());
            const uint8_t sync[5] = {0, 0, 0, 0xFF, 0xFF};
            p.z.insert(p.z.end(), sync, sync + 5);
            uint64_t a = 0, bb = 0;
            for (size_t i = 0; i < n; i++) { a += line[i]; bb += (uint64_t)(n - i) * line[i]; }
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

static uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

int main()
{
    int bad = 0;
    // the depth rule and the geometry that follows from it
    const uint32_t depth_of[][2] = {{1, 1}, {2, 1}, {3, 2}, {4, 2}, {5, 4}, {16, 4}, {17, 8}, {255, 8}, {256, 8}};
    for (auto &nd : depth_of)
        if (png_idx_depth(nd[0]) != nd[1]) { printf("depth of %u colours\n", nd[0]); bad++; }
    if (png_idx_row_bytes(1, 1) != 1 || png_idx_row_bytes(8, 1) != 1 || png_idx_row_bytes(9, 1) != 2 || png_idx_row_bytes(5, 4) != 3 ||
        png_idx_row_bytes(1u << 20, 8) != 1u << 20 || png_idx_row_segments(768) != 1 || png_idx_row_segments(769) != 2 ||
        png_idx_slot_bytes(768) != PNG_SLOT_MAX || png_idx_slot_bytes(1) != 32)
        { printf("row geometry\n"); bad++; }

    const uint32_t cases[][3] = {{1, 1, 1}, {5, 3, 2}, {9, 4, 3}, {67, 41, 4}, {33, 7, 5}, {300, 77, 16}, {301, 20, 17}, {257, 9, 256}, {30000, 3, 2}};
    for (auto &c : cases) {
        const uint32_t w = c[0], h = c[1], n = std::min<uint32_t>(c[2], w * h);
        // a raster over n colours (every one used), the sorted palette, the packed rows
        std::set<uint32_t> keys;
        uint32_t x = 12345u * w + h;
        while (keys.size() < n) { x = x * 1664525u + 1013904223u; keys.insert(x >> 8); }
        const std::vector<uint32_t> sorted(keys.begin(), keys.end());
        std::vector<uint8_t> palette;
        for (uint32_t k : sorted) { palette.push_back((uint8_t)(k >> 16)); palette.push_back((uint8_t)(k >> 8)); palette.push_back((uint8_t)k); }
        const uint32_t d = png_idx_depth(n), rb = png_idx_row_bytes(w, d);
        std::vector<uint8_t> img((size_t)w * h * 3), packed((size_t)rb * h, 0);
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t px = 0; px < w; px++) {
                const size_t i = (size_t)y * w + px;
                x = x * 1664525u + 1013904223u;
                const uint32_t idx = i < n ? (uint32_t)i : (x >> 16) % n;
                memcpy(&img[3 * i], &palette[3 * idx], 3);
                packed[(size_t)y * rb + (size_t)px * d / 8] |= (uint8_t)(idx << (8 - d - (px * d) % 8));
            }
        std::vector<uint8_t> first;
        for (uint32_t tile : {h, 1u, 2u, 7u})
            for (uint32_t band : {1u, 3u, 1000u}) {
                std::vector<PngPiece> pieces;
                for (uint32_t y = 0; y < h; y += tile) { pieces.emplace_back(); host_piece(packed, rb, y, std::min(h, y + tile), band, pieces.back()); }
                std::vector<const PngPiece *> order;
                for (auto &p : pieces) order.push_back(&p);
                const std::vector<uint8_t> file = png_assemble_indexed(w, h, palette.data(), n, order);
                if (first.empty()) first = file;
                if (file != first) { printf("%ux%u tile %u band %u: the file depends on the cut\n", w, h, tile, band); bad++; }
                uint8_t *rgb = nullptr;
                uint32_t w2 = 0, h2 = 0;
                const int rc = png_decode(file, &rgb, &w2, &h2);
                if (rc || w2 != w || h2 != h || memcmp(rgb, img.data(), img.size())) { printf("%ux%u tile %u band %u: rc %d %s\n", w, h, tile, band, rc, g_last.c_str()); bad++; }
                free(rgb);
            }
        // the container: IHDR of depth d and colour type 3, PLTE of exactly 3 n bytes next, then IDAT
        const uint8_t *f = first.data();
        if (first.size() < 8 + 25 + 12 + 3 * (size_t)n + 12 || be32(f + 8) != 13 || memcmp(f + 12, "IHDR", 4) || be32(f + 16) != w || be32(f + 20) != h ||
            f[24] != d || f[25] != 3 || f[26] || f[27] || f[28] || be32(f + 33) != 3 * n || memcmp(f + 37, "PLTE", 4) ||
            memcmp(f + 41, palette.data(), 3 * (size_t)n) || memcmp(f + 41 + 3 * (size_t)n + 4 + 4, "IDAT", 4) || memcmp(first.data() + first.size() - 8, "IEND", 4))
            { printf("%ux%u: the container\n", w, h); bad++; }
        // what is refused: no palette, more than 256 colours, pieces short of the image
        PngPiece p;
        host_piece(packed, rb, 0, h, 1000, p);
        try { png_assemble_indexed(w, h, nullptr, n, {&p}); bad++; } catch (const Error &) {}
        try { png_assemble_indexed(w, h, palette.data(), 0, {&p}); bad++; } catch (const Error &) {}
        try { png_assemble_indexed(w, h, palette.data(), 257, {&p}); bad++; } catch (const Error &) {}
        p.y1 = h + 1;
        try { png_assemble_indexed(w, h, palette.data(), n, {&p}); bad++; } catch (const Error &) {}
        printf("%ux%u, %u colours, depth %u ok\n", w, h, n, d);
    }
    // the entry point that times kernels refuses its arguments before it looks for a device
    try { png_time_kernels_color(0, (const unsigned char *)0x1000, 4, 4, MARAY_PNG_COLOR_RGB, 1, nullptr); bad++; }      // (never read)
    catch (const Error &e) { if (e.code != MARAY_E_ARG) bad++; }
    printf("%s\n", bad ? "FAILED" : "all ok");
    return bad ? 1 : 0;
}
