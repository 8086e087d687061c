// png_dynamic_asan.cpp — host-only sanitizer harness for the host code of the device PNG encoder's dynamic coder (test
// infrastructure).  Built with -fsanitize=address,undefined together with maray_amd/csrc/png_device.cpp and png.cpp; needs no
// device and launches nothing (the kernel launchers are stubs that fail).  It plays the device's part on the host: per band
// of rows it cuts the raster into the encoder's tokens, counts them, asks the library for the code (maray_png_dynamic_codes:
// code lengths, header writer), for the canonical codes (png_dynamic_table) and, after writing the tokens' bits behind the
// header's, for the piece's end (png_dynamic_close); png_assemble puts the file around the pieces.  Every file is decoded
// by the library's reader here, and written with its raster to the directory given as argv[1] for the Python test to inflate.
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

struct Tok { uint32_t sym[3]; uint32_t n_sym; uint32_t extra, extra_bits; bool match; };

static uint32_t length_symbol(uint32_t len, uint32_t *eb, uint32_t *extra)
{
    static const uint32_t base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const uint32_t bits[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    uint32_t k = 28;
    while (base[k] > len) k--;
    *eb = bits[k]; *extra = len - base[k];
    return 257 + k;
}

// the tokens of rows [y0, y1): the filter byte, then per segment of PNG_SEG pixels a literal first pixel and, in steps of 64
// pixels, runs of pixels equal to the pixel before them as matches of distance 3
static std::vector<Tok> tokens_of(const std::vector<uint8_t> &img, uint32_t w, uint32_t y0, uint32_t y1)
{
    std::vector<Tok> out;
    for (uint32_t y = y0; y < y1; y++) {
        out.push_back(Tok{{0, 0, 0}, 1, 0, 0, false});
        const uint8_t *row = img.data() + (size_t)y * w * 3;
        for (uint32_t s0 = 0; s0 < w; s0 += PNG_SEG) {
            const uint32_t npix = std::min(PNG_SEG, w - s0);
            for (uint32_t p0 = 0; p0 < npix; p0 += 64) {
                const uint32_t end = std::min(npix, p0 + 64);
                for (uint32_t p = p0; p < end;) {
                    const uint8_t *px = row + (size_t)(s0 + p) * 3;
                    if (p == 0 || memcmp(px, px - 3, 3)) { out.push_back(Tok{{px[0], px[1], px[2]}, 3, 0, 0, false}); p++; continue; }
                    uint32_t run = 1;
                    while (p + run < end && !memcmp(px + 3 * run, px, 3)) run++;
                    Tok t{{0, 0, 0}, 1, 0, 0, true};
                    t.sym[0] = length_symbol(3 * run, &t.extra_bits, &t.extra);
                    out.push_back(t);
                    p += run;
                }
            }
        }
    }
    return out;
}

static void put_bits(std::vector<uint8_t> &z, uint64_t &at, uint32_t value, uint32_t n)
{
    for (uint32_t b = 0; b < n; b++, at++) {
        if ((at >> 3) >= z.size()) z.push_back(0);
        z[(size_t)(at >> 3)] = (uint8_t)(z[(size_t)(at >> 3)] | (((value >> b) & 1u) << (at & 7)));
    }
}

static int g_bad = 0;

// rows [y0, y1) in bands of `band` rows, each one dynamic block
static void host_piece(const std::vector<uint8_t> &img, uint32_t w, uint32_t y0, uint32_t y1, uint32_t band, PngPiece &p)
{
    p.y0 = y0; p.y1 = y1;
    const uint32_t row_bytes = 3 * w + 1;
    for (uint32_t b0 = y0; b0 < y1; b0 += band) {
        const uint32_t b1 = std::min(y1, b0 + band), rows = b1 - b0;
        const std::vector<Tok> toks = tokens_of(img, w, b0, b1);
        uint32_t lit[286] = {0}, dist[30] = {0};
        for (const Tok &t : toks) {
            for (uint32_t k = 0; k < t.n_sym; k++) lit[t.sym[k]]++;
            if (t.match) dist[2]++;
        }
        lit[256] = 1;
        uint8_t lit_lens[286], dist_lens[30], header[512];
        size_t header_bits = 0;
        if (maray_png_dynamic_codes(lit, dist, lit_lens, dist_lens, header, sizeof header, &header_bits)) { printf("codes: %s\n", g_last.c_str()); g_bad++; return; }
        if ((dist[2] != 0) != (dist_lens[2] == 1)) g_bad++;
        uint32_t table[PNG_LIT_SYMS];
        png_dynamic_table(lit_lens, table);
        std::vector<uint8_t> z(header, header + (header_bits + 7) / 8);
        uint64_t at = header_bits;
        for (const Tok &t : toks) {
            for (uint32_t k = 0; k < t.n_sym; k++) {
                if (!(table[t.sym[k]] >> 16)) { printf("symbol %u has no code\n", t.sym[k]); g_bad++; }
                put_bits(z, at, table[t.sym[k]] & 0xFFFFu, table[t.sym[k]] >> 16);
            }
            if (t.match) { put_bits(z, at, t.extra, t.extra_bits); put_bits(z, at, 0, 1); }
        }
        png_dynamic_close(z, at, table[256]);
        p.z.insert(p.z.end(), z.begin(), z.end());
        // the band's Adler part, directly
        AdlerPart part;
        uint64_t a = 0, bb = 0;
        const uint64_t n = (uint64_t)rows * row_bytes;
        uint64_t i = 0;
        for (uint32_t y = b0; y < b1; y++) {
            i++;                                                   // the filter byte 0
            for (uint32_t x = 0; x < 3 * w; x++, i++) {
                const uint64_t v = img[(size_t)y * w * 3 + x];
                a = (a + v) % PNG_ADLER_MOD;
                bb = (bb + ((n - i) % PNG_ADLER_MOD) * v) % PNG_ADLER_MOD;
            }
        }
        part.n = (uint32_t)(n % PNG_ADLER_MOD); part.a = (uint32_t)a; part.b = (uint32_t)bb;
        p.adler.append(part);
    }
}

static void write_file(const std::string &path, const uint8_t *p, size_t n)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(p, 1, n, f) != n) { printf("cannot write %s\n", path.c_str()); g_bad++; }
    if (f) fclose(f);
}

int main(int argc, char **argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    // kind 0: random bytes; 1: few colours in runs; 2: one colour; 3: thirty byte values with Fibonacci counts (a tree deeper than 15)
    const uint32_t cases[][3] = {{1, 1, 0}, {5, 3, 0}, {67, 41, 0}, {300, 20, 1}, {700, 9, 1}, {513, 4, 2}, {1, 40, 2}, {509, 1426, 3}, {64, 8, 1}};
    int index = 0;
    for (auto &c : cases) {
        const uint32_t w = c[0], h = c[1], kind = c[2];
        std::vector<uint8_t> img((size_t)w * h * 3);
        uint32_t x = 12345u * w + h;
        auto rnd = [&] { x = x * 1664525u + 1013904223u; return x >> 8; };
        if (kind == 0) for (auto &v : img) v = (uint8_t)rnd();
        if (kind == 1)
            for (size_t px = 0; px < (size_t)w * h;) {
                const uint32_t run = 1 + rnd() % 90, colour = rnd() % 5;
                for (uint32_t k = 0; k < run && px < (size_t)w * h; k++, px++) { img[3 * px] = (uint8_t)(40 * colour); img[3 * px + 1] = (uint8_t)(200 - colour); img[3 * px + 2] = 7; }
            }
        if (kind == 2) for (auto &v : img) v = 200;
        if (kind == 3) {
            // values 100 .. 129 with counts 1, 1, 2, 3, 5, ...: filled in order, then shuffled
            uint64_t f0 = 1, f1 = 1;
            size_t at = 0;
            for (uint32_t v = 0; v < 30 && at < img.size(); v++) {
                for (uint64_t k = 0; k < f0 && at < img.size(); k++) img[at++] = (uint8_t)(100 + v);
                const uint64_t f2 = f0 + f1; f0 = f1; f1 = f2;
            }
            while (at < img.size()) img[at++] = 129;
            for (size_t i = img.size() - 1; i > 0; i--) std::swap(img[i], img[rnd() % (i + 1)]);
        }
        for (uint32_t tile : {h, 7u})
            for (uint32_t band : {1u, 3u, 1000u}) {
                if (kind == 3 && band != 1000u) continue;              // (a deep tree needs the whole raster's counts)
                std::vector<PngPiece> pieces;
                for (uint32_t y = 0; y < h; y += tile) { pieces.emplace_back(); host_piece(img, w, y, std::min(h, y + tile), band, pieces.back()); }
                std::vector<const PngPiece *> order;
                for (auto &p : pieces) order.push_back(&p);
                const std::vector<uint8_t> file = png_assemble(w, h, order);
                uint8_t *rgb = nullptr;
                uint32_t w2 = 0, h2 = 0;
                const int rc = png_decode(file, &rgb, &w2, &h2);
                if (rc || w2 != w || h2 != h || memcmp(rgb, img.data(), img.size())) { printf("%ux%u tile %u band %u: rc %d %s\n", w, h, tile, band, rc, g_last.c_str()); g_bad++; }
                free(rgb);
                char name[96];
                snprintf(name, sizeof name, "/case%02d_%ux%u", index++, w, h);
                write_file(dir + name + ".png", file.data(), file.size());
                write_file(dir + name + ".rgb", img.data(), img.size());
            }
        printf("%ux%u kind %u ok\n", w, h, kind);
    }
    // counts no band has, and a buffer too small
    {
        uint32_t lit[286] = {0}, dist[30] = {0};
        uint8_t ll[286], dl[30], header[512];
        size_t bits = 0;
        lit[0] = 4;
        if (maray_png_dynamic_codes(lit, dist, ll, dl, header, sizeof header, &bits) != MARAY_E_ARG) g_bad++;
        lit[256] = 1;
        if (maray_png_dynamic_codes(lit, dist, ll, dl, header, 3, &bits) != MARAY_E_ARG) g_bad++;
        if (maray_png_dynamic_codes(lit, dist, ll, dl, header, sizeof header, &bits) != MARAY_OK || ll[0] != 1 || ll[256] != 1) g_bad++;
        dist[7] = 1;
        if (maray_png_dynamic_codes(lit, dist, ll, dl, header, sizeof header, &bits) != MARAY_E_ARG) g_bad++;
    }
    printf("%s\n", g_bad ? "FAILED" : "all ok");
    return g_bad ? 1 : 0;
}
