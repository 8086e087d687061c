// png_container.hpp — the PNG container around a zlib stream, shared by the two writers (png.cpp: host zlib; png_device.cpp:
// the device encoder): big-endian words, chunks with their CRC-32 (zlib's crc32), and the file of an 8-bit truecolour image
// -- signature, IHDR, the stream in IDAT chunks of at most 2^30 bytes, IEND.
#pragma once

#include <zlib.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace maray {

inline void put_be32(std::vector<uint8_t> &v, uint32_t x) { v.push_back(x >> 24); v.push_back(x >> 16); v.push_back(x >> 8); v.push_back(x); }

inline void chunk(std::vector<uint8_t> &out, const char *type, const uint8_t *data, size_t n)
{
    put_be32(out, (uint32_t)n);
    size_t start = out.size();
    out.insert(out.end(), type, type + 4);
    if (n) out.insert(out.end(), data, data + n);
    uint32_t crc = (uint32_t)crc32(0L, out.data() + start, (uInt)(n + 4));
    put_be32(out, crc);
}

// Raster sizes this library will read or write: 2^20 pixels a side (the evaluators' own limit,
// MARAY_DOMAIN_MAX) and 16 GiB of filtered scanlines.  A crafted IHDR beyond that is rejected, not allocated.
constexpr uint64_t MARAY_PNG_MAX_BYTES = 1ull << 34;

// The file of a w x h RGB8 image whose zlib stream is z[0 .. zn)
inline std::vector<uint8_t> png_file(uint32_t w, uint32_t h, const uint8_t *z, size_t zn)
{
    std::vector<uint8_t> out = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    out.reserve(zn + 12 * (zn >> 30) + 128);
    std::vector<uint8_t> ihdr;
    put_be32(ihdr, w); put_be32(ihdr, h);
    ihdr.push_back(8); ihdr.push_back(2); ihdr.push_back(0); ihdr.push_back(0); ihdr.push_back(0);   // 8-bit, truecolour
    chunk(out, "IHDR", ihdr.data(), ihdr.size());
    for (size_t off = 0; off < zn || off == 0; off += (size_t)1 << 30) {          // a chunk's length field holds 31 bits
        chunk(out, "IDAT", z + off, std::min<size_t>((size_t)1 << 30, zn - off));
        if (zn == 0) break;
    }
    chunk(out, "IEND", nullptr, 0);
    return out;
}

// The file of a w x h indexed-colour image (colour type 3) of bit depth 1, 2, 4 or 8 whose palette is the n <= 256 colours
// palette[0 .. 3 n) and whose zlib stream is z[0 .. zn): signature, IHDR, PLTE, IDAT chunks, IEND.  No tRNS.
inline std::vector<uint8_t> png_file_indexed(uint32_t w, uint32_t h, uint32_t depth, const uint8_t *palette, uint32_t n, const uint8_t *z, size_t zn)
{
    std::vector<uint8_t> out = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    out.reserve(zn + 12 * (zn >> 30) + 128 + 3 * (size_t)n);
    std::vector<uint8_t> ihdr;
    put_be32(ihdr, w); put_be32(ihdr, h);
    ihdr.push_back((uint8_t)depth); ihdr.push_back(3); ihdr.push_back(0); ihdr.push_back(0); ihdr.push_back(0);
    chunk(out, "IHDR", ihdr.data(), ihdr.size());
    chunk(out, "PLTE", palette, 3 * (size_t)n);
    for (size_t off = 0; off < zn || off == 0; off += (size_t)1 << 30) {
        chunk(out, "IDAT", z + off, std::min<size_t>((size_t)1 << 30, zn - off));
        if (zn == 0) break;
    }
    chunk(out, "IEND", nullptr, 0);
    return out;
}

// ---- APNG (the animation writer, apng_device.cpp): a PNG whose IDAT image is frame 0 and whose later frames are complete
// zlib streams of sub-rectangles in fdAT chunks.  fcTL and fdAT share one run of sequence numbers, 0, 1, 2, ...
constexpr size_t PNG_CHUNK_MAX = (size_t)1 << 30;

inline void put_be16(std::vector<uint8_t> &v, uint32_t x) { v.push_back((uint8_t)(x >> 8)); v.push_back((uint8_t)x); }

// signature, IHDR, acTL
inline void apng_begin(std::vector<uint8_t> &out, uint32_t w, uint32_t h, uint32_t n_frames, uint32_t n_plays)
{
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    out.insert(out.end(), sig, sig + 8);
    std::vector<uint8_t> d;
    put_be32(d, w); put_be32(d, h);
    d.push_back(8); d.push_back(2); d.push_back(0); d.push_back(0); d.push_back(0);
    chunk(out, "IHDR", d.data(), d.size());
    d.clear();
    put_be32(d, n_frames); put_be32(d, n_plays);
    chunk(out, "acTL", d.data(), d.size());
}

// fcTL of a bw x bh frame at (x, y): dispose NONE, blend SOURCE; takes the next sequence number
inline void apng_fctl(std::vector<uint8_t> &out, uint32_t &seq, uint32_t bw, uint32_t bh, uint32_t x, uint32_t y, uint32_t delay_num, uint32_t delay_den)
{
    std::vector<uint8_t> d;
    put_be32(d, seq++); put_be32(d, bw); put_be32(d, bh); put_be32(d, x); put_be32(d, y);
    put_be16(d, delay_num); put_be16(d, delay_den);
    d.push_back(0); d.push_back(0);
    chunk(out, "fcTL", d.data(), d.size());
}

// frame 0's stream: IDAT chunks of at most `limit` bytes
inline void apng_idat(std::vector<uint8_t> &out, const uint8_t *z, size_t zn, size_t limit = PNG_CHUNK_MAX)
{
    for (size_t off = 0; off < zn; off += limit) chunk(out, "IDAT", z + off, std::min(limit, zn - off));
}

// a later frame's stream: fdAT chunks of at most `limit` bytes, each a sequence number and then up to limit - 4 bytes of it
inline void apng_fdat(std::vector<uint8_t> &out, uint32_t &seq, const uint8_t *z, size_t zn, size_t limit = PNG_CHUNK_MAX)
{
    std::vector<uint8_t> d;
    for (size_t off = 0; off < zn; off += limit - 4) {
        const size_t n = std::min(limit - 4, zn - off);
        d.clear();
        d.reserve(n + 4);
        put_be32(d, seq++);
        d.insert(d.end(), z + off, z + off + n);
        chunk(out, "fdAT", d.data(), d.size());
    }
}

inline void apng_end(std::vector<uint8_t> &out) { chunk(out, "IEND", nullptr, 0); }

}   // namespace maray
