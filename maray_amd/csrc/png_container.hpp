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

}   // namespace maray
