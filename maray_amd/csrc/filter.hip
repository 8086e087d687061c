// filter.hip — maray_filter_tent<K>: the tent reconstruction filter of a supersampled render (product code; include/
// maray_hip.h, "reconstruction filter").
//
// Memory-bound: 3 K^2 sample bytes are read and 3 bytes written per output pixel.  A block of 256 lanes computes a tile of
// 64 x 8 output pixels in two stages:
//   1. horizontal.  A lane takes one output pixel of one sample row: its footprint is 2K samples = 6K consecutive bytes (the
//      neighbouring lane's starts 3K bytes further on: a wavefront reads one contiguous stretch of the row).  It loads the
//      6K/4 + 1 aligned dwords that cover them, shifts them into place (v_alignbyte_b32) and forms the three channels' weighted
//      sums with 6K/4 v_dot4_u32_u8 each, against constant weight words that hold t(u) in a channel's byte positions and 0 in
//      the others'.  The sums (<= 255 * 2 K^2 = 32640) go to LDS as 16-bit values, 8K + K rows of 192.  Only the first and the
//      last pixel of an image row reach over the image's edge: those two lanes gather their bytes one by one, clamped by index.
//   2. vertical.  A wavefront takes an output row; lanes 0 .. 47 take four consecutive bytes of it each: 2K 8-byte LDS reads
//      down the column (contiguous across the lanes), 32-bit sums, round, shift, one dword store (bytes where the destination
//      is not aligned or the row ends).
// LDS: (9 K) * 384 bytes = 6.75 / 13.5 / 27 KiB for K = 2 / 4 / 8 (five blocks and more per CU).  No atomics, no scratch.
// Rows are clamped to the image by index (band_row0 says where the band lies in it), never to the band: an interior band
// must bring its halo rows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "filter.hpp"
#include "shutter.hpp"

namespace maray {

namespace {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            throw Error{MARAY_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)};           \
    } while (0)

constexpr int TW = (int)FILTER_TILE_W, TH = (int)FILTER_TILE_H, FT_BLOCK = 256;
constexpr int LDS_PITCH = TW * 3;       // 16-bit sums per LDS row

template <int K>
struct Tent {
    static constexpr int NW = 6 * K / 4;            // dwords of a pixel's footprint in one sample row
    static constexpr int ROWS = K * TH + K;         // sample rows a tile reads
    static constexpr int SHIFT = K == 2 ? 6 : K == 4 ? 10 : 14;        // log2(4 K^4)
    // t(u) for u = i - K/2, i = 0 .. 2K - 1
    static constexpr uint32_t t(int i) { const int d = 2 * i + 1 - 2 * K; return (uint32_t)(2 * K - (d < 0 ? -d : d)); }
    // dword d of the footprint holds bytes 4d .. 4d + 3; byte j is channel j % 3 of sample j / 3
    static constexpr uint32_t weights(int c, int d) {
        uint32_t r = 0;
        for (int b = 0; b < 4; b++) if ((4 * d + b) % 3 == c) r |= t((4 * d + b) / 3) << (8 * b);
        return r;
    }
};

template <int K>
__global__ __launch_bounds__(FT_BLOCK) void maray_filter_tent(const TentArgs a)
{
    using T = Tent<K>;
    __shared__ __attribute__((aligned(16))) unsigned short hs[T::ROWS * LDS_PITCH];
    const uint32_t px0 = blockIdx.x * TW, toy = blockIdx.y * TH;       // the tile: first pixel, first row (of this pass)
    const uint32_t n_oy = min((uint32_t)TH, a.n_out - toy);
    const uint32_t n_rows = K * n_oy + K;
    const uint32_t lane_px = threadIdx.x % TW, px = px0 + lane_px;
    if (px < a.w) {
        const size_t pitch = (size_t)a.sw * 3;
        const long long first = (long long)K * ((long long)a.oy0 + toy) - K / 2;      // image sample row of LDS row 0
        const int s0 = K * (int)px - K / 2;                                            // first sample of the footprint
        const bool inside = s0 >= 0 && (uint32_t)(s0 + 2 * K) <= a.sw;
        for (uint32_t r = threadIdx.x / TW; r < n_rows; r += FT_BLOCK / TW) {
            // clamped to the image; then kept inside the band whatever the host passed (the host guarantees it covers the row)
            long long b = std::min<long long>(std::max<long long>(first + r, 0), (long long)a.sh - 1) - (long long)a.band_row0;
            b = std::min<long long>(std::max<long long>(b, 0), (long long)a.band_rows - 1);
            const unsigned char *row = a.src + (size_t)b * pitch;
            uint32_t f[T::NW];
            if (inside) {
                const unsigned char *p = row + 3 * (size_t)s0;
                const uint32_t mis = (uint32_t)((uintptr_t)p & 3);
                const uint32_t *q = (const uint32_t *)(p - mis);
                uint32_t d[T::NW + 1];
#pragma unroll
                for (int i = 0; i <= T::NW; i++) d[i] = q[i];
#pragma unroll
                for (int i = 0; i < T::NW; i++) f[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], mis);
            } else {
#pragma unroll
                for (int i = 0; i < T::NW; i++) {
                    uint32_t v = 0;
#pragma unroll
                    for (int bb = 0; bb < 4; bb++) {
                        const int j = 4 * i + bb;
                        const int sa = std::min(std::max(s0 + j / 3, 0), (int)a.sw - 1);
                        v |= (uint32_t)row[(size_t)sa * 3 + j % 3] << (8 * bb);
                    }
                    f[i] = v;
                }
            }
            uint32_t h0 = 0, h1 = 0, h2 = 0;
#pragma unroll
            for (int i = 0; i < T::NW; i++) {
                h0 = __builtin_amdgcn_udot4(f[i], T::weights(0, i), h0, false);
                h1 = __builtin_amdgcn_udot4(f[i], T::weights(1, i), h1, false);
                h2 = __builtin_amdgcn_udot4(f[i], T::weights(2, i), h2, false);
            }
            unsigned short *o = hs + r * LDS_PITCH + lane_px * 3;
            o[0] = (unsigned short)h0; o[1] = (unsigned short)h1; o[2] = (unsigned short)h2;
        }
    }
    __syncthreads();
    const uint32_t q4 = (threadIdx.x % 64) * 4;                         // first byte of this lane's four in the tile's row
    const uint32_t n_bytes = min((uint32_t)TW, a.w - px0) * 3;
    if (q4 < n_bytes) {
        for (uint32_t oy = threadIdx.x / 64; oy < n_oy; oy += FT_BLOCK / 64) {
            uint32_t s[4] = {0, 0, 0, 0};
#pragma unroll
            for (int v = 0; v < 2 * K; v++) {
                const uint2 x = *(const uint2 *)(hs + (K * oy + v) * LDS_PITCH + q4);
                s[0] += T::t(v) * (x.x & 0xFFFFu); s[1] += T::t(v) * (x.x >> 16);
                s[2] += T::t(v) * (x.y & 0xFFFFu); s[3] += T::t(v) * (x.y >> 16);
            }
            uint32_t o[4];
#pragma unroll
            for (int i = 0; i < 4; i++) o[i] = (s[i] + (1u << (T::SHIFT - 1))) >> T::SHIFT;
            unsigned char *dst = a.dst + ((size_t)(toy + oy) * a.w + px0) * 3 + q4;
            const uint32_t n = min(4u, n_bytes - q4);
            if (n == 4 && ((uintptr_t)dst & 3) == 0) *(uint32_t *)dst = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
            else for (uint32_t i = 0; i < n; i++) dst[i] = (unsigned char)o[i];
        }
    }
}

template <int K>
void launch_k(const TentArgs &a, dim3 grid, hipStream_t st)
{
    hipLaunchKernelGGL(maray_filter_tent<K>, grid, dim3(FT_BLOCK), 0, st, a);
}

}   // namespace

void filter_tent(uint32_t k, const TentArgs &a, hipStream_t st)
{
    if (!a.n_out || !a.w) return;
    if (!filter_samples_ok(k) || !a.src || !a.dst || (uint64_t)a.w * k != a.sw || !a.sh || !a.band_rows)
        throw Error{MARAY_E_INTERNAL, "tent filter: bad arguments"};
    const uint64_t lo = (uint64_t)k * a.oy0 >= k / 2 ? (uint64_t)k * a.oy0 - k / 2 : 0;
    const uint64_t hi = std::min<uint64_t>(a.sh, (uint64_t)k * ((uint64_t)a.oy0 + a.n_out) + k / 2);
    if (a.band_row0 > lo || (uint64_t)a.band_row0 + a.band_rows < hi || hi > a.sh || lo >= hi)
        throw Error{MARAY_E_INTERNAL, "tent filter: the band does not cover the rows' footprint"};
    const dim3 grid((a.w + FILTER_TILE_W - 1) / FILTER_TILE_W, (a.n_out + FILTER_TILE_H - 1) / FILTER_TILE_H);
    if (grid.y > 65535u) throw Error{MARAY_E_INTERNAL, "tent filter: too many rows in one pass"};
    (void)hipGetLastError();
    switch (k) {
    case 2: launch_k<2>(a, grid, st); break;
    case 4: launch_k<4>(a, grid, st); break;
    default: launch_k<8>(a, grid, st); break;
    }
    HIP_TRY(hipGetLastError());
}

float filter_time_tent(int device, uint32_t w, uint32_t rows, uint32_t k, int reps)
{
    if (!filter_samples_ok(k) || !w || !rows || reps <= 0 || (uint64_t)w * k > MARAY_DOMAIN_MAX || (uint64_t)rows * k > MARAY_DOMAIN_MAX ||
        (rows + FILTER_TILE_H - 1) / FILTER_TILE_H > 65535u)
        throw Error{MARAY_E_ARG, "filter_time_tent: k in {2, 4, 8}, w, rows and reps > 0, k w and k rows within the domain"};
    HIP_TRY(hipSetDevice(device));
    struct Own {
        unsigned char *src = nullptr, *dst = nullptr; hipStream_t st = nullptr; hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Own() { (void)hipFree(src); (void)hipFree(dst); if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); if (st) (void)hipStreamDestroy(st); }
    } o;
    const size_t src_bytes = (size_t)rows * k * w * k * 3, dst_bytes = (size_t)rows * w * 3;
    HIP_TRY(hipMalloc((void **)&o.src, src_bytes + 2 * FILTER_PAD));
    HIP_TRY(hipMalloc((void **)&o.dst, dst_bytes));
    measurement_fill(o.src, src_bytes + 2 * FILTER_PAD);
    HIP_TRY(hipStreamCreate(&o.st));
    HIP_TRY(hipEventCreate(&o.e0)); HIP_TRY(hipEventCreate(&o.e1));
    const TentArgs a{o.src + FILTER_PAD, o.dst, w, w * k, rows * k, 0, rows * k, 0, rows};
    filter_tent(k, a, o.st);
    HIP_TRY(hipEventRecord(o.e0, o.st));
    for (int i = 0; i < reps; i++) filter_tent(k, a, o.st);
    HIP_TRY(hipEventRecord(o.e1, o.st));
    HIP_TRY(hipEventSynchronize(o.e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, o.e0, o.e1));
    return ms / (float)reps;
}

}   // namespace maray
