// catrom.hip — maray_filter_catrom<K>: the Catmull-Rom reconstruction filter of a supersampled render (product code;
// include/maray_hip.h, "reconstruction filter").
//
// The tent's two stages (filter.hip) with a footprint twice as wide, signed weights and wider sums.  A block of 256 lanes
// computes a tile of TW x TH output pixels (64 x 16 / 64 x 8 / 32 x 8 for K = 2 / 4 / 8):
//   1. horizontal.  A lane takes one output pixel of one sample row: its footprint is 4K samples = 12K consecutive bytes (the
//      neighbouring lane's starts 3K bytes further on).  It loads the 3K + 1 aligned dwords that cover them, shifts them into
//      place (v_alignbyte_b32) and forms the three channels' sums byte by byte: the weights e(u) are signed and up to 14 bits,
//      so v_dot4_u32_u8 does not apply; a byte times a weight is a 24-bit multiply.  The sums (26 bits signed at K = 8) go to
//      LDS as 32-bit values, K TH + 3K rows of 3 TW.  The first two and the last two pixels of an image row reach over the
//      image's edge: those lanes gather their bytes one by one, clamped by index.
//   2. vertical.  A lane takes four consecutive bytes of one output row of the tile: 4K 16-byte LDS reads down the column,
//      sums of 32 bits at K = 2 (26 bits signed) and of 64 bits at K = 4 and 8 (34 and 42 bits signed: 32 would be wrong),
//      round, arithmetic shift, clamp to 0 .. 255, one dword store (bytes where the destination is not aligned or the row ends).
// LDS: 38 * 768 = 28.5 KiB, 44 * 768 = 33 KiB, 88 * 384 = 33 KiB for K = 2 / 4 / 8 (four blocks and more per CU).  No atomics,
// no scratch.  Rows are clamped to the image by index (band_row0 says where the band lies in it), never to the band: an
// interior band must bring its halo rows, 3K/2 on either side.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <type_traits>

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

constexpr int CR_BLOCK = 256;

template <int K>
struct Catrom {
    static constexpr int TW = (int)catrom_tile_w(K), TH = (int)catrom_tile_h(K);
    static constexpr int PITCH = TW * 3;            // 32-bit sums per LDS row
    static constexpr int NW = 3 * K;                // dwords of a pixel's footprint in one sample row (12K bytes)
    static constexpr int ROWS = K * TH + 3 * K;     // sample rows a tile reads
    static constexpr int SHIFT = K == 2 ? 16 : K == 4 ? 24 : 32;       // log2((16 K^4)^2)
    // e(u) for u = i - 3K/2, i = 0 .. 4K - 1: 2 D^3 CatmullRom(n / D) with n = |2u + 1 - K|, D = 2K
    static constexpr int e(int i) {
        const int d = 2 * i + 1 - 4 * K, n = d < 0 ? -d : d, D = 2 * K;
        return n < D ? 3 * n * n * n - 5 * n * n * D + 2 * D * D * D : -n * n * n + 5 * n * n * D - 8 * n * D * D + 4 * D * D * D;
    }
    using Acc = typename std::conditional<K == 2, int, long long>::type;       // the vertical sums
};

template <int K>
__global__ __launch_bounds__(CR_BLOCK) void maray_filter_catrom(const TentArgs a)
{
    using T = Catrom<K>;
    constexpr int TW = T::TW, TH = T::TH, PITCH = T::PITCH;
    __shared__ __attribute__((aligned(16))) int hs[T::ROWS * PITCH];
    const uint32_t px0 = blockIdx.x * TW, toy = blockIdx.y * TH;       // the tile: first pixel, first row (of this pass)
    const uint32_t n_oy = min((uint32_t)TH, a.n_out - toy);
    const uint32_t n_rows = K * n_oy + 3 * K;
    const uint32_t lane_px = threadIdx.x % TW, px = px0 + lane_px;
    if (px < a.w) {
        const size_t pitch = (size_t)a.sw * 3;
        const long long first = (long long)K * ((long long)a.oy0 + toy) - 3 * K / 2;  // image sample row of LDS row 0
        const int s0 = K * (int)px - 3 * K / 2;                                        // first sample of the footprint
        const bool inside = s0 >= 0 && (uint32_t)(s0 + 4 * K) <= a.sw;
        for (uint32_t r = threadIdx.x / TW; r < n_rows; r += CR_BLOCK / TW) {
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
            // byte j of the footprint is channel j % 3 of sample j / 3
            int h[3] = {0, 0, 0};
#pragma unroll
            for (int j = 0; j < 4 * T::NW; j++) h[j % 3] += T::e(j / 3) * (int)((f[j / 4] >> (8 * (j % 4))) & 0xFFu);
            int *o = hs + r * PITCH + lane_px * 3;
            o[0] = h[0]; o[1] = h[1]; o[2] = h[2];
        }
    }
    __syncthreads();
    const uint32_t n_bytes = min((uint32_t)TW, a.w - px0) * 3;
    constexpr uint32_t Q = PITCH / 4;                                   // lanes a tile's row takes, four bytes each
    for (uint32_t item = threadIdx.x; item < n_oy * Q; item += CR_BLOCK) {
        const uint32_t oy = item / Q, q4 = (item % Q) * 4;             // the row; the first byte of this lane's four in it
        if (q4 >= n_bytes) continue;
        typename T::Acc s[4] = {0, 0, 0, 0};
#pragma unroll
        for (int v = 0; v < 4 * K; v++) {
            const int4 x = *(const int4 *)(hs + (K * oy + v) * PITCH + q4);
            s[0] += (typename T::Acc)T::e(v) * x.x; s[1] += (typename T::Acc)T::e(v) * x.y;
            s[2] += (typename T::Acc)T::e(v) * x.z; s[3] += (typename T::Acc)T::e(v) * x.w;
        }
        uint32_t o[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            // (an arithmetic shift of a signed sum; how it rounds a negative sum cannot show: the clamp makes it 0)
            const typename T::Acc m = (s[i] + ((typename T::Acc)1 << (T::SHIFT - 1))) >> T::SHIFT;
            o[i] = (uint32_t)std::min<typename T::Acc>(std::max<typename T::Acc>(m, 0), 255);
        }
        unsigned char *dst = a.dst + ((size_t)(toy + oy) * a.w + px0) * 3 + q4;
        const uint32_t n = min(4u, n_bytes - q4);
        if (n == 4 && ((uintptr_t)dst & 3) == 0) *(uint32_t *)dst = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
        else for (uint32_t i = 0; i < n; i++) dst[i] = (unsigned char)o[i];
    }
}

template <int K>
void launch_k(const TentArgs &a, hipStream_t st)
{
    const dim3 grid((a.w + catrom_tile_w(K) - 1) / catrom_tile_w(K), (a.n_out + catrom_tile_h(K) - 1) / catrom_tile_h(K));
    if (grid.y > 65535u) throw Error{MARAY_E_INTERNAL, "catrom filter: too many rows in one pass"};
    hipLaunchKernelGGL(maray_filter_catrom<K>, grid, dim3(CR_BLOCK), 0, st, a);
}

}   // namespace

void filter_catrom(uint32_t k, const TentArgs &a, hipStream_t st)
{
    if (!a.n_out || !a.w) return;
    if (!filter_samples_ok(k) || !a.src || !a.dst || (uint64_t)a.w * k != a.sw || !a.sh || !a.band_rows)
        throw Error{MARAY_E_INTERNAL, "catrom filter: bad arguments"};
    const uint64_t halo = filter_halo(MARAY_FILTER_CATROM, k);
    const uint64_t lo = (uint64_t)k * a.oy0 >= halo ? (uint64_t)k * a.oy0 - halo : 0;
    const uint64_t hi = std::min<uint64_t>(a.sh, (uint64_t)k * ((uint64_t)a.oy0 + a.n_out) + halo);
    if (a.band_row0 > lo || (uint64_t)a.band_row0 + a.band_rows < hi || hi > a.sh || lo >= hi)
        throw Error{MARAY_E_INTERNAL, "catrom filter: the band does not cover the rows' footprint"};
    (void)hipGetLastError();
    switch (k) {
    case 2: launch_k<2>(a, st); break;
    case 4: launch_k<4>(a, st); break;
    default: launch_k<8>(a, st); break;
    }
    HIP_TRY(hipGetLastError());
}

float filter_time_catrom(int device, uint32_t w, uint32_t rows, uint32_t k, int reps)
{
    if (!filter_samples_ok(k) || !w || !rows || reps <= 0 || (uint64_t)w * k > MARAY_DOMAIN_MAX || (uint64_t)rows * k > MARAY_DOMAIN_MAX ||
        (rows + catrom_tile_h(k) - 1) / catrom_tile_h(k) > 65535u)
        throw Error{MARAY_E_ARG, "filter_time_catrom: k in {2, 4, 8}, w, rows and reps > 0, k w and k rows within the domain"};
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
    filter_catrom(k, a, o.st);
    HIP_TRY(hipEventRecord(o.e0, o.st));
    for (int i = 0; i < reps; i++) filter_catrom(k, a, o.st);
    HIP_TRY(hipEventRecord(o.e1, o.st));
    HIP_TRY(hipEventSynchronize(o.e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, o.e0, o.e1));
    return ms / (float)reps;
}

}   // namespace maray
