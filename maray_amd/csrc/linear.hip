// linear.hip — the reduces in linear light (product code; include/maray_hip.h, "transfer"): maray_filter_box_lin<K>,
// maray_filter_tent_lin<K> and maray_shutter_reduce_lin<NF>.  Each is its byte kernel's contract (filter.hip, shutter.hip) with
// a decode in front of the sum and an encode behind it: out = E((SUM w_i D[s_i] + W/2) >> log2 W), integers throughout.
//
// Tables.  D (256 x 16 bits) and the encode table (4096 x 16 bits, one entry per 16-wide bin of M: the count c of thresholds up
// to the bin's end in the low byte, and above it the offset inside the bin of the one threshold the bin may hold, so that
// E(M) = c - ((M & 15) < offset): one read and one compare, no search) are built at compile time from the literals of
// include/maray_transfer_table.h and copied into LDS once per block, 8.5 KiB as 544 16-byte vectors.  Blocks therefore loop
// over tiles of rows (at most ~2048 blocks a pass) instead of taking one tile each: at K = 2 a tile's samples are fewer bytes
// than the tables.
// Layout: both tables stay PACKED 16-bit.  A byte-indexed read (ds_read_u16) is banked by dword address modulo 32 within a
// 32-lane group and equal dwords broadcast; lanes that read different dwords of one bank serialise.  Packing halves the
// distinct dwords a group can touch (128 for D) and makes neighbouring sample values -- what adjacent lanes hold wherever the
// picture is smooth -- share a dword or sit on adjacent banks; one copy per group of lanes (replication) would need 32 copies
// to be conflict-free, 16 KiB for D alone and 272 KiB for both.  What is left is the random-value case: 32 reads over 32 banks,
// about 3 to 4 deep.  Unconfirmed until a counter run (SQ_LDS_BANK_CONFLICT) exists.
//
// maray_filter_box_lin<K>: a lane takes one output pixel of one output row: K sample rows of 3 K consecutive bytes (the
// neighbouring lane's start 3 K further on: a wavefront reads contiguous stretches), each row as ceil(3K / 4) + 1 aligned dwords
// shifted into place (v_alignbyte_b32), every byte decoded through LDS, three 32-bit sums (<= 64 * 65535), three byte stores.  No
// halo, no clamp: every footprint lies in the image.
// maray_filter_tent_lin<K>: filter.hip's two stages.  Horizontal sums are <= 65535 * 2 K^2 (24 bits at K = 8), so the LDS
// intermediate is 32-bit, (K TH + K) rows of 64 * 3 dwords; v_dot4_u32_u8 no longer applies (16-bit operands), the weights are
// v_mad_u32_u24 against constants.  Tile: 64 pixels wide for every K (a wavefront's loads stay one contiguous stretch), TH rows
// high: TH = 8 for K = 2, 4 (13.5 / 27 KiB + the tables: 7 / 4 blocks per CU of 160 KiB), TH = 4 for K = 8 -- 64 x 8 would take
// 54 KiB + tables = 2 blocks (8 waves) per CU; 64 x 4 takes 30 KiB + tables = 4 blocks, at the price of reading 1/4 instead of
// 1/8 of the tile's sample rows twice.
// maray_shutter_reduce_lin<NF>: shutter.hip's pass with 16 decoded sums of 32 bits per lane; partial sums between groups of 8
// frames are 32-bit in plain element order (64 bytes per lane).
// No inline assembly, no scratch memory (every array is unrolled into registers), no atomics; nothing outside the destination
// rows is written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "filter.hpp"
#include "maray_transfer_table.h"
#include "shutter.hpp"

namespace maray {

namespace {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            throw Error{MARAY_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)};           \
    } while (0)

// ---- the tables ---------------------------------------------------------------------------------------------------------
constexpr int LUT_D = 0, LUT_E = 256, LUT_N = 256 + 4096;      // 16-bit entries
struct alignas(16) LinTables { unsigned short v[LUT_N]; };

constexpr LinTables make_lin_tables()
{
    LinTables t{};
    const unsigned short d[256] = {MARAY_SRGB_DECODE_LIST};
    for (int v = 0; v < 256; v++) t.v[LUT_D + v] = d[v];
    int c = 0;                                      // thresholds T[1 .. c] lie at or below the end of the bin before
    for (int b = 0; b < 4096; b++) {
        unsigned off = 0;
        while (c < 255) {
            const unsigned T = ((unsigned)d[c] + d[c + 1] + 1) >> 1;       // T[c + 1]
            if (T > 16u * b + 15u) break;
            c++; off = T & 15u;                     // in this bin: every earlier bin took what lies below it
        }
        t.v[LUT_E + b] = (unsigned short)(c | (off << 8));
    }
    return t;
}

// what the one-compare encoder rests on: no 16-wide bin holds two thresholds
constexpr bool one_threshold_per_bin()
{
    const unsigned short d[256] = {MARAY_SRGB_DECODE_LIST};
    unsigned last = 0xFFFFFFFFu;
    for (int v = 1; v < 256; v++) {
        const unsigned b = (((unsigned)d[v - 1] + d[v] + 1) >> 1) >> 4;
        if (b == last) return false;
        last = b;
    }
    return d[0] == 0 && d[255] == 65535;
}
static_assert(one_threshold_per_bin(), "the decode table's thresholds must fall into distinct 16-wide bins");

__device__ const LinTables g_lin_tables = make_lin_tables();

constexpr int LIN_BLOCK = 256;

__device__ __forceinline__ void lin_fill(unsigned short *lut)
{
    static_assert(sizeof(LinTables) % 16 == 0, "whole vectors");
    for (uint32_t i = threadIdx.x; i < sizeof(LinTables) / 16; i += LIN_BLOCK) ((uint4 *)lut)[i] = ((const uint4 *)g_lin_tables.v)[i];
}

__device__ __forceinline__ uint32_t lin_decode(const unsigned short *lut, uint32_t byte) { return lut[LUT_D + byte]; }

__device__ __forceinline__ uint32_t lin_encode(const unsigned short *lut, uint32_t m)       // m <= 65535
{
    const uint32_t e = lut[LUT_E + (m >> 4)];
    return (e & 0xFFu) - ((m & 15u) < (e >> 8) ? 1u : 0u);
}

constexpr int TW = (int)FILTER_TILE_W;
constexpr uint32_t LIN_MAX_BLOCKS = 2048;

// ---- box ----------------------------------------------------------------------------------------------------------------
template <int K>
struct BoxLin {
    static constexpr int NW = (3 * K + 3) / 4;      // dwords that hold a pixel's 3 K bytes of one sample row
    static constexpr int SHIFT = K == 2 ? 2 : K == 4 ? 4 : 6;          // log2(K^2)
};

template <int K>
__global__ __launch_bounds__(LIN_BLOCK) void maray_filter_box_lin(const TentArgs a)
{
    using B = BoxLin<K>;
    __shared__ __attribute__((aligned(16))) unsigned short lut[LUT_N];
    lin_fill(lut);
    __syncthreads();
    const uint32_t px = blockIdx.x * TW + threadIdx.x % TW;
    if (px >= a.w) return;
    const size_t pitch = (size_t)a.sw * 3;
    for (uint32_t oy = blockIdx.y * (LIN_BLOCK / TW) + threadIdx.x / TW; oy < a.n_out; oy += gridDim.y * (LIN_BLOCK / TW)) {
        const long long first = (long long)K * ((long long)a.oy0 + oy) - (long long)a.band_row0;      // band row of the pixel's first sample row
        uint32_t s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
        for (int j = 0; j < K; j++) {
            // kept inside the band whatever the host passed (the host guarantees it covers the rows)
            const long long b = std::min<long long>(std::max<long long>(first + j, 0), (long long)a.band_rows - 1);
            const unsigned char *p = a.src + (size_t)b * pitch + 3 * (size_t)K * px;
            const uint32_t mis = (uint32_t)((uintptr_t)p & 3);
            const uint32_t *q = (const uint32_t *)(p - mis);
            uint32_t d[B::NW + 1];
#pragma unroll
            for (int i = 0; i <= B::NW; i++) d[i] = q[i];
#pragma unroll
            for (int i = 0; i < B::NW; i++) {
                const uint32_t f = __builtin_amdgcn_alignbyte(d[i + 1], d[i], mis);
#pragma unroll
                for (int bb = 0; bb < 4; bb++) {
                    const int jj = 4 * i + bb;
                    if (jj < 3 * K) {
                        const uint32_t v = lin_decode(lut, (f >> (8 * bb)) & 0xFFu);
                        if (jj % 3 == 0) s0 += v; else if (jj % 3 == 1) s1 += v; else s2 += v;
                    }
                }
            }
        }
        constexpr uint32_t half = 1u << (B::SHIFT - 1);
        unsigned char *dst = a.dst + ((size_t)oy * a.w + px) * 3;
        dst[0] = (unsigned char)lin_encode(lut, (s0 + half) >> B::SHIFT);
        dst[1] = (unsigned char)lin_encode(lut, (s1 + half) >> B::SHIFT);
        dst[2] = (unsigned char)lin_encode(lut, (s2 + half) >> B::SHIFT);
    }
}

// ---- tent ---------------------------------------------------------------------------------------------------------------
constexpr int LDS_PITCH = TW * 3;       // 32-bit sums per LDS row

template <int K>
struct TentLin {
    static constexpr int NW = 6 * K / 4;            // dwords of a pixel's footprint in one sample row
    static constexpr int TH = K == 8 ? 4 : 8;       // output rows of a tile (see the head of this file)
    static constexpr int ROWS = K * TH + K;         // sample rows a tile reads
    static constexpr int SHIFT = K == 2 ? 6 : K == 4 ? 10 : 14;        // log2(4 K^4)
    static constexpr uint32_t t(int i) { const int d = 2 * i + 1 - 2 * K; return (uint32_t)(2 * K - (d < 0 ? -d : d)); }
};

template <int K>
__global__ __launch_bounds__(LIN_BLOCK) void maray_filter_tent_lin(const TentArgs a, const uint32_t tiles_y)
{
    using T = TentLin<K>;
    __shared__ __attribute__((aligned(16))) unsigned short lut[LUT_N];
    __shared__ __attribute__((aligned(16))) uint32_t hs[T::ROWS * LDS_PITCH];
    lin_fill(lut);
    const uint32_t px0 = blockIdx.x * TW;
    const uint32_t lane_px = threadIdx.x % TW, px = px0 + lane_px;
    const size_t pitch = (size_t)a.sw * 3;
    const int s0 = K * (int)px - K / 2;                                            // first sample of the footprint
    const bool inside = s0 >= 0 && (uint32_t)(s0 + 2 * K) <= a.sw;
    for (uint32_t ty = blockIdx.y; ty < tiles_y; ty += gridDim.y) {      // (uniform in the block: the barriers are met by all)
        __syncthreads();        // the tables are filled; the tile before is read
        const uint32_t toy = ty * T::TH;
        const uint32_t n_oy = min((uint32_t)T::TH, a.n_out - toy);
        const uint32_t n_rows = K * n_oy + K;
        if (px < a.w) {
            const long long first = (long long)K * ((long long)a.oy0 + toy) - K / 2;      // image sample row of LDS row 0
            for (uint32_t r = threadIdx.x / TW; r < n_rows; r += LIN_BLOCK / TW) {
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
#pragma unroll
                    for (int bb = 0; bb < 4; bb++) {
                        const int j = 4 * i + bb;
                        const uint32_t v = T::t(j / 3) * lin_decode(lut, (f[i] >> (8 * bb)) & 0xFFu);
                        if (j % 3 == 0) h0 += v; else if (j % 3 == 1) h1 += v; else h2 += v;
                    }
                }
                uint32_t *o = hs + r * LDS_PITCH + lane_px * 3;
                o[0] = h0; o[1] = h1; o[2] = h2;
            }
        }
        __syncthreads();
        const uint32_t q4 = (threadIdx.x % 64) * 4;                         // first byte of this lane's four in the tile's row
        const uint32_t n_bytes = min((uint32_t)TW, a.w - px0) * 3;
        if (q4 < n_bytes) {
            for (uint32_t oy = threadIdx.x / 64; oy < n_oy; oy += LIN_BLOCK / 64) {
                uint32_t s[4] = {0, 0, 0, 0};
#pragma unroll
                for (int v = 0; v < 2 * K; v++) {
                    const uint4 x = *(const uint4 *)(hs + (K * oy + v) * LDS_PITCH + q4);
                    s[0] += T::t(v) * x.x; s[1] += T::t(v) * x.y; s[2] += T::t(v) * x.z; s[3] += T::t(v) * x.w;
                }
                uint32_t o[4];
#pragma unroll
                for (int i = 0; i < 4; i++) o[i] = lin_encode(lut, (s[i] + (1u << (T::SHIFT - 1))) >> T::SHIFT);
                unsigned char *dst = a.dst + ((size_t)(toy + oy) * a.w + px0) * 3 + q4;
                const uint32_t n = min(4u, n_bytes - q4);
                if (n == 4 && ((uintptr_t)dst & 3) == 0) *(uint32_t *)dst = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
                else for (uint32_t i = 0; i < n; i++) dst[i] = (unsigned char)o[i];
            }
        }
    }
}

template <int K>
void launch_filter_k(uint32_t filter, const TentArgs &a, hipStream_t st)
{
    const uint32_t gx = (a.w + FILTER_TILE_W - 1) / FILTER_TILE_W;
    const uint32_t by_budget = std::max(1u, LIN_MAX_BLOCKS / gx);
    if (filter == MARAY_FILTER_TENT) {
        const uint32_t tiles_y = (a.n_out + TentLin<K>::TH - 1) / TentLin<K>::TH;
        hipLaunchKernelGGL(maray_filter_tent_lin<K>, dim3(gx, std::min(tiles_y, by_budget)), dim3(LIN_BLOCK), 0, st, a, tiles_y);
    } else {
        const uint32_t groups = (a.n_out + LIN_BLOCK / TW - 1) / (LIN_BLOCK / TW);      // of 4 rows
        hipLaunchKernelGGL(maray_filter_box_lin<K>, dim3(gx, std::min(groups, by_budget)), dim3(LIN_BLOCK), 0, st, a);
    }
}

// ---- shutter ------------------------------------------------------------------------------------------------------------
constexpr uint32_t SH_BLOCK = 256;

template <int NF>
__global__ __launch_bounds__(SH_BLOCK) void maray_shutter_reduce_lin(const ShutterLinArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned short lut[LUT_N];
    lin_fill(lut);
    __syncthreads();
    // the pointers are congruent modulo 16: `head` bytes up to the first 16-byte boundary, whole vectors, a tail
    const size_t mis = (size_t)((uintptr_t)a.frames[0] & 15);
    const size_t head = mis ? (16 - mis < a.bytes ? 16 - mis : a.bytes) : 0;
    const size_t n_vec = (a.bytes - head) / 16;
    const size_t stride = (size_t)gridDim.x * SH_BLOCK;
    for (size_t v = (size_t)blockIdx.x * SH_BLOCK + threadIdx.x; v < n_vec; v += stride) {
        const size_t at = head + v * 16;
        uint4 f[NF];
#pragma unroll
        for (int k = 0; k < NF; k++) f[k] = *(const uint4 *)(a.frames[k] + at);
        uint32_t s[16];         // element order
        if (a.acc_in) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint4 x = *(const uint4 *)(a.acc_in + at + 4 * j);
                s[4 * j] = x.x; s[4 * j + 1] = x.y; s[4 * j + 2] = x.z; s[4 * j + 3] = x.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 16; j++) s[j] = 0;
        }
#pragma unroll
        for (int k = 0; k < NF; k++) {
            const uint32_t d[4] = {f[k].x, f[k].y, f[k].z, f[k].w};
#pragma unroll
            for (int j = 0; j < 16; j++) s[j] += lin_decode(lut, (d[j / 4] >> (8 * (j % 4))) & 0xFFu);
        }
        if (a.acc_out) {
#pragma unroll
            for (int j = 0; j < 4; j++) *(uint4 *)(a.acc_out + at + 4 * j) = make_uint4(s[4 * j], s[4 * j + 1], s[4 * j + 2], s[4 * j + 3]);
        } else {
            uint32_t o[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                o[j] = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) o[j] |= lin_encode(lut, (s[4 * j + b] + a.round) >> a.shift) << (8 * b);
            }
            *(uint4 *)(a.dst + at) = make_uint4(o[0], o[1], o[2], o[3]);
        }
    }
    // head and tail, fewer than 16 bytes each, byte by byte
    if (blockIdx.x == 0 && threadIdx.x < 32) {
        const size_t tail0 = head + n_vec * 16;
        const size_t i = threadIdx.x < 16 ? (size_t)threadIdx.x : tail0 + (threadIdx.x - 16);
        const bool mine = threadIdx.x < 16 ? i < head : i < a.bytes;
        if (mine) {
            uint32_t sum = a.acc_in ? a.acc_in[i] : 0u;
#pragma unroll
            for (int k = 0; k < NF; k++) sum += lin_decode(lut, a.frames[k][i]);
            if (a.acc_out) a.acc_out[i] = sum;
            else a.dst[i] = (unsigned char)lin_encode(lut, (sum + a.round) >> a.shift);
        }
    }
}

template <int NF>
void launch_shutter_nf(const ShutterLinArgs &a, uint32_t grid, hipStream_t st)
{
    hipLaunchKernelGGL(maray_shutter_reduce_lin<NF>, dim3(grid), dim3(SH_BLOCK), 0, st, a);
}

}   // namespace

void filter_lin(uint32_t filter, uint32_t k, const TentArgs &a, hipStream_t st)
{
    if (!a.n_out || !a.w) return;
    const bool tent = filter == MARAY_FILTER_TENT;
    if (!filter_samples_ok(k) || (filter != MARAY_FILTER_BOX && !tent) || !a.src || !a.dst || (uint64_t)a.w * k != a.sw || !a.sh || !a.band_rows)
        throw Error{MARAY_E_INTERNAL, "linear filter: bad arguments"};
    const uint32_t halo = tent ? k / 2 : 0;
    const uint64_t lo = (uint64_t)k * a.oy0 >= halo ? (uint64_t)k * a.oy0 - halo : 0;
    const uint64_t hi = std::min<uint64_t>(a.sh, (uint64_t)k * ((uint64_t)a.oy0 + a.n_out) + halo);
    if (a.band_row0 > lo || (uint64_t)a.band_row0 + a.band_rows < hi || hi > a.sh || lo >= hi || (uint64_t)k * ((uint64_t)a.oy0 + a.n_out) > a.sh)
        throw Error{MARAY_E_INTERNAL, "linear filter: the band does not cover the rows' footprint"};
    (void)hipGetLastError();
    switch (k) {
    case 2: launch_filter_k<2>(filter, a, st); break;
    case 4: launch_filter_k<4>(filter, a, st); break;
    default: launch_filter_k<8>(filter, a, st); break;
    }
    HIP_TRY(hipGetLastError());
}

float filter_time_lin(int device, uint32_t w, uint32_t rows, uint32_t k, uint32_t filter, int reps)
{
    if (!filter_samples_ok(k) || (filter != MARAY_FILTER_BOX && filter != MARAY_FILTER_TENT) || !w || !rows || reps <= 0 ||
        (uint64_t)w * k > MARAY_DOMAIN_MAX || (uint64_t)rows * k > MARAY_DOMAIN_MAX)
        throw Error{MARAY_E_ARG, "filter_time_lin: k in {2, 4, 8}, filter box or tent, w, rows and reps > 0, k w and k rows within the domain"};
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
    filter_lin(filter, k, a, o.st);
    HIP_TRY(hipEventRecord(o.e0, o.st));
    for (int i = 0; i < reps; i++) filter_lin(filter, k, a, o.st);
    HIP_TRY(hipEventRecord(o.e1, o.st));
    HIP_TRY(hipEventSynchronize(o.e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, o.e0, o.e1));
    return ms / (float)reps;
}

void shutter_reduce_lin(const ShutterLinArgs &a, hipStream_t st)
{
    if (!a.bytes) return;
    if (!a.n_frames || a.n_frames > SHUTTER_GROUP || (!a.acc_out && !a.dst) || a.shift > 6)
        throw Error{MARAY_E_INTERNAL, "linear shutter reduce: bad arguments"};
    const uintptr_t mis = (uintptr_t)a.frames[0] & 15;
    bool ok = !a.dst || ((uintptr_t)a.dst & 15) == mis;
    for (uint32_t k = 0; k < a.n_frames; k++) ok = ok && a.frames[k] && ((uintptr_t)a.frames[k] & 15) == mis;
    for (const uint32_t *acc : {a.acc_in, (const uint32_t *)a.acc_out}) ok = ok && (!acc || ((uintptr_t)acc & 63) == 4 * mis);
    if (!ok) throw Error{MARAY_E_INTERNAL, "linear shutter reduce: pointers are not congruent modulo 16"};
    const uint32_t grid = shutter_reduce_blocks(a.bytes);
    (void)hipGetLastError();
    switch (a.n_frames) {
    case 1: launch_shutter_nf<1>(a, grid, st); break;
    case 2: launch_shutter_nf<2>(a, grid, st); break;
    case 3: launch_shutter_nf<3>(a, grid, st); break;
    case 4: launch_shutter_nf<4>(a, grid, st); break;
    case 5: launch_shutter_nf<5>(a, grid, st); break;
    case 6: launch_shutter_nf<6>(a, grid, st); break;
    case 7: launch_shutter_nf<7>(a, grid, st); break;
    default: launch_shutter_nf<8>(a, grid, st); break;
    }
    HIP_TRY(hipGetLastError());
}

}   // namespace maray
