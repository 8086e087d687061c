// shutter.hip — maray_shutter_reduce: the integer mean of n frames in HBM (product code; include/maray_hip.h, "shutter").
//
// Memory-bound: every byte of every frame is read once and one byte per pixel channel is written.  A lane takes 16 bytes
// of each frame as one global_load_dwordx4, widens even and odd bytes into packed 16-bit fields (& 0x00FF00FF) and adds
// them as dwords: a field holds at most 255 * 64 + 32 = 16352, so no carry crosses a field.  Up to 8 frames a pass; more
// frames go through 16-bit partial sums (32 bytes per lane, kept in the packed order -- the layout is the kernel's own),
// and the last pass rounds, shifts and writes bytes.  No atomics: a lane owns its 16 bytes.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>
#include <vector>

#include "shutter.hpp"

namespace maray {

namespace {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            throw Error{MARAY_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)};           \
    } while (0)

constexpr uint32_t SH_BLOCK = 256, SH_MAX_BLOCKS = 2048;      // grid-stride: a pass of the grid covers 2048 * 256 * 16 B = 8 MiB

template <int NF>
__global__ __launch_bounds__(256) void maray_shutter_reduce(const ShutterArgs a)
{
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
        // s[2 d] = bytes 4 d and 4 d + 2 of the vector, s[2 d + 1] = bytes 4 d + 1 and 4 d + 3, as 16-bit fields
        uint32_t s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (a.acc_in) {
            const uint4 lo = *(const uint4 *)(a.acc_in + at), hi = *(const uint4 *)(a.acc_in + at + 8);
            s[0] = lo.x; s[1] = lo.y; s[2] = lo.z; s[3] = lo.w; s[4] = hi.x; s[5] = hi.y; s[6] = hi.z; s[7] = hi.w;
        }
#pragma unroll
        for (int k = 0; k < NF; k++) {
            const uint32_t d[4] = {f[k].x, f[k].y, f[k].z, f[k].w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                s[2 * j] += d[j] & 0x00FF00FFu;
                s[2 * j + 1] += (d[j] >> 8) & 0x00FF00FFu;
            }
        }
        if (a.acc_out) {
            *(uint4 *)(a.acc_out + at) = make_uint4(s[0], s[1], s[2], s[3]);
            *(uint4 *)(a.acc_out + at + 8) = make_uint4(s[4], s[5], s[6], s[7]);
        } else {
            // per field: (sum + round) >> shift <= 255; the bits the shift drags in from the upper field land at bit
            // 16 - shift >= 10 and up, outside the byte the mask keeps
            const uint32_t r = a.round * 0x00010001u;
            uint32_t o[4];
#pragma unroll
            for (int j = 0; j < 4; j++)
                o[j] = (((s[2 * j] + r) >> a.shift) & 0x00FF00FFu) | ((((s[2 * j + 1] + r) >> a.shift) & 0x00FF00FFu) << 8);
            *(uint4 *)(a.dst + at) = make_uint4(o[0], o[1], o[2], o[3]);
        }
    }
    // head and tail, fewer than 16 bytes each, byte by byte (partial sums in plain element order: no vector covers them)
    if (blockIdx.x == 0 && threadIdx.x < 32) {
        const size_t tail0 = head + n_vec * 16;
        const size_t i = threadIdx.x < 16 ? (size_t)threadIdx.x : tail0 + (threadIdx.x - 16);
        const bool mine = threadIdx.x < 16 ? i < head : i < a.bytes;
        if (mine) {
            uint32_t sum = a.acc_in ? a.acc_in[i] : 0u;
#pragma unroll
            for (int k = 0; k < NF; k++) sum += a.frames[k][i];
            if (a.acc_out) a.acc_out[i] = (unsigned short)sum;
            else a.dst[i] = (unsigned char)((sum + a.round) >> a.shift);
        }
    }
}

template <int NF>
void launch_nf(const ShutterArgs &a, uint32_t grid, hipStream_t st)
{
    hipLaunchKernelGGL(maray_shutter_reduce<NF>, dim3(grid), dim3(SH_BLOCK), 0, st, a);
}

}   // namespace

uint32_t shutter_reduce_blocks(size_t bytes)
{
    const size_t blocks = (bytes / 16 + SH_BLOCK - 1) / SH_BLOCK;
    return (uint32_t)std::min<size_t>(std::max<size_t>(blocks, 1), SH_MAX_BLOCKS);
}

void shutter_reduce(const ShutterArgs &a, hipStream_t st)
{
    if (!a.bytes) return;
    if (!a.n_frames || a.n_frames > SHUTTER_GROUP || (!a.acc_out && !a.dst) || a.shift > 6)
        throw Error{MARAY_E_INTERNAL, "shutter reduce: bad arguments"};
    const uintptr_t mis = (uintptr_t)a.frames[0] & 15;
    bool ok = !a.dst || ((uintptr_t)a.dst & 15) == mis;
    for (uint32_t k = 0; k < a.n_frames; k++) ok = ok && a.frames[k] && ((uintptr_t)a.frames[k] & 15) == mis;
    for (const unsigned short *acc : {a.acc_in, (const unsigned short *)a.acc_out}) ok = ok && (!acc || ((uintptr_t)acc & 31) == 2 * mis);
    if (!ok) throw Error{MARAY_E_INTERNAL, "shutter reduce: pointers are not congruent modulo 16"};
    const uint32_t grid = shutter_reduce_blocks(a.bytes);
    (void)hipGetLastError();
    switch (a.n_frames) {
    case 1: launch_nf<1>(a, grid, st); break;
    case 2: launch_nf<2>(a, grid, st); break;
    case 3: launch_nf<3>(a, grid, st); break;
    case 4: launch_nf<4>(a, grid, st); break;
    case 5: launch_nf<5>(a, grid, st); break;
    case 6: launch_nf<6>(a, grid, st); break;
    case 7: launch_nf<7>(a, grid, st); break;
    default: launch_nf<8>(a, grid, st); break;
    }
    HIP_TRY(hipGetLastError());
}

void ShutterScratch::ensure(size_t bytes, uint32_t n, bool lin)
{
    const size_t want = need(bytes, n, lin);
    if (want <= cap) return;
    if (base) HIP_TRY(hipFree(base));
    base = nullptr; cap = 0;
    HIP_TRY(hipMalloc((void **)&base, want));
    cap = want;
}

void ShutterScratch::release()
{
    if (base) (void)hipFree(base);
    base = nullptr; cap = 0;
}

void measurement_fill(unsigned char *d_buf, size_t bytes)
{
    const char *e = getenv("MARAY_TIME_RANDOM_BYTES");
    if (!e || e[0] != '1') { HIP_TRY(hipMemset(d_buf, 0x5A, bytes)); return; }
    std::vector<uint64_t> host((bytes + 7) / 8);
    uint64_t x = 0x9e3779b97f4a7c15ull;
    for (uint64_t &w : host) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; w = x * 0x2545f4914f6cdd1dull; }      // xorshift64*: every byte of a word is used
    HIP_TRY(hipMemcpy(d_buf, host.data(), bytes, hipMemcpyHostToDevice));
}

float shutter_time_reduce(int device, size_t bytes, uint32_t n, int reps, uint32_t transfer)
{
    if (!shutter_frames_ok(n) || n < 2 || !bytes || reps <= 0) throw Error{MARAY_E_ARG, "shutter_time_reduce: n in 2 .. 64 (a power of two), bytes and reps > 0"};
    HIP_TRY(hipSetDevice(device));
    struct Own {
        ShutterScratch s; unsigned char *dst = nullptr; hipStream_t st = nullptr; hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Own() { s.release(); (void)hipFree(dst); if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); if (st) (void)hipStreamDestroy(st); }
    } o;
    HIP_TRY(hipMalloc((void **)&o.dst, bytes));
    o.s.ensure(bytes, n, transfer == MARAY_TRANSFER_SRGB);
    measurement_fill(o.s.base, o.s.cap);
    HIP_TRY(hipStreamCreate(&o.st));
    HIP_TRY(hipEventCreate(&o.e0)); HIP_TRY(hipEventCreate(&o.e1));
    auto once = [&] { shutter_render(o.s, nullptr, n, 0, bytes, o.dst, o.st, [](const double *) {}, [](unsigned char *) {}, transfer); };
    once();
    HIP_TRY(hipEventRecord(o.e0, o.st));
    for (int i = 0; i < reps; i++) once();
    HIP_TRY(hipEventRecord(o.e1, o.st));
    HIP_TRY(hipEventSynchronize(o.e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, o.e0, o.e1));
    return ms / (float)reps;
}

}   // namespace maray
