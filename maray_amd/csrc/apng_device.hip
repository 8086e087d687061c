// apng_device.hip — the kernels of the animation writer (product code; include/maray_hip.h, "animation").
//
//   maray_frame_delta      the two rasters as 3 w h bytes each.  A lane takes 16 bytes per step: `cur` as one aligned 16-byte
//                          vector (the bytes in front of the first boundary and behind the last whole vector, fewer than 16
//                          each, go byte by byte to the first lanes of block 0), `prev` -- at any other alignment -- as the
//                          two aligned vectors that hold the same 16 bytes, shifted into place (the dword offset by selects
//                          on a wave-uniform value, the byte offset by v_alignbyte_b32).  Where the XOR is zero, which is
//                          nearly everywhere in an animation, that is all.  Else the lane makes the 16-bit mask of its
//                          differing bytes, divides once to find the pixel (x, y) of its first byte and walks the at most
//                          seven pixels its bytes belong to.  Lanes keep a box (min x, min y, max x + 1, max y + 1); a
//                          wavefront reduces its lanes' boxes by shuffles, a block its wavefronts' through LDS, and every
//                          block STORES its box: partials[blockIdx.x].  The grid is capped at DELTA_MAX_BLOCKS and lanes
//                          stride over the vectors.
//   maray_frame_delta_box  one block: the partial boxes reduced the same way, the empty box written as 0 0 0 0.
// No atomics, no inline assembly, no scratch memory; nothing is written but the partial boxes and the box.
#include <hip/hip_runtime.h>

#include <string>

#include "apng_device.hpp"
#include "shutter.hpp"

namespace maray {

namespace {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            throw Error{MARAY_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)};           \
    } while (0)

struct DeltaArgs {
    const unsigned char *prev, *cur;
    uint32_t *partials;             // gridDim.x boxes
    uint32_t w, bytes;              // 3 w h <= 2^30
};

struct Box {                        // empty: x0 = y0 = ~0, x1 = y1 = 0
    uint32_t x0, y0, x1, y1;
    __device__ __forceinline__ void add(uint32_t x, uint32_t y) { x0 = min(x0, x); y0 = min(y0, y); x1 = max(x1, x + 1u); y1 = max(y1, y + 1u); }
    __device__ __forceinline__ void join(const Box &o) { x0 = min(x0, o.x0); y0 = min(y0, o.y0); x1 = max(x1, o.x1); y1 = max(y1, o.y1); }
};

__device__ __forceinline__ Box wave_box(Box b)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        Box o;
        o.x0 = (uint32_t)__shfl_xor((int)b.x0, d); o.y0 = (uint32_t)__shfl_xor((int)b.y0, d);
        o.x1 = (uint32_t)__shfl_xor((int)b.x1, d); o.y1 = (uint32_t)__shfl_xor((int)b.y1, d);
        b.join(o);
    }
    return b;
}

// the block's box, in thread 0
__device__ __forceinline__ Box block_box(Box b)
{
    constexpr uint32_t WAVES = DELTA_BLOCK / 64;
    __shared__ uint32_t part[WAVES][4];
    b = wave_box(b);
    if ((threadIdx.x & 63u) == 0u) {
        uint32_t *p = part[threadIdx.x >> 6];
        p[0] = b.x0; p[1] = b.y0; p[2] = b.x1; p[3] = b.y1;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (uint32_t v = 1; v < WAVES; v++) b.join(Box{part[v][0], part[v][1], part[v][2], part[v][3]});
    return b;
}

// which of a dword's four bytes are not zero, as four bits
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t x)
{
    return ((x & 0xFFu) ? 1u : 0u) | ((x & 0xFF00u) ? 2u : 0u) | ((x & 0xFF0000u) ? 4u : 0u) | ((x & 0xFF000000u) ? 8u : 0u);
}

__global__ __launch_bounds__(DELTA_BLOCK) void maray_frame_delta(const DeltaArgs a)
{
    Box box{0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u};
    // `head` bytes up to cur's first 16-byte boundary, whole vectors, a tail
    const uint32_t mis = (uint32_t)((uintptr_t)a.cur & 15);
    const uint32_t head = mis ? (16u - mis < a.bytes ? 16u - mis : a.bytes) : 0u;
    const uint32_t n_vec = (a.bytes - head) / 16u;
    const uint32_t stride = gridDim.x * DELTA_BLOCK;
    const uint4 *cq = (const uint4 *)(a.cur + head);
    // prev's bytes of the same vector: pm bytes into an aligned vector (the same for every lane), dword dw, byte r
    const unsigned char *p0 = a.prev + head;
    const uint32_t pm = (uint32_t)((uintptr_t)p0 & 15), dw = pm >> 2, r = pm & 3u;
    const uint4 *pq = (const uint4 *)(p0 - pm);
    for (uint32_t v = blockIdx.x * DELTA_BLOCK + threadIdx.x; v < n_vec; v += stride) {
        const uint4 c = cq[v];
        const uint4 lo = pq[v];
        // (with pm > 0 the next aligned vector holds this one's last pm bytes: it is inside the raster)
        const uint4 hi = pm ? pq[v + 1u] : make_uint4(0u, 0u, 0u, 0u);
        const uint32_t d[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        uint32_t e[5];
#pragma unroll
        for (int k = 0; k < 5; k++) e[k] = dw == 0u ? d[k] : dw == 1u ? d[k + 1] : dw == 2u ? d[k + 2] : d[k + 3];
        const uint32_t x0 = __builtin_amdgcn_alignbyte(e[1], e[0], r) ^ c.x, x1 = __builtin_amdgcn_alignbyte(e[2], e[1], r) ^ c.y;
        const uint32_t x2 = __builtin_amdgcn_alignbyte(e[3], e[2], r) ^ c.z, x3 = __builtin_amdgcn_alignbyte(e[4], e[3], r) ^ c.w;
        if (x0 | x1 | x2 | x3) {
            const uint32_t diff = nonzero_bytes(x0) | (nonzero_bytes(x1) << 4) | (nonzero_bytes(x2) << 8) | (nonzero_bytes(x3) << 12);
            // the vector's first byte is byte `rem` of pixel `pix`; pixel pix + k holds the vector's bytes 3 k - rem .. 3 k - rem + 2
            const uint32_t at = head + 16u * v, pix = at / 3u, rem = at - 3u * pix;
            uint32_t y = pix / a.w, x = pix - y * a.w;
#pragma unroll
            for (int k = 0; k < 7; k++) {
                if (diff & (((7u << (3 * k)) >> rem) & 0xFFFFu)) box.add(x, y);
                if (++x == a.w) { x = 0u; y++; }
            }
        }
    }
    // head and tail, fewer than 16 bytes each, byte by byte
    if (blockIdx.x == 0 && threadIdx.x < 32) {
        const uint32_t tail0 = head + n_vec * 16u;
        const uint32_t i = threadIdx.x < 16 ? threadIdx.x : tail0 + (threadIdx.x - 16u);
        const bool mine = threadIdx.x < 16 ? i < head : i < a.bytes;
        if (mine && a.prev[i] != a.cur[i]) {
            const uint32_t pix = i / 3u, y = pix / a.w;
            box.add(pix - y * a.w, y);
        }
    }
    box = block_box(box);
    if (threadIdx.x == 0) *(uint4 *)(a.partials + 4 * (size_t)blockIdx.x) = make_uint4(box.x0, box.y0, box.x1, box.y1);
}

__global__ __launch_bounds__(DELTA_BLOCK) void maray_frame_delta_box(const uint32_t *partials, const uint32_t n, uint32_t *out)
{
    Box box{0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u};
    for (uint32_t i = threadIdx.x; i < n; i += DELTA_BLOCK) {
        const uint4 p = *(const uint4 *)(partials + 4 * (size_t)i);
        box.join(Box{p.x, p.y, p.z, p.w});
    }
    box = block_box(box);
    if (threadIdx.x == 0) {
        const bool empty = box.x1 == 0u;
        *(uint4 *)out = empty ? make_uint4(0u, 0u, 0u, 0u) : make_uint4(box.x0, box.y0, box.x1, box.y1);
    }
}

}   // namespace

void frame_delta(const unsigned char *d_prev, const unsigned char *d_cur, uint32_t w, uint32_t h, uint32_t *d_partials, uint32_t *d_box, hipStream_t st)
{
    if (!d_prev || !d_cur || !d_partials || !d_box || !w || !h || ((uintptr_t)d_partials & 15) || ((uintptr_t)d_box & 15) ||
        (uint64_t)w * 3 * h > APNG_FRAME_MAX_BYTES)
        throw Error{MARAY_E_INTERNAL, "frame delta: bad arguments"};
    const DeltaArgs a{d_prev, d_cur, d_partials, w, (uint32_t)((size_t)w * 3 * h)};
    const uint32_t grid = frame_delta_blocks(a.bytes);
    (void)hipGetLastError();
    hipLaunchKernelGGL(maray_frame_delta, dim3(grid), dim3(DELTA_BLOCK), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(maray_frame_delta_box, dim3(1), dim3(DELTA_BLOCK), 0, st, (const uint32_t *)d_partials, grid, d_box);
    HIP_TRY(hipGetLastError());
}

namespace {
constexpr size_t DELTA_SCRATCH = (size_t)DELTA_MAX_BLOCKS * 16 + 16;       // the partial boxes, then the box
}

void frame_delta_once(int device, const unsigned char *d_prev, const unsigned char *d_cur, uint32_t w, uint32_t h, hipStream_t st, uint32_t box[4])
{
    HIP_TRY(hipSetDevice(device));
    struct Own {
        uint32_t *d = nullptr, *host = nullptr;
        ~Own() { (void)hipFree(d); if (host) (void)hipHostFree(host); }
    } o;
    HIP_TRY(hipMalloc((void **)&o.d, DELTA_SCRATCH));
    HIP_TRY(hipHostMalloc((void **)&o.host, 16, hipHostMallocDefault));
    uint32_t *d_box = o.d + 4 * (size_t)DELTA_MAX_BLOCKS;
    frame_delta(d_prev, d_cur, w, h, o.d, d_box, st);
    HIP_TRY(hipMemcpyAsync(o.host, d_box, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < 4; i++) box[i] = o.host[i];
}

float frame_delta_time(int device, uint32_t w, uint32_t h, int reps, float *copy_ms)
{
    if (!w || !h || reps <= 0) throw Error{MARAY_E_ARG, "frame_delta_time: w, h and reps > 0"};
    apng_check_frame(w, h);
    HIP_TRY(hipSetDevice(device));
    struct Own {
        unsigned char *a = nullptr, *b = nullptr; uint32_t *d = nullptr; hipStream_t st = nullptr; hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Own() { (void)hipFree(a); (void)hipFree(b); (void)hipFree(d); if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); if (st) (void)hipStreamDestroy(st); }
    } o;
    const size_t bytes = (size_t)w * 3 * h;
    HIP_TRY(hipMalloc((void **)&o.a, bytes));
    HIP_TRY(hipMalloc((void **)&o.b, bytes));
    HIP_TRY(hipMalloc((void **)&o.d, DELTA_SCRATCH));
    measurement_fill(o.a, bytes);
    HIP_TRY(hipStreamCreate(&o.st));
    HIP_TRY(hipEventCreate(&o.e0)); HIP_TRY(hipEventCreate(&o.e1));
    // b = a but for the first and the last byte: the full box, found at the two ends of the grid
    HIP_TRY(hipMemcpyAsync(o.b, o.a, bytes, hipMemcpyDeviceToDevice, o.st));
    HIP_TRY(hipMemsetAsync(o.b, 0xA5, 1, o.st));
    HIP_TRY(hipMemsetAsync(o.b + bytes - 1, 0xA5, 1, o.st));
    uint32_t *d_box = o.d + 4 * (size_t)DELTA_MAX_BLOCKS;
    float ms = 0.f;
    frame_delta(o.a, o.b, w, h, o.d, d_box, o.st);
    HIP_TRY(hipEventRecord(o.e0, o.st));
    for (int i = 0; i < reps; i++) frame_delta(o.a, o.b, w, h, o.d, d_box, o.st);
    HIP_TRY(hipEventRecord(o.e1, o.st));
    HIP_TRY(hipEventSynchronize(o.e1));
    HIP_TRY(hipEventElapsedTime(&ms, o.e0, o.e1));
    uint32_t got[4];
    HIP_TRY(hipMemcpy(got, d_box, 16, hipMemcpyDeviceToHost));
    if (got[0] != 0 || got[1] != 0 || got[2] != w || got[3] != h) throw Error{MARAY_E_INTERNAL, "frame_delta_time: the timed kernel found the wrong box"};
    if (copy_ms) {
        HIP_TRY(hipEventRecord(o.e0, o.st));
        for (int i = 0; i < reps; i++) HIP_TRY(hipMemcpyAsync(o.b, o.a, bytes, hipMemcpyDeviceToDevice, o.st));
        HIP_TRY(hipEventRecord(o.e1, o.st));
        HIP_TRY(hipEventSynchronize(o.e1));
        HIP_TRY(hipEventElapsedTime(copy_ms, o.e0, o.e1));
        *copy_ms /= (float)reps;
    }
    return ms / (float)reps;
}

}   // namespace maray
