// yuv.hip — maray_rgb_to_ycc<SAMPLING>: a packed RGB8 raster to the three planes of a limited-range Y'CbCr frame, 4:2:0 or
// 4:4:4 (product code; include/maray_hip.h, "raw video").
//
// Memory-bound: 3 bytes are read and 1.5 (4:2:0) or 3 (4:4:4) written per pixel.  A lane takes YCC_LANE_PIXELS = 8 adjacent
// pixels of two rows, 2j and 2j + 1: per row the 24 bytes as the six or seven aligned dwords that hold them (a row pitch of 3 w
// puts every row at another alignment; the seventh dword is read only where the row's bytes reach into it, so no dword is read
// that holds no byte of the raster), shifted into place by v_alignbyte_b32 and again into one dword per pixel (R, G, B, and
// a byte no weight reads).  Every sum is a v_dot4_u32_u8 against a weight word: Y' one, a chroma sample the dot with the
// row's positive weights minus the dot with its negative weights' magnitudes -- at 4:2:0 both accumulated over the block's
// four pixels, which is the contract's c . (Rs, Gs, Bs) term by term.  Outputs: two dwords of Y' per row and one dword each
// of Cb and Cr (4:2:0), or two dwords of every plane per row (4:4:4); bytes where a plane's row is not dword-aligned there or
// the image's row ends inside the lane's eight pixels.  Those last lanes gather their pixels one by one, clamped to the image
// by index, and an odd height's last row pairs with itself.
// A block's four wavefronts lie under each other: a tile of YCC_BLOCK_PIXELS x YCC_BLOCK_ROWS pixels; blocks stride over the
// tiles (the grid is capped at YCC_MAX_BLOCKS).  The matrix arrives as five wave-uniform weight words.
// No atomics, no LDS, no inline assembly, no scratch memory; nothing is written but the planes.
#include <hip/hip_runtime.h>

#include <string>

#include "shutter.hpp"
#include "yuv.hpp"

namespace maray {

namespace {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            throw Error{MARAY_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)};           \
    } while (0)

constexpr int NP = (int)YCC_LANE_PIXELS;
static_assert(NP == 8, "the loads, the pixel shifts and the stores below are written for eight pixels a lane");

struct YccArgs {
    const unsigned char *rgb;
    unsigned char *y, *cb, *cr;
    uint32_t w, h, tiles_x, n_tiles;
    uint32_t yw, cbp, cbn, crp, crn;        // weights of R, G, B in bytes 0, 1, 2: luma; chroma's positive ones and the others' magnitudes
};

// px[k] = pixel x0 + k of the row as R | G << 8 | B << 16 (byte 3: anything).  whole: the row holds all eight.
__device__ __forceinline__ void load_pixels(const unsigned char *row, uint32_t x0, uint32_t w, bool whole, uint32_t px[NP])
{
    if (whole) {
        const unsigned char *p = row + 3 * (size_t)x0;
        const uint32_t mis = (uint32_t)((uintptr_t)p & 3);
        const uint32_t *q = (const uint32_t *)(p - mis);
        uint32_t d[7], f[6];
#pragma unroll
        for (int i = 0; i < 6; i++) d[i] = q[i];
        d[6] = mis ? q[6] : 0u;         // (with mis > 0 it holds the 24 bytes' last mis ones; with mis = 0 it may lie past the raster)
#pragma unroll
        for (int i = 0; i < 6; i++) f[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], mis);
#pragma unroll
        for (int k = 0; k < NP; k++) {
            const int j = (3 * k) >> 2, s = (3 * k) & 3;
            px[k] = s == 0 ? f[j] : j + 1 < 6 ? __builtin_amdgcn_alignbyte(f[j + 1 < 6 ? j + 1 : j], f[j], s) : f[j] >> (8 * s);
        }
    } else {
#pragma unroll
        for (int k = 0; k < NP; k++) {
            const uint32_t xc = min(x0 + (uint32_t)k, w - 1u);
            const unsigned char *p = row + 3 * (size_t)xc;
            px[k] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
        }
    }
}

// the first n of N values (each 0 .. 255) as bytes at dst: whole dwords where all N are wanted and dst is aligned
template <int N>
__device__ __forceinline__ void store_bytes(unsigned char *dst, const uint32_t v[N], uint32_t n)
{
    if (n == (uint32_t)N && ((uintptr_t)dst & 3) == 0) {
#pragma unroll
        for (int i = 0; i < N; i += 4) *(uint32_t *)(dst + i) = v[i] | (v[i + 1] << 8) | (v[i + 2] << 16) | (v[i + 3] << 24);
    } else {
#pragma unroll
        for (int i = 0; i < N; i++)
            if ((uint32_t)i < n) dst[i] = (unsigned char)v[i];
    }
}

__device__ __forceinline__ uint32_t dot(uint32_t px, uint32_t weights, uint32_t acc) { return __builtin_amdgcn_udot4(px, weights, acc, false); }

// one row's eight samples of a full-resolution plane: ((pos . p - neg . p + 128) >> 8) + offset (luma has no negative weight)
template <bool SIGNED>
__device__ __forceinline__ void plane_row(const uint32_t px[NP], uint32_t pos, uint32_t neg, int offset, unsigned char *dst, uint32_t n)
{
    uint32_t v[NP];
#pragma unroll
    for (int k = 0; k < NP; k++) {
        const int s = (int)dot(px[k], pos, 128u) - (SIGNED ? (int)dot(px[k], neg, 0u) : 0);
        v[k] = (uint32_t)((s >> 8) + offset);
    }
    store_bytes<NP>(dst, v, n);
}

// four samples of a half-resolution plane from the two rows' eight pixels: ((c . (Rs, Gs, Bs) + 512) >> 10) + 128
__device__ __forceinline__ void chroma_420(const uint32_t p0[NP], const uint32_t p1[NP], uint32_t pos, uint32_t neg, unsigned char *dst, uint32_t n)
{
    uint32_t v[NP / 2];
#pragma unroll
    for (int i = 0; i < NP / 2; i++) {
        const uint32_t a = dot(p1[2 * i + 1], pos, dot(p1[2 * i], pos, dot(p0[2 * i + 1], pos, dot(p0[2 * i], pos, 512u))));
        const uint32_t b = dot(p1[2 * i + 1], neg, dot(p1[2 * i], neg, dot(p0[2 * i + 1], neg, dot(p0[2 * i], neg, 0u))));
        v[i] = (uint32_t)((((int)a - (int)b) >> 10) + 128);
    }
    store_bytes<NP / 2>(dst, v, n);
}

template <uint32_t SAMPLING>
__global__ __launch_bounds__(YCC_BLOCK) void maray_rgb_to_ycc(const YccArgs a)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const size_t pitch = (size_t)a.w * 3;
    for (uint32_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        const uint32_t ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
        const uint32_t x0 = tx * YCC_BLOCK_PIXELS + lane * YCC_LANE_PIXELS, r0 = ty * YCC_BLOCK_ROWS + 2u * wave;
        if (x0 >= a.w || r0 >= a.h) continue;
        const uint32_t n = min(YCC_LANE_PIXELS, a.w - x0);
        const bool whole = n == YCC_LANE_PIXELS, two = r0 + 1u < a.h;
        const uint32_t r1 = two ? r0 + 1u : r0;                 // an odd height's last row: clamped by index
        uint32_t p0[NP], p1[NP];
        load_pixels(a.rgb + (size_t)r0 * pitch, x0, a.w, whole, p0);
        load_pixels(a.rgb + (size_t)r1 * pitch, x0, a.w, whole, p1);
        const size_t at0 = (size_t)r0 * a.w + x0, at1 = (size_t)r1 * a.w + x0;
        plane_row<false>(p0, a.yw, 0u, 16, a.y + at0, n);
        if (two) plane_row<false>(p1, a.yw, 0u, 16, a.y + at1, n);
        if (SAMPLING == MARAY_YCC_444) {
            plane_row<true>(p0, a.cbp, a.cbn, 128, a.cb + at0, n);
            plane_row<true>(p0, a.crp, a.crn, 128, a.cr + at0, n);
            if (two) {
                plane_row<true>(p1, a.cbp, a.cbn, 128, a.cb + at1, n);
                plane_row<true>(p1, a.crp, a.crn, 128, a.cr + at1, n);
            }
        } else {
            const uint32_t cw = (a.w + 1u) / 2u;
            const size_t at = (size_t)(r0 / 2u) * cw + x0 / 2u;
            chroma_420(p0, p1, a.cbp, a.cbn, a.cb + at, (n + 1u) / 2u);
            chroma_420(p0, p1, a.crp, a.crn, a.cr + at, (n + 1u) / 2u);
        }
    }
}

// the coefficient rows (y; cb; cr) of include/maray_hip.h
constexpr int COEFF[2][9] = {{66, 129, 25, -38, -74, 112, 112, -94, -18},          // MARAY_YCC_BT601
                             {47, 157, 16, -26, -86, 112, 112, -102, -10}};        // MARAY_YCC_BT709

uint32_t weight_word(const int *row, int sign)
{
    uint32_t r = 0;
    for (int i = 0; i < 3; i++)
        if (row[i] * sign > 0) r |= (uint32_t)(row[i] * sign) << (8 * i);
    return r;
}

}   // namespace

void ycc_opts_words(const maray_ycc_opts *opts, uint32_t *sampling, uint32_t *matrix)
{
    *sampling = opts ? opts->sampling : (uint32_t)MARAY_YCC_420;
    *matrix = opts ? opts->matrix : (uint32_t)MARAY_YCC_BT601;
    if (*sampling != MARAY_YCC_420 && *sampling != MARAY_YCC_444) throw Error{MARAY_E_ARG, "unknown Y'CbCr sampling"};
    if (*matrix != MARAY_YCC_BT601 && *matrix != MARAY_YCC_BT709) throw Error{MARAY_E_ARG, "unknown Y'CbCr matrix"};
    for (int i = 0; opts && i < 6; i++)
        if (opts->reserved[i]) throw Error{MARAY_E_ARG, "maray_ycc_opts: a reserved word is not 0"};
}

void ycc_check_frame(uint32_t w, uint32_t h)
{
    if (!w || !h) throw Error{MARAY_E_ARG, "empty image"};
    if (w > MARAY_DOMAIN_MAX || h > MARAY_DOMAIN_MAX) throw Error{MARAY_E_LIMIT, "image exceeds " + std::to_string(MARAY_DOMAIN_MAX) + " pixels in x or y"};
    if ((uint64_t)w * 3 * h > YCC_FRAME_MAX_BYTES) throw Error{MARAY_E_LIMIT, "frame too large for the Y'CbCr conversion: more than 2^30 bytes"};
}

void rgb_to_ycc(const unsigned char *d_rgb, uint32_t w, uint32_t h, uint32_t sampling, uint32_t matrix, unsigned char *d_planes, hipStream_t st)
{
    if (!d_rgb || !d_planes || !w || !h || (uint64_t)w * 3 * h > YCC_FRAME_MAX_BYTES || (sampling != MARAY_YCC_420 && sampling != MARAY_YCC_444) ||
        (matrix != MARAY_YCC_BT601 && matrix != MARAY_YCC_BT709))
        throw Error{MARAY_E_INTERNAL, "rgb_to_ycc: bad arguments"};
    const int *m = COEFF[matrix == MARAY_YCC_BT709 ? 1 : 0];
    YccArgs a;
    a.rgb = d_rgb;
    a.y = d_planes;
    a.cb = a.y + (size_t)w * h;
    a.cr = a.cb + (ycc_frame_bytes(w, h, sampling) - (size_t)w * h) / 2;
    a.w = w; a.h = h;
    a.tiles_x = ycc_tiles_x(w);
    a.n_tiles = a.tiles_x * ycc_tiles_y(h);
    a.yw = weight_word(m, 1);
    a.cbp = weight_word(m + 3, 1); a.cbn = weight_word(m + 3, -1);
    a.crp = weight_word(m + 6, 1); a.crn = weight_word(m + 6, -1);
    const dim3 grid(ycc_blocks(w, h));
    (void)hipGetLastError();
    if (sampling == MARAY_YCC_444) hipLaunchKernelGGL(maray_rgb_to_ycc<MARAY_YCC_444>, grid, dim3(YCC_BLOCK), 0, st, a);
    else hipLaunchKernelGGL(maray_rgb_to_ycc<MARAY_YCC_420>, grid, dim3(YCC_BLOCK), 0, st, a);
    HIP_TRY(hipGetLastError());
}

float rgb_to_ycc_time(int device, uint32_t w, uint32_t h, uint32_t sampling, uint32_t matrix, int reps, float *copy_ms)
{
    if (reps <= 0) throw Error{MARAY_E_ARG, "rgb_to_ycc_time: reps > 0"};
    ycc_check_frame(w, h);
    HIP_TRY(hipSetDevice(device));
    struct Own {
        unsigned char *rgb = nullptr, *planes = nullptr; hipStream_t st = nullptr; hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Own() { (void)hipFree(rgb); (void)hipFree(planes); if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); if (st) (void)hipStreamDestroy(st); }
    } o;
    const size_t rgb_bytes = (size_t)w * 3 * h, out_bytes = ycc_frame_bytes(w, h, sampling);
    const size_t copy_bytes = (rgb_bytes + out_bytes) / 2;         // a copy reads and writes every byte: as many bytes moved
    HIP_TRY(hipMalloc((void **)&o.rgb, rgb_bytes));
    HIP_TRY(hipMalloc((void **)&o.planes, std::max(out_bytes, copy_bytes)));
    measurement_fill(o.rgb, rgb_bytes);
    HIP_TRY(hipStreamCreate(&o.st));
    HIP_TRY(hipEventCreate(&o.e0)); HIP_TRY(hipEventCreate(&o.e1));
    float ms = 0.f;
    rgb_to_ycc(o.rgb, w, h, sampling, matrix, o.planes, o.st);
    HIP_TRY(hipEventRecord(o.e0, o.st));
    for (int i = 0; i < reps; i++) rgb_to_ycc(o.rgb, w, h, sampling, matrix, o.planes, o.st);
    HIP_TRY(hipEventRecord(o.e1, o.st));
    HIP_TRY(hipEventSynchronize(o.e1));
    HIP_TRY(hipEventElapsedTime(&ms, o.e0, o.e1));
    if (copy_ms) {
        HIP_TRY(hipMemcpyAsync(o.planes, o.rgb, copy_bytes, hipMemcpyDeviceToDevice, o.st));
        HIP_TRY(hipEventRecord(o.e0, o.st));
        for (int i = 0; i < reps; i++) HIP_TRY(hipMemcpyAsync(o.planes, o.rgb, copy_bytes, hipMemcpyDeviceToDevice, o.st));
        HIP_TRY(hipEventRecord(o.e1, o.st));
        HIP_TRY(hipEventSynchronize(o.e1));
        HIP_TRY(hipEventElapsedTime(copy_ms, o.e0, o.e1));
        *copy_ms /= (float)reps;
    }
    return ms / (float)reps;
}

}   // namespace maray
